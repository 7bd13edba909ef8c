"""CPU: decoder scoring's host-side pieces (ast_dec_score_workspace_bytes), scoring.quantize, and
the Python layer of scoring.py and its CLI against a numpy stand-in scorer (score_oracle.NumpyScorer,
injected the way decoder_oracle.NumpyDecoder is); the two input modes in the oracle."""
import ctypes
import json
import os

import numpy as np
import pytest

import decoder_oracle as O
import score_oracle as SO
from audio_style_transfer_amd import _lib, encoding, scoring, synthesis
from audio_style_transfer_amd.weights import synthetic_decoder_weights

SMALL = dict(width=64, skip_width=32, n_layers=4)
HOP = synthesis.HOP


def _ws(batch, T, cfg_batch=1, **kw):
    c = dict(batch=cfg_batch, width=512, skip_width=256, n_layers=30, n_stages=10, n_z=16, hop=512)
    c.update(kw)
    cfg = _lib.AstDecCfg(*[c[k] for k in ('batch', 'width', 'skip_width', 'n_layers', 'n_stages', 'n_z', 'hop')])
    lib = _lib.load()
    n = ctypes.c_size_t(0)
    rc = lib.ast_dec_score_workspace_bytes(ctypes.byref(cfg), batch, T, ctypes.byref(n))
    return rc, n.value, lib.ast_last_error().decode()


def test_workspace_bytes_grow_with_batch_and_length_and_bad_arguments_fail():
    rc, one, _ = _ws(1, 16384)
    assert rc == 0
    # l, d [T, 512] and s [T, 256] in fp32: 5 KiB per sample, 80 MiB per 16384-sample clip
    assert one == 16384 * (2 * 512 + 256) * 4 == 80 << 20
    last = 0
    for batch, T in ((1, 1), (1, 37), (1, 512), (2, 512), (3, 512), (3, 16384), (16, 16384)):
        rc, n, _ = _ws(batch, T)
        assert rc == 0 and n > last and n >= batch * T * (2 * 512 + 256) * 4
        last = n
    for kw, word in ((dict(batch=0, T=16), 'batch'), (dict(batch=-1, T=16), 'batch'), (dict(batch=1, T=0), 'T 0'),
                     (dict(batch=1, T=-5), 'T -5')):
        rc, _, msg = _ws(kw['batch'], kw['T'])
        assert rc == -1 and word in msg, (kw, rc, msg)
    rc, _, msg = _ws(1, 16, width=100)
    assert rc == -1 and 'width' in msg
    assert _lib.load().ast_dec_score_workspace_bytes(None, 1, 16, ctypes.byref(ctypes.c_size_t())) == -1
    cfg = _lib.AstDecCfg(1, 512, 256, 30, 10, 16, 512)
    assert _lib.load().ast_dec_score_workspace_bytes(ctypes.byref(cfg), 1, 16, None) == -1
    # independent of cfg.batch
    assert _ws(2, 640, cfg_batch=7)[1] == _ws(2, 640, cfg_batch=1)[1]


def test_quantize_is_the_graph_mu_law_plus_128_clamped():
    rng = np.random.RandomState(0)
    x = np.concatenate([rng.uniform(-1, 1, 4000), [0.0, 1.0, -1.0, 1e-9, -1e-9, 0.999999, -0.999999]]).astype(np.float32)
    q = scoring.quantize(x)
    want = O.mu_law_floor(x).astype(np.int64) + 128
    assert q.dtype == np.int32 and q.shape == x.shape
    assert (q == np.clip(want, 0, 255)).all()
    assert want[4001] == 256 and q[4001] == 255          # 1.0: the one clamped value
    assert q[4000] == 128 and q[4002] == 0 and want.min() == 0
    assert (want[np.abs(x) < 1] <= 255).all()
    # every bin's own audio value quantises back to the bin (the synthesis table's round trip)
    audio, xs = O.tables()
    assert (scoring.quantize(audio) == np.round(xs * 128).astype(np.int32) + 128).all()
    assert scoring.quantize(np.zeros((2, 3))).shape == (2, 3)


def test_input_modes_differ_only_where_the_tables_differ():
    """Mode 0 feeds xs256[bin], mode 1 (bin - 128) / 128.  In float32 the round trip
    bin -> audio -> floor(mu_law) lands on bin - 128 for every bin, so the tables are equal and the
    modes score alike; a table moved at one bin changes exactly the columns after that bin."""
    t0, t1 = SO.input_table(0), SO.input_table(1)
    differ = np.nonzero(t0 != t1)[0]
    print('bins where xs256[bin] != (bin - 128) / 128:', differ)
    W = synthetic_decoder_weights(3, **SMALL)
    rng = np.random.RandomState(4)
    enc = rng.randn(2, 5, 16)
    bins = rng.randint(0, 256, size=(2, 40))
    a = SO.score(W, enc, 4, 2, 8, bins, 0)
    b = SO.score(W, enc, 4, 2, 8, bins, 1)
    hit = np.isin(bins, differ)                                   # [B, T]: a differing input at t feeds t + 1..
    later = np.concatenate([np.zeros((2, 1), bool), np.cumsum(hit, axis=1)[:, :-1] > 0], axis=1)
    changed = (a['logits'] != b['logits']).any(axis=2)
    assert not (changed & ~later).any()
    if differ.size == 0:
        assert (a['logp'] == b['logp']).all() and (a['nll'] == b['nll']).all()
    with pytest.raises(ValueError):
        SO.input_table(2)
    # logp and nll are what they are defined to be
    lab = np.take_along_axis(a['pmf'], bins[..., None], axis=2)[..., 0]
    assert np.abs(a['logp'] - np.log(lab)).max() < 1e-12
    assert np.abs(a['nll'] + a['logp'].mean(axis=1)).max() < 1e-12
    r64, e32, a32 = SO.yardstick(W, enc, 4, 2, 8, bins, 1)
    assert 0 < e32 < 1e-5 and 0 < a32 < 1e-4 and (r64['logp'] == b['logp']).all()


class Scorer(SO.NumpyScorer):
    def __init__(self, batch, weights, device=None):
        SO.NumpyScorer.__init__(self, batch, weights, n_layers=4, n_stages=2, hop=HOP)


def _fake_encode(wav, checkpoint_path=None, sample_length=64000):
    """A deterministic stand-in for encoding.encode: per-hop statistics of the audio."""
    wav = np.asarray(wav, dtype=np.float32)
    h = wav.reshape(wav.shape[0], -1, HOP)
    return np.stack([h.mean(axis=2) * (k + 1) for k in range(16)], axis=2).astype(np.float32)


def test_score_trims_encodes_quantises_and_scores_in_mode_1():
    W = synthetic_decoder_weights(5, **SMALL)
    rng = np.random.RandomState(2)
    wav = rng.uniform(-0.9, 0.9, size=(2, 2 * HOP + 100)).astype(np.float32)
    SO.NumpyScorer.calls = []
    r = scoring.score(wav, sample_length=64000, weights=W, engine_cls=Scorer, encode_fn=_fake_encode)
    bins, enc, mode = SO.NumpyScorer.calls[-1]
    assert mode == 1 and bins.shape == (2, 2 * HOP) and enc.shape == (2, 2, 16)
    assert (bins == scoring.quantize(wav[:, :2 * HOP])).all()
    assert (enc == _fake_encode(wav[:, :2 * HOP])).all()
    want = SO.score(W, enc, 4, 2, HOP, bins, 1, np.float32)
    assert (r['logp'] == want['logp']).all() and (r['nll'] == want['nll']).all()
    assert sorted(r) == ['bits', 'logp', 'nll']
    assert np.allclose(r['bits'], r['nll'] / np.log(2.0), rtol=1e-6, atol=0)
    # sample_length cuts first, then whole hops; 1-D input is one clip; given encodings are used as is
    r1 = scoring.score(wav[0], sample_length=HOP + 7, weights=W, engine_cls=Scorer, encode_fn=_fake_encode)
    assert r1['logp'].shape == (1, HOP) and SO.NumpyScorer.calls[-1][1].shape == (1, 1, 16)
    other = rng.randn(2, 2, 16).astype(np.float32)
    scoring.score(wav, weights=W, engine_cls=Scorer, encodings=other,
                  encode_fn=lambda *a, **k: pytest.fail('encode must not run'))
    assert (SO.NumpyScorer.calls[-1][1] == other).all()
    with pytest.raises(ValueError, match='do not fit'):
        scoring.score(wav, weights=W, engine_cls=Scorer, encodings=other[:, :1])
    with pytest.raises(ValueError, match='at least'):
        scoring.score(wav[:, :HOP - 1], weights=W, engine_cls=Scorer, encode_fn=_fake_encode)


def _write_wavs(folder, rng, lengths):
    from scipy.io import wavfile
    os.makedirs(folder, exist_ok=True)
    clips = {}
    for name, n in lengths.items():
        a = rng.uniform(-0.8, 0.8, n).astype(np.float32)
        wavfile.write(os.path.join(folder, name + '.wav'), 16000, a)
        clips[name] = a
    return clips


def test_cli_scores_json_logp_and_encodings_pairing(tmp_path):
    W = synthetic_decoder_weights(6, **SMALL)
    rng = np.random.RandomState(3)
    src = str(tmp_path / 'src')
    clips = _write_wavs(src, rng, dict(flute=2 * HOP + 30, bell=3 * HOP, oboe=2 * HOP + 500))
    (tmp_path / 'src' / 'notes.txt').write_text('not audio')

    def score_fn(wav, checkpoint_path=None, sample_length=64000, encodings=None):
        return scoring.score(wav, checkpoint_path, sample_length=sample_length, encodings=encodings, weights=W,
                             engine_cls=Scorer, encode_fn=_fake_encode)

    out = str(tmp_path / 'out')
    args = scoring.make_parser().parse_args(['--source_path', src, '--save_path', out, '--logp',
                                             '--sample_length', str(2 * HOP + 40)])
    assert args.batch_size == 1 and args.gpu_number == 0 and args.encodings is None
    scores = scoring.score_files(args, score_fn=score_fn)
    disk = json.load(open(os.path.join(out, 'scores.json')))
    assert disk == scores and sorted(disk) == ['bell', 'flute', 'oboe']
    for name, a in clips.items():
        T = 2 * HOP
        want = scoring.score(a, sample_length=2 * HOP + 40, weights=W, engine_cls=Scorer, encode_fn=_fake_encode)
        assert disk[name]['samples'] == T
        assert disk[name]['nll_nats'] == float(want['nll'][0])
        assert disk[name]['bits_per_sample'] == float(want['bits'][0])
        assert abs(disk[name]['bits_per_sample'] - disk[name]['nll_nats'] / np.log(2.0)) <= 1e-6 * disk[name]['bits_per_sample']
        assert sorted(disk[name]) == ['bits_per_sample', 'nll_nats', 'samples']
        logp = np.load(os.path.join(out, name + '_logp.npy'))
        assert logp.shape == (T,) and (logp == want['logp'][0]).all()

    # --encodings: each file against DIR/<name>_embeddings.npy (the embeddings CLI's name rule)
    encdir = str(tmp_path / 'enc')
    os.makedirs(encdir)
    given = {}
    for name in clips:
        given[name] = rng.randn(2, 16).astype(np.float32)
        np.save(os.path.join(encdir, encoding.embedding_name(name + '.wav')), given[name])
    out2 = str(tmp_path / 'out2')
    args = scoring.make_parser().parse_args(['--source_path', src, '--save_path', out2, '--encodings', encdir,
                                             '--sample_length', str(2 * HOP + 40), '--batch_size', '2'])
    SO.NumpyScorer.calls = []
    scores2 = scoring.score_files(args, score_fn=score_fn)
    assert [c[1].shape for c in SO.NumpyScorer.calls] == [(2, 2, 16), (1, 2, 16)]      # bell + flute, oboe
    assert (SO.NumpyScorer.calls[0][1] == np.stack([given['bell'], given['flute']])).all()
    assert (SO.NumpyScorer.calls[1][1][0] == given['oboe']).all()
    assert not os.path.exists(os.path.join(out2, 'bell_logp.npy'))
    for name, a in clips.items():
        want = scoring.score(a, sample_length=2 * HOP + 40, weights=W, engine_cls=Scorer, encodings=given[name][None])
        assert abs(scores2[name]['nll_nats'] - float(want['nll'][0])) <= 1e-5 * float(want['nll'][0])
        assert abs(scores2[name]['nll_nats'] - scores[name]['nll_nats']) > 1e-3

    # a row count that does not match the trimmed length names the file; so does a missing encoding
    np.save(os.path.join(encdir, encoding.embedding_name('flute.wav')), rng.randn(3, 16).astype(np.float32))
    with pytest.raises(ValueError, match='flute'):
        scoring.score_files(args, score_fn=score_fn)
    os.remove(os.path.join(encdir, encoding.embedding_name('bell.wav')))
    with pytest.raises(ValueError, match='bell'):
        scoring.score_files(args, score_fn=score_fn)
    # one file; no save path
    args = scoring.make_parser().parse_args(['--source_path', os.path.join(src, 'oboe.wav'), '--save_path', out2])
    assert sorted(scoring.score_files(args, score_fn=score_fn)) == ['oboe']
    with pytest.raises(RuntimeError):
        scoring.score_files(scoring.make_parser().parse_args(['--source_path', src]), score_fn=score_fn)
