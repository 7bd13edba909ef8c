"""CPU: the host side of the NSynth encoding (audio_style_transfer_amd/encoding.py: fastgen.encode
and nsynth_save_embeddings.py restated) with a stub engine, the refusal of --enc outside
methods, and the argument rules of set_encoding_target that need no device."""
import ctypes
import os

import numpy as np
import pytest

import encoding_stub
from audio_style_transfer_amd import _lib, batch, encoding, longform, methods, utils
from audio_style_transfer_amd.engine import check_encoding_target

STUB = dict(engine_cls=encoding_stub.EncStubEngine, device='cpu', weights={})


def test_trim_1d_2d_and_short():
    a = np.arange(70000, dtype=np.float32)
    w, n = encoding.trim_for_encoding(a, 64000)
    assert n == 64000 and w.shape == (64000,) and w[-1] == 63999
    w, n = encoding.trim_for_encoding(a[:1300], 64000)          # shorter than sample_length
    assert n == 1024 and w.shape == (1024,)
    w, n = encoding.trim_for_encoding(a, 1000)                  # a cap that is no multiple of 512
    assert n == 512 and w.shape == (512,)
    b = np.stack([a[:2000], a[5:2005]])
    w, n = encoding.trim_for_encoding(b, 64000)
    assert n == 1536 and w.shape == (2, 1536) and w[1, 0] == 5
    w, n = encoding.trim_for_encoding(b, 1024)
    assert n == 1024 and w.shape == (2, 1024)
    with pytest.raises(ValueError):
        encoding.trim_for_encoding(np.zeros((1, 2, 3)), 512)


def test_encode_shapes_and_mu_law():
    rng = np.random.default_rng(0)
    wav = rng.uniform(-0.5, 0.5, (2, 1300)).astype(np.float32)
    del encoding_stub.BUILT[:]
    e = encoding.encode(wav, sample_length=64000, **STUB)
    assert e.shape == (2, 2, 16) and e.dtype == np.float32
    assert encoding_stub.BUILT[-1][:2] == (2, 1024) and encoding_stub.BUILT[-1][2]['encoding'] is True
    want = utils.mu_law_numpy(wav[:, :1024]).reshape(2, 2, 512).mean(2)
    assert np.allclose(e[:, :, 0], want, rtol=1e-6, atol=1e-6) and np.allclose(e[:, :, 15], 16 * want, rtol=1e-6, atol=1e-5)
    e1 = encoding.encode(wav[0], sample_length=64000, **STUB)           # 1-D input: a batch of one
    assert e1.shape == (1, 2, 16) and np.array_equal(e1[0], e[0])
    with pytest.raises(ValueError, match='at least 512'):
        encoding.encode(wav[0, :300], **STUB)


def test_embedding_names_strip_characters():
    names = ['flute.wav', 'wave.wav', 'dir/a.b/viola.wav', 'x.WAV', 'aww.wav', 'drum.wav.wav']
    got = [encoding.embedding_name(n) for n in names]
    assert got == ['flute_embeddings.npy', 'e_embeddings.npy', 'iol_embeddings.npy',
                   'x.WAV_embeddings.npy', '_embeddings.npy', 'drum_embeddings.npy']


def _write(path, sig, sr=16000):
    from scipy.io import wavfile
    wavfile.write(path, sr, (sig * 32767).astype(np.int16))


def test_cli_batches_with_filler_and_writes_only_real_files(tmp_path):
    src, dst = tmp_path / 'src', tmp_path / 'out' / 'emb'
    src.mkdir()
    rng = np.random.default_rng(1)
    clips = {}
    for k, name in enumerate(['b.wav', 'a.wav', 'c.wav', 'd.WAV', 'e.wav']):
        clips[name] = rng.uniform(-0.9, 0.9, 1200 + 10 * k).astype(np.float32)
        _write(str(src / name), clips[name])
    (src / 'notes.txt').write_text('not audio')
    del encoding_stub.BUILT[:]
    rc = encoding.main(['--source_path', str(src), '--save_path', str(dst), '--sample_length', '1100',
                        '--batch_size', '2', '--engine', 'encoding_stub:EncStubEngine'])
    assert rc == 0
    # 5 files in batches of 2: the last batch holds e.wav twice, every batch is a full 2 x 1024
    assert [b[:2] for b in encoding_stub.BUILT] == [(2, 1024)] * 3
    assert sorted(os.listdir(dst)) == ['_embeddings.npy', 'b_embeddings.npy', 'c_embeddings.npy',
                                       'd.WAV_embeddings.npy', 'e_embeddings.npy']
    got = np.load(str(dst / 'c_embeddings.npy'))
    assert got.shape == (2, 16)
    q = (clips['c.wav'] * 32767).astype(np.int16).astype(np.float32) / 32768.0
    want = utils.mu_law_numpy(q[:1024]).reshape(2, 512).mean(1)
    assert np.allclose(got[:, 0], want, rtol=1e-6, atol=1e-6)


def test_cli_refuses_a_short_file(tmp_path, capsys):
    src = tmp_path / 'src'
    src.mkdir()
    _write(str(src / 'short.wav'), np.zeros(900, np.float32))
    with pytest.raises(SystemExit):
        encoding.main(['--source_path', str(src), '--save_path', str(tmp_path / 'o'),
                       '--sample_length', '1024', '--engine', 'encoding_stub:EncStubEngine'])
    err = capsys.readouterr().err
    assert 'short.wav' in err and 'fewer than --sample_length 1024' in err


def test_batch_and_longform_refuse_enc():
    a = batch.make_parser().parse_args(['--pairs', 'a:b', '--enc', '2'])
    with pytest.raises(ValueError, match='--enc'):
        batch.check_args(a)
    batch.check_args(batch.make_parser().parse_args(['--pairs', 'a:b']))
    a = longform.make_parser().parse_args(['c', 's', '--optimizer', 'device', '--enc', '0.5'])
    with pytest.raises(ValueError, match='--enc'):
        longform.check_args(a)
    longform.check_args(longform.make_parser().parse_args(['c', 's', '--optimizer', 'device', '--enc', '0']))


def test_enc_flag_stays_out_of_the_output_dir(tmp_path):
    p = methods.make_parser()
    assert p.parse_args(['c', 's']).enc == 0.0
    a, b = p.parse_args(['c', 's', '--stack', '0']), p.parse_args(['c', 's', '--stack', '0', '--enc', '5'])
    assert methods.get_dir(str(tmp_path), a) == methods.get_dir(str(tmp_path), b)
    with pytest.raises(ValueError):
        methods.GatysNet(enc=-1.0, weights={}, engine_cls=None)


def test_set_encoding_target_argument_rules():
    check_encoding_target((3, 2, 16), 1.0, 3, 1024)
    check_encoding_target((2, 16), 0.0, 3, 1024)                # shared
    check_encoding_target(None, 0.0, 3, 1024)                   # clearing
    for shape in ((3, 2, 8), (2, 2, 16), (3, 3, 16), (16,), (1, 3, 2, 16)):
        with pytest.raises(ValueError, match='phi_e'):
            check_encoding_target(shape, 1.0, 3, 1024)
    for omega in (-1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='omega'):
            check_encoding_target((3, 2, 16), omega, 3, 1024)
    with pytest.raises(_lib.AstError):
        check_encoding_target((3, 2, 16), 1.0, 3, 1024, with_encoding=False)


def test_workspace_grows_only_with_the_field():
    """with_encoding = 0 is the parent's size (tests/test_abi.py pins that formula); = 1 in a
    fused-content split configuration adds the content-gradient buffer the unfused path and the
    term need, B x T x 128 fp32, and the small encoding buffers."""
    lib = _lib.load()

    def ws(enc, **kw):
        c = _lib.AstCfg()
        c.batch, c.T, c.n_cont, c.n_style = 2, 16384, 1, 30
        c.cont_ids[0] = 29
        for i in range(30):
            c.style_ids[i] = i
        c.cnt_channels = c.nb_channels = 128
        c.precision, c.lambd = kw.get('precision', 2), 100.0
        c.with_encoding = enc
        n = ctypes.c_size_t()
        rc = lib.ast_workspace_bytes(ctypes.byref(c), ctypes.byref(n))
        return rc, n.value
    (rc0, n0), (rc1, n1) = ws(0), ws(1)
    assert rc0 == 0 and rc1 == 0
    assert n1 - n0 == 2 * 16384 * 128 * 4 + 2 * (32 * 33 + 1) * 4
    assert ws(2)[0] == -1
    # fp32, content 29: the tap already owns cg_buf[30]; only the small buffers are new
    (_, m0), (_, m1) = ws(0, precision=0), ws(1, precision=0)
    assert m1 - m0 == 2 * (32 * 33 + 1) * 4
