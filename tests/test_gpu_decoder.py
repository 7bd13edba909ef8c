"""GPU: the WaveNet decoder (ast_dec_*, synthesis.Decoder) against the numpy oracle
(decoder_oracle.py), and its bit-exact statements.

Configurations: S = width 64, skip 32, 4 layers, 2 stages (rates 1, 2, 1, 2), hop 8, total 40;
M = width 512, skip 256, 11 layers, 10 stages (rates 1..512, then 1), hop 512, 2 clips, total 1100
(past the rate-512 ring's wrap at 1024 and two hop boundaries); F = the full default network,
1 clip, total 64.  SP = S with logits/W x 8 (a peaked pmf).

The yardstick of every tolerance is the oracle's own float32 run against its float64 run on the
same inputs: e32 = rel-L2 of the float32 logits, c32 = max |cdf32 - cdf64|.  The device's pmf must be
within max(4 e32, 1e-6) rel-L2 of the float64 pmf, and with uniforms screened to keep
delta = max(4 c32, 1e-6) away from every float64 cdf boundary the device must draw exactly the
float64 oracle's bins.  The measured figures are in the tests' docstrings and DESIGN.md §7e.
"""
import ctypes

import numpy as np
import pytest
import torch

import decoder_oracle as O
from audio_style_transfer_amd import _lib, synthesis
from audio_style_transfer_amd.weights import synthetic_decoder_weights

pytestmark = pytest.mark.gpu

CFG = {
    'S': dict(width=64, skip_width=32, n_layers=4, n_stages=2, hop=8, total=40, batch=1),
    'SP': dict(width=64, skip_width=32, n_layers=4, n_stages=2, hop=8, total=40, batch=1, peak=8.0),
    'M': dict(width=512, skip_width=256, n_layers=11, n_stages=10, hop=512, total=1100, batch=2),
    'F': dict(width=512, skip_width=256, n_layers=30, n_stages=10, hop=512, total=64, batch=1),
}
_W = {}


def weights_of(name):
    c = CFG[name]
    key = (c['width'], c['skip_width'], c['n_layers'], c.get('peak'))
    if key not in _W:
        W = synthetic_decoder_weights(11, width=c['width'], skip_width=c['skip_width'], n_layers=c['n_layers'])
        if c.get('peak'):
            W['logits/W'] = W['logits/W'] * np.float32(c['peak'])
        _W[key] = W
    return _W[key]


def make_decoder(name, batch=None, **kw):
    c = CFG[name]
    return synthesis.Decoder(batch or c['batch'], weights_of(name), width=c['width'], skip_width=c['skip_width'],
                             n_layers=c['n_layers'], n_stages=c['n_stages'], hop=c['hop'], **kw)


def enc_of(name, batch, seed=0):
    c = CFG[name]
    R = -(-c['total'] // c['hop'])
    return np.random.RandomState(100 + seed).randn(batch, R, 16).astype(np.float32)


def yardstick(name, enc, bins):
    """The float64 oracle teacher-forced on ``bins`` and its float32 run: (ref64, e32, c32)."""
    c = CFG[name]
    W = weights_of(name)
    r64 = O.sequence_run(W, enc, c['n_layers'], c['n_stages'], c['hop'], bins, dtype=np.float64)
    r32 = O.sequence_run(W, enc, c['n_layers'], c['n_stages'], c['hop'], bins, dtype=np.float32)
    e32 = O.rel_l2(r32['logits'], r64['logits'])
    c32 = float(np.abs(r32['cdf'].astype(np.float64) - r64['cdf']).max())
    return r64, e32, c32


def run_device(name, enc, u, force=None, **kw):
    dec = make_decoder(name, batch=enc.shape[0], **kw)
    try:
        dec.start(enc, u, force=force, want_pmf=True)
        assert dec.run() == u.shape[1]
        return dict(pmf=dec.pmf(), bins=dec.bins(), audio=dec.audio())
    finally:
        dec.close()


@pytest.mark.parametrize('name', ['S', 'SP', 'M', 'F'])
def test_forced_accuracy_and_exact_draws(name):
    """Checks 1 and 2: teacher-forced on random bins.  Measured on MI355X (the test prints them),
    e32 / device pmf rel-L2 against float64 / the bar max(4 e32, 1e-6):
      S  1.57e-7 / 3.12e-7 / 1e-6      SP 1.57e-7 / 6.06e-7 / 1e-6  (max pmf 0.985)
      M  4.48e-7 / 4.94e-7 / 1.79e-6   F  6.73e-7 / 7.74e-7 / 2.69e-6
    c32 4.8e-7 .. 1.2e-6, so delta 1.9e-6 .. 4.9e-6; every bin equals the float64 oracle's."""
    c = CFG[name]
    B, total = c['batch'], c['total']
    enc = enc_of(name, B)
    force = np.random.RandomState(5).randint(0, 256, size=(B, total))
    r64, e32, c32 = yardstick(name, enc, force)
    delta = max(4 * c32, 1e-6)
    u = O.screened_uniforms(r64['cdf'], delta, seed=9)
    want = np.stack([O.draw(r64['cdf'][b], u[b]) for b in range(B)])
    got = run_device(name, enc, u, force=force)
    err = O.rel_l2(got['pmf'], r64['pmf'])
    bar = max(4 * e32, 1e-6)
    print('%s: e32 %.3g c32 %.3g delta %.3g | device pmf rel-L2 %.3g (bar %.3g), max pmf %.3g, distinct bins %d'
          % (name, e32, c32, delta, err, bar, r64['pmf'].max(), len(np.unique(want))))
    assert err <= bar, (err, bar)
    assert (got['bins'] == want).all()
    tab_audio, _ = O.tables()
    assert (got['audio'] == tab_audio[want]).all()
    assert np.abs(got['pmf'].astype(np.float64).sum(-1) - 1).max() < 1e-5


@pytest.mark.parametrize('name,batch', [('S', 3), ('M', 2)])
def test_free_run_is_admissible_and_equals_the_forced_path(name, batch):
    """Check 3: a free run; the float64 oracle teacher-forced on the device's own bins must admit
    every step (the pmf bar per step, and u inside the drawn bin's cdf interval widened by delta);
    a forced device run on those bins reproduces the free run bit for bit.  Measured on MI355X,
    worst step pmf rel-L2 / bar: S 8.45e-7 / 1e-6, M 1.53e-6 / 1.72e-6 (e32 1.67e-7, 4.29e-7)."""
    c = CFG[name]
    total = c['total']
    enc = enc_of(name, batch, seed=1)
    u = np.random.RandomState(21).rand(batch, total).astype(np.float32).astype(np.float64)
    free = run_device(name, enc, u)
    bins = free['bins']
    assert bins.min() >= 0 and bins.max() <= 255 and len(np.unique(bins)) > 8
    r64, e32, c32 = yardstick(name, enc, bins)
    delta, bar = max(4 * c32, 1e-6), max(4 * e32, 1e-6)
    d = free['pmf'].astype(np.float64) - r64['pmf']
    step_err = np.linalg.norm(d, axis=2) / np.linalg.norm(r64['pmf'], axis=2)
    cdf = r64['cdf']
    hi = np.take_along_axis(cdf, bins[..., None].astype(np.int64), axis=2)[..., 0]
    lo = np.where(bins > 0, np.take_along_axis(cdf, np.maximum(bins - 1, 0)[..., None].astype(np.int64), axis=2)[..., 0], 0.0)
    hi = np.where(bins == 255, np.inf, hi)          # the clamp: bin 255 takes everything above
    print('%s free: e32 %.3g c32 %.3g | worst step pmf rel-L2 %.3g (bar %.3g), worst margin %.3g (delta %.3g)'
          % (name, e32, c32, step_err.max(), bar, min((u - lo).min(), (hi - u).min()), delta))
    assert (step_err <= bar).all(), (step_err.max(), bar)
    assert ((lo - delta < u) & (u <= hi + delta)).all()
    forced = run_device(name, enc, u, force=bins)
    for k in ('pmf', 'bins', 'audio'):
        assert (forced[k] == free[k]).all(), k


def test_a_clip_is_bit_identical_in_any_slot_of_any_batch():
    """Check 4: batch 1, each slot of batch 3, slot 16 of batch 17 (the second MFMA column tile)."""
    total = CFG['S']['total']
    enc = enc_of('S', 17, seed=2)
    u = np.random.RandomState(22).rand(17, total).astype(np.float32)
    b17 = run_device('S', enc, u)
    b3 = run_device('S', enc[[16, 0, 1]], u[[16, 0, 1]])
    for slot, clip in enumerate([16, 0, 1]):
        one = run_device('S', enc[[clip]], u[[clip]])
        for k in ('pmf', 'bins', 'audio'):
            assert (one[k][0] == b3[k][slot]).all(), (k, slot)
            assert (one[k][0] == b17[k][clip]).all(), (k, clip)
    assert len({b17['bins'][i].tobytes() for i in range(17)}) == 17      # the clips do differ


def test_reset_eager_graph_canaries_and_chunks():
    """Check 4: two runs after a reset agree; eager single steps equal a K = 16 graph replayed 3
    times for total 40, whose 8 surplus steps write nothing (canaries, position); audio is the
    table of bins; a run in two chunks with other library work between equals one run."""
    B, total, PAD = 3, CFG['S']['total'], 64
    enc = enc_of('S', B, seed=3)
    u = np.random.RandomState(23).rand(B, total).astype(np.float32)
    dev = torch.device('cuda', torch.cuda.current_device())

    def padded(dtype, n, canary):
        full = torch.full((n + PAD,), canary, dtype=dtype, device=dev)
        return full

    fb, fa, fp = padded(torch.int32, B * total, -77), padded(torch.float32, B * total, 7.5), \
        padded(torch.float32, B * total * 256, 7.5)
    out = dict(bins=fb[:B * total].view(B, total), audio=fa[:B * total].view(B, total),
               pmf=fp[:B * total * 256].view(B, total, 256))
    dec = make_decoder('S', batch=B, graph_steps=16)
    other = make_decoder('S', batch=2)
    try:
        dec.start(enc, u, want_pmf=True)                # eager, one step per call
        for _ in range(total + 5):                      # 5 calls past the end do nothing
            dec.step()
        assert dec.position() == total
        eager = dict(pmf=dec.pmf(), bins=dec.bins(), audio=dec.audio())

        dec.start(enc, u, out=out)                      # the same context after a reset: 3 replays
        assert dec.run(16) == 16 and dec.run(16) == 32 and dec.run(16) == total
        graph = dict(pmf=dec.pmf(), bins=dec.bins(), audio=dec.audio())
        for k in eager:
            assert (eager[k] == graph[k]).all(), k
        assert (fb[B * total:] == -77).all() and (fa[B * total:] == 7.5).all() and (fp[B * total * 256:] == 7.5).all()
        assert dec.run(16) == total                     # one more replay: all no-ops
        assert (dec.bins() == graph['bins']).all() and (fb[B * total:] == -77).all()
        tab_audio, _ = O.tables()
        assert (graph['audio'] == tab_audio[graph['bins']]).all()

        dec.start(enc, u, want_pmf=True)                # two chunks, another context's steps between
        assert dec.run(16) == 16
        other.start(enc[:2], u[:2])
        other.run(8)
        torch.cuda.synchronize()
        assert dec.run() == total
        for k in eager:
            assert (eager[k] == getattr(dec, k)()).all(), k
    finally:
        dec.close()
        other.close()


def test_names_counts_and_step_arguments_are_checked():
    dec = make_decoder('S')
    try:
        lib = _lib.load()
        fp = ctypes.POINTER(ctypes.c_float)

        def setw(name, n):
            a = np.zeros(max(n, 1), np.float32)
            return lib.ast_dec_set_weight(dec.h, name.encode(), a.ctypes.data_as(fp), n), lib.ast_last_error().decode()

        assert setw('res_1/W', 64 * 64)[0] == 0
        for name, n in (('res_1/W', 64 * 63), ('res_5/W', 64 * 64), ('res_0/W', 64 * 64), ('ae_res_1/W', 64 * 64),
                        ('logits/biases', 255), ('dilatedconv_1/W', 2 * 64 * 128), ('res_1/weights', 64 * 64),
                        ('cond_map_out1/W', 16 * 64)):
            rc, msg = setw(name, n)
            assert rc == -4 and name in msg, (name, rc, msg)
        enc = enc_of('S', 1)
        u = np.zeros((1, 41), np.float32)               # total 41 > R hop = 40
        with pytest.raises(_lib.AstError, match='total'):
            dec.start(enc, u)
    finally:
        dec.close()


def test_synthesize_on_the_device(tmp_path):
    """The public entry point with the default network: one hop (512 samples) from a seed equals
    the Decoder driven by hand with the reference's uniforms, and the file holds the audio."""
    from scipy.io import wavfile
    W = weights_of('F')
    enc = enc_of('F', 1, seed=4)[:, :1]
    path = str(tmp_path / 'gen_x.wav')
    audio = synthesis.synthesize(enc, [path], weights=W, samples_per_save=200, seed=31)
    assert audio.shape == (1, 512) and audio.dtype == np.float32
    dec = synthesis.Decoder(1, W)
    try:
        dec.start(enc, synthesis.draw_uniforms(512, 1, seed=31))
        dec.run()
        assert (dec.audio() == audio).all() and len(np.unique(dec.bins())) > 8
    finally:
        dec.close()
    sr, data = wavfile.read(path)
    assert sr == 16000 and (data == audio[0]).all()
