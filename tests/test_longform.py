"""CPU: the long-form mode (audio_style_transfer_amd/longform.py) -- its geometry, window
placement and CLI logic on the CPU stand-in engine with the anchor surface
(tests/longform_stub.py).  The runs are in-process (longform.run), so the stand-in's record of
the anchor state at every minimize call can be read afterwards."""
import glob
import os

import numpy as np
import pytest
from scipy.io import wavfile

from audio_style_transfer_amd import batch, longform

SR = 16000
T = 4096


def _wavs(d):
    os.makedirs(d, exist_ok=True)
    t = np.arange(2 * SR) / SR
    for k, (name, f) in enumerate((('a', 220.0), ('b', 330.0))):
        a = 0.5 * np.sin(2 * np.pi * f * t) + 0.1 * np.random.default_rng(k).normal(size=t.size)
        wavfile.write(os.path.join(d, name + '.wav'), SR, (np.clip(a, -1, 1) * 32767).astype(np.int16))


def _common(tmp, tag, engine, epochs):
    return ['--engine', 'longform_stub:' + engine, '--batch_size', str(T), '--epochs', str(epochs),
            '--no_plots', '--stack', '0', '--dir', os.path.join(tmp, 'src'),
            '--outdir', os.path.join(tmp, 'out_' + tag), '--logdir', os.path.join(tmp, 'log_' + tag)]


def _long(tmp, tag, extra, engine='AnchorStubEngine', epochs=2):
    args = longform.make_parser().parse_args(['a', 'b'] + _common(tmp, tag, engine, epochs) + extra)
    return longform.run(args, log=lambda m: None)


@pytest.fixture()
def tmp(tmp_path):
    _wavs(str(tmp_path / 'src'))
    return str(tmp_path)


@pytest.mark.parametrize('Tn,late', [(4096, 48), (8192, 96), (12288, 144), (16384, 192)])
def test_late(Tn, late):
    assert longform.geometry(Tn, 256).late == late
    assert longform.geometry(Tn, 256).hop == Tn - 2 * late - 256


@pytest.mark.parametrize('n', [1, 2, 5])
@pytest.mark.parametrize('F', [0, 1, 256])
def test_weights_sum_to_one(n, F):
    g = longform.geometry(T, F, n)
    assert g.n_out == (n - 1) * g.hop + T - 2 * g.late
    tot = np.zeros(g.n_out)
    cover = np.zeros(g.n_out, int)
    for k in range(n):
        w = longform.window_weights(g, k)
        assert w.dtype == np.float64 and not w[:g.late].any() and not w[T - g.late:].any()
        tot[k * g.hop:k * g.hop + T - 2 * g.late] += w[g.late:T - g.late]
        cover[k * g.hop:k * g.hop + T - 2 * g.late] += 1
    assert np.array_equal(tot, np.ones(g.n_out))
    assert cover.max() <= 2 and (cover == 2).sum() == (n - 1) * F


def test_weights_follow_the_stated_formula():
    g = longform.geometry(T, 256, 3)
    w = longform.window_weights(g, 1)
    r = lambda u: np.sin(0.5 * np.pi * u) ** 2
    i = np.arange(T, dtype=np.float64)
    np.testing.assert_allclose(w[g.late:g.late + 256], r((i[g.late:g.late + 256] - g.late + 0.5) / 256), rtol=0, atol=1e-15)
    lo = T - g.late - 256
    np.testing.assert_allclose(w[lo:T - g.late], r((T - g.late - i[lo:T - g.late] - 0.5) / 256), rtol=0, atol=1e-15)
    assert (w[g.late + 256:lo] == 1).all()
    assert (longform.window_weights(g, 0)[g.late:lo] == 1).all()          # no fade-in on window 0
    assert (longform.window_weights(g, 2)[g.late + 256:T - g.late] == 1).all()   # no fade-out on the last


@pytest.mark.parametrize('Tn,F', [(2048, 0), (4095, 16), (4096, -1), (4096, 2001), (8192, 4001)])
def test_refused_geometry(Tn, F):
    with pytest.raises(ValueError):
        longform.geometry(Tn, F)


def test_limit_geometry_is_accepted():
    assert longform.geometry(4096, 2000).hop == 2000


def test_window_count():
    g = longform.geometry(T, 256)
    n_samples, st = 2 * SR, SR - g.late
    assert longform.count_windows(T, 256, n_samples, st) == (n_samples - st - T) // g.hop + 1
    assert longform.count_windows(T, 256, n_samples, st, windows=2) == 2
    n = longform.count_windows(T, 256, n_samples, st, seconds=0.5)
    assert longform.geometry(T, 256, n).n_out >= 0.5 * SR > longform.geometry(T, 256, n - 1).n_out
    with pytest.raises(ValueError):
        longform.count_windows(T, 256, n_samples, st, windows=99)


def test_refused_flags(tmp):
    for extra in (['--optimizer', 'scipy'], ['--resume']):
        with pytest.raises(ValueError):
            _long(tmp, 'x', ['--windows', '1'] + extra)


def test_one_window_equals_batch_mode(tmp):
    """--windows 1 --seam 0: window 0 is the clip GatysNet.targets takes (ori.wav equal to the
    batch mode's), the end point is the batch mode's for the same pair on the same stand-in,
    and ep-0.wav has T - 2 late samples."""
    res = _long(tmp, 'lf', ['--windows', '1', '--seam', '0'])
    args = batch.make_parser().parse_args(['--pairs', 'a:b', '--backend', 'gloo']
                                          + _common(tmp, 'bt', 'AnchorStubEngine', 2))
    import torch
    xb = batch.run_rank(args, [('a', 'b')], 1, 0, torch.device('cpu'), log=lambda m: None)[0]
    assert res['x'].shape == (1, T) and np.array_equal(res['x'][0], xb)
    late = res['geo'].late
    ep0 = wavfile.read(os.path.join(res['savepath'], 'ep-0.wav'))[1]
    assert ep0.shape == (T - 2 * late,)
    ori_b = glob.glob(os.path.join(tmp, 'out_bt', '*', '*', 'ori.wav'))
    assert len(ori_b) == 1
    assert np.array_equal(wavfile.read(os.path.join(res['savepath'], 'ori.wav'))[1],
                          wavfile.read(ori_b[0])[1])
    assert np.array_equal(wavfile.read(os.path.join(res['savepath'], 'style.wav'))[1],
                          wavfile.read(ori_b[0].replace('ori.wav', 'style.wav'))[1])


def test_three_windows_are_three_independent_runs(tmp):
    res = _long(tmp, 'w3', ['--windows', '3', '--seam', '0'], engine='IllCondAnchorStubEngine')
    g = res['geo']
    assert res['x'].shape == (3, T) and res['epochs'] == 2
    ep1 = wavfile.read(os.path.join(res['savepath'], 'ep-1.wav'))[1]
    assert ep1.shape == (2 * g.hop + T - 2 * g.late,)
    ori = wavfile.read(os.path.join(res['savepath'], 'ori.wav'))[1]
    assert ori.shape == ep1.shape
    st = int(1.0 * SR - g.late)
    for k in range(3):
        start = (st + k * g.hop + g.late + 0.5) / SR        # int(start sr - late) = st + k hop
        one = _long(tmp, 'w1_%d' % k, ['--windows', '1', '--seam', '0', '--start', repr(start)],
                    engine='IllCondAnchorStubEngine')
        assert np.array_equal(one['x'][0], res['x'][k]), k
        o1 = wavfile.read(os.path.join(one['savepath'], 'ori.wav'))[1]
        assert np.array_equal(o1, ori[k * g.hop:k * g.hop + T - 2 * g.late])


def test_seam_term_reaches_the_engine(tmp):
    import longform_stub
    e0 = _long(tmp, 'e1', ['--windows', '3', '--seam', '1'], engine='IllCondAnchorStubEngine', epochs=1)
    del longform_stub.LOG[:], longform_stub.CALLS[:]
    res = _long(tmp, 'e2', ['--windows', '3', '--seam', '1'], engine='IllCondAnchorStubEngine', epochs=2)
    g = res['geo']
    log = list(longform_stub.LOG)
    assert len(log) == 2 and log[0] is None            # epoch 0 runs without the term
    assert longform_stub.CALLS == ['set']              # set once, before epoch 1
    ref, w, mu = log[1]
    assert mu == 1.0
    stitched = longform.stitch_numpy(e0['x'], g)       # epoch 0's end points
    want_w = np.zeros((3, T), np.float32)
    for k in range(3):
        spans = longform.seam_spans(g, k)
        assert len(spans) == (1 if k in (0, 2) else 2)
        for lo, hi in spans:
            want_w[k, lo:hi] = 1.0
            pos = k * g.hop + np.arange(lo, hi) - g.late
            assert np.array_equal(ref[k, lo:hi].numpy(), stitched[pos].astype(np.float32)), k
    assert np.array_equal(w.numpy(), want_w)
    assert want_w.sum() == 4 * g.fade
    # the term changed epoch 1: the end points differ from the --seam 0 run's
    off = _long(tmp, 'e3', ['--windows', '3', '--seam', '0'], engine='IllCondAnchorStubEngine', epochs=2)
    assert not np.array_equal(off['x'], res['x'])


def test_later_chunk_is_anchored_to_the_earlier_one(tmp):
    """--chunk 2 with 3 windows: the second chunk's first window is anchored on its fade-in to
    the first chunk's last window already in epoch 0; with --seam 0 chunking changes nothing."""
    import longform_stub
    del longform_stub.LOG[:], longform_stub.CALLS[:]
    res = _long(tmp, 'c2', ['--windows', '3', '--seam', '1', '--chunk', '2'],
                engine='IllCondAnchorStubEngine', epochs=1)
    g = res['geo']
    log = list(longform_stub.LOG)
    assert len(log) == 2 and log[0] is None and log[1] is not None
    ref, w, _ = log[1]
    from audio_style_transfer_amd import utils
    a = utils.inv_mu_law_numpy(res['x'][1])
    assert np.array_equal(ref[0, g.late:g.late + g.fade].numpy(),
                          a[T - g.late - g.fade:T - g.late].astype(np.float32))
    assert w[0, g.late:g.late + g.fade].min() == 1 and w.sum() == g.fade
    a0 = _long(tmp, 'c3', ['--windows', '3', '--chunk', '2'], engine='IllCondAnchorStubEngine')
    a1 = _long(tmp, 'c4', ['--windows', '3'], engine='IllCondAnchorStubEngine')
    assert np.array_equal(a0['x'], a1['x'])


def test_output_dir_follows_the_reference_naming(tmp_path):
    from audio_style_transfer_amd import methods
    common = ['a', 'b', '--outdir', str(tmp_path / 'o'), '--logdir', str(tmp_path / 'l')]
    args = longform.make_parser().parse_args(common + ['--windows', '4', '--fade', '128', '--seam', '2',
                                                       '--chunk', '2'])
    ref = methods.make_parser().parse_args(common + ['--optimizer', 'device'])
    assert longform.out_dirs(args)[0] == methods.get_dir(ref.outdir, ref)


def test_command_line(tmp):
    argv = ['a', 'b'] + _common(tmp, 'cli', 'AnchorStubEngine', 1)
    assert longform.main(argv + ['--seconds', '0.3']) == 0       # 4800 samples: 2 windows
    wav = glob.glob(os.path.join(tmp, 'out_cli', '*', '*', 'ep-0.wav'))
    assert len(wav) == 1
    g = longform.geometry(T, 256, 2)
    assert wavfile.read(wav[0])[1].shape == (g.n_out,)
    for bad in (['--fade', '2001'], ['--fade', '-1'], ['--batch_size', '2048'], ['--resume'],
                ['--optimizer', 'scipy'], ['--windows', '2', '--seconds', '1']):
        with pytest.raises(SystemExit):
            longform.main(argv + bad)
