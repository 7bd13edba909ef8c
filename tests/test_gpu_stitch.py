"""ast_stitch (stitch.hip), the device-side join of overlapping windows -- run on an MI355X.

Against a numpy float64 restatement built from longform.geometry / window_weights: maximum
absolute error <= 1e-6 (values are <= 1; two fp32 weights, two products, one sum and one exp2f).
Windows cut from one signal must return that signal: within 4 fp32 ulps of 1.0 (4.8e-7) of
inv_mu_law_numpy.  Refused geometries return AST_E_ARG and launch nothing."""
import ctypes

import numpy as np
import pytest
import torch

from audio_style_transfer_amd import _lib, longform, utils

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda', 0)


def _inv_mu_law64(x):
    """utils.inv_mu_law_numpy in float64 (x the float32 values)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    o = (x + 0.5) * 2.0 / 256.0
    return np.where(x == 0, 0.0, np.sign(o) / 255.0 * (256.0 ** np.abs(o) - 1.0))


def _stitch64(x, g):
    out = np.zeros(g.n_out)
    V = g.T - 2 * g.late
    for k in range(g.n):
        out[k * g.hop:k * g.hop + V] += (longform.window_weights(g, k) * _inv_mu_law64(x[k]))[g.late:g.T - g.late]
    return out


@pytest.mark.parametrize('T,n,F', [(4096, n, F) for n in (1, 2, 3) for F in (0, 1, 256)] + [(8192, 2, 256)])
def test_stitch_matches_numpy(T, n, F, dev):
    from audio_style_transfer_amd.engine import stitch
    g = longform.geometry(T, F, n)
    rng = np.random.default_rng(T + 10 * n + F)
    x = rng.uniform(-128, 127, (n, T)).astype(np.float32)
    x[rng.random((n, T)) < 0.05] = 0.0               # inv_mu_law_numpy's x == 0 branch
    x[rng.random((n, T)) < 0.05] = 0.5
    x[rng.random((n, T)) < 0.05] = -0.5              # o == 0
    x[:, g.late] = 0.0                               # ... also at the first sample of a fade-in
    x[:, T - g.late - 1] = -0.5                      # ... and the last of a fade-out
    out = stitch(torch.tensor(x, device=dev), g.late, F)
    assert out.shape == (g.n_out,) and out.dtype == torch.float32
    ref = _stitch64(x, g)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    print('T %d n %d F %d: max abs err %.3g' % (T, n, F, err))
    assert err <= 1e-6
    assert torch.equal(out, stitch(torch.tensor(x, device=dev), g.late, F))    # deterministic


@pytest.mark.parametrize('n,F', [(1, 256), (3, 0), (3, 1), (3, 256), (4, 2000)])
def test_one_signal_returns_itself(n, F, dev):
    from audio_style_transfer_amd.engine import stitch
    T = 4096
    g = longform.geometry(T, F, n)
    total = (n - 1) * g.hop + T
    codes = np.random.default_rng(n + F).integers(-128, 128, total).astype(np.float32)
    x = np.stack([codes[k * g.hop:k * g.hop + T] for k in range(n)])
    out = stitch(torch.tensor(x, device=dev), g.late, F).cpu().numpy()
    want = utils.inv_mu_law_numpy(codes)[g.late:g.late + g.n_out]
    err = float(np.abs(out.astype(np.float64) - want.astype(np.float64)).max())
    print('n %d F %d: max abs err %.3g' % (n, F, err))
    assert err <= 4 * 2.0 ** -23


@pytest.mark.parametrize('T,late,F', [(2048, 24, 0), (4096, 48, -1), (4096, 48, 2001), (8192, 96, 4001)])
def test_bad_geometry_is_refused(T, late, F, dev):
    from audio_style_transfer_amd.engine import stitch
    lib = _lib.load()
    x = torch.zeros(2, T, device=dev)
    out = torch.full((2 * T,), 7.0, device=dev)
    rc = lib.ast_stitch(ctypes.c_void_p(x.data_ptr()), 2, T, late, F, ctypes.c_void_p(out.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == -1                                   # AST_E_ARG
    assert bool((out == 7.0).all())                   # nothing was launched
    with pytest.raises(_lib.AstError):
        stitch(x, late, F)
