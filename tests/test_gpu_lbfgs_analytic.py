"""The device L-BFGS-B kernels (lbfgs.hip: ast_lbfgs_begin / _step / _state / _history) driven by
analytic objectives, against the fp64 restatement of tests/lbfgs_oracle.py -- which
test_lbfgs_oracle_cpu.py pins to scipy, branch by branch.  The real style loss
(test_gpu_lbfgs.py) ends almost every line search at the first or second trial; these objectives
reach every reachable branch of the state machine (all of lbfgs_oracle.COUNTERS but warn_xtol,
which dcsrch's own order of tests shadows, and the three stpmin branches: see the CPU test).

The kernels take grad_dev and parts_dev as arguments, so a test-local subclass of
engine.LbfgsLoop replaces the loss: its _eager copies x to the host, evaluates each clip's own
wrapped objective, writes grad and parts (column 0 = f, columns 1-3 recognisable per clip and
step) and calls ast_lbfgs_step.  The context is the smallest engine there is (one block); its
loss is never called.

Each group below is one loop (one workspace) of B = 4 clips, every clip another objective, so a
launch holds clips in different phases, clips that finished long before the others, and (where a
name is None) a clip inactive from begin.  T = 512 has fewer elements than the 1024 threads,
1536 is no multiple of them, 2048 is the tested length; m is 1, 2, 10 and 32 (LB_MMAX: full rho[]
and alpha[], and the ring wrapped many times at m 1 and 2); maxls 1, 2, 3 and 20; two groups run
a continuation epoch (begin(None)).  Per clip:
  * info (phase 0, iterations, evaluations, reason) equals the restatement's;
  * the fp32 x buffer after every step is within TRIAL_BAR of the restatement's, and the final
    fp64 point within FINAL_BAR -- the bars measured restatement-against-scipy in the CPU test
    (1e-6 and 1e-9 rel-L2), two fp64 implementations that differ in reduction order, as here;
    not re-tuned on the device;
  * ast_lbfgs_history returns exactly the rows fed, in order, and NaN past the clip's own count;
  * finished and inactive clips do not move, whatever is fed for them (NaN);
  * the clip is bit-identical (info, every fp32 buffer, the fp64 point) to the same objective
    run alone in a B = 1 context.

Measured on an MI355X: every count and reason equal; fp32 buffers identical in all clips but
three (stepf_shift at T 2048 3.6e-9, cos at T 1536 1.8e-13, liar_late at T 2048 3e-15); final fp64
point at most 1.9e-13 (rosen, T 2048, m 2), typically 1e-14.  Against the kernel as it was before
it took scipy's two counting rules, all seven groups fail on info: iterations one too many after
every abnormal end (liar, liar_late, rosen at maxls 2, flip, quart at maxls 3), evaluations one
too many where a trial repeats (quart, cos).
"""
import numpy as np
import pytest

import lbfgs_oracle as L
from test_lbfgs_oracle_cpu import FINAL_BAR, TRIAL_BAR, rel

pytestmark = pytest.mark.gpu

B = 4

# (id, T, loop options, the four clips' cases (None = inactive from begin), epochs)
GROUPS = [
    ('T512_m1', 512, dict(m=1, maxiter=30, maxls=20), ('quad_m1', 'quart', 'atmin', None), 2),
    ('T512_m32', 512, dict(m=32, maxiter=40, maxls=20), ('rosen_m5', 'well', 'lin', 'liar_late'), 1),
    ('T512_maxls2', 512, dict(m=10, maxiter=40, maxls=2), ('rosen_m5', 'liar', 'flip', 'stepf_shift'), 1),
    ('T1536_m2_gtol', 1536, dict(m=2, maxiter=40, maxls=20, gtol=-1.0),
     ('shelf', 'quad_m10', 'cos', 'kink'), 1),
    ('T1536_maxls1', 1536, dict(m=10, maxiter=30, maxls=1), ('liar', 'rosen_m5', 'atmin', 'abs'), 1),
    ('T2048_m10', 2048, dict(m=10, maxiter=60, maxls=20), ('stepf_shift', 'flip', None, 'liar_late'), 2),
    ('T2048_m2_maxls3', 2048, dict(m=2, maxiter=40, maxls=3), ('rosen_m5', 'quart', 'far', 'logc_shift'), 1),
]

_case_sets = {}


def case(T, name):
    if T not in _case_sets:
        _case_sets[T] = {c.name: c for c in L.cases(T)}
    return _case_sets[T][name]


def start_points(T, names):
    """x0 [B, T]; an inactive clip gets a recognisable point that is not float32-exact."""
    idle = 0.1 + np.arange(T) * 1e-3
    return np.stack([idle if n is None else case(T, n).x0 for n in names])


def expected(T, opts, names, epochs):
    """Per clip, the restatement's Result of every epoch (None for the inactive clip)."""
    out = []
    for n in names:
        out.append(None if n is None else L.minimize(case(T, n).fun, case(T, n).x0, epochs=epochs, **opts))
    return out


@pytest.fixture(scope='module')
def dev():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def engines(weights, dev):
    """The smallest context per (batch, T): one block, one tap; made once."""
    from audio_style_transfer_amd.engine import StyleEngine
    made = {}

    def get(batch, T):
        if (batch, T) not in made:
            made[batch, T] = StyleEngine(batch, T, [0], [0], weights=weights, device=dev)
        return made[batch, T]

    yield get
    for e in made.values():
        e.close()


def make_loop(eng, funs, **opts):
    import torch
    from audio_style_transfer_amd import _lib
    from audio_style_transfer_amd.engine import LbfgsLoop

    class DrivenLoop(LbfgsLoop):
        """LbfgsLoop whose loss is each clip's own analytic objective, evaluated on the host."""

        def __init__(self, eng, funs, **kw):
            super().__init__(eng, **kw)
            self.funs = funs
            self.k = 0
            self.fed = None          # the parts rows of the last step, [B, 4] float32

        def _eager(self):
            eng = self.eng
            x = self.x.cpu().numpy()
            nb = eng.batch
            grad = np.full((nb, eng.T), np.nan, np.float32)
            parts = np.full((nb, 4), np.nan, np.float32)
            for b, fun in enumerate(self.funs):
                if fun is None:
                    continue              # inactive: the kernel must not read the NaNs
                f, g = fun(x[b].astype(np.float64))
                grad[b] = g
                parts[b] = (f, 1000.0 * b + self.k + 0.25, -(self.k + 1.0), b + 0.5)
            self.grad.copy_(torch.from_numpy(grad))
            self.parts.copy_(torch.from_numpy(parts))
            self.fed = parts
            self.k += 1
            _lib.check(eng.lib.ast_lbfgs_step(eng.h, self._p(self.ws), self._p(self.x),
                                              self._p(self.grad), self._p(self.parts),
                                              eng._stream()))

    return DrivenLoop(eng, funs, **opts)


def history(loop, cap):
    import torch
    from audio_style_transfer_amd import _lib
    out = torch.empty(loop.eng.batch, cap, 4, device=loop.eng.device)
    _lib.check(loop.eng.lib.ast_lbfgs_history(loop.eng.h, loop._p(loop.ws), loop._p(out), cap,
                                              loop.eng._stream()))
    return out.cpu().numpy()


def drive(loop, max_steps=400):
    """Step until every clip has finished.  Per clip: the fp32 buffer after each of its steps and
    the rows fed to it; checks on the way that a clip that is not running does not move."""
    nb = loop.eng.batch
    after = [[] for _ in range(nb)]
    rows = [[] for _ in range(nb)]
    info, x64 = loop.state(with_x=True)
    info, x64, xbuf = info.copy(), x64.cpu().numpy(), loop.x.cpu().numpy()
    for _ in range(max_steps):
        run = info[:, 0] != 0
        if not run.any():
            return after, rows, info, x64
        loop.step()
        info2, x642 = loop.state(with_x=True)
        info2, x642, xbuf2 = info2.copy(), x642.cpu().numpy(), loop.x.cpu().numpy()
        for b in range(nb):
            if run[b]:
                after[b].append(xbuf2[b].copy())
                rows[b].append(loop.fed[b].copy())
            else:
                assert (info2[b] == info[b]).all(), (b, info[b], info2[b])
                assert np.array_equal(x642[b], x64[b]) and np.array_equal(xbuf2[b], xbuf[b]), b
        info, x64, xbuf = info2, x642, xbuf2
    raise AssertionError('not finished after %d steps: %s' % (max_steps, info))


def run_group(eng, T, opts, names, epochs, x0):
    """Every epoch's (after, rows, info, x64, history) of one loop over `names`."""
    import torch
    nb = len(names)
    funs = [None if n is None else case(T, n).fun for n in names]
    loop = make_loop(eng, funs, **opts)
    active = torch.tensor([0 if n is None else 1 for n in names])
    out = []
    for ep in range(epochs):
        loop.begin(torch.tensor(x0) if ep == 0 else None, active)
        after, rows, info, x64 = drive(loop)
        cap = max(1, int(info[:, 2].max())) + 3
        out.append((after, rows, info, x64, history(loop, cap)))
    assert nb == eng.batch
    return out


@pytest.mark.parametrize('gid,T,opts,names,epochs', GROUPS, ids=[g[0] for g in GROUPS])
def test_device_lbfgs_on_analytic_objectives(gid, T, opts, names, epochs, engines, dev):
    x0 = start_points(T, names)
    want = expected(T, opts, names, epochs)
    got = run_group(engines(B, T), T, opts, names, epochs, x0)
    alone = [None if n is None else
             run_group(engines(1, T), T, opts, (n,), epochs, x0[b:b + 1]) for b, n in enumerate(names)]
    for ep in range(epochs):
        after, rows, info, x64, hist = got[ep]
        for b, n in enumerate(names):
            if n is None:                    # inactive from begin: nothing counted, nothing moved
                assert info[b].tolist() == [0, 0, 0, L.RUNNING]
                assert np.array_equal(x64[b], x0[b]) and not after[b]
                assert np.isnan(hist[b]).all()
                continue
            r = want[b][ep]
            et = max([rel(a, w) for a, w in zip(after[b], r.after)] or [0.0])
            ex = rel(x64[b], r.x)
            print('%s epoch %d clip %d %-10s device it %d fev %d reason %d | restatement it %d fev %d '
                  'reason %d | buffers %.3g final %.3g'
                  % (gid, ep, b, n, info[b, 1], info[b, 2], info[b, 3], r.nit, r.nfev, r.reason,
                     et, ex))
            assert info[b].tolist() == [0, r.nit, r.nfev, r.reason]
            assert len(after[b]) == r.nfev
            assert et <= TRIAL_BAR
            assert ex <= FINAL_BAR
            # the history: exactly the rows fed, in order, NaN past this clip's count
            fed = np.array(rows[b], np.float32).reshape(-1, 4)
            assert np.array_equal(hist[b, :r.nfev], fed)
            assert np.isnan(hist[b, r.nfev:]).all() and hist.shape[1] > r.nfev
            # alone in a B = 1 context: bit-identical
            a_after, _, a_info, a_x64, _ = alone[b][ep]
            assert (a_info[0] == info[b]).all()
            assert np.array_equal(a_x64[0], x64[b])
            assert len(a_after[0]) == len(after[b])
            assert all(np.array_equal(p, q) for p, q in zip(a_after[0], after[b]))
