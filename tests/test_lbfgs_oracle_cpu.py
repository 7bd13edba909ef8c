"""The fp64 restatement of the device L-BFGS-B (tests/lbfgs_oracle.py) pinned to
scipy.optimize.minimize(method='L-BFGS-B') on analytic objectives.  CPU only.

Every case of lbfgs_oracle.cases() runs two epochs (the second from float32 of the first's end
point) through both, on the same wrapped function.  Asserted per case and epoch:
  * equal nit, nfev and stop reason -- with no correction: the restatement holds scipy's two
    rules itself (nit counts accepted points only; a trial bit-identical to the previous one is
    served from the cache and not counted);
  * every fp32 trial point within TRIAL_BAR, the final fp64 point within FINAL_BAR (rel-L2).

The bars.  Restatement and scipy are two fp64 implementations that differ in reduction order
(np.dot and the two-loop recursion against L-BFGS-B's compact form) -- the situation of the device
kernel against the restatement, so test_gpu_lbfgs_analytic.py uses the same two bars.  maxiter is
kept small enough per case that the two agree to 1e-9: quad is cut to 30 iterations (at 40, m = 3
drifts to 1.3e-9 in the second epoch; at 100 to 1e-5), rosen and far to 40 (at 150 rosen's counts
part), the others to 60.  Two objectives have their minimiser at 0, where rel-L2 of x is the
ratio of two roundings once a run gets there (logc 6e-8 at 40 iterations, stepf 4e-9 at 2): logc
stops at 12 iterations and stepf at 1 per epoch.  logc_shift (minimiser at 1) and stepf_shift run
the full length; stepf_shift has unit steps under a bowl centred elsewhere, which the search has
to climb (83 evaluations in the first epoch, a restart, repeated trials); with quarter steps
restatement and scipy part ways after 17 trials, one fp32 ulp flipping a floor().
Measured final-point rel-L2, epoch 1 / epoch 2 (scipy 1.15.3):

    quad_m1 3e-15 / 1e-14    quad_m3 4e-13 / 3e-14    quad_m10 1e-14 / 6e-14   quad_m32 5e-15 / 8e-15
    quad_T1536 4e-15 / 6e-15 rosen_m5 3e-12 / 8e-14   rosen_m2 2e-12 / 2e-12   logc 8e-15 / 2e-14
    abs 7e-12 / 1e-11        quart 7e-16 / 0          cos 3e-16 / 0            well 4e-14 / 0
    lin 0 / 0                kink 3e-13 / 4e-13       far 7e-15 / 5e-14        atmin 0 / 0
    liar 0 / 0               liar_late 2e-15 / 0      flip 0 / 0               stepf 0 / 0
    logc_shift 3e-15 / 0     stepf_shift 5e-16 / 0
    liar_maxls1,2,3 0 / 0    rosen_maxls1 0 / 0       rosen_maxls2 3e-13 / 0   rosen_maxls3 3e-12 / 8e-14
    mild_gtol 3e-14 / 0      mild_ftol 6e-14 / 3e-17  shelf 0 / 0

The largest is 1.0e-11 (abs), so FINAL_BAR = 100 x that = 1e-9 (below the 1e-6 cap, the bar
test_gpu_lbfgs.py uses).  Trial points are compared in fp32, where a difference of 1e-12 in fp64
can flip the rounding of an element by one ulp: measured largest 1.1e-7 (well, whose elements are
all equal and flip together), next abs 3.5e-10; 100 x 1.1e-7 is above the cap, so TRIAL_BAR = 1e-6.

Coverage.  Summed over the set every counter of lbfgs_oracle.COUNTERS is non-zero except
warn_xtol, and so is `repeat` (the cached-trial rule: quart, lin, flip, stepf_shift).
  * not_descent IS reached (case shelf): with a positive-definite memory -g'Hg < 0 whatever g is,
    so a lying gradient cannot do it; a gradient that is exactly zero at an accepted point does,
    once gtol < 0 keeps the run from stopping there.  Both attempts (memory, then empty) then end
    abnormally, as in scipy.
  * warn_xtol is unreached, and cannot be reached: dcsrch tests `brackt and stp outside
    (stmin, stmax)` (warn_round) before the xtol width test, and whenever the width test would
    hold at entry, the same test at the end of the previous call has already set stp = stx, an end
    of the bracket -- so warn_round fires first.  The first call after a start has brackt = 0.
  * the three stpmin branches are not in the required set.  With stpmin = 0: unbracketed, every
    trial lies beyond stx (stmin = stp + 1.1 (stp - stx)), so dcstep's case 4 never takes its
    `stp <= stx` arm; the stpmin warning needs stp == 0, which only `stp = stx` with stx = 0 in a
    bracket gives, and there warn_round fires first.  Case 3's stpmin arm needs a bracketed trial
    below stx whose cubic has no minimiser beyond it; nothing excludes that, but no case does it.
    The restatement counts the three as extras; all are 0 over the set.
"""
import collections

import numpy as np
import pytest

import lbfgs_oracle as L

FINAL_BAR = 1e-9
TRIAL_BAR = 1e-6
EPOCHS = 2

CASES = L.cases()


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def scipy_reason(res):
    msg = str(res.message).upper()
    if 'ITERATIONS' in msg:
        return L.STOP_ITER
    if 'PROJ' in msg or 'PGTOL' in msg:
        return L.CONV_PGTOL
    if 'REL_REDUCTION' in msg or 'FACTR' in msg:
        return L.CONV_REL_F
    return L.ABNORMAL


def scipy_run(case, x0):
    from scipy.optimize import minimize
    pts = []

    def fg(v):
        pts.append(v.astype(np.float32))
        return case.fun(v)

    o = case.opts
    res = minimize(fg, x0, jac=True, method='L-BFGS-B',
                   options=dict(maxcor=o['m'], maxiter=o['maxiter'], maxls=o['maxls'],
                                ftol=o['ftol'], gtol=o['gtol']))
    return res, pts


_cache = {}


def both(case):
    """(restatement Results, [(scipy result, scipy trial points)], counters), computed once."""
    if case.name not in _cache:
        cnt = collections.Counter()
        ours = L.minimize(case.fun, case.x0, count=cnt, epochs=EPOCHS, **case.opts)
        theirs, x0 = [], case.x0
        for r in ours:
            theirs.append(scipy_run(case, x0))
            x0 = r.x.astype(np.float32).astype(np.float64)    # the next epoch's start
        _cache[case.name] = ours, theirs, cnt
    return _cache[case.name]


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_restatement_matches_scipy(case):
    ours, theirs, cnt = both(case)
    for ep, (r, (res, pts)) in enumerate(zip(ours, theirs)):
        ex = rel(r.x, res.x)
        et = max([rel(a, b) for a, b in zip(r.trials, pts)] or [0.0])
        print('%s epoch %d: nit %d / %d, nfev %d / %d, reason %d / %d (%s), final %.3g, trials %.3g'
              % (case.name, ep, r.nit, res.nit, r.nfev, res.nfev, r.reason, scipy_reason(res),
                 res.message, ex, et))
        assert r.nit == res.nit
        assert r.nfev == res.nfev == len(pts) == len(r.trials) == len(r.rows)
        assert r.reason == scipy_reason(res)
        assert et <= TRIAL_BAR
        assert ex <= FINAL_BAR
        # the buffer after the last step is the end point (an abnormal end restores the base)
        assert np.array_equal(r.after[-1], r.x.astype(np.float32))
    print('   ', dict(cnt))


def test_every_branch_is_reached():
    tot = collections.Counter()
    for case in CASES:
        tot.update(both(case)[2])
    print({k: tot[k] for k in L.COUNTERS + L.EXTRA})
    unreached = [k for k in L.COUNTERS if tot[k] == 0]
    assert unreached == ['warn_xtol']
    assert tot['repeat'] > 0
    assert set(tot) <= set(L.COUNTERS + L.EXTRA)


def test_begin_inactive_and_step_when_idle_do_not_move():
    """The restatement's own inactive clip: begin(active=False) evaluates nothing, and a step on
    a finished machine changes nothing (the kernel returns at phase 0)."""
    case = CASES[0]
    m = L.Machine(case.T, **case.opts)
    r = L.run_epoch(m, case.fun, case.x0)
    x, info = m.x.copy(), (m.iter, m.nfev, m.reason)
    m.step(1.0, np.ones(case.T))
    assert np.array_equal(m.x, x) and (m.iter, m.nfev, m.reason) == info
    m.begin(None, active=False)
    assert m.phase == 0 and m.nfev == 0 and np.array_equal(m.x, r.x)
