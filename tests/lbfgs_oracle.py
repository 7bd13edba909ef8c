"""A plain fp64 restatement of the device L-BFGS-B (csrc/lbfgs.hip), with branch counters, and the
analytic objectives it is driven with.  numpy only.

The restatement follows the kernel's own structure line by line -- dcstep, dcsrch start and
continuation, the direction (two-loop recursion, z = x + dsub, d = z - x), lnsrlb's first step and
maxls handling, the NEW_X tests and the pair update -- with np.dot where the kernel reduces over
the block.  `Machine` has the kernel's interface: begin(x0) hands out the first fp32 point,
step(f, g, row) consumes one evaluation and hands out the next.  Every named branch bumps
`Machine.count`, so a case set can be shown to reach it (test_lbfgs_oracle_cpu.py).

Two rules are scipy.optimize.minimize's and not the Fortran's:
  * iterations count accepted points only (scipy's nit), so an abnormal end adds none;
  * a trial point that is bit-identical (the whole fp64 array) to the previous one is not handed
    out again: scipy's ScalarFunction serves it from its cache, so the search is re-entered at
    once with the same f and g; ifun advances (the maxls test still applies), the evaluation
    count and the history do not.

Every objective goes through `wrap`, which makes all sides evaluate the identical function:
x rounded to fp32 and widened, f and g computed in fp64, f rounded to fp32, g rounded to fp32
and widened -- what the device loss hands the kernel, and what ScipyOptimizerInterface hands scipy.
"""
import collections

import numpy as np

EPSMCH = 2.220446049250313e-16
STPMX = 1e10
LS_FTOL, LS_GTOL, LS_XTOL = 1e-3, 0.9, 0.1
FTOL = 2.220446049250313e-09      # scipy minimize(method='L-BFGS-B') defaults
GTOL = 1e-5

RUNNING, STOP_ITER, CONV_PGTOL, CONV_REL_F, ABNORMAL = 0, 1, 2, 3, 4

# every branch the restatement names (the issue's list; `repeat` is the cached-trial rule)
COUNTERS = ('step1', 'step2', 'step3_unbracketed', 'step3_bracketed', 'step3_to_stpmax',
            'step4_bracketed', 'step4_to_stpmax', 'modified', 'stage2', 'bisect', 'stp_to_stx',
            'warn_round', 'warn_xtol', 'warn_stpmax', 'conv', 'maxls', 'restart',
            'abnormal_empty', 'not_descent', 'pg_at_start', 'skip_update', 'ring_full',
            'stp_ne_1', 'reason1', 'reason2', 'reason3', 'reason4')
# not in that list: the cached-trial rule, and the three branches that need stpmin > 0
EXTRA = ('repeat', 'warn_stpmin', 'step3_to_stpmin', 'step4_to_stpmin')

_f64 = np.float64
_fmax, _fmin = np.fmax, np.fmin      # C fmax / fmin: a NaN operand is ignored


def _sqrt(v):
    return np.sqrt(_f64(v))


class Machine:
    """One clip of k_lbfgs_begin / k_lbfgs_step."""

    def __init__(self, T, m=10, maxiter=100, maxls=20, ftol=FTOL, gtol=GTOL, count=None):
        self.T, self.m, self.maxiter, self.maxls = T, int(m), int(maxiter), int(maxls)
        self.tol, self.pgtol = _f64(ftol), _f64(gtol)
        self.count = collections.Counter() if count is None else count
        self.X = [np.zeros(T), np.zeros(T)]
        self.R = np.zeros(T)
        self.D = np.zeros(T)
        self.S = np.zeros((self.m, T))
        self.Y = np.zeros((self.m, T))
        self.rho = np.zeros(self.m)
        self.xi = 0
        self.phase = 0
        self.x32 = np.zeros(T, np.float32)

    # ---- k_lbfgs_begin
    def begin(self, x0=None, active=True):
        if x0 is not None:
            self.xi = 0
            self.X[0] = np.array(x0, np.float64)
        elif active:
            self.X[self.xi] = self.X[self.xi].astype(np.float32).astype(np.float64)
        self.col, self.head, self.theta = 0, 0, _f64(1.0)
        self.iter, self.nfev, self.ifun = 0, 0, 0
        self.reason = RUNNING
        self.phase = 1 if active else 0
        self.rows = []
        self.x32 = self.X[self.xi].astype(np.float32)

    @property
    def x(self):
        return self.X[self.xi]

    def _c(self, name):
        self.count[name] += 1

    def _finish(self, reason):
        self.phase = 0
        self.reason = reason
        self._c('reason%d' % reason)

    # ---- MINPACK-2 dcstep; stx fx dx sty fy dy stp are passed and returned
    def _dcstep(self, stx, fx, dx, sty, fy, dy, stp, fp, dp, brackt, stpmin, stpmax):
        sgnd = dp * (dx / abs(dx))
        if fp > fx:
            self._c('step1')
            theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
            s = _fmax(_fmax(abs(theta), abs(dx)), abs(dp))
            gamma = s * _sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s))
            if stp < stx:
                gamma = -gamma
            p = (gamma - dx) + theta
            q = ((gamma - dx) + gamma) + dp
            r = p / q
            stpc = stx + r * (stp - stx)
            stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / 2.0) * (stp - stx)
            if abs(stpc - stx) < abs(stpq - stx):
                stpf = stpc
            else:
                stpf = stpc + (stpq - stpc) / 2.0
            brackt = 1
        elif sgnd < 0.0:
            self._c('step2')
            theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
            s = _fmax(_fmax(abs(theta), abs(dx)), abs(dp))
            gamma = s * _sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s))
            if stp > stx:
                gamma = -gamma
            p = (gamma - dp) + theta
            q = ((gamma - dp) + gamma) + dx
            r = p / q
            stpc = stp + r * (stx - stp)
            stpq = stp + (dp / (dp - dx)) * (stx - stp)
            stpf = stpc if abs(stpc - stp) > abs(stpq - stp) else stpq
            brackt = 1
        elif abs(dp) < abs(dx):
            self._c('step3_bracketed' if brackt else 'step3_unbracketed')
            theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
            s = _fmax(_fmax(abs(theta), abs(dx)), abs(dp))
            gamma = s * _sqrt(_fmax(0.0, (theta / s) * (theta / s) - (dx / s) * (dp / s)))
            if stp > stx:
                gamma = -gamma
            p = (gamma - dp) + theta
            q = (gamma + (dx - dp)) + gamma
            r = p / q
            if r < 0.0 and gamma != 0.0:
                stpc = stp + r * (stx - stp)
            elif stp > stx:
                self._c('step3_to_stpmax')
                stpc = stpmax
            else:
                self._c('step3_to_stpmin')
                stpc = stpmin
            stpq = stp + (dp / (dp - dx)) * (stx - stp)
            if brackt:
                stpf = stpc if abs(stpc - stp) < abs(stpq - stp) else stpq
                if stp > stx:
                    stpf = _fmin(stp + 0.66 * (sty - stp), stpf)
                else:
                    stpf = _fmax(stp + 0.66 * (sty - stp), stpf)
            else:
                stpf = stpc if abs(stpc - stp) > abs(stpq - stp) else stpq
                stpf = _fmin(stpmax, stpf)
                stpf = _fmax(stpmin, stpf)
        else:
            if brackt:
                self._c('step4_bracketed')
                theta = 3.0 * (fp - fy) / (sty - stp) + dy + dp
                s = _fmax(_fmax(abs(theta), abs(dy)), abs(dp))
                gamma = s * _sqrt((theta / s) * (theta / s) - (dy / s) * (dp / s))
                if stp > sty:
                    gamma = -gamma
                p = (gamma - dp) + theta
                q = ((gamma - dp) + gamma) + dy
                r = p / q
                stpf = stp + r * (sty - stp)
            elif stp > stx:
                self._c('step4_to_stpmax')
                stpf = stpmax
            else:
                self._c('step4_to_stpmin')
                stpf = stpmin
        if fp > fx:
            sty, fy, dy = stp, fp, dp
        else:
            if sgnd < 0.0:
                sty, fy, dy = stx, fx, dx
            stx, fx, dx = stp, fp, dp
        return stx, fx, dx, sty, fy, dy, stpf, brackt

    # ---- dcsrch START
    def _dcsrch_start(self, f, g, stp):
        self.brackt = 0
        self.stage = 1
        self.finit, self.ginit = f, g
        self.gtest = LS_FTOL * g
        self.width = _f64(STPMX - 0.0)
        self.width1 = self.width / 0.5
        self.stx, self.fx, self.gx = _f64(0.0), f, g
        self.sty, self.fy, self.gy = _f64(0.0), f, g
        self.stmin = _f64(0.0)
        self.stmax = stp + 4.0 * stp
        self.stp = stp

    # ---- dcsrch continuation: 1 = FG (new self.stp), 0 = CONV / WARN (accept self.stp)
    def _dcsrch_iter(self, f, g):
        stpmin, stpmax = _f64(0.0), _f64(STPMX)
        stp = self.stp
        ftest = self.finit + stp * self.gtest
        if self.stage == 1 and f <= ftest and g >= 0.0:
            self.stage = 2
            self._c('stage2')
        if self.brackt and (stp <= self.stmin or stp >= self.stmax):
            self._c('warn_round')
            return 0
        if self.brackt and self.stmax - self.stmin <= LS_XTOL * self.stmax:
            self._c('warn_xtol')
            return 0
        if stp == stpmax and f <= ftest and g <= self.gtest:
            self._c('warn_stpmax')
            return 0
        if stp == stpmin and (f > ftest or g >= self.gtest):
            self._c('warn_stpmin')
            return 0
        if f <= ftest and abs(g) <= LS_GTOL * (-self.ginit):
            self._c('conv')
            return 0
        if self.stage == 1 and f <= self.fx and f > ftest:
            self._c('modified')
            fm = f - stp * self.gtest
            fxm = self.fx - self.stx * self.gtest
            fym = self.fy - self.sty * self.gtest
            gm = g - self.gtest
            gxm = self.gx - self.gtest
            gym = self.gy - self.gtest
            (self.stx, fxm, gxm, self.sty, fym, gym, stp, self.brackt) = self._dcstep(
                self.stx, fxm, gxm, self.sty, fym, gym, stp, fm, gm, self.brackt, self.stmin,
                self.stmax)
            self.fx = fxm + self.stx * self.gtest
            self.fy = fym + self.sty * self.gtest
            self.gx = gxm + self.gtest
            self.gy = gym + self.gtest
        else:
            (self.stx, self.fx, self.gx, self.sty, self.fy, self.gy, stp, self.brackt) = \
                self._dcstep(self.stx, self.fx, self.gx, self.sty, self.fy, self.gy, stp, f, g,
                             self.brackt, self.stmin, self.stmax)
        if self.brackt:
            if abs(self.sty - self.stx) >= 0.66 * self.width1:
                self._c('bisect')
                stp = self.stx + 0.5 * (self.sty - self.stx)
            self.width1 = self.width
            self.width = abs(self.sty - self.stx)
        if self.brackt:
            self.stmin = _fmin(self.stx, self.sty)
            self.stmax = _fmax(self.stx, self.sty)
        else:
            self.stmin = stp + 1.1 * (stp - self.stx)
            self.stmax = stp + 4.0 * (stp - self.stx)
        stp = _fmax(stp, stpmin)
        stp = _fmin(stp, stpmax)
        if (self.brackt and (stp <= self.stmin or stp >= self.stmax)) or \
                (self.brackt and self.stmax - self.stmin <= LS_XTOL * self.stmax):
            self._c('stp_to_stx')
            stp = self.stx
        self.stp = stp
        return 1

    # ---- new_direction: 0, or 1 = not a descent direction even with an empty memory
    def _new_direction(self):
        m = self.m
        for _ in range(2):
            t = self.X[self.xi]
            q = self.R.copy()
            if self.col > 0:
                alpha = []
                for k in range(self.col):                      # newest -> oldest
                    j = (self.head - 1 - k + 2 * m) % m
                    a = self.rho[j] * np.dot(self.S[j], q)
                    alpha.append(a)
                    q -= a * self.Y[j]
                q *= 1.0 / self.theta
                for k in range(self.col - 1, -1, -1):          # oldest -> newest
                    j = (self.head - 1 - k + 2 * m) % m
                    beta = self.rho[j] * np.dot(self.Y[j], q)
                    q += (alpha[k] - beta) * self.S[j]
            z = t + (-q)
            d = z - t
            self.D = d
            dd = np.dot(d, d)
            gd = np.dot(self.R, d)
            self.dnorm = _sqrt(dd)
            if gd >= 0.0:                                      # lnsrlb info = -4
                self._c('not_descent')
                if self.col == 0:
                    return 1
                self.col, self.head, self.theta = 0, 0, _f64(1.0)
                continue
            stp = _fmin(1.0 / self.dnorm, STPMX) if self.iter == 0 else _f64(1.0)
            self.gdold = gd
            self._dcsrch_start(self.fold, gd, stp)
            self.ifun = 1
            trial = z.copy() if stp == 1.0 else stp * d + t
            self.X[1 - self.xi] = trial
            self.x32 = trial.astype(np.float32)
            self.phase = 2
            return 0
        return 1

    # ---- k_lbfgs_step: one evaluation (f fp32 value, g fp32 values, row = the four loss parts)
    def step(self, f, g, row=None):
        if self.phase == 0:
            return
        with np.errstate(all='ignore'):
            self._step(_f64(f), np.asarray(g, np.float64), row)

    def _step(self, f, g, row):
        self.rows.append((float(f), 0.0, 0.0, 0.0) if row is None else tuple(row))
        self.nfev += 1
        if self.phase == 1:                                    # f, g at the start point
            self.R = g.copy()
            gmax = np.max(np.abs(g)) if g.size else 0.0
            self.fold = f
            self.col, self.head, self.theta, self.iter = 0, 0, _f64(1.0), 0
            if gmax <= self.pgtol:
                self._c('pg_at_start')
                self._finish(CONV_PGTOL)
            elif self._new_direction():
                self._finish(ABNORMAL)
            return
        gd = np.dot(g, self.D)                                 # line-search evaluation
        while True:
            if not self._dcsrch_iter(f, gd):
                self._new_x(f, g, gd)
                return
            self.ifun += 1                                     # FG: another trial
            if self.ifun - 1 >= self.maxls:                    # iback >= maxls: give up
                self._c('maxls')
                self.x32 = self.X[self.xi].astype(np.float32)  # restore the base point
                if self.col == 0:
                    self._c('abnormal_empty')
                    self._finish(ABNORMAL)
                else:
                    self._c('restart')
                    self.col, self.head, self.theta = 0, 0, _f64(1.0)
                    if self._new_direction():
                        self._finish(ABNORMAL)
                return
            t = self.X[self.xi]
            v = self.stp * self.D + t          # at stp == 1 this is z again, bit for bit
            same = np.array_equal(v, self.X[1 - self.xi])
            self.X[1 - self.xi] = v
            self.x32 = v.astype(np.float32)
            if not same:
                return
            self._c('repeat')          # scipy serves this point from its cache: same f, same g

    def _new_x(self, f, g, gd):
        self.iter += 1
        stp = self.stp
        if stp != 1.0:
            self._c('stp_ne_1')
        y = g - self.R
        gmax = np.max(np.abs(g))
        rr = np.dot(y, y)
        fold = self.fold
        self.xi ^= 1                                           # the trial is the new base
        if self.iter >= self.maxiter:
            self._finish(STOP_ITER)
        elif gmax <= self.pgtol:
            self._finish(CONV_PGTOL)
        elif fold - f <= self.tol * _fmax(_fmax(abs(fold), abs(f)), 1.0):
            self._finish(CONV_REL_F)
        else:
            if stp == 1.0:
                dr, ddum = gd - self.gdold, -self.gdold
            else:
                dr, ddum = (gd - self.gdold) * stp, -self.gdold * stp
            if dr > EPSMCH * ddum:
                slot = self.head
                if self.col == self.m:
                    self._c('ring_full')
                self.S[slot] = self.D if stp == 1.0 else stp * self.D
                self.Y[slot] = y
                self.rho[slot] = 1.0 / dr
                self.theta = rr / dr
                self.head = (self.head + 1) % self.m
                if self.col < self.m:
                    self.col += 1
            else:
                self._c('skip_update')
            self.R = g.copy()
            self.fold = f
            if self._new_direction():
                self._finish(ABNORMAL)


class Result:
    pass


def run_epoch(mach, fun, x0=None):
    """One minimize call on `mach` (from x0, or a continuation from its own point): every trial
    point in evaluation order (fp32), the fp32 buffer after every step, and the loss rows."""
    mach.begin(x0)
    trials, after = [], []
    while mach.phase:
        trials.append(mach.x32.copy())
        f, g = fun(mach.x32.astype(np.float64))
        mach.step(f, g)
        after.append(mach.x32.copy())
    r = Result()
    r.x = mach.x.copy()
    r.nit, r.nfev, r.reason = mach.iter, mach.nfev, mach.reason
    r.trials, r.after, r.rows = trials, after, list(mach.rows)
    return r


def minimize(fun, x0, m=10, maxiter=100, maxls=20, ftol=FTOL, gtol=GTOL, count=None, epochs=1):
    """`epochs` minimize calls in a row, each continuing from float32 of the last point (as the
    reference's epochs do); a list of Results, one per epoch."""
    mach = Machine(len(x0), m, maxiter, maxls, ftol, gtol, count)
    return [run_epoch(mach, fun, x0 if e == 0 else None) for e in range(epochs)]


# ---------------------------------------------------------------------------------------------
# objectives

def wrap(fun):
    def w(x64):
        x = np.asarray(x64, np.float64).astype(np.float32).astype(np.float64)
        with np.errstate(all='ignore'):
            f, g = fun(x)
            return (float(np.float32(f)),
                    np.asarray(g, np.float64).astype(np.float32).astype(np.float64))
    return w


def _quad(a):
    return lambda x: (0.5 * np.sum(a * x * x), a * x)


def _rosen(x):
    a, b = x[:-1], x[1:]
    f = np.sum(100.0 * (b - a * a) ** 2 + (1.0 - a) ** 2)
    g = np.zeros_like(x)
    g[:-1] += -400.0 * a * (b - a * a) - 2.0 * (1.0 - a)
    g[1:] += 200.0 * (b - a * a)
    return f, g


def _logc(x):
    return np.sum(np.log1p(x * x)), 2.0 * x / (1.0 + x * x)


def _logc_shift(x):
    """logc with its minimiser at 1: a run may converge and the relative error of x still
    means something (at a minimiser of 0 it is the ratio of two roundings)."""
    return _logc(x - 1.0)


def _abs(x):
    return np.sum(np.abs(x)) + 0.5 * np.sum(x * x), np.sign(x) + x


def _quart(x):
    return np.sum(x ** 4) - np.sum(x * x) + 0.1 * np.sum(x), 4.0 * x ** 3 - 2.0 * x + 0.1


def _cos(x):
    return np.sum(1.0 - np.cos(3.0 * x)) + 0.05 * np.sum(x * x), 3.0 * np.sin(3.0 * x) + 0.1 * x


def _well(x):
    e = np.exp(-50.0 * (x - 0.3) ** 2)
    return -np.sum(e) + 1e-3 * np.sum(x * x), 100.0 * (x - 0.3) * e + 2e-3 * x


def _lin(c):
    return lambda x: (np.dot(c, x), c.copy())


def _kink(x):
    return (np.sum(5.0 * np.maximum(x, 0.0) + 0.1 * np.maximum(-x, 0.0)),
            np.where(x > 0.0, 5.0, np.where(x < 0.0, -0.1, 0.0)))


def _liar(x):
    return np.sum(x * x), -2.0 * x


def _liar_late(a):
    def fun(x):
        f, g = 0.5 * np.sum(a * x * x), a * x
        return f, (-g if f < 1e3 else g)
    return fun


def _flip(a):
    def fun(x):
        f, g = 0.5 * np.sum(a * x * x), a * x
        return f, (-0.3 * g if int(7.0 * abs(f)) % 3 == 0 else g)
    return fun


def _stepf(x):
    return np.sum(np.floor(4.0 * np.abs(x)) / 4.0) + 0.01 * np.sum(x * x), 0.02 * x


def _stepf_shift(c):
    """Unit steps the gradient knows nothing of, under a bowl centred at c: moving towards c
    climbs the steps, so f and g disagree in most searches (in _stepf the bowl and the steps
    agree, and the second iteration lands on the minimiser 0)."""
    def fun(x):
        return (0.25 * np.sum(np.floor(np.abs(x))) + 0.01 * np.sum((x - c) ** 2),
                0.02 * (x - c))
    return fun


def _shelf(x):
    """Linear down to zero, then flat with a zero gradient: with gtol < 0 the run goes on from a
    base point whose gradient is exactly 0, where no direction is a descent direction."""
    return np.sum(np.maximum(x, 0.0)), (x > 0.0).astype(np.float64)


class Case:
    def __init__(self, name, fun, x0, m=10, maxiter=40, maxls=20, ftol=FTOL, gtol=GTOL):
        self.name, self.raw, self.fun = name, fun, wrap(fun)
        self.x0 = np.asarray(x0, np.float64)
        self.T = self.x0.size
        self.opts = dict(m=m, maxiter=maxiter, maxls=maxls, ftol=ftol, gtol=gtol)

    def __repr__(self):
        return self.name


def _normal(seed, T, scale=1.0):
    return np.random.default_rng(seed).normal(0.0, scale, T)


CASES_T = 512


def cases(T=CASES_T):
    """The case set.  maxiter is cut where a longer run would let restatement and scipy drift
    apart by reduction order alone, or would converge to a minimiser of 0, where a relative error
    of x means nothing (quad, rosen, far, logc, stepf: see test_lbfgs_oracle_cpu.py)."""
    a = np.logspace(0, 4, T)
    a3 = np.logspace(0, 4, 3 * T)
    mild = np.linspace(1.0, 100.0, T)
    rs = np.tile([-1.2, 1.0], T // 2 + 1)[:T]
    c = np.random.default_rng(5).normal(0.0, 1.0, T)
    out = []
    for m in (1, 3, 10, 32):
        out.append(Case('quad_m%d' % m, _quad(a), _normal(1, T), m=m, maxiter=30))
    out.append(Case('quad_T%d' % (3 * T), _quad(a3), _normal(2, 3 * T), maxiter=30))
    out.append(Case('rosen_m5', _rosen, rs, m=5))
    out.append(Case('rosen_m2', _rosen, rs, m=2))
    out.append(Case('logc', _logc, _normal(3, T, 3.0), maxiter=12))
    out.append(Case('logc_shift', _logc_shift, _normal(3, T, 3.0), maxiter=60))
    out.append(Case('abs', _abs, _normal(4, T), maxiter=60))
    out.append(Case('quart', _quart, _normal(6, T), maxiter=60))
    out.append(Case('cos', _cos, _normal(7, T, 2.0), maxiter=60))
    out.append(Case('well', _well, np.full(T, 1.5), maxiter=60))
    out.append(Case('lin', _lin(c), np.zeros(T), maxiter=60))
    out.append(Case('kink', _kink, _normal(8, T), maxiter=60))
    out.append(Case('far', _quad(a), _normal(9, T, 1e6)))
    out.append(Case('atmin', _quad(a), np.zeros(T)))
    out.append(Case('liar', _liar, _normal(10, T)))
    out.append(Case('liar_late', _liar_late(a), _normal(1, T), maxiter=60))
    out.append(Case('flip', _flip(a), _normal(11, T), maxiter=60))
    out.append(Case('stepf', _stepf, _normal(12, T, 20.0), maxiter=1))
    out.append(Case('stepf_shift', _stepf_shift(np.linspace(-2.0, 2.0, T)), np.zeros(T), maxiter=60))
    for ls in (1, 2, 3):
        out.append(Case('liar_maxls%d' % ls, _liar, _normal(10, T), maxls=ls))
        out.append(Case('rosen_maxls%d' % ls, _rosen, rs, m=5, maxls=ls))
    out.append(Case('mild_gtol', _quad(mild), _normal(13, T), gtol=0.5, maxiter=60))
    out.append(Case('mild_ftol', _quad(mild), _normal(13, T), ftol=1e-2, maxiter=60))
    out.append(Case('shelf', _shelf, np.full(T, 0.5), gtol=-1.0))
    return out
