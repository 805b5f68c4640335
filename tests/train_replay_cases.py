"""Gate of the gradients that gpmpc_train_multistart's restart search runs on, shared by the emulator tier
(tests/test_emu_train_replay.py) and the GPU tier (tests/test_gpu_train_replay.py).

Why: the lock-step batch code of api_train.inl (nll_batch, nll_batch_core, nll_grad_retained) has one caller, the training
search, and the search forgives a wrong gradient -- an accepted step always lowers the NLL, so the outcome tests only see a
search that is a little worse.  gpmpc_nll, which check_nll_gradient gates, takes another workspace, another alpha solve and
possibly another factorisation.

Method: `minimize_box_lbfgs` and `run_restart` below are line-by-line ports of minimize_box_lbfgs (gp_mpc_amd/csrc/
train_native.hpp) and of run_restart and the slot bookkeeping of nll_batch (gp_mpc_amd/csrc/api_train.inl): deterministic host
code that only sees (f, g).  A change there has to be made here as well; train_native.hpp says the same about this file.
The port is driven by the ORACLE (gp_oracle.nll_mean / nll_mean_grad / nll_prior and the analytic prior gradient), and its
table of (NLL, theta) per restart and its iteration / evaluation totals are compared with the device's.  theta after
iteration k >= 2 depends on the gradients of iterations 1 .. k-1, the first step is normalised to unit size, so a relative
gradient error eps moves theta by about eps: a bar of 1e-10 on theta gates the gradient 1e4 times more sharply than the 1e-6
of check_nll_gradient.

Inputs: synthetic_problem(sn = 0.05); box ell, sf in [1e-2, 1e2] (log variables), sn in [1e-4, 1] (linear, second-stage polish
when iterations are left), mean parameters in +-5; starts = generating row * (1 + 0.3 u), seeded u in [-1, 1], mean parameters
0.1.  (The production box -- sn in [1e-10, 1e-2] -- and Latin-hypercube starts clip most first steps at the sn bound and halve
them 7 to 20 times: the step is then no longer proportional to g.)
The jitter case: N_DUP training points are held twice, so K is exactly singular for every theta whose sn^2 is below
rounding, and the last restart starts at sn = 1e-18; that case alone lowers the sn bound to 1e-20 (no point with sn >= 1e-4
needs the jitter: lambda_min(K) >= 1e-8 there, five orders above the N eps sf^2 a Cholesky loses).  A start that is singular
only to rounding (long length scales) leaves the decision to rounding somewhere along its line search, and device and oracle
then part through no fault of either (docs/train_replay.md); here the replay asserts that no evaluated point has sn / sf
between 1e-9 and 1e-5.  Device (gpmpc_nll's jitter_out) and oracle (chol_jitter) must agree on which start takes the jitter.
The trials of the other restarts that clip at the sn bound take it too: value-only batches are repeated in many rounds.

Conditions on the inputs, asserted from the replay alone (CheckedReplay): every Armijo margin |f + 1e-4 dec - fn| >= 1e-6
(|f| + N); no variable of a gated restart on a bound, at any accepted point; where a subset is asked for, a round whose
grad_of_last requests come from a proper subset of the live restarts that does not start at restart 0 and whose slots are
not 0 .. m-1 (`zmap` is then no identity); the spread r between the replay and the same replay with the training points in
another order <= 1e-11.

Bars: theta (log where the search is in log space) and obj / (|f| + N) within max(10 r, 1e-10) -- 1e-10 is the project's
standing parity bar -- for restarts that never stood on a point that took the jitter (a rejected trial that took it only has
to be rejected: the Armijo margin); max(1e-10, 50 eps cond(K + 1e-8 I)) at the start point for one that did.  Iteration and
evaluation totals, retained gradients and jitter repeats: equal to the replay's.

Measured (device against replay; r: the permuted replay's spread), emulator tier | MI355X:
    see docs/train_replay.md -- the figures of every case are printed by the checks (-s) and collected there."""
import math

import numpy as np

import gp_oracle as go
from gp_mpc_amd._lib import Handle

EPS = float(np.finfo(np.float64).eps)
INF = float('inf')
TOL = 1e-8                    # gpmpc_train_multistart's default, passed explicitly
ARMIJO_MARGIN = 1e-6          # of |f| + N
SPREAD_MAX = 1e-11
PARITY_BAR = 1e-10
N_DUP = 20                    # training points that the jitter case holds twice

RECORD = []                   # (label, worst theta error, worst obj error, bar, r) of every comparison of this process


# ------------------------------------------------------------------------------------------------ the port
def minimize_box_lbfgs(n, lb, ub, logv, theta0, max_iter, tol, has_grad_last, rec):
    """minimize_box_lbfgs of train_native.hpp as a generator: yields ('fg' | 'f' | 'g', theta) -- value + gradient, value
    only, gradient of the point evaluated last -- and is sent (ok, f, grad).  Returns dict(theta, f, iters, evals, ok).
    rec collects margins, free sets, accepted steps and every point the search stood on."""
    M = 8
    R = dict(theta=[0.0] * n, f=INF, iters=0, evals=0, ok=False)
    lo, hi, x = [0.0] * n, [0.0] * n, [0.0] * n
    for k in range(n):
        lo[k] = math.log(lb[k]) if logv[k] else lb[k]
        hi[k] = math.log(ub[k]) if logv[k] else ub[k]
        t0 = theta0[k]
        if t0 < lb[k]:
            t0 = lb[k]
        if t0 > ub[k]:
            t0 = ub[k]
        x[k] = math.log(t0) if logv[k] else t0

    def theta_of(xx):
        return [math.exp(xx[k]) if logv[k] else xx[k] for k in range(n)]

    def chain(th, gt):
        gx = [gt[k] * th[k] if logv[k] else gt[k] for k in range(n)]       # d f / d log(theta) = theta d f / d theta
        return None if any(v != v for v in gx) else gx

    def fun(xx):
        th = theta_of(xx)
        R['evals'] += 1
        ok, f, gt = yield ('fg', th)
        if not ok or f != f:
            return INF, None
        gx = chain(th, gt)
        return (INF, None) if gx is None else (f, gx)

    def fun_value(xx):
        th = theta_of(xx)
        R['evals'] += 1
        ok, f, _ = yield ('f', th)
        return INF if (not ok or f != f) else f

    def grad_of_last(xx):
        th = theta_of(xx)
        ok, _, gt = yield ('g', th)
        return chain(th, gt) if ok else None

    f, g = yield from fun(x)
    if f == INF:
        R['theta'] = theta_of(x)
        return R                                                # unusable start: this restart has failed
    rec['points'].append((list(x), lo, hi))
    rec['stood'].append(theta_of(x))
    Sv, Yv, rho = [], [], []
    fr_prev = None
    for it in range(max_iter):
        R['iters'] = it + 1
        pgn = 0.0
        fr = [True] * n
        for k in range(n):
            at_lo = x[k] <= lo[k] and g[k] > 0.0
            at_hi = x[k] >= hi[k] and g[k] < 0.0
            fr[k] = not (at_lo or at_hi)
            if fr[k]:
                pgn = max(pgn, abs(g[k]))
        if pgn <= tol * max(1.0, abs(f)):
            break
        rec['free'].append(list(fr))
        if fr_prev is not None and fr_prev != fr:
            Sv, Yv, rho = [], [], []
        fr_prev = list(fr)
        q = [g[k] if fr[k] else 0.0 for k in range(n)]
        m = len(Sv)
        al = [0.0] * M
        for i in range(m - 1, -1, -1):
            a = 0.0
            for k in range(n):
                if fr[k]:
                    a += Sv[i][k] * q[k]
            a *= rho[i]
            al[i] = a
            for k in range(n):
                if fr[k]:
                    q[k] -= a * Yv[i][k]
        gamma = 1.0
        if m > 0:
            sy = yy = 0.0
            for k in range(n):
                sy += Sv[m - 1][k] * Yv[m - 1][k]
                yy += Yv[m - 1][k] * Yv[m - 1][k]
            if yy > 0.0:
                gamma = sy / yy
        for k in range(n):
            q[k] *= gamma
        for i in range(m):
            b = 0.0
            for k in range(n):
                if fr[k]:
                    b += Yv[i][k] * q[k]
            b *= rho[i]
            for k in range(n):
                if fr[k]:
                    q[k] += (al[i] - b) * Sv[i][k]
        slope = 0.0
        d_ = [0.0] * n
        for k in range(n):
            d_[k] = -q[k] if fr[k] else 0.0
            slope += d_[k] * g[k]
        if not (slope < 0.0):                                   # not a descent direction: steepest descent on the free set
            slope = 0.0
            for k in range(n):
                d_[k] = -g[k] if fr[k] else 0.0
                slope += d_[k] * g[k]
            Sv, Yv, rho = [], [], []
        t = 1.0
        if not Sv:
            dn = 0.0
            for k in range(n):
                dn = max(dn, abs(d_[k]))
            if dn > 0.0:
                t = min(1.0, 1.0 / dn)
        fn, gn = INF, None
        moved = False
        xn = [0.0] * n
        for ls in range(40):
            if ls:
                t *= 0.5
            dec = 0.0
            any_ = False
            for k in range(n):
                v = x[k] + t * d_[k]
                if v < lo[k]:
                    v = lo[k]
                if v > hi[k]:
                    v = hi[k]
                xn[k] = v
                dec += g[k] * (v - x[k])
                any_ |= v != x[k]
            if not any_:
                break
            if not (dec < 0.0):
                continue
            if has_grad_last:
                fn = yield from fun_value(xn)
            else:
                fn, gn = yield from fun(xn)
            rec['margins'].append((f + 1e-4 * dec - fn, f))
            if fn <= f + 1e-4 * dec:
                if has_grad_last:
                    gn = yield from grad_of_last(xn)
                    if gn is None:
                        fn, gn = yield from fun(xn)
                        rec['margins'].append((f + 1e-4 * dec - fn, f))
                moved = fn <= f + 1e-4 * dec
                if moved:
                    rec['steps'].append(dict(t=t, ls=ls, x0=list(x), x1=list(xn), g0=list(g), first=not Sv))
                break
        if not moved:
            break
        s = [xn[k] - x[k] for k in range(n)]
        y = [gn[k] - g[k] for k in range(n)]
        sy = 0.0
        for k in range(n):
            sy += s[k] * y[k]
        fdec = f - fn
        x, g, f = list(xn), list(gn), fn
        rec['points'].append((list(x), lo, hi))
        rec['stood'].append(theta_of(x))
        if sy > 1e-12:
            if len(Sv) == M:
                Sv.pop(0), Yv.pop(0), rho.pop(0)
            Sv.append(s), Yv.append(y), rho.append(1.0 / sy)
        if fdec <= tol * max(1.0, abs(f)) * 1e-3:
            break
    R['theta'] = theta_of(x)
    R['f'] = f
    R['ok'] = True
    return R


def stage_logv(lb, ub, d, n, stage):
    """Which variables gpmpc_train_multistart searches in log space: ell and sf with a positive finite box; sn in stage 2."""
    logv = [k < d + 1 and lb[k] > 0.0 and ub[k] < INF for k in range(n)]
    if stage == 2:
        logv[d + 1] = True
    return logv


def run_restart(d, lb, ub, theta0, max_iter, tol, has_grad_last, rec):
    """run_restart of gpmpc_train_multistart: the search, then -- iterations to spare -- the polish with sn in log space."""
    n = len(lb)
    res = yield from minimize_box_lbfgs(n, lb, ub, stage_logv(lb, ub, d, n, 1), theta0, max_iter, tol, has_grad_last, rec)
    iters, evals = res['iters'], res['evals']
    res['stage'] = 1
    if res['ok'] and res['iters'] < max_iter and lb[d + 1] > 0.0 and ub[d + 1] < INF:
        res2 = yield from minimize_box_lbfgs(n, lb, ub, stage_logv(lb, ub, d, n, 2), res['theta'], max_iter - res['iters'], tol,
                                             has_grad_last, rec)
        iters += res2['iters']
        evals += res2['evals']
        if res2['ok'] and res2['f'] < res['f']:
            res = res2
            res['stage'] = 2
    res['iters_total'], res['evals_total'] = iters, evals
    return res


class Oracle:
    """(f, g) of one output from gp_oracle.  info: 1 where the point took the reference's one-shot jitter."""

    def __init__(self, X, y, mean='zero', prior=None, track_jitter=True):
        self.X, self.y, self.mean, self.prior, self.d, self.track_jitter = X, y, mean, prior, X.shape[1], track_jitter

    def _info(self, th):
        d = self.d
        if not self.track_jitter:                               # (a box with sn >= 1e-4: lambda_min(K) >= 1e-8, no point needs it)
            return 0
        try:
            np.linalg.cholesky(go.gram(self.X, th[:d], th[d] ** 2, th[d + 1] ** 2))
            return 0
        except np.linalg.LinAlgError:
            return 1

    def _prior_grad(self, th):
        """Gradient of calc_NLL's log-prior (optimize.py:82-93: Gaussians in ell_i, sf^2 and sn^2)."""
        d, p = self.d, self.prior
        g = np.zeros(len(th))
        g[:d] = -(th[:d] - p['ell_mean']) / p['ell_std'] ** 2
        g[d] = -(th[d] ** 2 - p['sf_mean']) / p['sf_std'] ** 2 * 2.0 * th[d]
        g[d + 1] = -(th[d + 1] ** 2 - p['sn_mean']) / p['sn_std'] ** 2 * 2.0 * th[d + 1]
        return g

    def evaluate(self, th, want_grad):
        """(ok, f, g, info); a point that is not positive definite even with the jitter: ok = False."""
        th = np.asarray(th, dtype=np.float64)
        try:
            info = self._info(th)
            if not want_grad:
                f = go.nll_mean(th, self.X, self.y, self.mean) if self.prior is None else go.nll_prior(th, self.X, self.y, self.prior, self.mean)
                return True, float(f), None, info
            # (zero mean: nll_mean_grad is nll_grad on y, without the second fit it makes for the mean parameters)
            f, g = go.nll_grad(th, self.X, self.y) if self.mean == 'zero' else go.nll_mean_grad(th, self.X, self.y, self.mean)
            if self.prior is not None:
                f = f + (go.nll_prior(th, self.X, self.y, self.prior, self.mean) - go.nll_mean(th, self.X, self.y, self.mean))
                g = g + self._prior_grad(th)
            return True, float(f), [float(v) for v in g], info
        except np.linalg.LinAlgError:
            return False, INF, None, 1


def replay(oracle, d, lb, ub, starts, max_iter, mode, cap=0, tol=TOL):
    """The restart search of one output on the oracle.  mode 'lockstep': nll_batch's rounds with its slot bookkeeping (retained
    factors, the slot remap after a jitter repeat, refused grad_of_last requests); cap > 0: `train_batch_cap`, and restarts
    that do not fit one batch evaluate every trial with its gradient.  mode 'single': one restart after the other on
    gpmpc_nll + nll_grad_last.  Returns dict(res[nstart], rec[nstart], rounds, retained, jitter_repeats, jitter_restarts)."""
    nstart = len(starts)
    lb, ub = [float(v) for v in lb], [float(v) for v in ub]
    recs = [dict(margins=[], free=[], steps=[], points=[], stood=[], kinds=[], evaluated=[], took_jitter=[]) for _ in range(nstart)]
    out = dict(res=[None] * nstart, rec=recs, rounds=[], retained=0, jitter_repeats=0, jitter_restarts=set(), jitter_start=[0] * nstart)
    first_eval = [True] * nstart

    def serve(i, kind, th):
        ok, f, g, info = oracle.evaluate(th, kind != 'f')
        recs[i]['kinds'].append(kind)
        recs[i]['evaluated'].append(list(th))
        recs[i]['took_jitter'].append(info)
        if first_eval[i]:
            out['jitter_start'][i], first_eval[i] = info, False
        return ok, f, g, info

    if mode == 'single':
        for i in range(nstart):
            gen = run_restart(d, lb, ub, [float(v) for v in starts[i]], max_iter, tol, True, recs[i])
            try:
                req = next(gen)
                while True:
                    ok, f, g, _ = serve(i, req[0], req[1])
                    req = gen.send((ok, f, g))
            except StopIteration as e:
                out['res'][i] = e.value
        return _cond_limited(out)

    batch = min(nstart, cap) if cap > 0 else nstart             # h->bws.batch after ensure_batch_ws(mine.size())
    retain = batch >= nstart
    gens = [run_restart(d, lb, ub, [float(v) for v in starts[i]], max_iter, tol, retain, recs[i]) for i in range(nstart)]
    pending = {}
    for i, gen in enumerate(gens):
        pending[i] = next(gen)                                  # (every search begins with an evaluation)
    lock_ret = [dict(pos=-1, theta=None) for _ in range(nstart)]
    while pending:
        live = sorted(pending)
        answer = {}
        last, last_pos = [], []
        group = {0: [], 1: []}
        for i in live:
            kind, th = pending[i]
            if kind == 'g':
                answer[i] = (False, INF, None)                  # unless the slot still holds this point
                if lock_ret[i]['pos'] >= 0 and lock_ret[i]['theta'] == th:
                    last.append(i)
                    last_pos.append(lock_ret[i]['pos'])
            else:
                group[1 if kind == 'fg' else 0].append(i)
        for i in last:                                          # nll_grad_retained
            answer[i] = serve(i, 'g', pending[i][1])[:3]
        out['retained'] += len(last)
        out['rounds'].append(dict(live=live, asked=[i for i in live if pending[i][0] == 'g'], served=last, pos=last_pos))
        if group[0] or group[1]:
            for lr in lock_ret:
                lr['pos'] = -1
            for wg in (1, 0):
                G = group[wg]
                for b0 in range(0, len(G), batch):
                    n = min(batch, len(G) - b0)
                    failed = []
                    batch_out = [serve(i, 'fg' if wg else 'f', pending[i][1]) for i in G[b0:b0 + n]]
                    for j in range(n):
                        i = G[b0 + j]
                        ok, f, g, info = batch_out[j]
                        answer[i] = (ok, f, g)
                        if info:
                            failed.append(j)
                    slot_of = list(range(n))
                    if failed:
                        out['jitter_repeats'] += len(failed)
                        m = len(failed)
                        for j in range(min(m, n)):
                            slot_of[j] = -1
                        for j in range(m):
                            slot_of[failed[j]] = j
                    if wg == 0 and retain and len(G) <= batch:
                        for j in range(n):
                            i = G[j]
                            if not answer[i][0] or slot_of[j] < 0:
                                continue
                            lock_ret[i] = dict(pos=slot_of[j], theta=list(pending[i][1]))
        nxt = {}
        for i in live:
            try:
                nxt[i] = gens[i].send(answer[i])
            except StopIteration as e:
                out['res'][i] = e.value
        pending = nxt
    return _cond_limited(out)


def _cond_limited(out):
    """jitter_restarts: the restarts that STOOD on a point that took the jitter (start or accepted point: their gradients are
    cond-limited).  A rejected trial that took it only has to be rejected, which the Armijo margin covers."""
    for i, rec in enumerate(out['rec']):
        took = [th for th, info in zip(rec['evaluated'], rec['took_jitter']) if info]
        if any(th in took for th in rec['stood']):
            out['jitter_restarts'].add(i)
    return out


# ------------------------------------------------------------------------------------------------ cases
class Case:
    """One training problem, its box and starts, and the oracle's replay -- evaluated once and shared by the device runs."""

    def __init__(self, N, d, max_iter, useeds, Ny=1, mean='zero', prior=False, jitter=False, seed=5):
        nstart = len(useeds)
        self.N, self.d, self.Ny, self.nstart, self.max_iter, self.mean, self.jitter = N, d, Ny, nstart, max_iter, mean, jitter
        p = go.synthetic_problem(N, d, Ny, 1, seed=seed, sn=0.05)
        self.X, self.Y = p['X'], p['Y']
        if jitter:                                              # (module docstring: K exactly singular for every theta)
            self.X[-N_DUP:], self.Y[-N_DUP:] = self.X[:N_DUP], self.Y[:N_DUP]
        nm = go.mean_param_count(mean, d)
        self.nh = d + 2 + nm
        sn_lo = 1e-20 if jitter else 1e-4                       # (module docstring: no point with sn >= 1e-4 needs the jitter)
        lb = np.concatenate([1e-2 * np.ones(d + 1), [sn_lo], -5.0 * np.ones(nm)])
        ub = np.concatenate([1e2 * np.ones(d + 1), [1.0], 5.0 * np.ones(nm)])
        self.lb, self.ub = np.tile(lb, (Ny, 1)), np.tile(ub, (Ny, 1))
        # (one seed per restart: a restart's search does not depend on its neighbours, so its seed is chosen on its own)
        u = np.stack([np.random.default_rng(us).uniform(-1.0, 1.0, (Ny, d + 2)) for us in useeds], axis=1)
        self.starts = np.zeros((Ny, nstart, self.nh))
        self.starts[:, :, :d + 2] = p['hyper'][:, None, :] * (1.0 + 0.3 * u)
        self.starts[:, :, d + 2:] = 0.1
        if jitter:
            self.starts[0, -1, d + 1] = 1e-18                   # the LAST restart: its factors move to slot 0 after the repeat
        self.prior = dict(ell_mean=2.0, ell_std=1.0, sf_mean=1.0, sf_std=0.5, sn_mean=0.0, sn_std=0.1) if prior else None
        self.perm = np.random.default_rng(seed + 1).permutation(N)
        self._replays = {}

    def label(self):
        return (f'N={self.N} d={self.d} Ny={self.Ny} restarts={self.nstart} iters={self.max_iter} mean={self.mean}'
                f'{" prior" if self.prior else ""}{" jitter" if self.jitter else ""}')

    def replay(self, mode, cap=0, permuted=False):
        key = (mode, cap, permuted)
        if key not in self._replays:
            X, Y = (self.X[self.perm], self.Y[self.perm]) if permuted else (self.X, self.Y)
            self._replays[key] = [replay(Oracle(X, Y[:, a], self.mean, self.prior, self.jitter), self.d, self.lb[a], self.ub[a], self.starts[a],
                                         self.max_iter, mode, cap) for a in range(self.Ny)]
        return self._replays[key]


_CASES = {}


def case(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _CASES:
        _CASES[key] = Case(**kw)
    return _CASES[key]


def transformed(cs, a, theta, stage):
    """theta in the variables the search ran in: log where logv."""
    logv = stage_logv(cs.lb[a], cs.ub[a], cs.d, cs.nh, stage)
    return np.array([math.log(theta[k]) if logv[k] else theta[k] for k in range(cs.nh)])


class CheckedReplay:
    """The replay of a case for one route, its input conditions asserted, its spread r and the per-restart bars."""

    def __init__(self, cs, mode, cap, need_subset):
        self.cs, self.mode, self.cap = cs, mode, cap
        self.rep = cs.replay(mode, cap)
        perm = cs.replay(mode, cap, True)
        N = cs.N
        worst_margin = INF
        self.bar = np.zeros((cs.Ny, cs.nstart))
        subset_round = False
        for a in range(cs.Ny):                                  # what the replay alone shows (the permuted one costs as much again)
            R = self.rep[a]
            for i in range(cs.nstart):
                res, rec = R['res'][i], R['rec'][i]
                assert res['ok'] and math.isfinite(res['f']), (cs.label(), a, i)
                for margin, f in rec['margins']:
                    worst_margin = min(worst_margin, abs(margin) / (abs(f) + N))
                if i in R['jitter_restarts']:
                    th0 = cs.starts[a, i]
                    ev = np.linalg.eigvalsh(go.gram(cs.X, th0[:cs.d], th0[cs.d] ** 2, th0[cs.d + 1] ** 2) + 1e-8 * np.eye(N))
                    self.bar[a, i] = max(PARITY_BAR, 50.0 * EPS * abs(ev[-1]) / abs(ev[0]))
                    continue
                for x, lo, hi in rec['points']:                 # no variable of a gated restart on a bound
                    assert all(lo[k] < x[k] < hi[k] for k in range(cs.nh)), (cs.label(), 'on a bound', a, i, x)
                assert all(all(fr) for fr in rec['free']), (cs.label(), a, i)
            if cs.jitter:                                       # no evaluation where rounding decides whether the jitter is taken
                for rec in R['rec']:
                    for th in rec['evaluated']:
                        ratio = th[cs.d + 1] / th[cs.d]
                        assert ratio <= 1e-9 or ratio >= 1e-5, (cs.label(), 'sn / sf in the zone of a rounding-dependent jitter', ratio)
            for rd in R['rounds']:
                m = len(rd['served'])
                if 0 < m < len(rd['live']) and rd['served'][0] != 0 and rd['pos'] != list(range(m)):
                    subset_round = True
        assert worst_margin >= ARMIJO_MARGIN, (cs.label(), 'Armijo margin', worst_margin)
        if need_subset:
            assert subset_round, (cs.label(), 'no zmap subset', [(rd['live'], rd['served'], rd['pos']) for rd in self.rep[0]['rounds']])
        r = 0.0
        for a in range(cs.Ny):
            R, Pm = self.rep[a], perm[a]
            for i in range(cs.nstart):
                if i in R['jitter_restarts']:
                    continue
                res, pres = R['res'][i], Pm['res'][i]
                assert (pres['iters_total'], pres['evals_total'], pres['stage']) == (res['iters_total'], res['evals_total'], res['stage'])
                dx = np.max(np.abs(transformed(cs, a, res['theta'], res['stage']) - transformed(cs, a, pres['theta'], res['stage'])))
                r = max(r, float(dx), abs(res['f'] - pres['f']) / (abs(res['f']) + N))
        self.r, self.worst_margin, self.subset_round = r, worst_margin, subset_round
        self.bar[self.bar == 0.0] = max(10.0 * r, PARITY_BAR)
        print(f'[replay {cs.label()} {mode} cap={cap}] smallest Armijo margin {worst_margin:.2e} of |f|+N (needs >= {ARMIJO_MARGIN:.0e}); '
              f'permuted-replay spread r = {r:.2e} (needs <= {SPREAD_MAX:.0e}); zmap-subset round: {subset_round}; '
              f'retained gradients {sum(R["retained"] for R in self.rep)}, jitter repeats {sum(R["jitter_repeats"] for R in self.rep)}')
        assert r <= SPREAD_MAX, (cs.label(), 'spread', r)

    def total(self, key):
        return sum(res[key] for R in self.rep for res in R['res'])


# ------------------------------------------------------------------------------------------------ the check
def check_replay(lib, route='retained', cap=0, persist=-1, need_subset=False, **size):
    """The device's table and counters against the oracle's replay.  route: 'retained' (lock-step, restarts fit one batch),
    'split' (train_batch_cap = cap < restarts: no retention) or 'single' (nstart = 1: gpmpc_nll + nll_grad_last)."""
    cs = case(**size)
    mode = 'single' if route == 'single' else 'lockstep'
    assert (cs.nstart == 1) == (route == 'single') and (route == 'split') == (0 < cap < cs.nstart)
    ck = CheckedReplay(cs, mode, cap, need_subset)
    h = Handle(lib, cs.X, cs.Y)
    if cs.mean != 'zero':
        h.set_mean_func(cs.mean, add_to_prediction=False)
    if cs.prior is not None:
        h.set_hyper_prior(cs.prior)
    assert h.nh == cs.nh
    if cs.jitter:                                               # device and oracle agree on which start takes the jitter
        for i in range(cs.nstart):
            h.nll(0, cs.starts[0, i])
            assert h.last_jitter == ck.rep[0]['jitter_start'][i], (i, h.last_jitter)
        assert sum(ck.rep[0]['jitter_start']) == 1
    lib.set_tuning('train_batch_cap', cap)
    lib.set_tuning('vargemm_persist', persist)
    try:
        dev = h.train_multistart(cs.starts, cs.lb, cs.ub, max_iter=cs.max_iter, tol=TOL)
    finally:
        lib.set_tuning('train_batch_cap', 0)
        lib.set_tuning('vargemm_persist', -1)
    retained, repeats = h.counter('train_retained_gradients'), h.counter('train_jitter_repeats')
    h.close()
    label = f'{cs.label()} {route} cap={cap} persist={persist}'
    worst_x = worst_f = 0.0
    fails = []
    for a in range(cs.Ny):
        R = ck.rep[a]
        for i in range(cs.nstart):
            res = R['res'][i]
            ex = float(np.max(np.abs(transformed(cs, a, dev['theta'][a, i], res['stage']) - transformed(cs, a, res['theta'], res['stage']))))
            ef = abs(dev['obj'][a, i] - res['f']) / (abs(res['f']) + cs.N)
            jit = i in R['jitter_restarts']
            print(f'[{label}] output {a} restart {i}{" (jitter)" if jit else ""}: |dx| {ex:.2e}  |dobj|/(|f|+N) {ef:.2e}  (bar {ck.bar[a, i]:.1e})')
            if not jit:
                worst_x, worst_f = max(worst_x, ex), max(worst_f, ef)
            if not (ex <= ck.bar[a, i] and ef <= ck.bar[a, i]):
                fails.append((a, i, ex, ef))
            if cs.max_iter == 1 and R['rec'][i]['steps']:       # the gradient the first (normalised) step was made of
                st = R['rec'][i]['steps'][0]
                x1 = transformed(cs, a, dev['theta'][a, i], 1)
                grec = (np.array(st['x0']) - x1) / (st['t'])
                g0 = np.array(st['g0'])
                print(f'[{label}]   gradient recovered from the step against the oracle\'s: {np.max(np.abs(grec - g0)) / np.max(np.abs(g0)):.2e} of max|g|')
    want_it, want_ev = ck.total('iters_total'), ck.total('evals_total')
    print(f'[{label}] iterations {dev["iterations"]} (replay {want_it})  evaluations {dev["evaluations"]} (replay {want_ev})  '
          f'retained gradients {retained}  jitter repeats {repeats}')
    RECORD.append((label, worst_x, worst_f, float(ck.bar.min()), ck.r))
    assert not fails, (label, fails)
    assert (dev['iterations'], dev['evaluations']) == (want_it, want_ev), label
    # the route ran: the device's counters against the replay's bookkeeping
    want_ret, want_rep = sum(R['retained'] for R in ck.rep), sum(R['jitter_repeats'] for R in ck.rep)
    if route == 'retained':
        assert retained > 0 and retained == want_ret, (label, retained, want_ret)
        assert repeats == want_rep and (repeats >= 1) == cs.jitter, (label, repeats, want_rep)
    else:
        assert retained == 0, (label, retained)
        assert repeats == (want_rep if route == 'split' else 0), (label, repeats)
    return dev
