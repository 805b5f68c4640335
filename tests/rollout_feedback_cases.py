"""Checks of gpmpc_rollout_multi_feedback (closed-loop roll-outs in lock-step) and GP.rollout_closed_loop, shared by the
emulator tier (tests/test_emu_rollout_feedback.py) and the GPU tier (tests/test_gpu_rollout_feedback.py).

Yardsticks: gpmpc_rollout_feedback (one closed trajectory per call), gpmpc_rollout_multi (open loop in lock-step) and
OracleGP.rollout(feedback=True) called with ONE method at a time -- its `covar` is then fresh, so the trajectory is an
independent one (with several methods the reference carries the control blocks of `covar` from one method into the next,
gp_class.py:777-804).  Bars: bitwise where the same kernels run on the same inputs; the lock-step bars of
parity_cases.check_rollout_multi (1e-10 scaled) where an 'ME' / 'TA' trajectory moves from the one-column variance kernel
to the batched one; the bars of parity_cases.check_feedback_rollout against the oracle."""
import ctypes

import numpy as np

import gp_oracle as go
from gp_mpc_amd._lib import EINVAL, GpmpcError, Handle


class Problem:
    """A fitted synthetic model (sn = 0.1, K^-1 present) with T-step inputs for several trajectories: starts z[i] = [x_0,
    u_0], small gains (0.05 * N(0, 1), as check_feedback_rollout: the loop must not amplify rounding differences) that
    differ per trajectory, two initial covariances and open-loop controls."""

    def __init__(self, lib, N, Ny, d, T, seed=33, ntraj=6):
        self.p = p = go.synthetic_problem(N, d, Ny, T + ntraj, seed=seed, sn=0.1)
        self.N, self.Ny, self.d, self.T, self.Nu = N, Ny, d, T, d - Ny
        self.H = p['hyper']
        self.h = Handle(lib, p['X'], p['Y'])
        assert np.all(self.h.fit(self.H, want_invK=True) == 0)
        rng = np.random.default_rng(seed)
        Nu = self.Nu
        self.z = [p['Z'][i].copy() for i in range(ntraj)]
        self.Kz = [0.05 * rng.standard_normal((Nu, Ny)) for _ in range(ntraj)]
        self.k0 = [0.05 * rng.standard_normal(Nu) for _ in range(ntraj)]
        self.Kc = [0.05 * rng.standard_normal((Nu, Ny)) for _ in range(ntraj)]
        self.U = [0.3 * rng.standard_normal((T, Nu)) for _ in range(ntraj)]
        S0 = np.eye(d) * 1e-6                                           # gp_class.py:764
        S0[:Ny, :Ny] = np.diag(self.H[:, d + 1] ** 2)                   # gp_class.py:780
        self.S = [S0, 2.0 * S0, 0.5 * S0, S0, 2.0 * S0, S0][:ntraj]
        self.sf2 = (self.H[:, d] ** 2).max()

    def single_closed(self, method, i):
        return self.h.rollout_feedback(method, self.T, self.z[i], self.S[i], self.Kz[i], self.k0[i], self.Kc[i])

    def multi(self, methods, idx, closed=None):
        """Trajectories idx[k] (start, covariance, gains, controls of that index) under methods[k] in one call."""
        g = lambda a: np.stack([a[i] for i in idx])
        return self.h.rollout_multi_feedback(list(methods), g(self.z), g(self.S), g(self.Kz), g(self.k0), g(self.Kc),
                                             closed=closed, U=g(self.U))

    def close(self):
        self.h.close()


def equal3(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def traj(res, k):
    """(mean, cov, U) of trajectory k of a lock-step result."""
    return tuple(a[k] for a in res)


def lockstep_close(pr, got, ref, label):
    """check_rollout_multi's bars for an 'ME' / 'TA' trajectory against its single call; controls 1e-10 * max(1, max|U|)."""
    em, ec, eu = (np.max(np.abs(got[k] - ref[k])) for k in range(3))
    bm, bc, bu = 1e-10 * max(1.0, np.abs(ref[0]).max()), 1e-10 * pr.sf2, 1e-10 * max(1.0, np.abs(ref[2]).max())
    print(f'[{label}] |dmean| {em:.2e} (bar {bm:.1e})  |dcov| {ec:.2e} (bar {bc:.1e})  |dU| {eu:.2e} (bar {bu:.1e})')
    assert em <= bm and ec <= bc and eu <= bu, (label, em, ec, eu)


def check_single_closed(lib, N=150, Ny=2, d=4, T=5, methods=('ME', 'TA', 'EM', 'old_ME')):
    """1. One closed trajectory per call, every method: mean, cov and the controls are the bits of gpmpc_rollout_feedback
    (also with closed=[1] spelt out, and when the single call has gone over to its replayed graph)."""
    pr = Problem(lib, N, Ny, d, T)
    for j, m in enumerate(methods):
        i = j % len(pr.z)
        ref = pr.single_closed(m, i)
        assert np.array_equal(ref[2][0], pr.z[i][Ny:])                   # the first control came with z0
        assert np.max(np.abs(ref[2][1:] - ref[2][:1])) > 0               # ... the others from the law
        got = traj(pr.multi([m], [i]), 0)
        assert equal3(got, ref), m
        assert equal3(traj(pr.multi([m], [i], closed=[1]), 0), ref), m
        for _ in range(3):
            again = pr.single_closed(m, i)
        assert equal3(got, again), m
    pr.close()


def check_all_open(lib, N=150, Ny=2, d=4, T=5, moment='EM'):
    """2. closed all 0: the bits of gpmpc_rollout_multi on the same inputs (gains present and ignored, and absent);
    U_out returns the given controls."""
    pr = Problem(lib, N, Ny, d, T)
    methods, idx = ['TA', 'ME', moment, 'TA'], [0, 1, 2, 3]
    g = lambda a: np.stack([a[i] for i in idx])
    ref = pr.h.rollout_multi(methods, g(pr.z), g(pr.U), g(pr.S))
    got = pr.multi(methods, idx, closed=[0, 0, 0, 0])
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], g(pr.U))
    bare = pr.h.rollout_multi_feedback(methods, g(pr.z), g(pr.S), None, None, None, closed=[0, 0, 0, 0], U=g(pr.U))
    assert equal3(bare, got)
    pr.close()


MIXED = (['TA', 'ME', 'TA', 'EM'], [0, 1, 2, 3], [1, 1, 0, 1])     # closed 'TA', closed 'ME', open 'TA', closed 'EM'


def check_mixed(lib, N=150, Ny=2, d=4, T=5):
    """3. Closed and open trajectories in one call, different starts, gains and Sigma0: the moment-method trajectory is
    bitwise its single call, the 'ME' / 'TA' ones agree with theirs at the lock-step bars."""
    pr = Problem(lib, N, Ny, d, T)
    methods, idx, closed = MIXED
    got = pr.multi(methods, idx, closed=closed)
    for k, (m, i, c) in enumerate(zip(methods, idx, closed)):
        if c:
            ref = pr.single_closed(m, i)
        else:
            mm, cc = pr.h.rollout(m, pr.z[i], pr.U[i], pr.S[i])
            ref = (mm, cc, pr.U[i])
        mine = traj(got, k)
        if m in ('ME', 'TA'):
            lockstep_close(pr, mine, ref, f'mixed N={N} {m} {"closed" if c else "open"}')
        else:
            assert equal3(mine, ref), m
    assert np.array_equal(got[2][2], pr.U[2])                            # the open trajectory's controls are the given ones
    pr.close()


def check_position_invariance(lib, N=150, Ny=2, d=4, T=5):
    """4. The same closed 'TA' trajectory in two calls with other neighbours and another position (both with >= 2 'ME' /
    'TA' trajectories): the same bits, controls included."""
    pr = Problem(lib, N, Ny, d, T)
    a = pr.multi(['TA', 'ME'], [0, 1], closed=[1, 1])
    b = pr.multi(['ME', 'EM', 'TA', 'TA', 'ME'], [4, 3, 2, 0, 5], closed=[0, 1, 1, 1, 1])
    assert all(np.array_equal(x[0], y[3]) for x, y in zip(a, b))
    c = pr.multi(['ME', 'TA'], [2, 0], closed=[1, 1])
    assert all(np.array_equal(x[0], y[1]) for x, y in zip(a, c))
    assert np.max(np.abs(a[2][0][1:] - a[2][0][:1])) > 0
    pr.close()


def check_without_invK(lib, N=150, Ny=2, d=4, T=5):
    """6. A model fitted WITHOUT K^-1: a call with 'EM' + 'ME' + 'TA' forms it itself (on the moment methods' queue, next to
    the 'ME' / 'TA' group's steps); the trajectories have the bits they have in the mixed call of check_mixed."""
    pr = Problem(lib, N, Ny, d, T)
    methods, idx, closed = MIXED
    ref = pr.multi(methods, idx, closed=closed)                          # with K^-1 from the fit
    em_single = pr.single_closed('EM', 3)
    assert np.all(pr.h.fit(pr.H) == 0)                                   # ... and without
    got = pr.multi(['EM', 'ME', 'TA'], [3, 1, 0], closed=[1, 1, 1])
    for k, kr in ((0, 3), (1, 1), (2, 0)):
        assert all(np.array_equal(g[k], r[kr]) for g, r in zip(got, ref)), (k, kr)
    assert all(np.array_equal(g[0], r) for g, r in zip(got, em_single))
    pr.close()


def check_argument_errors(lib, N=150, Ny=2, d=4, T=5):
    """7. GPMPC_EINVAL for M = 0, M = 65, a bad method code, a closed trajectory with NULL gains, an open trajectory with
    NULL U, Nu = 0 with a closed trajectory; the handle serves the next call as before."""
    pr = Problem(lib, N, Ny, d, T)
    good = pr.multi(['TA', 'ME'], [0, 1])
    h = pr.h
    one = lambda a: a[0]
    bad_calls = {
        'M = 0': lambda: h.rollout_multi_feedback([], one(pr.z), one(pr.S), one(pr.Kz), one(pr.k0), one(pr.Kc), T=T),
        'M = 65': lambda: h.rollout_multi_feedback(['TA'] * 65, one(pr.z), one(pr.S), one(pr.Kz), one(pr.k0), one(pr.Kc), T=T),
        'method code 9': lambda: h.rollout_multi_feedback(['TA', 9], one(pr.z), one(pr.S), one(pr.Kz), one(pr.k0), one(pr.Kc), T=T),
        'closed, NULL Kz': lambda: h.rollout_multi_feedback(['TA', 'ME'], one(pr.z), one(pr.S), None, one(pr.k0), one(pr.Kc), T=T),
        'closed, NULL k0': lambda: h.rollout_multi_feedback(['TA', 'ME'], one(pr.z), one(pr.S), one(pr.Kz), None, one(pr.Kc), T=T),
        'closed, NULL Kc': lambda: h.rollout_multi_feedback(['TA', 'ME'], one(pr.z), one(pr.S), one(pr.Kz), one(pr.k0), None,
                                                            closed=[0, 1], U=one(pr.U)),
        'open, NULL U': lambda: h.rollout_multi_feedback(['TA', 'ME'], one(pr.z), one(pr.S), one(pr.Kz), one(pr.k0), one(pr.Kc),
                                                         closed=[1, 0], T=T),
    }
    for label, call in bad_calls.items():
        try:
            call()
        except GpmpcError as e:
            assert e.code == EINVAL, (label, e)
        else:
            raise AssertionError(f'{label}: no error')
        assert equal3(pr.multi(['TA', 'ME'], [0, 1]), good), label
    pr.close()
    # a model without controls (d == Ny): open trajectories run, a closed one is refused -- raw call, so that gains are not NULL
    q = go.synthetic_problem(N, Ny, Ny, T, seed=5, sn=0.1)
    h = Handle(lib, q['X'], q['Y'])
    assert np.all(h.fit(q['hyper'], want_invK=True) == 0)
    S0 = np.eye(Ny) * 1e-6
    codes = np.array([1, 0], dtype=np.int32)
    z0 = np.ascontiguousarray(np.stack([q['Z'][0], q['Z'][1]]))
    S2 = np.ascontiguousarray(np.stack([S0, S0]))
    dummy = np.zeros((2, 1, Ny))
    mean, cov, Uo = np.zeros((2, T, Ny)), np.zeros((2, T, Ny, Ny)), np.zeros((2, T, 1))
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def raw(closed):
        cl = np.array(closed, dtype=np.int32)
        return lib.dll.gpmpc_rollout_multi_feedback(h.h, 2, vp(codes), T, vp(z0), vp(S2), None, None, vp(cl), vp(dummy), vp(dummy),
                                                    vp(dummy), None, vp(mean), vp(cov), vp(Uo))
    assert raw([0, 1]) == EINVAL
    assert raw([0, 0]) == 0
    ref = h.rollout_multi(['TA', 'ME'], z0, np.zeros((2, T, 1)), S2)
    assert np.array_equal(mean, ref[0]) and np.array_equal(cov, ref[1])
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. GP.rollout_closed_loop against the oracle, one method per oracle call
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_closed_loop(og, X0, u0, T, methods, **kw):
    S, Ny, Nu = len(X0), og.Ny, og.Nx - og.Ny
    om, ov, oc = np.zeros((S, len(methods), T + 1, Ny)), np.zeros((S, len(methods), T + 1, Ny)), np.zeros((S, len(methods), T, Nu))
    U = np.tile(u0, (T, 1))                                              # (only U[0] is used: the linearisation point)
    for s in range(S):
        for i, m in enumerate(methods):
            a, b = og.rollout(X0[s], U, methods=(m,), feedback=True, **kw)
            om[s, i], ov[s, i], oc[s, i] = a[0], b[0], og.controls[0]
    return om, np.clip(ov, 0, None), oc


def check_closed_loop_vs_oracle_tank(lib, g, T=5):
    """The standardised tank model ('TA', 'ME'), three start states, a given gain and the LQR gain: check_feedback_rollout's
    bars (rtol 1e-7 / atol 1e-8 scaled on controls and mean, rtol 1e-5 on the variance)."""
    from gp_mpc_amd.gp import GP
    hyper = dict(hyper=g['hyper'], chol=g['chol'], alpha=g['alpha'], invK=g['invK'])
    gp = GP(g['X'], g['Y'], hyper=hyper, gp_method='TA', normalize=True, lib=lib, meta=g['meta'], xlb=g['xlb'], xub=g['xub'],
            ulb=g['ulb'], uub=g['uub'])
    og = go.OracleGP(g['X'], g['Y'], g['hyper'], g['chol'], g['alpha'], g['invK'], normalize=True, meta=g['meta'], gp_method='TA')
    N, Ny, Nu = gp.get_size()
    X0 = np.stack([g['meta']['meanX'] + a * g['meta']['stdX'] for a in (0.3, -0.2, 0.1)])
    u0 = g['meta']['meanU'] - 0.2 * g['meta']['stdU']
    x_ref = X0[0] * 0.9
    Kgain = 0.05 * np.random.default_rng(2).standard_normal((Nu, Ny))
    methods = ['TA', 'ME']
    for Kin in (Kgain, None):
        m, v, c = gp.rollout_closed_loop(X0, T, methods=methods, x_ref=x_ref, K=Kin, u0=u0, return_controls=True)
        om, ov, oc = _oracle_closed_loop(og, X0, u0, T, methods, x_ref=x_ref, K=Kin)
        assert m.shape == (3, 2, T + 1, Ny) and v.shape == m.shape and c.shape == (3, 2, T, Nu)
        print(f'[tank K={"given" if Kin is not None else "lqr"}] |dU| {np.abs(c - oc).max():.2e} |dmean| {np.abs(m - om).max():.2e} '
              f'|dvar| {np.abs(v - ov).max():.2e} (max|var| {np.abs(ov).max():.2e})')
        assert np.allclose(c, oc, rtol=1e-7, atol=1e-8 * max(1.0, np.abs(oc).max())), np.abs(c - oc).max()
        assert np.allclose(m, om, rtol=1e-7, atol=1e-8 * max(1.0, np.abs(om).max())), np.abs(m - om).max()
        assert np.allclose(v, ov, rtol=1e-5, atol=1e-9 * max(1.0, np.abs(ov).max())), np.abs(v - ov).max()
    gp.close()


def check_closed_loop_vs_oracle_synthetic(lib, N=120, T=5):
    """An un-normalised synthetic model, all three methods, three start states, the LQR gain (Q = 2 I, R = 0.5 I) and a given
    gain: 1e-8 scaled on controls and mean, 1e-8 on the variance (check_feedback_rollout); under the LQR gain every
    trajectory's controls vary along the horizon by more than 1e-3 -- they come from the law."""
    from gp_mpc_amd.gp import GP
    p = go.synthetic_problem(N, 5, 3, T + 3, seed=21, sn=0.1)
    o = go.fit(p['X'], p['Y'], p['hyper'])
    gp = GP(p['X'], p['Y'], hyper=dict(hyper=p['hyper'], chol=o['chol'], alpha=o['alpha'], invK=o['invK']),
            normalize=False, gp_method='EM', lib=lib)
    og = go.OracleGP(p['X'], p['Y'], p['hyper'], o['chol'], o['alpha'], o['invK'], gp_method='EM')
    X0, u0 = p['Z'][:3, :3], p['Z'][0, 3:] * 0.3
    methods = ['EM', 'TA', 'ME']
    Kgain = 0.05 * np.random.default_rng(3).standard_normal((2, 3))
    for kw in (dict(Q=np.eye(3) * 2.0, R=np.eye(2) * 0.5), dict(K=Kgain, x_ref=0.5 * X0[1])):
        m, v, c = gp.rollout_closed_loop(X0, T, methods=methods, u0=u0, return_controls=True, **kw)
        om, ov, oc = _oracle_closed_loop(og, X0, u0, T, methods, **kw)
        print(f'[synthetic {sorted(kw)}] |dU| {np.abs(c - oc).max():.2e} |dmean| {np.abs(m - om).max():.2e} |dvar| {np.abs(v - ov).max():.2e}')
        assert np.max(np.abs(c - oc)) <= 1e-8 * max(1.0, np.abs(oc).max())
        assert np.max(np.abs(m - om)) <= 1e-8 * max(1.0, np.abs(om).max())
        # the variance bar is scaled per trajectory: under an LQR gain of several units 'TA' multiplies its variance every
        # step (control blocks K C K^T of the input covariance: 1e3 - 1e4 after five steps from some starts)
        ev, sv = np.abs(v - ov).max(axis=(2, 3)), np.maximum(1.0, np.abs(ov).max(axis=(2, 3)))
        print('[synthetic] |dvar| / max(1, max|var|) per trajectory', (ev / sv).ravel())
        assert np.all(ev <= 1e-8 * sv), ev / sv
        if 'K' not in kw:
            swing = np.abs(c[:, :, 1:] - c[:, :, :1]).max(axis=(2, 3))
            print('[synthetic] control swing per trajectory', swing.ravel())
            assert np.all(swing > 1e-3), swing
    assert gp._GP__gp_method == 'EM'                                     # the linearisations leave the selected method alone
    gp.close()


def check_closed_loop_split(lib, N=120, T=4):
    """More than 64 trajectories (33 starts x ['TA', 'ME'] = 66) are split over two device calls, 64 + 2.  The two
    trajectories of the second call are bitwise those of a call with that start alone (same batch of two); a trajectory
    of the 64-wide call agrees with a narrow call at the lock-step bars of parity_cases.check_rollout_multi (1e-10 scaled:
    a prediction batch wider than 32 takes another variance kernel than a batch of 2..32, i.e. another summation order)."""
    from gp_mpc_amd.gp import GP
    p = go.synthetic_problem(N, 5, 3, 40, seed=21, sn=0.1)
    o = go.fit(p['X'], p['Y'], p['hyper'])
    gp = GP(p['X'], p['Y'], hyper=dict(hyper=p['hyper'], chol=o['chol'], alpha=o['alpha'], invK=o['invK']),
            normalize=False, gp_method='TA', lib=lib)
    X0 = p['Z'][:33, :3]
    Kgain = 0.05 * np.random.default_rng(4).standard_normal((2, 3))
    m, v, c = gp.rollout_closed_loop(X0, T, methods=['TA', 'ME'], K=Kgain, return_controls=True)
    assert m.shape == (33, 2, T + 1, 3) and np.all(np.isfinite(m)) and np.all(v >= 0)
    m2, v2, c2 = gp.rollout_closed_loop(X0[32:], T, methods=['TA', 'ME'], K=Kgain, return_controls=True)
    assert np.array_equal(m2[0], m[32]) and np.array_equal(v2[0], v[32]) and np.array_equal(c2[0], c[32])
    m3, v3, c3 = gp.rollout_closed_loop(X0[:2], T, methods=['TA', 'ME'], K=Kgain, return_controls=True)
    sf2 = (p['hyper'][:, 5] ** 2).max()
    em, ev, ec = np.abs(m3 - m[:2]).max(), np.abs(v3 - v[:2]).max(), np.abs(c3 - c[:2]).max()
    print(f'[split] 64-wide against 4-wide call: |dmean| {em:.2e} |dvar| {ev:.2e} |dU| {ec:.2e}')
    assert em <= 1e-10 * max(1.0, np.abs(m).max()) and ev <= 1e-10 * sf2 and ec <= 1e-10 * max(1.0, np.abs(c).max())
    gp.close()
