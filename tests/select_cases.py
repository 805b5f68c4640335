"""Checks of gpmpc_append_select (greedy max-variance selection of new training points on the device, then gpmpc_append of
the chosen rows) and GP.update_data_select, shared by the emulator tier (tests/test_emu_select.py) and the GPU tier
(tests/test_gpu_select.py).

Yardstick: `yardstick` below, a numpy loop that knows nothing of the code under test -- per step a FULL fit of
X + picks per output (np.linalg.cholesky of k + sn^2 I), the noise-free variances sf^2 - |L^-1 ks|^2 of all remaining
candidates summed over the outputs, np.argmax.  It is evaluated once per problem and shared by the checks.

Bars: the picks are exact -- the test first shows, on the yardstick alone, that at every step the best score leads the
second best by 1e-6 relative and 1e-9 sum_a sf_a^2 absolute, four orders above the 1e-10 sf^2 the device's variances are
held to.  Gains: 1e-10 sum_a sf_a^2, the bar of gpmpc_covar (1e-10 sf^2 per output).  The model after the call: bitwise a
twin handle's gpmpc_append of the same rows, and the bars of parity_cases.check_append against the oracle's full fit."""
import ctypes

import numpy as np
from scipy.linalg import solve_triangular

import gp_oracle as go
from gp_mpc_amd._lib import EINVAL, ENOTFIT, GpmpcError, Handle
from gp_mpc_amd.synthetic import synthetic_problem
from parity_cases import mean_scale, relF


# ------------------------------------------------------------------------------------------------ yardstick
def yardstick(X, H, C, k, forced=None):
    """Greedy max-variance picks among the rows of C by full refits.  forced: a pick sequence to follow instead of the
    arg-max (the scores are still those of every candidate at every step).  Returns picks[k], gains[k] (score of the pick),
    best[k] (largest score), second[k] (second largest; -inf when one candidate is left)."""
    d = X.shape[1]
    Ny, n = H.shape[0], C.shape[0]
    # kernel values once (an entry of k depends on its two points only); the FITS below are from scratch at every step
    Kxc = [go.cov_se_ard(X, C, H[a, :d], H[a, d] ** 2) for a in range(Ny)]
    Kcc = [go.cov_se_ard(C, C, H[a, :d], H[a, d] ** 2) for a in range(Ny)]
    K = [go.cov_se_ard(X, X, H[a, :d], H[a, d] ** 2) + H[a, d + 1] ** 2 * np.eye(len(X)) for a in range(Ny)]
    free = np.ones(n, dtype=bool)
    picks, gains, best, second = [], [], [], []
    for t in range(k):
        score = np.zeros(n)
        for a in range(Ny):
            L = np.linalg.cholesky(K[a])                      # full fit of X + picks
            V = solve_triangular(L, np.vstack([Kxc[a], Kcc[a][picks]]), lower=True)
            score += H[a, d] ** 2 - np.sum(V * V, axis=0)
        masked = np.where(free, score, -np.inf)
        p = int(np.argmax(masked)) if forced is None else int(forced[t])
        order = np.sort(masked)
        gains.append(score[p])
        best.append(order[-1])
        second.append(order[-2] if n > 1 else -np.inf)
        free[p] = False
        for a in range(Ny):                                   # K of the enlarged data set: k + sn^2 I
            kx = np.concatenate([Kxc[a][:, p], Kcc[a][picks, p]])
            K[a] = np.block([[K[a], kx[:, None]], [kx[None, :], np.array([[Kcc[a][p, p] + H[a, d + 1] ** 2]])]])
        picks.append(p)
    return np.array(picks), np.array(gains), np.array(best), np.array(second)


class Case:
    """A synthetic model, its candidates (the generator's Z), seeded candidate outputs and the yardstick's answer."""

    def __init__(self, N, n, k, d, Ny, sn=1e-2):
        self.N, self.n, self.k, self.d, self.Ny, self.sn = N, n, k, d, Ny, sn
        p = synthetic_problem(N, d, Ny, B=n, seed=1234, sn=sn)
        self.X, self.Y, self.H, self.C = p['X'], p['Y'], p['hyper'], p['Z']
        rng = np.random.default_rng(4321)
        self.Yc = rng.standard_normal((n, Ny))
        self.Zt = rng.standard_normal((25, d))                # where predictions are compared
        self.sf2 = float(np.sum(self.H[:, d] ** 2))
        self.picks, self.gains, best, second = yardstick(self.X, self.H, self.C, k)
        # the condition on the INPUTS that makes "the same picks" a fair demand: every step, no exemption
        lead = best - second
        self.rel_lead = float(np.min(lead / best))
        print(f'[yardstick N={N} n={n} k={k} d={d} Ny={Ny} sn={sn}] smallest lead: {self.rel_lead:.2e} relative, '
              f'{np.min(lead) / self.sf2:.2e} of sum sf^2')
        assert np.all(lead >= 1e-6 * best) and np.all(lead >= 1e-9 * self.sf2), (self.rel_lead, np.min(lead))

    def handle(self, lib):
        h = Handle(lib, self.X, self.Y)
        assert np.all(h.fit(self.H) == 0)
        return h


_CASES = {}


def case(N, n, k, d, Ny, sn=1e-2):
    key = (N, n, k, d, Ny, sn)
    if key not in _CASES:
        _CASES[key] = Case(*key)
    return _CASES[key]


def bitwise_factors(f, g):
    return all(np.array_equal(f[key], g[key]) for key in ('hyper', 'chol', 'alpha'))


def assert_picks_and_gains(cs, sel, gain, upto=None, label=''):
    m = len(cs.picks) if upto is None else upto
    assert len(sel) == m and len(gain) == m, (label, len(sel), m)
    err = np.max(np.abs(gain - cs.gains[:m])) if m else 0.0
    print(f'[{label}] picks equal: {np.array_equal(sel, cs.picks[:m])}  |dgain| {err:.2e} (bar {1e-10 * cs.sf2:.1e})')
    assert np.array_equal(sel, cs.picks[:m]), (label, sel, cs.picks[:m])
    assert err <= 1e-10 * cs.sf2, (label, err)
    assert np.all(gain >= 0.0) and np.all(np.diff(gain) <= 1e-10 * cs.sf2), label


def assert_model_matches_oracle(h, X, Y, H, Zt, label=''):
    """parity_cases.check_append's bars against the oracle's full fit of the enlarged data set."""
    d = X.shape[1]
    f = h.get_factors()
    o = go.fit(X, Y, H, want_invK=False)
    rl = max(relF(f['chol'][a], o['chol'][a]) for a in range(H.shape[0]))
    mean, var = h.predict_mean_var(Zt)
    om, ov, _ = go.mean_var_jac(Zt, X, H, o['alpha'], o['chol'], False)
    em = np.max(np.abs(mean - om) / mean_scale(X, Zt, H, o['alpha']))
    ev = np.max(np.abs(var - ov) / H[:, d] ** 2)
    print(f'[{label}] chol relF {rl:.2e}  mean {em:.2e}  var {ev:.2e} (bars 1e-10)')
    assert rl <= 1e-10 and em <= 1e-10 and ev <= 1e-10, (label, rl, em, ev)


# ------------------------------------------------------------------------------------------------ checks
def check_picks_gains_model(lib, **size):
    """1-3. The picks are the yardstick's, the gains within 1e-10 sum sf^2, non-increasing and >= 0; the model is bitwise a
    twin's gpmpc_append of the same rows in the same order and matches the oracle's full fit; get_size reports N + k."""
    cs = case(**size)
    h, twin = cs.handle(lib), cs.handle(lib)
    sel, gain = h.append_select(cs.C, cs.Yc, cs.k)
    assert_picks_and_gains(cs, sel, gain, label='select+append')
    assert h.N == cs.N + cs.k and np.all(h.info == 0)
    twin.append(cs.C[sel], cs.Yc[sel])
    assert bitwise_factors(h.get_factors(), twin.get_factors())
    assert_model_matches_oracle(h, np.vstack([cs.X, cs.C[sel]]), np.vstack([cs.Y, cs.Yc[sel]]), cs.H, cs.Zt, 'after append')
    h.close()
    twin.close()


def check_single_pick(lib, **size):
    """k = 1: the candidate of largest variance under the model as it is."""
    full = case(**size)
    cs = case(**dict(size, k=1))
    assert cs.picks[0] == full.picks[0]
    h = cs.handle(lib)
    sel, gain = h.append_select(cs.C, cs.Yc, 1)
    assert_picks_and_gains(cs, sel, gain, label='k=1')
    assert h.N == cs.N + 1
    assert_model_matches_oracle(h, np.vstack([cs.X, cs.C[sel]]), np.vstack([cs.Y, cs.Yc[sel]]), cs.H, cs.Zt, 'k=1')
    h.close()


def check_selection_only(lib, **size):
    """4. Ycand = None: the same picks and gains, and nothing of the model moves -- factors, size and a prediction bitwise."""
    cs = case(**size)
    h = cs.handle(lib)
    m0, v0 = h.predict_mean_var(cs.Zt)
    f0 = h.get_factors()
    sel, gain = h.append_select(cs.C, None, cs.k)
    assert_picks_and_gains(cs, sel, gain, label='selection only')
    assert h.N == cs.N and bitwise_factors(f0, h.get_factors())
    m1, v1 = h.predict_mean_var(cs.Zt)
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
    sel2, gain2 = h.append_select(cs.C, cs.Yc, cs.k)          # ... and the call with outputs picks the same, bit for bit
    assert np.array_equal(sel, sel2) and np.array_equal(gain, gain2) and h.N == cs.N + cs.k
    h.close()


def check_early_stop(lib, **size):
    """5. min_gain midway between the yardstick's scores of steps t and t+1: t+1 picks, unchanged, the model grows by t+1;
    min_gain above the first score: no pick, GPMPC_OK, the model bitwise unchanged."""
    cs = case(**size)
    lo, hi = cs.k // 3, max(cs.k // 3 + 1, 2 * cs.k // 3)
    gaps = cs.gains[lo:hi] - cs.gains[lo + 1:hi + 1]
    t = lo + int(np.argmax(gaps))                             # a step in the middle whose successor is clearly lower
    assert cs.gains[t] - cs.gains[t + 1] >= 1e-8 * cs.sf2, 'the inputs leave no room for a threshold between two steps'
    h, twin = cs.handle(lib), cs.handle(lib)
    sel, gain = h.append_select(cs.C, cs.Yc, cs.k, min_gain=0.5 * (cs.gains[t] + cs.gains[t + 1]))
    assert_picks_and_gains(cs, sel, gain, upto=t + 1, label=f'early stop after step {t}')
    assert h.N == cs.N + t + 1
    twin.append(cs.C[sel], cs.Yc[sel])
    assert bitwise_factors(h.get_factors(), twin.get_factors())
    f0 = h.get_factors()
    sel, gain = h.append_select(cs.C, cs.Yc, cs.k, min_gain=2.0 * cs.sf2)       # no variance exceeds sum sf^2
    assert len(sel) == 0 and len(gain) == 0 and h.N == cs.N + t + 1 and bitwise_factors(f0, h.get_factors())
    h.close()
    twin.close()


def check_degenerate(lib, N=100, n=70, k=70, d=4, Ny=2, sn=0.1):
    """6. A candidate equal to a training point and two identical candidates: the call succeeds, gains finite and >= 0, no
    index twice; greedy in the tie-proof sense -- along the DEVICE's pick sequence the yardstick's score of each pick is within
    1e-10 sum sf^2 of the yardstick's maximum at that step; the model matches the oracle's full fit."""
    p = synthetic_problem(N, d, Ny, B=n, seed=1234, sn=sn)
    X, Y, H, C = p['X'], p['Y'], p['hyper'], p['Z'].copy()
    C[11] = X[37]
    C[52] = C[5]
    Yc = np.random.default_rng(4321).standard_normal((n, Ny))
    Yc[11], Yc[52] = Y[37], Yc[5]
    sf2 = float(np.sum(H[:, d] ** 2))
    h = Handle(lib, X, Y)
    assert np.all(h.fit(H) == 0)
    sel, gain = h.append_select(C, Yc, k)
    assert len(sel) == k and len(set(sel.tolist())) == k and h.N == N + k
    assert np.all(np.isfinite(gain)) and np.all(gain >= 0.0)
    _, own, best, _ = yardstick(X, H, C, k, forced=sel)
    short = np.max(best - own)
    print(f'[degenerate] device picks fall short of the yardstick maximum by at most {short:.2e} (bar {1e-10 * sf2:.1e}); '
          f'|dgain| {np.max(np.abs(gain - own)):.2e}')
    assert short <= 1e-10 * sf2 and np.max(np.abs(gain - own)) <= 1e-10 * sf2
    assert_model_matches_oracle(h, np.vstack([X, C[sel]]), np.vstack([Y, Yc[sel]]), H, np.random.default_rng(7).standard_normal((25, d)),
                                'degenerate')
    h.close()


def check_mean_function(lib, N=100, n=70, k=20, d=4, Ny=2, sn=0.1):
    """7. gpmpc_set_mean_func(LINEAR, 1): the picks are those of the zero-mean model with the same kernel hyper-parameters;
    after the append alpha is K^-1 (y - m(X)) of the enlarged data (the residual is refreshed)."""
    cs = case(N, n, k, d, Ny, sn)
    rng = np.random.default_rng(31)
    Y = cs.Y + 0.4 + 0.3 * cs.X[:, :1]
    Yc = cs.Yc + 0.4 + 0.3 * cs.C[:, :1]
    H = np.hstack([cs.H, rng.uniform(-0.3, 0.3, (Ny, go.mean_param_count('linear', d)))])
    h = Handle(lib, cs.X, Y)
    h.set_mean_func('linear', True)
    assert np.all(h.fit(H) == 0)
    sel, gain = h.append_select(cs.C, Yc, k)
    assert_picks_and_gains(cs, sel, gain, label='linear mean')
    f = h.get_factors()
    o = go.fit_mean(np.vstack([cs.X, cs.C[sel]]), np.vstack([Y, Yc[sel]]), H, 'linear', want_invK=False)
    for a in range(Ny):                                       # the bars of parity_cases.check_mean_functions
        assert relF(f['chol'][a], o['chol'][a]) <= 1e-10 and relF(f['alpha'][a], o['alpha'][a]) <= 1e-9, a
    h.close()


def _raw(lib, h, n, X, Y, k, min_gain, sel, gain=None):
    kout = ctypes.c_int(-1)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.dll.gpmpc_append_select(h.h, n, p(X), p(Y), k, min_gain, p(sel), p(gain), ctypes.byref(kout), None)
    return rc, kout.value


def check_argument_errors(lib, N=100, n=70, k=20, d=4, Ny=2, sn=1e-2):
    """8. GPMPC_EINVAL for k = 0, k > n, n above the chunk limit, NULL selected, NaN min_gain; GPMPC_ENOTFIT without factors;
    after each error a valid call on the same handle gives the yardstick's picks and gains."""
    cs = case(N, n, k, d, Ny, sn)
    h = cs.handle(lib)
    sel = np.zeros(n, dtype=np.int32)

    def still_fine(hh):
        s, g = hh.append_select(cs.C, None, k)
        assert_picks_and_gains(cs, s, g, label='after an error')

    assert _raw(lib, h, n, cs.C, cs.Yc, 0, 0.0, sel)[0] == EINVAL
    still_fine(h)
    assert _raw(lib, h, n, cs.C, cs.Yc, n + 1, 0.0, sel)[0] == EINVAL
    still_fine(h)
    lib.set_tuning('predict_chunk', 64)
    try:
        assert _raw(lib, h, n, cs.C, cs.Yc, k, 0.0, sel)[0] == EINVAL
    finally:
        lib.set_tuning('predict_chunk', 0)
    still_fine(h)
    assert _raw(lib, h, n, cs.C, cs.Yc, k, 0.0, None)[0] == EINVAL
    still_fine(h)
    assert _raw(lib, h, n, cs.C, cs.Yc, k, float('nan'), sel)[0] == EINVAL
    still_fine(h)
    assert h.N == N                                           # none of the refused calls touched the model
    rc, kout = _raw(lib, h, n, cs.C, cs.Yc, k, 0.0, sel)       # gain = NULL, info = NULL are allowed
    assert rc == 0 and kout == k and np.array_equal(sel[:k], cs.picks)
    h.close()
    fresh = Handle(lib, cs.X, cs.Y)
    try:
        fresh.append_select(cs.C, cs.Yc, k)
        assert False
    except GpmpcError as e:
        assert e.code == ENOTFIT
    assert np.all(fresh.fit(cs.H) == 0)
    still_fine(fresh)
    fresh.close()


def check_python(lib, N=100, n=70, k=20, d=4, Ny=2, sn=0.1):
    """9. GP.update_data_select on a normalised model: the yardstick's picks (on the standardised rows), the model of
    update_data_all of the chosen RAW rows -- predict bitwise equal on a twin object; Y_new = None changes nothing;
    GP.update_data still raises."""
    from gp_mpc_amd.gp import GP
    p = synthetic_problem(N, d, Ny, B=n, seed=1234, sn=sn)
    rng = np.random.default_rng(99)
    Nu = d - Ny
    meta = dict(meanY=rng.standard_normal(Ny), stdY=rng.uniform(0.5, 2.0, Ny), meanZ=rng.standard_normal(d),
                stdZ=rng.uniform(0.5, 2.0, d))
    meta.update(meanX=meta['meanZ'][:Ny], stdX=meta['stdZ'][:Ny], meanU=meta['meanZ'][Ny:], stdU=meta['stdZ'][Ny:])
    o = go.fit(p['X'], p['Y'], p['hyper'])

    def make():
        return GP(p['X'], p['Y'], hyper=dict(hyper=p['hyper'], chol=o['chol'], alpha=o['alpha'], invK=o['invK']), normalize=True,
                  meta=meta, xlb=np.zeros(Ny), xub=np.ones(Ny), ulb=np.zeros(Nu), uub=np.ones(Nu), lib=lib, gp_method='TA')
    gp, twin = make(), make()
    Xraw = meta['meanZ'] + meta['stdZ'] * p['Z']
    Yraw = meta['meanY'] + meta['stdY'] * rng.standard_normal((n, Ny))
    Cs = (Xraw - meta['meanZ']) / meta['stdZ']                # what the object hands to the device
    picks, gains, best, second = yardstick(p['X'], p['hyper'], Cs, k)
    sf2 = float(np.sum(p['hyper'][:, d] ** 2))
    assert np.all(best - second >= 1e-6 * best) and np.all(best - second >= 1e-9 * sf2)
    z = meta['meanZ'] + 0.4 * meta['stdZ'] * rng.standard_normal(d)
    S = 1e-3 * np.eye(d)
    m0, c0 = gp.predict(z[:Ny], z[Ny:], S)
    sel, gain = gp.update_data_select(Xraw, None, N_new=k)
    assert np.array_equal(sel, picks) and np.max(np.abs(gain - gains)) <= 1e-10 * sf2
    m1, c1 = gp.predict(z[:Ny], z[Ny:], S)
    assert gp.get_size()[0] == N and np.array_equal(m0, m1) and np.array_equal(c0, c1)
    sel, gain = gp.update_data_select(Xraw, Yraw, N_new=k)
    assert np.array_equal(sel, picks) and gp.get_size()[0] == N + k
    twin.update_data_all(Xraw[sel], Yraw[sel])
    ma, ca = gp.predict(z[:Ny], z[Ny:], S)
    mb, cb = twin.predict(z[:Ny], z[Ny:], S)
    assert np.array_equal(ma, mb) and np.array_equal(ca, cb) and not np.array_equal(ma, m0)
    try:
        gp.update_data(Xraw[:2], Yraw[:2])
        assert False
    except NotImplementedError as e:
        assert 'update_data_select' in str(e)
    gp.close()
    twin.close()
