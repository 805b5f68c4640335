"""Checks of gpmpc_remove (training points taken out of the model: Householder downdate of L and L^-1 on the device, or
a refit where that cannot pay) and of GP.remove_data / GP.update_data_window, shared by the emulator tier
(tests/test_emu_remove.py) and the GPU tier (tests/test_gpu_remove.py).

Yardstick: the oracle's full fit (gp_oracle.fit, np.linalg.cholesky) on the remaining rows in their original order.

Bars: those of parity_cases.check_append -- relF(chol) <= 1e-10 per output, np.triu(chol, 1) == 0 exactly, mean error
<= 1e-10 of mean_scale, variance error <= 1e-10 sf^2 (the variance is what checks L'^-1).  A numpy run of the sequential
algorithm with n = 40 gives relF(L') 2e-14 at sn = 0.1 and 5e-13 .. 9e-13 at sn = 1e-2 (cond 1e6), so with sn in {0.1, 1e-2}
the method itself sits more than 100x inside the bar."""
import ctypes

import numpy as np

import gp_oracle as go
from gp_mpc_amd._lib import EINVAL, ENOTFIT, GpmpcError, Handle
from gp_mpc_amd.synthetic import synthetic_problem
from parity_cases import mean_scale, relF


class Case:
    """A synthetic model of N points and a pool of extra rows (the generator's Z with seeded outputs)."""

    def __init__(self, N, d, Ny, sn):
        p = synthetic_problem(N, d, Ny, B=64, seed=1234, sn=sn)
        self.N, self.d, self.Ny = N, d, Ny
        self.X, self.Y, self.H = p['X'], p['Y'], p['hyper']
        rng = np.random.default_rng(4321)
        self.Xe, self.Ye = p['Z'], rng.standard_normal((64, Ny))
        self.Zt = rng.standard_normal((25, d))                # where predictions are compared
        self._fits = {}

    def handle(self, lib, want_invK=False):
        h = Handle(lib, self.X, self.Y)
        assert np.all(h.fit(self.H, want_invK=want_invK) == 0)
        return h

    def oracle(self, idx, want_invK=False):
        """The oracle's fit without the rows idx (computed once per index set)."""
        key = (tuple(int(i) for i in idx), want_invK)
        if key not in self._fits:
            keep = np.ones(self.N, dtype=bool)
            keep[list(key[0])] = False
            X, Y = self.X[keep], self.Y[keep]
            self._fits[key] = (X, Y, go.fit(X, Y, self.H, want_invK=want_invK))
        return self._fits[key]


_CASES = {}


def case(N, d=4, Ny=2, sn=1e-2, **_):
    key = (N, d, Ny, sn)
    if key not in _CASES:
        _CASES[key] = Case(*key)
    return _CASES[key]


def index_sets(N, n, kind):
    if kind == 'oldest':
        return np.arange(n)
    if kind == 'scattered':                                   # contains index 0 and index N - 1
        rng = np.random.default_rng(77)
        mid = rng.choice(np.arange(1, N - 1), size=n - 2, replace=False)
        return rng.permutation(np.concatenate([[0, N - 1], mid]))
    if kind == 'single':
        return np.array([N // 2])
    if kind == 'run':                                         # a contiguous run across a 64-boundary
        s = 64 * max(1, (N // 2) // 64) - min(n, 64) // 2
        return np.arange(s, s + n)
    if kind == 'trailing':
        return np.arange(N - n, N)
    raise ValueError(kind)


def assert_matches(h, X, Y, H, Zt, o, label):
    """parity_cases.check_append's bars against the oracle's full fit `o` of (X, Y)."""
    d = X.shape[1]
    assert h.N == len(X), (label, h.N, len(X))
    f = h.get_factors()
    rl = max(relF(f['chol'][a], o['chol'][a]) for a in range(H.shape[0]))
    upper = max(np.max(np.abs(np.triu(f['chol'][a], 1))) for a in range(H.shape[0])) if len(X) > 1 else 0.0
    mean, var = h.predict_mean_var(Zt)
    om, ov, _ = go.mean_var_jac(Zt, X, H, o['alpha'], o['chol'], False)
    em = np.max(np.abs(mean - om) / mean_scale(X, Zt, H, o['alpha']))
    ev = np.max(np.abs(var - ov) / H[:, d] ** 2)
    print(f'[{label}] chol relF {rl:.2e}  upper {upper:.1e}  mean {em:.2e}  var {ev:.2e} (bars 1e-10)')
    assert upper == 0.0, (label, upper)
    assert rl <= 1e-10 and em <= 1e-10 and ev <= 1e-10, (label, rl, em, ev)


class mode:
    """remove_mode for the duration of a block; -1 afterwards."""

    def __init__(self, lib, value):
        self.lib, self.value = lib, value

    def __enter__(self):
        self.lib.set_tuning('remove_mode', self.value)

    def __exit__(self, *exc):
        self.lib.set_tuning('remove_mode', -1)


def remove_downdate(lib, h, idx):
    """h.remove(idx) on the downdate path, recognised by its counter."""
    before = h.counter('remove_downdates'), h.counter('remove_refits')
    with mode(lib, 1):
        h.remove(idx)
    assert (h.counter('remove_downdates'), h.counter('remove_refits')) == (before[0] + 1, before[1])


# ------------------------------------------------------------------------------------------------ checks
def check_vs_fit(lib, N, n, kind, **size):
    """1. Factors and predictions against a fit on the remaining rows."""
    cs = case(N, **size)
    idx = index_sets(N, n, kind)
    h = cs.handle(lib)
    remove_downdate(lib, h, idx)
    X, Y, o = cs.oracle(idx)
    assert_matches(h, X, Y, cs.H, cs.Zt, o, f'N={N} n={len(idx)} {kind}')
    h.close()


def check_trailing(lib, N, n, **size):
    """2. Trailing indices: nothing is reflected, chol is the old leading block bit for bit."""
    cs = case(N, **size)
    h = cs.handle(lib)
    L0 = h.get_factors()['chol']
    idx = index_sets(N, n, 'trailing')
    remove_downdate(lib, h, idx[::-1])
    L1 = h.get_factors()['chol']
    assert L1.shape == (cs.Ny, N - n, N - n) and np.array_equal(L1, L0[:, :N - n, :N - n])
    X, Y, o = cs.oracle(idx)
    assert_matches(h, X, Y, cs.H, cs.Zt, o, f'N={N} n={n} trailing')
    h.close()


def check_sliding_window(lib, N, rounds=6, step=20, **size):
    """3. Six rounds of append 20 / remove the oldest 20 against the oracle after every round, then the NLL path as
    parity_cases.check_append: the errors do not pile up past the bar."""
    cs = case(N, **size)
    p = synthetic_problem(rounds * step, cs.d, cs.Ny, B=1, seed=99, sn=0.1)
    h = cs.handle(lib)
    X, Y = cs.X, cs.Y
    for k in range(rounds):
        xs, ys = p['X'][k * step:(k + 1) * step], p['Y'][k * step:(k + 1) * step]
        assert np.all(h.append(xs, ys) == 0)
        remove_downdate(lib, h, np.arange(step))
        X, Y = np.vstack([X, xs])[step:], np.vstack([Y, ys])[step:]
        assert_matches(h, X, Y, cs.H, cs.Zt, go.fit(X, Y, cs.H, want_invK=False), f'window round {k}')
    ref = go.nll(cs.H[0], X, Y[:, 0])
    assert abs(h.nll(0, cs.H[0]) - ref) / (abs(ref) + len(X)) <= 1e-10
    h.close()


def check_remove_then_append(lib, N, n, **size):
    """4. Remove scattered rows, append the same rows again: the oracle's fit on the reordered data."""
    cs = case(N, **size)
    idx = np.sort(index_sets(N, n, 'scattered'))
    h = cs.handle(lib)
    remove_downdate(lib, h, idx)
    assert np.all(h.append(cs.X[idx], cs.Y[idx]) == 0)
    keep = np.ones(N, dtype=bool)
    keep[idx] = False
    X, Y = np.vstack([cs.X[keep], cs.X[idx]]), np.vstack([cs.Y[keep], cs.Y[idx]])
    assert_matches(h, X, Y, cs.H, cs.Zt, go.fit(X, Y, cs.H, want_invK=False), 'remove then append')
    h.close()


def check_after_set_factors(lib, N, n, **size):
    """5. A model loaded through set_factors (no jitter rule ever ran), as parity_cases.check_append_after_set_factors."""
    cs = case(N, **size)
    o0 = go.fit(cs.X, cs.Y, cs.H, want_invK=False)
    h = Handle(lib, cs.X, cs.Y)
    h.set_factors(cs.H, o0['chol'], o0['alpha'])
    idx = index_sets(N, n, 'scattered')
    remove_downdate(lib, h, idx)
    X, Y, o = cs.oracle(idx)
    assert_matches(h, X, Y, cs.H, cs.Zt, o, 'after set_factors')
    h.close()


def check_mean_function(lib, N, n, sn=0.1, **size):
    """6. gpmpc_set_mean_func(LINEAR, 1): alpha is K^-1 (y - m(X)) of the remaining rows (the residual is refreshed) and the
    prediction adds m(z); bars of parity_cases.check_mean_functions (chol 1e-10, alpha 1e-9) and check_append's for the mean."""
    cs = case(N, sn=sn, **size)
    rng = np.random.default_rng(31)
    Y = cs.Y + 0.4 + 0.3 * cs.X[:, :1]
    H = np.hstack([cs.H, rng.uniform(-0.3, 0.3, (cs.Ny, go.mean_param_count('linear', cs.d)))])
    h = Handle(lib, cs.X, Y)
    h.set_mean_func('linear', True)
    assert np.all(h.fit(H) == 0)
    idx = index_sets(N, n, 'scattered')
    remove_downdate(lib, h, idx)
    keep = np.ones(N, dtype=bool)
    keep[idx] = False
    o = go.fit_mean(cs.X[keep], Y[keep], H, 'linear', want_invK=False)
    f = h.get_factors()
    for a in range(cs.Ny):
        assert relF(f['chol'][a], o['chol'][a]) <= 1e-10 and relF(f['alpha'][a], o['alpha'][a]) <= 1e-9, a
    mean, var = h.predict_mean_var(cs.Zt)
    om, ov, _ = go.mean_var_jac(cs.Zt, cs.X[keep], H, o['alpha'], o['chol'], False, mean_func='linear')
    scale = mean_scale(cs.X[keep], cs.Zt, H, o['alpha']) + np.abs(om)
    assert np.max(np.abs(mean - om) / scale) <= 1e-10 and np.max(np.abs(var - ov) / H[:, cs.d] ** 2) <= 1e-10
    h.close()


def check_invK(lib, N, n, sn=0.1, **size):
    """7. Fit with K^-1, remove, K^-1 again (rebuilt lazily) against the oracle's: 1e-10 relative in Frobenius norm."""
    cs = case(N, sn=sn, **size)
    h = cs.handle(lib, want_invK=True)
    idx = index_sets(N, n, 'scattered')
    remove_downdate(lib, h, idx)
    _, _, o = cs.oracle(idx, want_invK=True)
    iK = h.get_factors(invK=True)['invK']
    err = max(relF(iK[a], o['invK'][a]) for a in range(cs.Ny))
    print(f'[invK] relF {err:.2e} (bar 1e-10)')
    assert err <= 1e-10
    h.close()


def check_refit_branch(lib, N, n, **size):
    """8. remove_mode 2: the same bars, remove_refits advances; mode 0: the two counters together advance by one per call."""
    cs = case(N, **size)
    idx = index_sets(N, n, 'scattered')
    h = cs.handle(lib)
    with mode(lib, 2):
        h.remove(idx)
    assert h.counter('remove_refits') == 1 and h.counter('remove_downdates') == 0
    X, Y, o = cs.oracle(idx)
    assert_matches(h, X, Y, cs.H, cs.Zt, o, 'refit branch')
    h.close()
    h = cs.handle(lib)
    with mode(lib, 0):
        h.remove(idx)
        assert h.counter('remove_refits') + h.counter('remove_downdates') == 1
        assert_matches(h, X, Y, cs.H, cs.Zt, o, 'automatic')
        h.remove([0])
        assert h.counter('remove_refits') + h.counter('remove_downdates') == 2
    keep = np.ones(len(X), dtype=bool)
    keep[0] = False
    assert_matches(h, X[keep], Y[keep], cs.H, cs.Zt, go.fit(X[keep], Y[keep], cs.H, want_invK=False), 'automatic, second call')
    h.close()


def check_automatic_refits(lib, N, n, **size):
    """The automatic rule at a size where the downdate cannot pay: the refit runs and is right."""
    cs = case(N, **size)
    idx = index_sets(N, n, 'oldest')
    h = cs.handle(lib)
    h.remove(idx)
    assert h.counter('remove_refits') == 1 and h.counter('remove_downdates') == 0
    X, Y, o = cs.oracle(idx)
    assert_matches(h, X, Y, cs.H, cs.Zt, o, f'N={N} n={n} automatic')
    h.close()


def _raw(lib, h, n, idx):
    p = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32).ctypes.data_as(ctypes.c_void_p)
    return lib.dll.gpmpc_remove(h.h if h is not None else None, n, p)


def check_argument_errors(lib, N, **size):
    """9. GPMPC_EINVAL for duplicates, indices out of range, n >= N, n <= 0, NULL handle, NULL idx; GPMPC_ENOTFIT without
    factors; after each refused call the predictions are bitwise what they were; a good removal still works."""
    cs = case(N, **size)
    h = cs.handle(lib)
    m0, v0 = h.predict_mean_var(cs.Zt)

    def untouched():
        m1, v1 = h.predict_mean_var(cs.Zt)
        n = ctypes.c_int(0)
        lib.dll.gpmpc_get_size(h.h, ctypes.byref(n), None, None)
        assert n.value == N and np.array_equal(m0, m1) and np.array_equal(v0, v1)

    for mode_value in (1, 2):
        with mode(lib, mode_value):
            for n, idx in ((3, [5, 9, 5]), (2, [0, N]), (2, [-1, 3]), (N, np.arange(N)), (N + 1, np.arange(N + 1)), (0, [1]),
                           (-2, [1]), (2, None)):
                assert _raw(lib, h, n, idx) == EINVAL, (n, idx)
                untouched()
    assert _raw(lib, None, 1, [0]) == EINVAL
    untouched()
    fresh = Handle(lib, cs.X, cs.Y)
    try:
        fresh.remove([1])
        assert False
    except GpmpcError as e:
        assert e.code == ENOTFIT
    assert fresh.N == N
    fresh.close()
    idx = index_sets(N, 5, 'scattered')
    remove_downdate(lib, h, idx)
    X, Y, o = cs.oracle(idx)
    assert_matches(h, X, Y, cs.H, cs.Zt, o, 'after the refused calls')
    h.close()


def check_python(lib, N=100, n=30, d=4, Ny=2, sn=0.1):
    """10. GP.remove_data and GP.update_data_window on a normalised model: the object's data and size are the expected
    rows, and GP.predict matches a GP constructed on those rows with the same hyper-parameters to 1e-9 of max|mean|; with
    len(X_new) >= N_max the window is replace_data_all of the last N_max new rows."""
    from gp_mpc_amd.gp import GP
    p = synthetic_problem(N, d, Ny, B=64, seed=1234, sn=sn)
    rng = np.random.default_rng(99)
    Nu = d - Ny
    meta = dict(meanY=rng.standard_normal(Ny), stdY=rng.uniform(0.5, 2.0, Ny), meanZ=rng.standard_normal(d),
                stdZ=rng.uniform(0.5, 2.0, d))
    meta.update(meanX=meta['meanZ'][:Ny], stdX=meta['stdZ'][:Ny], meanU=meta['meanZ'][Ny:], stdU=meta['stdZ'][Ny:])

    def make(Xs, Ys):
        o = go.fit(Xs, Ys, p['hyper'])
        return GP(Xs, Ys, hyper=dict(hyper=p['hyper'], chol=o['chol'], alpha=o['alpha'], invK=o['invK']), normalize=True,
                  meta=meta, xlb=np.zeros(Ny), xub=np.ones(Ny), ulb=np.zeros(Nu), uub=np.ones(Nu), lib=lib, gp_method='TA')

    z = meta['meanZ'] + 0.4 * meta['stdZ'] * rng.standard_normal(d)
    S = 1e-3 * np.eye(d)

    def same_model(gp, Xs, Ys, label):
        assert gp.get_size()[0] == len(Xs), (label, gp.get_size(), len(Xs))
        got = np.array(gp._GP__X), np.array(gp._GP__Y)
        assert np.array_equal(got[0], Xs) and np.array_equal(got[1], Ys), label
        twin = make(Xs, Ys)
        ma, ca = gp.predict(z[:Ny], z[Ny:], S)
        mb, cb = twin.predict(z[:Ny], z[Ny:], S)
        twin.close()
        scale = np.max(np.abs(mb))
        print(f'[python {label}] |dmean| {np.max(np.abs(ma - mb)) / scale:.2e}  |dcov| {np.max(np.abs(ca - cb)) / np.max(np.abs(cb)):.2e}')
        assert np.max(np.abs(ma - mb)) <= 1e-9 * scale and np.max(np.abs(ca - cb)) <= 1e-9 * np.max(np.abs(cb)), label

    Xs, Ys = p['X'], p['Y']                                  # standardised rows (the load_model branch takes them as they are)
    gp = make(Xs, Ys)
    idx = index_sets(N, n, 'scattered')
    with mode(lib, 1):
        gp.remove_data(idx)
    keep = np.ones(N, dtype=bool)
    keep[idx] = False
    Xs, Ys = Xs[keep], Ys[keep]
    same_model(gp, Xs, Ys, 'remove_data')
    try:                                                      # a refused call: the bookkeeping follows the handle
        gp.remove_data([0, 0])
        assert False
    except GpmpcError as e:
        assert e.code == EINVAL
    same_model(gp, Xs, Ys, 'after a refused remove_data')
    # window: 25 new rows into a budget of 80 -> the 15 oldest go, the new ones follow
    Xn_s, Yn_s = p['Z'][:25], rng.standard_normal((25, Ny))
    Xn, Yn = meta['meanZ'] + meta['stdZ'] * Xn_s, meta['meanY'] + meta['stdY'] * Yn_s
    Xn_s, Yn_s = (Xn - meta['meanZ']) / meta['stdZ'], (Yn - meta['meanY']) / meta['stdY']     # what the object hands on
    with mode(lib, 1):
        gp.update_data_window(Xn, Yn, 80)
    Xs, Ys = np.vstack([Xs, Xn_s])[-80:], np.vstack([Ys, Yn_s])[-80:]
    same_model(gp, Xs, Ys, 'update_data_window')
    gp.update_data_window(Xn[:3], Yn[:3], 90)                 # below the budget: a plain append
    Xs, Ys = np.vstack([Xs, Xn_s[:3]]), np.vstack([Ys, Yn_s[:3]])
    same_model(gp, Xs, Ys, 'update_data_window below the budget')
    gp.update_data_window(Xn, Yn, 20)                         # len(X_new) >= N_max: replace_data_all on the last N_max new rows
    same_model(gp, Xn_s[-20:], Yn_s[-20:], 'update_data_window, replace')
    gp.close()
