"""Checks of gpmpc_sparse_fitc (a FITC model on M inducing points, built on the device and handed out as an ordinary handle
of size M) and GP.sparse, shared by the emulator tier (tests/test_emu_fitc.py) and the GPU tier (tests/test_gpu_fitc.py).

Truth: no reference implementation exists (the reference's GP.sparse is empty).  `fitc_truth` restates the textbook
construction directly -- Kuu + 1e-6 sf^2 I, V = Luu^-1 Kuf, lambda, B = I + Vs Vs^T, alpha_u = Luu^-T B^-1 r,
P = Luu^-T (I - B^-1) Luu^-1, mean = k alpha_u, var = sf^2 - k P k^T, no W anywhere -- once in float64 (numpy / LAPACK) and
once in np.longdouble with its own Cholesky and triangular-inverse loops.

Gate (the convention of the extended-precision gates of this suite): the device's distance from the longdouble value, in
units of max|mean| and of sf^2, must be <= 10 x the fp64-numpy distance measured in the same test, with a floor of 1e-13
on the bar (M eps for M <= 450).  Both distances are printed; the GPU tier records them in profiles/fitc_digits.txt.

The sparse handle as an ordinary model: the oracle's own functions evaluated on the exported (Xu, Yu, hyper, chol, alpha,
invK) at the tolerances parity_cases.py uses for the same calls on an exact model."""
import ctypes

import numpy as np
from scipy.linalg import solve_triangular

import gp_oracle as go
from gp_mpc_amd._lib import EINVAL, ENOTFIT, GpmpcError, Handle
from gp_mpc_amd.synthetic import synthetic_problem
from parity_cases import _longdouble_or_skip, mean_scale, moment_bars

LD = np.longdouble
DIGITS = []            # (label, e_dev_mean, e_np_mean, e_dev_var, e_np_var) of every truth gate that ran


# ------------------------------------------------------------------------------------------------ truth
def _se(X, Z, ell, sf2):
    """sf2 exp(-1/2 sum ((x - z) / ell)^2) in the dtype of X (direct differences, dimension by dimension)."""
    dist = np.zeros((X.shape[0], Z.shape[0]), dtype=X.dtype)
    for k in range(X.shape[1]):
        df = (X[:, k][:, None] - Z[:, k][None, :]) / ell[k]
        dist += df * df
    return sf2 * np.exp(-dist / 2)


def _chol_ld(A):
    """Lower Cholesky factor in the dtype of A (column by column; LAPACK has no extended type)."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]          # (rows of L: contiguous along the contraction)
        assert v[0] > 0, ('truth: not positive definite at', j)
        L[j:, j] = v / np.sqrt(v[0])
    return L


def _trinv_ld(L):
    """Inverse of a lower triangular matrix in its dtype: row by row forward substitution on the identity (kept transposed
    while it grows, so that the contraction runs along rows)."""
    n = L.shape[0]
    TT = np.zeros_like(L)
    for i in range(n):
        TT[:i, i] = -(TT[:i, :i] @ L[i, :i]) / L[i, i]
        TT[i, i] = 1 / L[i, i]
    return np.ascontiguousarray(TT.T)


def _mm(A, B):
    """A @ B with both operands laid out along the contraction index (numpy's extended-precision product is a plain loop:
    a strided operand costs it a cache miss per term)."""
    return np.ascontiguousarray(A) @ np.ascontiguousarray(B.T).T


def _tri_times(T, K, bs=64):
    """T @ K for a lower triangular T, block row by block row (half the multiply-adds of the full product)."""
    out = np.zeros((T.shape[0], K.shape[1]), dtype=T.dtype)
    for i in range(0, T.shape[0], bs):
        e = min(i + bs, T.shape[0])
        out[i:e] = _mm(T[i:e, :e], K[:e])
    return out


def _gram_rows(V, bs=64):
    """V @ V.T from its lower block triangle, mirrored (half the multiply-adds; symmetric to the bit)."""
    M = V.shape[0]
    out = np.zeros((M, M), dtype=V.dtype)
    for i in range(0, M, bs):
        e = min(i + bs, M)
        out[i:e, :e] = _mm(V[i:e], V[:e].T)
    return np.tril(out) + np.tril(out, -1).T


def fitc_truth(X, Y, H, Xu, Zt, dtype):
    """mean[B x Ny], var[B x Ny] of the FITC predictor, steps 1-5 of the construction in `dtype`."""
    ext = dtype is LD
    X, Y, H, Xu, Zt = (np.asarray(v, dtype=dtype) for v in (X, Y, H, Xu, Zt))
    d, M = X.shape[1], Xu.shape[0]
    mean = np.zeros((Zt.shape[0], H.shape[0]), dtype=dtype)
    var = np.zeros_like(mean)
    one, eye = dtype(1), np.eye(M, dtype=dtype)
    for a in range(H.shape[0]):
        ell, sf2, sn2 = H[a, :d], H[a, d] * H[a, d], H[a, d + 1] * H[a, d + 1]
        Kuu = _se(Xu, Xu, ell, sf2) + dtype(1e-6) * sf2 * eye
        Kuf = _se(Xu, X, ell, sf2)
        if ext:
            Luu = _chol_ld(Kuu)
            Tuu = _trinv_ld(Luu)
        else:
            Luu = np.linalg.cholesky(Kuu)
            Tuu = solve_triangular(Luu, eye, lower=True)
        V = _tri_times(Tuu, Kuf) if ext else solve_triangular(Luu, Kuf, lower=True)
        lam = np.maximum(sf2 - np.sum(V * V, axis=0), 0) + sn2
        isq = one / np.sqrt(lam)
        Vs = V * isq[None, :]
        B = eye + (_gram_rows(Vs) if ext else Vs @ Vs.T)
        r = Vs @ (Y[:, a] * isq)
        if ext:
            TB = _trinv_ld(_chol_ld(B))
        else:
            TB = solve_triangular(np.linalg.cholesky(B), eye, lower=True)
        Binv = _mm(TB.T, TB)
        alpha = Tuu.T @ (Binv @ r)
        P = _mm(_mm(Tuu.T, eye - Binv), Tuu)
        ks = _se(Zt, Xu, ell, sf2)
        mean[:, a] = ks @ alpha
        var[:, a] = sf2 - np.sum(_mm(ks, P) * ks, axis=1)
    return mean, var


# ------------------------------------------------------------------------------------------------ cases
def greedy_inducing(lib, X, Y, H, M):
    """Row 0, then gpmpc_append_select's selection-only picks among the other rows on a seed model of row 0."""
    seed = Handle(lib, X[:1], Y[:1])
    seed.fit(H)
    sel, _ = seed.append_select(X[1:], None, M - 1)
    seed.close()
    assert len(sel) == M - 1
    return np.concatenate([[0], sel.astype(np.int64) + 1])


class Case:
    """A synthetic data set, its inducing subset, 300 test points (half of them outside the data's box) and the truth twice."""

    def __init__(self, lib, N, M, d, Ny, sn=1e-2, inducing='random', dup=False):
        self.N, self.M, self.d, self.Ny, self.sn = N, M, d, Ny, sn
        self.label = f'N{N}M{M}d{d}Ny{Ny}sn{sn}{"dup" if dup else ""}'
        p = synthetic_problem(N, d, Ny, B=8, seed=1234, sn=sn)
        self.X, self.Y, self.H, self.Zs, self.Ss = p['X'], p['Y'], p['hyper'], p['Z'], p['Sigma']
        rng = np.random.default_rng(97)
        if inducing == 'greedy':
            self.idx = greedy_inducing(lib, self.X, self.Y, self.H, M)
        else:
            self.idx = np.sort(rng.choice(N, M, replace=False))
        self.Xu = np.ascontiguousarray(self.X[self.idx])
        if dup:
            self.Xu[1] = self.Xu[0]
        lo, hi = self.X.min(axis=0), self.X.max(axis=0)
        inside = lo + (hi - lo) * rng.uniform(size=(150, d))
        outside = lo + (hi - lo) * rng.uniform(size=(150, d))
        k = rng.integers(0, d, 150)                            # one coordinate pushed beyond the box, either side
        push = (hi - lo)[k] * rng.uniform(0.05, 0.5, 150)
        side = rng.integers(0, 2, 150)
        outside[np.arange(150), k] = np.where(side == 1, hi[k] + push, lo[k] - push)
        self.Zt = np.vstack([inside, outside])
        self.sf2 = self.H[:, d] ** 2
        self._truth = None

    def truth(self):
        if self._truth is None:
            _longdouble_or_skip()
            self._truth = (fitc_truth(self.X, self.Y, self.H, self.Xu, self.Zt, LD),
                           fitc_truth(self.X, self.Y, self.H, self.Xu, self.Zt, np.float64))
        return self._truth

    def source(self, lib, fitted=True):
        h = Handle(lib, self.X, self.Y)
        if fitted:
            assert np.all(h.fit(self.H) == 0)
        return h


_CASES = {}


def case(lib, **kw):
    key = tuple(sorted(kw.items()))
    if key not in _CASES:
        _CASES[key] = Case(lib, **kw)
    return _CASES[key]


def gate_truth(cs, mean, var, label):
    """Check 1: the device's (mean, var) at cs.Zt against the longdouble value, relative to fp64 numpy's own distance."""
    (m_ld, v_ld), (m_np, v_np) = cs.truth()
    msc = np.max(np.abs(m_ld), axis=0).astype(np.float64)
    e_dev_m = float(np.max(np.abs(mean.astype(LD) - m_ld).astype(np.float64) / msc))
    e_np_m = float(np.max(np.abs(m_np.astype(LD) - m_ld).astype(np.float64) / msc))
    e_dev_v = float(np.max(np.abs(var.astype(LD) - v_ld).astype(np.float64) / cs.sf2))
    e_np_v = float(np.max(np.abs(v_np.astype(LD) - v_ld).astype(np.float64) / cs.sf2))
    print(f'[{label} {cs.label}] mean: device {e_dev_m:.2e}  numpy {e_np_m:.2e} of max|mean|;  '
          f'var: device {e_dev_v:.2e}  numpy {e_np_v:.2e} of sf^2;  min var {np.min(var / cs.sf2):.2e} sf^2')
    DIGITS.append((f'{label} {cs.label}', e_dev_m, e_np_m, e_dev_v, e_np_v))
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(var)), label
    assert e_dev_m <= max(10.0 * e_np_m, 1e-13), (label, e_dev_m, e_np_m)
    assert e_dev_v <= max(10.0 * e_np_v, 1e-13), (label, e_dev_v, e_np_v)
    assert np.all(var >= -1e-12 * cs.sf2), (label, np.min(var / cs.sf2))


def bitwise_factors(f, g):
    return all(np.array_equal(f[k], g[k]) for k in ('hyper', 'chol', 'alpha', 'invK'))


def pseudo_targets(f):
    """Yu = L L^T alpha_u from exported factors, [M x Ny]."""
    return np.stack([f['chol'][a] @ (f['chol'][a].T @ f['alpha'][a]) for a in range(len(f['alpha']))], axis=1)


# ------------------------------------------------------------------------------------------------ checks
def check_truth(lib, chunk=None, fitted=True, **size):
    """1 / 3. predict_mean_var of the sparse handle at 300 points against the truth; `chunk` sets "predict_chunk" for the
    build (the multi-chunk route of the loop over the training points); fitted = False: a source handle that was never
    fitted, with the hyper-parameters given (a size no exact fit is asked for)."""
    cs = case(lib, **size)
    h = cs.source(lib, fitted=fitted)
    if chunk:
        lib.set_tuning('predict_chunk', chunk)
    try:
        s = h.sparse_fitc(cs.Xu, None if fitted else cs.H)
    finally:
        if chunk:
            lib.set_tuning('predict_chunk', 0)
    assert (s.N, s.d, s.Ny) == (cs.M, cs.d, cs.Ny) and np.all(h.info >= 0)
    mean, var = s.predict_mean_var(cs.Zt)
    gate_truth(cs, mean, var, f'chunk={chunk or "default"}')
    s.close()
    h.close()


def check_ordinary_model(lib, **size):
    """2. The exported factors are those of an ordinary model, and every predicting entry point agrees with the oracle's own
    functions evaluated on them."""
    cs = case(lib, **size)
    d, Ny, M, H = cs.d, cs.Ny, cs.M, cs.H
    h = cs.source(lib)
    s = h.sparse_fitc(cs.Xu)
    f = s.get_factors(invK=True)
    assert np.array_equal(f['hyper'], H)
    Xu, Yu = cs.Xu, pseudo_targets(f)
    for a in range(Ny):
        L, iK, al = f['chol'][a], f['invK'][a], f['alpha'][a]
        assert np.array_equal(L, np.tril(L)) and np.all(np.diag(L) > 0)
        T = solve_triangular(L, np.eye(M), lower=True)
        e_ik = np.max(np.abs(iK - T.T @ T)) / np.max(np.abs(iK))
        e_al = np.max(np.abs(al - iK @ Yu[:, a])) / np.max(np.abs(al))
        print(f'[ordinary {cs.label} a={a}] invK vs (L L^T)^-1 {e_ik:.2e}  alpha vs invK Yu {e_al:.2e} (bars 1e-9)  cond(L)^2 {np.linalg.cond(L) ** 2:.2e}')
        assert e_ik <= 1e-9 and e_al <= 1e-9, (a, e_ik, e_al)
    Z, S = cs.Zs, cs.Ss
    sf2 = cs.sf2
    ell_min = H[:, :d].min(axis=1)
    om, ov, oJ = go.mean_var_jac(Z, Xu, H, f['alpha'], f['chol'])
    ms = mean_scale(Xu, Z, H, f['alpha'])
    # gpmpc_predict 'TA' (parity_cases.check_io_pack_boundary) and 'EM' (parity_cases.moment_bars)
    mt, ct = s.predict('TA', Z, S)
    oc = go.ta_cov(ov, oJ, S)
    e = (np.max(np.abs(mt - om) / ms), np.max(np.abs(ct - oc)) / (sf2.max() * max(1.0, np.abs(oc).max())))
    print(f'[ordinary {cs.label}] TA mean {e[0]:.2e} cov {e[1]:.2e} (bars 1e-10)')
    assert e[0] <= 1e-10 and e[1] <= 1e-10, e
    me, ce = s.predict('EM', Z, S)
    moment_bars(f['invK'], Xu, Yu, H, Z, S, em=(me, ce), tol=1e-10)
    # gpmpc_mean_jac and gpmpc_predict_sens (parity_cases.check_sensitivities)
    mj, J = s.mean_jac(Z)
    e = (np.max(np.abs(mj - om) / ms), np.max(np.abs(J - oJ) / (ms / ell_min)[..., None]))
    print(f'[ordinary {cs.label}] mean_jac mean {e[0]:.2e} J {e[1]:.2e} (bars 1e-10)')
    assert e[0] <= 1e-10 and e[1] <= 1e-10, e
    m2, v2, J2, Hm, dvar = s.predict_sens(Z)
    oH, odv = go.mean_var_sens(Z, Xu, H, f['alpha'], f['chol'])
    cond = max(np.linalg.cond(f['chol'][a]) ** 2 for a in range(Ny))
    tol = max(1e-10, 50 * np.finfo(float).eps * cond)                     # u = K^-1 ks is cond-limited
    e = (np.max(np.abs(m2 - om) / ms), np.max(np.abs(v2 - ov) / sf2), np.max(np.abs(J2 - oJ) / (ms / ell_min)[..., None]),
         np.max(np.abs(Hm - oH) / (ms / ell_min ** 2)[..., None, None]), np.max(np.abs(dvar - odv) / (sf2 / ell_min)[None, :, None]))
    print(f'[ordinary {cs.label}] sens mean {e[0]:.2e} var {e[1]:.2e} J {e[2]:.2e} H {e[3]:.2e} (bars 1e-10) dvar {e[4]:.2e} (bar {tol:.1e})')
    assert max(e[:4]) <= 1e-10 and e[4] <= tol, e
    # gpmpc_covar (parity_cases.check_model_fixture) and a 5-step 'TA' roll-out step by step along the device's trajectory
    # (parity_cases.check_rollout_vs_oracle)
    og = go.OracleGP(Xu, Yu, H, f['chol'], f['alpha'], f['invK'], gp_method='TA')
    cv = s.covar(Z[:6])
    e_cv = np.max(np.abs(cv - og.covar(Z[:6])[:Ny]) / sf2[:, None, None])
    print(f'[ordinary {cs.label}] covar {e_cv:.2e} (bar 1e-10)')
    assert e_cv <= 1e-10, e_cv
    T = 5
    x0, U = Z[0, :Ny], 0.3 * Z[:T, Ny:]
    S0 = np.eye(d) * 1e-6
    S0[:Ny, :Ny] = np.diag(H[:, d + 1] ** 2)
    mr, cr = s.rollout('TA', np.concatenate([x0, U[0]]), U, S0)
    mean_prev, Sg = x0.copy(), S0.copy()
    for t in range(T):
        omt, oct_ = og.predict(mean_prev, U[t], Sg)
        em = np.max(np.abs(mr[t] - omt[:, 0])) / max(1.0, np.abs(omt).max())
        ec = np.max(np.abs(cr[t] - oct_)) / max(sf2.max(), np.abs(oct_).max())
        assert em <= 1e-10 and ec <= 1e-9, ('rollout', t, em, ec)
        mean_prev = mr[t]
        Sg[:Ny, :Ny] = cr[t]
    s.close()
    h.close()


def check_fitted_and_unfitted_source(lib, **size):
    """4. An unfitted source with hyper given and a fitted source with hyper = NULL: bit for bit the same sparse model."""
    cs = case(lib, **size)
    h0, h1 = cs.source(lib, fitted=False), cs.source(lib)
    s0, s1 = h0.sparse_fitc(cs.Xu, cs.H), h1.sparse_fitc(cs.Xu)
    assert bitwise_factors(s0.get_factors(invK=True), s1.get_factors(invK=True))
    for x in (s0, s1, h0, h1):
        x.close()


def _raw(lib, h, hyper, M, Xu):
    out = ctypes.c_void_p(12345)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.dll.gpmpc_sparse_fitc(h.h if h is not None else None, p(hyper), M, p(Xu), None, ctypes.byref(out))
    return rc, out.value


def check_argument_errors(lib, **size):
    """5. GPMPC_EINVAL / GPMPC_ENOTFIT with *out == NULL; afterwards the source predicts the same bits.  A duplicated
    inducing point still builds and passes the truth gate."""
    cs = case(lib, **size)
    h = cs.source(lib)
    m0, v0 = h.predict_mean_var(cs.Zt)

    def same_bits():
        m1, v1 = h.predict_mean_var(cs.Zt)
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1)

    big = np.ascontiguousarray(np.vstack([cs.X, cs.X[:1]]))
    for M, Xu in ((0, cs.Xu), (cs.N + 1, big), (cs.M, None)):
        assert _raw(lib, h, None, M, Xu) == (EINVAL, None), M
        same_bits()
    assert lib.dll.gpmpc_sparse_fitc(h.h, None, cs.M, cs.Xu.ctypes.data_as(ctypes.c_void_p), None, None) == EINVAL    # NULL out
    same_bits()
    assert _raw(lib, None, cs.H, cs.M, cs.Xu) == (EINVAL, None)                                                          # NULL h
    fresh = cs.source(lib, fitted=False)
    assert _raw(lib, fresh, None, cs.M, cs.Xu) == (ENOTFIT, None)
    fresh.set_mean_func('const', False)
    Hc = np.hstack([cs.H, np.zeros((cs.Ny, 1))])
    assert _raw(lib, fresh, np.ascontiguousarray(Hc), cs.M, cs.Xu) == (EINVAL, None)                                   # non-zero mean kind
    fresh.close()
    same_bits()
    h.close()
    dup = case(lib, **dict(size, dup=True))
    assert np.array_equal(dup.Xu[0], dup.Xu[1])
    hd = dup.source(lib)
    s = hd.sparse_fitc(dup.Xu)
    gate_truth(dup, *s.predict_mean_var(dup.Zt), 'duplicated inducing point')
    s.close()
    hd.close()


def check_predict_only(lib, **size):
    """6. Every data- or factor-changing call is GPMPC_EINVAL on the sparse handle; predictions before and after are bit for
    bit equal."""
    cs = case(lib, **size)
    h = cs.source(lib)
    s = h.sparse_fitc(cs.Xu)
    m0, v0 = s.predict_mean_var(cs.Zt)
    f = s.get_factors(invK=True)
    H, Z = cs.H, np.ascontiguousarray(cs.Zt[:4])
    Yn = np.zeros((4, cs.Ny))
    calls = {
        'gpmpc_fit': lambda: s.fit(H),
        'gpmpc_fit_predict_mean_var': lambda: s.fit_predict_mean_var(H, Z),
        'gpmpc_append': lambda: s.append(Z, Yn),
        'gpmpc_append_select': lambda: s.append_select(Z, None, 2),
        'gpmpc_remove': lambda: s.remove([0]),
        'gpmpc_nll': lambda: s.nll(0, H[0]),
        'gpmpc_train_multistart': lambda: s.train_multistart(H[:, None, :].copy(), 0.5 * H, 2.0 * H),
        'gpmpc_set_mean_func': lambda: s.set_mean_func('const'),
        'gpmpc_set_factors': lambda: s.set_factors(H, f['chol'], f['alpha']),
    }
    for name, call in calls.items():
        try:
            call()
            assert False, name + ' was not refused'
        except GpmpcError as e:
            assert e.code == EINVAL and 'predict-only' in str(e), (name, str(e))
        assert s.N == cs.M
        m1, v1 = s.predict_mean_var(cs.Zt)
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1), name
    assert bitwise_factors(f, s.get_factors(invK=True))
    s.close()
    h.close()


def check_python(lib, tmp_path, N=200, M=70, d=4, Ny=2, sn=1e-2):
    """7. GP.sparse with normalisation on: predict in raw units is the truth pushed through the same standardisation;
    save_model -> load_model reproduces predict_batch; the default inducing set is the seed-model append_select's; the
    data-changing and training methods raise; M > N raises ValueError."""
    from gp_mpc_amd.gp import GP
    cs = case(lib, N=N, M=M, d=d, Ny=Ny, sn=sn, inducing='greedy')
    rng = np.random.default_rng(99)
    Nu = d - Ny
    meta = dict(meanY=rng.standard_normal(Ny), stdY=rng.uniform(0.5, 2.0, Ny), meanZ=rng.standard_normal(d),
                stdZ=rng.uniform(0.5, 2.0, d))
    meta.update(meanX=meta['meanZ'][:Ny], stdX=meta['stdZ'][:Ny], meanU=meta['meanZ'][Ny:], stdU=meta['stdZ'][Ny:])
    o = go.fit(cs.X, cs.Y, cs.H)
    gp = GP(cs.X, cs.Y, hyper=dict(hyper=cs.H, chol=o['chol'], alpha=o['alpha'], invK=o['invK']), normalize=True, meta=meta,
            xlb=np.zeros(Ny), xub=np.ones(Ny), ulb=np.zeros(Nu), uub=np.ones(Nu), lib=lib, gp_method='ME')
    idx = gp.sparse_default_inducing(M)
    assert np.array_equal(idx, cs.idx) and idx[0] == 0 and len(set(idx.tolist())) == M
    sp = gp.sparse(M)
    assert sp.get_size() == (M, Ny, Nu) and gp.get_size() == (N, Ny, Nu)
    (m_ld, v_ld), (m_np, v_np) = cs.truth()
    msc = np.max(np.abs(m_ld), axis=0).astype(np.float64)
    e_dev, e_np, e_dv, e_nv = 0.0, 0.0, 0.0, 0.0
    for b in range(0, 300, 15):
        zraw = meta['meanZ'] + meta['stdZ'] * cs.Zt[b]
        m, c = sp.predict(zraw[:Ny], zraw[Ny:], np.zeros((d, d)))
        mstd = (m[:, 0] - meta['meanY']) / meta['stdY']
        e_dev = max(e_dev, float(np.max(np.abs(mstd - m_ld[b].astype(np.float64)) / msc)))
        e_np = max(e_np, float(np.max(np.abs((m_np[b] - m_ld[b]).astype(np.float64)) / msc)))
        e_dv = max(e_dv, float(np.max(np.abs(np.diag(c) - v_ld[b].astype(np.float64)) / cs.sf2)))
        e_nv = max(e_nv, float(np.max(np.abs((v_np[b] - v_ld[b]).astype(np.float64)) / cs.sf2)))
    print(f'[python] mean: device {e_dev:.2e} numpy {e_np:.2e};  var: device {e_dv:.2e} numpy {e_nv:.2e}')
    # (the round trip raw -> standardised -> raw costs a few eps of |z| / ell and of |mean| on top of the gate's bar)
    assert e_dev <= max(10.0 * e_np, 1e-13) + 1e-13 and e_dv <= max(10.0 * e_nv, 1e-13) + 1e-13, (e_dev, e_np, e_dv, e_nv)
    # indices and raw points give the same model as the default
    by_idx = gp.sparse(M, inducing=cs.idx.astype(np.int64))
    by_pts = gp.sparse(M, inducing=meta['meanZ'] + meta['stdZ'] * cs.X[cs.idx])
    zr = meta['meanZ'] + meta['stdZ'] * cs.Zt[3]
    a = sp.predict(zr[:Ny], zr[Ny:], np.zeros((d, d)))
    b = by_idx.predict(zr[:Ny], zr[Ny:], np.zeros((d, d)))
    c = by_pts.predict(zr[:Ny], zr[Ny:], np.zeros((d, d)))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.allclose(a[0], c[0], rtol=1e-9, atol=1e-12) and np.allclose(a[1], c[1], rtol=1e-9, atol=1e-12)
    # save -> load
    Zraw = meta['meanZ'] + meta['stdZ'] * cs.Zt[:40]
    Sraw = np.tile(1e-4 * np.eye(d), (40, 1, 1))
    sp.set_method('TA')
    mb, cb = sp.predict_batch(Zraw, Sraw, standardized=False)
    path = str(tmp_path / 'fitc_model')
    sp.save_model(path)
    back = GP.load_model(path, lib=lib)
    back.set_method('TA')
    m2, c2 = back.predict_batch(Zraw, Sraw, standardized=False)
    e = (np.max(np.abs(m2 - mb)) / np.max(np.abs(mb)), np.max(np.abs(c2 - cb)) / np.max(np.abs(cb)))
    print(f'[python] save/load predict_batch: mean {e[0]:.2e} cov {e[1]:.2e} (bar 1e-12)')
    assert e[0] <= 1e-12 and e[1] <= 1e-12, e
    # the rest of the predicting interface runs
    A, Bm = sp.discrete_linearize(Zraw[0, :Ny], Zraw[0, Ny:], Sraw[0])
    assert A.shape == (Ny, Ny) and Bm.shape == (Ny, Nu) and np.all(np.isfinite(A)) and np.all(np.isfinite(Bm))
    assert np.all(np.isfinite(sp.jacobian(cs.Zt[0, :Ny], cs.Zt[0, Ny:], Sraw[0])))
    assert np.all(np.isfinite(sp.covar(cs.Zt[:3])))
    mr, vr = sp.rollout(Zraw[0, :Ny], Zraw[:4, Ny:], methods=['TA', 'ME'])
    assert np.all(np.isfinite(mr)) and np.all(vr >= 0)
    smse, mnlp = sp.validate(meta['meanZ'] + meta['stdZ'] * cs.X[:50], meta['meanY'] + meta['stdY'] * cs.Y[:50], verbose=False)
    assert np.all(np.isfinite(smse)) and np.all(np.isfinite(mnlp))
    # predict-only
    Xn, Yn = Zraw[:3], np.zeros((3, Ny))
    for name, call in (('update_data', lambda: sp.update_data(Xn, Yn)), ('update_data_all', lambda: sp.update_data_all(Xn, Yn)),
                       ('update_data_select', lambda: sp.update_data_select(Xn, Yn)),
                       ('update_data_window', lambda: sp.update_data_window(Xn, Yn, M)),
                       ('remove_data', lambda: sp.remove_data([0])), ('replace_data_all', lambda: sp.replace_data_all(Xn, Yn)),
                       ('optimize', lambda: sp.optimize())):
        try:
            call()
            assert False, name
        except RuntimeError as e:
            assert 'FITC' in str(e), (name, str(e))
    m3, c3 = sp.predict_batch(Zraw, Sraw, standardized=False)
    assert np.array_equal(m3, mb) and np.array_equal(c3, cb)
    for bad in (None, np.arange(N + 1), np.zeros((N + 1, d))):
        try:
            gp.sparse(N + 1, inducing=bad)
            assert False
        except ValueError:
            pass
    for g in (sp, by_idx, by_pts, back, gp):
        g.close()
