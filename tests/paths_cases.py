"""Checks of the pathwise posterior samples (gpmpc_paths_draw / _get / _eval / _eval_grid / _free, gpmpc_rollout_paths) and of
GP.sample_paths / paths_eval / rollout_paths, shared by the emulator tier (tests/test_emu_paths.py) and the GPU tier
(tests/test_gpu_paths.py).  The numpy restatements of the method live here, library-free, so that tools/paths_error_scale.py
can run them numpy against numpy.

Per output a and path s (standardised units, hyper row (ell, sf, sn)):
    omega_j = eps_j / ell, phi_2j(z) = c cos(omega_j . z), phi_2j+1(z) = c sin(omega_j . z), c = sf sqrt(2 / F);
    v_s = alpha - K^-1 (Phi w_s + sn xi_s);   f_s(z) = m(z) + phi(z) . w_s + sum_i v_s,i k(z, x_i).

Yardsticks.  Weights (check 3): the device's own L and alpha (get_factors) and the call's own draws taken as exact fp64
numbers; truth = longdouble Phi w + sn xi with a longdouble forward and back substitution; E_np = the same in numpy with
scipy's cho_solve on that L; gate per output: max and rms of |v_dev - truth| <= K_W x numpy's.  Evaluation (check 4): the
device's own v, omega, w (paths_get) taken as exact; truth = longdouble kernel by direct differences and longdouble sums;
gates: max and rms of the error over all (s, a) <= K_F x numpy's, per point E_dev <= K_P max(E_np, floor) with
floor = eps (sum_i |k_i v_i| (1 + y_i) + sum_j |phi_j w_j| (1 + |omega_j . z|)) (y_i the kernel's exponent: an fp64
evaluation of exp(-y) or of cos / sin(t) loses eps y resp. eps |t| relative to the summand before any sum is formed), and the
old-style bar 1e-10 (sum_i |k_i v_i| + sum_j |phi_j w_j|) as a backstop.  K_W, K_F, K_P: docs/paths_gates.md
(tools/paths_error_scale.py -> profiles/paths_error_scale.txt), fixed before the first run of the library."""
import numpy as np
from scipy.linalg import cho_solve

import gp_oracle as go
from gp_mpc_amd._lib import EINVAL, ENOTFIT, GpmpcError, Handle
from mc_cases import randn_ref
from parity_cases import mean_scale

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
STREAM_OMEGA, STREAM_W, STREAM_XI = 0x40000000, 0x50000000, 0x60000000

# docs/paths_gates.md: twice the worst numpy-against-numpy ratio over every model of both tiers, rounded up
K_W = 15.0      # path weights: max and rms against cho_solve's
K_F = 21.0      # evaluation: max and rms against numpy's
K_P = 3.0       # evaluation, per point: against max(E_np, floor)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def longdouble_or_skip():
    if np.finfo(LD).nmant < 63:
        import pytest
        pytest.skip(f'longdouble has {np.finfo(LD).nmant} mantissa bits here (x87 80-bit: 63): no yardstick')


# ---------------------------------------------------------------------------------------------------------------------
# the method, restated (dtype = np.float64: numpy's evaluation; LD: the yardstick)
# ---------------------------------------------------------------------------------------------------------------------
def kernel_and_exponent(X, Z, hk, dtype=np.float64):
    """k(z_b, x_i) [B, N] by direct differences, and its exponent y = 1/2 sum_k ((x_k - z_k) / ell_k)^2."""
    d = X.shape[1]
    y = np.zeros((len(Z), len(X)), dtype=dtype)
    for k in range(d):
        diff = (Z[:, k].astype(dtype)[:, None] - X[:, k].astype(dtype)[None, :]) / dtype(hk[k])
        y += diff * diff
    y *= dtype(0.5)
    return dtype(hk[d]) ** 2 * np.exp(-y), y


def features(Z, omega_a, sf, dtype=np.float64):
    """phi(z_b) [B, F] (columns 2j cosine, 2j + 1 sine) and the arguments omega_j . z_b [B, F/2]."""
    F = 2 * omega_a.shape[0]
    arg = Z.astype(dtype) @ omega_a.astype(dtype).T
    phi = np.zeros((len(Z), F), dtype=dtype)
    c = dtype(sf) * np.sqrt(dtype(2.0) / dtype(F))
    phi[:, 0::2], phi[:, 1::2] = c * np.cos(arg), c * np.sin(arg)
    return phi, arg


def eval_own(X, hk, omega_a, w_a, v_a, Z, dtype=np.float64, perm=None, ulp=None):
    """Path s at its own input Z[s]: f[S], and with dtype LD also (floor[S], scale[S]).  perm / ulp: the kernel sum in another
    order of the training points / every kernel value moved by ulp[s, i] in {-2, +2} units in the last place (error scale)."""
    ks, y = kernel_and_exponent(X, Z, hk, dtype)
    phi, arg = features(Z, omega_a, hk[X.shape[1]], dtype)
    if ulp is not None:
        ks = ks * (1.0 + ulp * EPS)
    tk, tf = ks * v_a.astype(dtype), phi * w_a.astype(dtype)
    if perm is not None:
        tk = tk[:, perm]
    f = tk.sum(axis=1) + tf.sum(axis=1)
    if dtype is not LD:
        return f
    ak, af = f64(np.abs(tk)), f64(np.abs(tf))
    floor = EPS * ((ak * (1.0 + f64(y))).sum(axis=1) + (af * (1.0 + np.repeat(np.abs(f64(arg)), 2, axis=1))).sum(axis=1))
    return f, floor, ak.sum(axis=1) + af.sum(axis=1)


def eval_grid(X, hk, omega_a, w_a, v_a, Z, dtype=np.float64):
    """Every path at the common points Z[B]: f[S, B] (LD: also floor and scale [S, B])."""
    ks, y = kernel_and_exponent(X, Z, hk, dtype)                          # [B, N]
    phi, arg = features(Z, omega_a, hk[X.shape[1]], dtype)                # [B, F]
    v, w = v_a.astype(dtype), w_a.astype(dtype)
    if dtype is not LD:
        return v @ ks.T + w @ phi.T
    tk = v[:, None, :] * ks[None, :, :]                                   # [S, B, N]
    tf = w[:, None, :] * phi[None, :, :]
    f = tk.sum(axis=2) + tf.sum(axis=2)
    ak, af = f64(np.abs(tk)), f64(np.abs(tf))
    floor = EPS * ((ak * (1.0 + f64(y))[None]).sum(axis=2) + (af * (1.0 + np.repeat(np.abs(f64(arg)), 2, axis=1))[None]).sum(axis=2))
    return f, floor, ak.sum(axis=2) + af.sum(axis=2)


def ld_solve_lower(L, R, transpose=False):
    """L t = R (or L^T t = R) by substitution in longdouble; L[N, N] lower triangular fp64 taken as exact, R[N, S]."""
    Ll, T, n = L.astype(LD), R.astype(LD).copy(), L.shape[0]
    if not transpose:
        for i in range(n):
            if i:
                T[i] -= Ll[i, :i] @ T[:i]
            T[i] /= Ll[i, i]
    else:
        for i in range(n - 1, -1, -1):
            if i + 1 < n:
                T[i] -= Ll[i + 1:, i] @ T[i + 1:]
            T[i] /= Ll[i, i]
    return T


def weights(X, hk, L, alpha_a, omega_a, w_a, xi_a, dtype=np.float64, route='cho', ulp=None):
    """v[S, N] = alpha - K^-1 (Phi w + sn xi) with K = L L^T.  LD: substitution in longdouble; fp64: scipy's cho_solve on L
    ('cho') or the explicit inverse L^-1 as the library holds it ('inv').  ulp[N, F]: feature values moved by +-2 ulp."""
    d = X.shape[1]
    phi, _ = features(X, omega_a, hk[d], dtype)                           # [N, F]
    if ulp is not None:
        phi = phi * (1.0 + ulp * EPS)
    R = phi @ w_a.astype(dtype).T + dtype(hk[d + 1]) * xi_a.astype(dtype).T          # [N, S]
    if dtype is LD:
        U = ld_solve_lower(L, ld_solve_lower(L, R), transpose=True)
    elif route == 'cho':
        U = cho_solve((L, True), R)
    else:
        Li = np.linalg.inv(L)
        U = Li.T @ (Li @ R)
    return (alpha_a.astype(dtype)[:, None] - U).T


def corr_cov(X, hk, omega_a, P):
    """Closed-form covariance of c = f - mean at the points P for given frequencies (fp64 numpy):
    C~ = k~(P, P) - A k~(X, P) - k~(P, X) A^T + A (k~(X, X) + sn^2 I) A^T,  k~ = phi . phi,  A = ks(P)^T K^-1.
    Returns (C~, A, phi(P), phi(X))."""
    d = X.shape[1]
    K = go.cov_se_ard_direct(X, X, hk[:d], hk[d] ** 2) + hk[d + 1] ** 2 * np.eye(len(X))
    Lk = np.linalg.cholesky(K)
    ks = go.cov_se_ard_direct(X, P, hk[:d], hk[d] ** 2)                   # [N, B]
    A = cho_solve((Lk, True), ks).T                                       # [B, N]
    pP, _ = features(P, omega_a, hk[d])
    pX, _ = features(X, omega_a, hk[d])
    kPX = pP @ pX.T
    C = pP @ pP.T - A @ kPX.T - kPX @ A.T + A @ (pX @ pX.T + hk[d + 1] ** 2 * np.eye(len(X))) @ A.T
    return C, A, pP, pX


def ratios(dev, ref_np, truth):
    """(max ratio, rms ratio, E_dev, E_np) of a device array against numpy's, both measured from the longdouble truth."""
    e_dev, e_np = f64(np.abs(dev.astype(LD) - truth)).ravel(), f64(np.abs(ref_np.astype(LD) - truth)).ravel()
    tiny = np.finfo(float).tiny
    return (e_dev.max() / max(e_np.max(), tiny), np.sqrt((e_dev ** 2).mean()) / max(np.sqrt((e_np ** 2).mean()), tiny),
            e_dev, e_np)


# ---------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------
class Model:
    """go.synthetic_problem on a fitted handle with roll-out inputs as mc_cases.Model builds them."""

    def __init__(self, lib, N, d, Ny, sn=0.1, seed=33, mean_func='zero', T=3):
        p = go.synthetic_problem(N, d, Ny, 8, seed=seed, sn=sn)
        self.lib, self.N, self.d, self.Ny, self.sn, self.T, self.Nu, self.mean_func = lib, N, d, Ny, sn, T, d - Ny, mean_func
        self.X, self.Y, self.Hk = p['X'], p['Y'], p['hyper']
        rng = np.random.default_rng(seed + 1)
        self.H = self.Hk
        if mean_func != 'zero':
            self.Y = self.Y + 0.4
            self.H = np.hstack([self.Hk, rng.uniform(0.2, 0.5, (Ny, go.mean_param_count(mean_func, d)))])
        self.h = Handle(lib, self.X, self.Y)
        if mean_func != 'zero':
            self.h.set_mean_func(mean_func, True)
        assert np.all(self.h.fit(self.H) == 0)
        f = self.h.get_factors()
        self.L, self.alpha = f['chol'], f['alpha']
        Nu = self.Nu
        self.z0 = p['Z'][0].copy()
        self.U = 0.3 * rng.standard_normal((T, max(Nu, 0)))
        self.Kz, self.k0 = 0.05 * rng.standard_normal((max(Nu, 0), Ny)), 0.05 * rng.standard_normal(max(Nu, 0))
        self.sa, self.sb = 1.0 - 0.05 * rng.random(Ny), 0.02 * rng.standard_normal(Ny)
        semi = np.zeros((d, d))
        semi[:Ny, :Ny] = np.diag(self.Hk[:, d + 1] ** 2)
        self.Sigma = {'full': p['Sigma'][0], 'semi': semi}
        self.label = f'N={N} d={d} Ny={Ny} sn={sn:g}'

    def factor(self, which):
        if which != 'semi':
            return np.linalg.cholesky(self.Sigma[which])
        L = np.zeros((self.d, self.d))
        L[:self.Ny, :self.Ny] = np.diag(self.Hk[:, self.d + 1])
        return L

    def draws(self, seed, S, F):
        """The generator's arrays of a draw (gpmpc_randn): eps_omega[Ny, F/2, d], w[Ny, S, F], xi[Ny, S, N]."""
        r = self.lib.randn
        return (np.stack([r(seed, STREAM_OMEGA + a, F // 2, self.d) for a in range(self.Ny)]),
                np.stack([r(seed, STREAM_W + a, S, F) for a in range(self.Ny)]),
                np.stack([r(seed, STREAM_XI + a, S, self.N) for a in range(self.Ny)]))

    def roll(self, closed=False, noise=False, sigma='full', **kw):
        a = dict(Kz=self.Kz, k0=self.k0) if closed else dict(U=self.U)
        return self.h.rollout_paths(self.T, self.z0, self.Sigma[sigma], sa=self.sa, sb=self.sb, noise=noise, return_particles=True,
                                    **a, **kw)

    def close(self):
        self.h.close()


_MODELS = {}


def model(lib, **kw):
    key = (id(lib), tuple(sorted(kw.items())))
    if key not in _MODELS:
        _MODELS[key] = Model(lib, **kw)
    return _MODELS[key]


def close_models():
    for m in _MODELS.values():
        m.close()
    _MODELS.clear()


A = dict(N=130, d=3, Ny=2, sn=0.1)
B1 = dict(N=330, d=4, Ny=2, sn=0.1)
B2 = dict(N=330, d=4, Ny=2, sn=1e-2)
C1 = dict(N=130, d=1, Ny=1, sn=0.1)
C16 = dict(N=130, d=16, Ny=1, sn=0.1)
BIG = dict(N=1024, d=4, Ny=2, sn=0.1)            # GPU tier only: the large GEMM tiles


# ---------------------------------------------------------------------------------------------------------------------
# 1. generator path = array path
# ---------------------------------------------------------------------------------------------------------------------
def check_generator_path_equals_array_path(lib, S, F, seed=0xDEADBEEFCAFEF00D, **size):
    md = model(lib, **size)
    h, Ny, d = md.h, md.Ny, md.d
    Z = np.random.default_rng(3).standard_normal((S, d))

    def everything():
        g = h.paths_get()
        out = [g['omega'], g['w'], g['v'], h.paths_eval(Z)]
        for closed, noise in ((False, True), (True, False)):
            out += list(md.roll(closed=closed, noise=noise, seed=seed))
        return out
    h.paths_draw(S, F, seed=seed)
    a = everything()
    eo, w, xi = md.draws(seed, S, F)
    for o in range(Ny):                                  # bitwise against gpmpc_randn, rtol 1e-13 against numpy
        assert np.array_equal(a[0][o], eo[o] / md.Hk[o, :d]), o
        assert np.array_equal(a[1][o], w[o]), o
        assert np.allclose(a[0][o], randn_ref(seed, STREAM_OMEGA + o, F // 2, d) / md.Hk[o, :d], rtol=1e-13, atol=0)
        assert np.allclose(a[1][o], randn_ref(seed, STREAM_W + o, S, F), rtol=1e-13, atol=0)
        assert np.allclose(xi[o], randn_ref(seed, STREAM_XI + o, S, md.N), rtol=1e-13, atol=0)
    h.paths_draw(S, F, seed=99, eps_omega=eo, w=w, xi=xi)          # (seed unused for the arrays; the roll-outs keep theirs)
    b = everything()
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), [np.array_equal(x, y) for x, y in zip(a, b)]
    h.paths_draw(S, F, seed=seed)
    c = everything()
    assert all(np.array_equal(x, y) for x, y in zip(a, c))
    h.paths_draw(S, F, seed=seed + 1)
    assert not np.array_equal(h.paths_get()['v'], a[2])
    assert np.all(np.isfinite(a[2])) and np.all(np.isfinite(a[3]))
    print(f'[paths {md.label} S={S} F={F}] generator path = array path = repeated call, bit for bit')


# ---------------------------------------------------------------------------------------------------------------------
# 2. zero draw = the predictive mean
# ---------------------------------------------------------------------------------------------------------------------
def check_zero_draw(lib, S, F, mean_func='zero', **size):
    md = model(lib, mean_func=mean_func, **size)
    h = md.h
    h.paths_draw(S, F, seed=1, w=np.zeros((md.Ny, S, F)), xi=np.zeros((md.Ny, S, md.N)))
    Z = np.random.default_rng(4).standard_normal((S, md.d))
    f = h.paths_eval(Z)
    m, _ = h.predict_mean_var(Z)
    bar = 1e-10 * (mean_scale(md.X, Z, md.Hk, md.alpha) + (0.0 if mean_func == 'zero' else 1.0))
    r = np.max(np.abs(f - m) / bar)
    g = h.paths_eval_grid(Z[:5])
    rg = np.max(np.abs(g - m[None, :5]) / bar[None, :5])
    print(f'[paths {md.label} mean {mean_func}] zero draw against predict_mean_var: own inputs {r:.2e}, grid {rg:.2e} of the bar')
    assert r <= 1.0 and rg <= 1.0, (r, rg)


# ---------------------------------------------------------------------------------------------------------------------
# 3. path weights, 4. evaluation: against extended precision
# ---------------------------------------------------------------------------------------------------------------------
def check_weights(lib, S, F, seed=11, cols=None, **size):
    """cols: the paths whose truth is formed (the substitution is column by column; None: all)."""
    longdouble_or_skip()
    md = model(lib, **size)
    md.h.paths_draw(S, F, seed=seed)
    g = md.h.paths_get()
    _, _, xi = md.draws(seed, S, F)
    cols = np.arange(S) if cols is None else np.asarray(cols)
    for a in range(md.Ny):
        args = (md.X, md.Hk[a], md.L[a], md.alpha[a], g['omega'][a] , g['w'][a][cols], xi[a][cols])
        truth = weights(*args, dtype=LD)
        r_max, r_rms, e_dev, e_np = ratios(g['v'][a][cols], weights(*args), truth)
        print(f'[weights {md.label} S={S} F={F} output {a}] max |dv| {e_dev.max():.2e} (numpy {e_np.max():.2e}): '
              f'{r_max:.2f} x numpy, rms {r_rms:.2f} x (bar {K_W:g})')
        assert r_max <= K_W and r_rms <= K_W, (a, r_max, r_rms)


def gate_eval(label, dev, ref_np, truth, floor, scale):
    r_max, r_rms, e_dev, e_np = ratios(dev, ref_np, truth)
    r_pt = float(np.max(e_dev / np.maximum(e_np, floor.ravel())))
    r_old = float(np.max(e_dev / (1e-10 * scale.ravel())))
    print(f'[eval {label}] max |df| {e_dev.max():.2e} (numpy {e_np.max():.2e}): {r_max:.2f} x numpy, rms {r_rms:.2f} x (bar {K_F:g}); '
          f'per point {r_pt:.2f} x max(E_np, floor) (bar {K_P:g}); {r_old:.1e} of the 1e-10 bar')
    assert r_max <= K_F and r_rms <= K_F and r_pt <= K_P and r_old <= 1.0, (label, r_max, r_rms, r_pt, r_old)
    return r_pt


def check_eval(lib, S, F, seed=12, **size):
    longdouble_or_skip()
    md = model(lib, **size)
    md.h.paths_draw(S, F, seed=seed)
    g = md.h.paths_get()
    Z = np.random.default_rng(6).standard_normal((S, md.d))
    f = md.h.paths_eval(Z)
    for a in range(md.Ny):
        args = (md.X, md.Hk[a], g['omega'][a], g['w'][a], g['v'][a], Z)
        truth, floor, scale = eval_own(*args, dtype=LD)
        gate_eval(f'{md.label} S={S} F={F} output {a}', f[:, a], eval_own(*args), truth, floor, scale)


def check_eval_grid(lib, S, F, Bs=(1, 33, 65), seed=13, **size):
    longdouble_or_skip()
    md = model(lib, **size)
    md.h.paths_draw(S, F, seed=seed)
    g = md.h.paths_get()
    for B in Bs:
        Z = np.random.default_rng(7 + B).standard_normal((B, md.d))
        f = md.h.paths_eval_grid(Z)
        assert f.shape == (S, B, md.Ny)
        for a in range(md.Ny):
            args = (md.X, md.Hk[a], g['omega'][a], g['w'][a], g['v'][a], Z)
            truth, floor, scale = eval_grid(*args, dtype=LD)
            gate_eval(f'grid {md.label} S={S} F={F} B={B} output {a}', f[:, :, a], eval_grid(*args), truth, floor, scale)


# ---------------------------------------------------------------------------------------------------------------------
# 5. roll-out replay (teacher forcing)
# ---------------------------------------------------------------------------------------------------------------------
VARIANTS = ((False, False, 'full'), (True, True, 'full'), (False, True, 'semi'), (True, False, 'semi'))


def check_rollout_replay(lib, S, F, seed=14, **size):
    """Path s evaluated at the device's own inputs step by step: check 4's per-point gate on every y (+ |eps| 1e-13 sn for the
    noise term); moments against numpy.mean / numpy.cov at mc_cases.check_moments' tolerance (1e-12 max|.|)."""
    longdouble_or_skip()
    md = model(lib, **size)
    md.h.paths_draw(S, F, seed=seed)
    g = md.h.paths_get()
    rng = np.random.default_rng(5)
    T, d, Ny = md.T, md.d, md.Ny
    for closed, noise, sigma in VARIANTS:
        eps0, eps = rng.standard_normal((S, d)), rng.standard_normal((T, S, Ny))
        mean, cov, P = md.roll(closed=closed, noise=noise, sigma=sigma, eps0=eps0, eps=eps)
        Zt = md.z0 + eps0 @ md.factor(sigma).T
        worst = 0.0
        for t in range(T):
            for a in range(Ny):
                args = (md.X, md.Hk[a], g['omega'][a], g['w'][a], g['v'][a], Zt)
                truth, floor, _ = eval_own(*args, dtype=LD)
                nz = md.Hk[a, d + 1] * eps[t, :, a] if noise else np.zeros(S)
                e_np = f64(np.abs(eval_own(*args).astype(LD) - truth))
                e_dev = f64(np.abs(P[t][:, a].astype(LD) - (truth + nz.astype(LD))))
                bar = K_P * np.maximum(e_np, floor) + np.abs(nz) * 1e-13
                worst = max(worst, float(np.max(e_dev / bar)))
            if t + 1 < T:
                u = P[t] @ md.Kz.T + md.k0 if closed else np.tile(md.U[t + 1], (S, 1))
                Zt = np.hstack([md.sa * P[t] + md.sb, u])
            rm, rc = P[t].mean(axis=0), np.cov(P[t], rowvar=False, ddof=1).reshape(Ny, Ny)
            assert np.abs(mean[t] - rm).max() <= 1e-12 * np.abs(rm).max(), (t, 'mean')
            assert np.abs(cov[t] - rc).max() <= 1e-12 * np.abs(rc).max(), (t, 'cov')
        print(f'[roll-out replay {md.label} S={S} closed={closed} noise={noise} Sigma0={sigma}] worst |dy| / bar {worst:.2f}')
        assert worst <= 1.0, (closed, noise, sigma, worst)
        m2, c2 = md.h.rollout_paths(T, md.z0, md.Sigma[sigma], sa=md.sa, sb=md.sb, noise=noise, eps0=eps0, eps=eps,
                                    **(dict(Kz=md.Kz, k0=md.k0) if closed else dict(U=md.U)))
        assert np.array_equal(m2, mean) and np.array_equal(c2, cov)          # without the particle record: the same bits
    # the same seed gives gpmpc_rollout_mc's initial particles: with noise 0 and T = 1 the step-0 inputs are those of stream 0
    P0 = md.roll(seed=21)[2][0]
    Z0 = md.z0 + lib.randn(21, 0, S, d) @ md.factor('full').T
    assert np.allclose(P0, md.h.paths_eval(Z0), rtol=0, atol=1e-12 * np.abs(P0).max())


# ---------------------------------------------------------------------------------------------------------------------
# 6. distribution: consistent paths, not independent draws
# ---------------------------------------------------------------------------------------------------------------------
DIST_SEED = 2024
DIST_S, DIST_F = 4096, 64


def dist_probes(d):
    P = np.random.default_rng(77).standard_normal((8, d))
    P[1] = P[0] + 0.05 * np.eye(d)[0]
    return P


def dist_ratios(c, C):
    """c[S, B]: samples of the correction at the probes; C: its closed-form covariance.  (mean ratio, worst covariance
    ratio, correlation of probes 0 and 1) in standard errors sqrt(C_pp / S) resp. sqrt((C_pp C_qq + C_pq^2) / (S - 1))."""
    S = c.shape[0]
    rm = np.max(np.abs(c.mean(axis=0)) / np.sqrt(np.diag(C) / S))
    cs = np.cov(c, rowvar=False, ddof=1)
    se = np.sqrt((np.outer(np.diag(C), np.diag(C)) + C * C) / (S - 1))
    return float(rm), float(np.max(np.abs(cs - C) / se)), float(cs[0, 1] / np.sqrt(cs[0, 0] * cs[1, 1]))


def numpy_dist_ratios(seed=DIST_SEED, S=DIST_S, F=DIST_F, **size):
    """The CPU pre-check of DIST_SEED: the correction c = phi(P) w - A (Phi w + sn xi) in numpy with the restated
    generator's normals.  No library involved.  Per output (mean ratio, covariance ratio, correlation)."""
    p = go.synthetic_problem(size['N'], size['d'], size['Ny'], 8, seed=33, sn=size['sn'])
    X, H, d = p['X'], p['hyper'], size['d']
    P, out = dist_probes(d), []
    for a in range(size['Ny']):
        om = randn_ref(seed, STREAM_OMEGA + a, F // 2, d) / H[a, :d]
        w, xi = randn_ref(seed, STREAM_W + a, S, F), randn_ref(seed, STREAM_XI + a, S, size['N'])
        C, Am, pP, pX = corr_cov(X, H[a], om, P)
        c = w @ pP.T - (w @ pX.T + H[a, d + 1] * xi) @ Am.T
        out.append(dist_ratios(c, C))
    return out


def check_distribution(lib, **size):
    md = model(lib, **size)
    h, S, F = md.h, DIST_S, DIST_F
    h.paths_draw(S, F, seed=DIST_SEED)
    P = dist_probes(md.d)
    f = h.paths_eval_grid(P)
    m, _ = h.predict_mean_var(P)
    om = h.paths_get(w=False, v=False)['omega']
    for a in range(md.Ny):
        C = corr_cov(md.X, md.Hk[a], om[a], P)[0]
        rm, rc, rho = dist_ratios(f[:, :, a] - m[None, :, a], C)
        print(f'[distribution {md.label} output {a}] mean within {rm:.2f}, covariance within {rc:.2f} standard errors (bar 5); '
              f'correlation of the two close probes {rho:.4f} (bar 0.9)')
        assert rm <= 5.0 and rc <= 5.0 and rho > 0.9, (a, rm, rc, rho)


# ---------------------------------------------------------------------------------------------------------------------
# 8. staleness and errors, 9. Python surface
# ---------------------------------------------------------------------------------------------------------------------
def _raises(code, call, label):
    try:
        call()
    except GpmpcError as e:
        assert e.code == code, (label, e)
    else:
        raise AssertionError(f'{label}: no error')


def check_staleness_and_errors(lib, S=96, F=6, **size):
    md = Model(lib, **size)                              # (its own handle: the data changes)
    h, d, Ny = md.h, md.d, md.Ny
    Zp = np.random.default_rng(8).standard_normal((7, d))
    Z = np.random.default_rng(9).standard_normal((S, d))
    roll = lambda: md.roll(seed=1)

    def stale(label):
        _raises(EINVAL, lambda: h.paths_eval(Z), label + ': paths_eval')
        _raises(EINVAL, roll, label + ': rollout_paths')
        _raises(EINVAL, lambda: h.paths_eval_grid(Zp), label + ': paths_eval_grid')
        h.paths_draw(S, F, seed=2)
        assert np.all(np.isfinite(h.paths_eval(Z))) and np.all(np.isfinite(roll()[0]))
    stale('no paths yet')
    ref = h.predict_mean_var(Zp)
    good = h.paths_eval(Z)
    for label, call in {'S = 0': lambda: h.paths_draw(0, F), 'S = 2^20 + 1': lambda: h.paths_draw((1 << 20) + 1, F),
                        'F odd': lambda: h.paths_draw(S, 7), 'F = 0': lambda: h.paths_draw(S, 0),
                        'F = 65538': lambda: h.paths_draw(S, 65538)}.items():
        _raises(EINVAL, call, label)
        again = h.predict_mean_var(Zp)
        assert np.array_equal(again[0], ref[0]) and np.array_equal(again[1], ref[1]), label
        assert np.array_equal(h.paths_eval(Z), good), label          # earlier paths stay valid
    h.fit(md.H)
    stale('after fit')
    xn, yn = np.random.default_rng(10).standard_normal((3, d)), np.random.default_rng(11).standard_normal((3, Ny))
    h.append(xn, yn)
    Z = np.random.default_rng(9).standard_normal((S, d))
    stale('after append')
    h.remove([0, 5])
    stale('after remove')
    f = h.get_factors()
    h.set_factors(f['hyper'], f['chol'], f['alpha'])
    stale('after set_factors')
    h.paths_free()
    _raises(EINVAL, lambda: h.paths_eval(Z), 'after paths_free')
    h2 = Handle(lib, md.X, md.Y)                          # no factors
    _raises(ENOTFIT, lambda: h2.paths_draw(S, F), 'unfitted: paths_draw')
    _raises(ENOTFIT, lambda: h2.paths_eval(Z), 'unfitted: paths_eval')
    h2.close()
    from gp_mpc_amd.gp import GP
    o = go.fit(md.X, md.Y, md.Hk)
    gp = GP(md.X, md.Y, hyper=dict(hyper=md.Hk, chol=o['chol'], alpha=o['alpha'], invK=o['invK']), normalize=False,
            gp_method='ME', lib=lib)
    sp = gp.sparse(32)
    before = sp.handle.predict_mean_var(Zp)
    _raises(EINVAL, lambda: sp.handle.paths_draw(S, F), 'FITC handle')
    after = sp.handle.predict_mean_var(Zp)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    sp.close()
    gp.close()
    md.close()


def check_python_surface(lib, tank, Nt=4, S=64, F=16):
    from gp_mpc_amd.gp import GP
    g = tank
    hyper = dict(hyper=g['hyper'], chol=g['chol'], alpha=g['alpha'], invK=g['invK'])
    gp = GP(g['X'], g['Y'], hyper=hyper, gp_method='ME', normalize=True, lib=lib, meta=g['meta'], xlb=g['xlb'], xub=g['xub'],
            ulb=g['ulb'], uub=g['uub'])
    N, Ny, Nu = gp.get_size()
    Nx = Ny + Nu
    meta = g['meta']
    x0 = meta['meanX'] + 0.3 * meta['stdX']
    u = np.tile(meta['meanU'] - 0.2 * meta['stdU'], (Nt, 1)) * (1.0 + 0.05 * np.arange(Nt))[:, None]
    gp.sample_paths(S, F, seed=3)
    zstd = np.random.default_rng(1).standard_normal((S, Nx)) * 0.5
    Zraw = zstd * np.asarray(meta['stdZ']) + np.asarray(meta['meanZ'])
    f = gp.paths_eval(Zraw)
    fg = gp.paths_eval(Zraw[:5], grid=True)
    assert f.shape == (S, Ny) and fg.shape == (S, 5, Ny)
    fs = gp.handle.paths_eval(zstd)                                    # units: un-standardised like predict_batch
    fu = fs * np.asarray(meta['stdY']) + np.asarray(meta['meanY'])      # (Zraw -> standardised is zstd to rounding only)
    assert np.allclose(f, fu, rtol=0, atol=1e-10 * np.abs(fu).max()), np.abs(f - fu).max()
    assert np.allclose(fg[np.arange(5), np.arange(5)], f[:5], rtol=1e-9, atol=1e-9 * np.abs(f).max())
    m, v, P = gp.rollout_paths(x0, u, S=S, F=F, seed=5, return_particles=True)
    assert m.shape == (Nt + 1, Ny) and v.shape == (Nt + 1, Ny) and P.shape == (Nt, S, Ny)
    assert np.array_equal(m[0], x0) and np.all(v[0] == 0) and np.all(v[1:] > 0) and np.all(np.isfinite(P))
    # against Handle.rollout_paths on the same draw, standardised by hand as GP.rollout_mc does
    stdX, meanX, stdU, meanU = (np.atleast_1d(meta[k]) for k in ('stdX', 'meanX', 'stdU', 'meanU'))
    stdY, meanY = np.atleast_1d(meta['stdY']), np.atleast_1d(meta['meanY'])
    covar = np.eye(Nx) * 1e-6
    covar[:Ny, :Ny] = np.diag(g['hyper'][:, Nx + 1] ** 2)
    Us = (u - meanU) / stdU
    gp.handle.paths_draw(S, F, seed=5)
    hm, hc, hP = gp.handle.rollout_paths(Nt, np.concatenate([(x0 - meanX) / stdX, Us[0]]), covar, U=Us, sa=stdY / stdX,
                                         sb=(meanY - meanX) / stdX, seed=5, return_particles=True)
    assert np.allclose(P, hP * stdY + meanY, rtol=1e-13, atol=0) and np.allclose(m[1:], hm * stdY + meanY, rtol=1e-13, atol=0)
    base = gp.predict_compare(x0, u, methods=['ME'])
    both = gp.predict_compare(x0, u, methods=['ME'], mc=S, mc_paths=F)
    assert sorted(both) == sorted(list(base) + ['mc_mean', 'mc_var']) and np.array_equal(both['mean'], base['mean'])
    assert both['mc_mean'].shape == (Nt + 1, Ny) and np.all(np.isfinite(both['mc_mean'])) and np.all(both['mc_var'][1:] > 0)
    indep = gp.predict_compare(x0, u, methods=['ME'], mc=S)
    assert not np.array_equal(indep['mc_mean'], both['mc_mean'])      # the default is still rollout_mc
    sp = gp.sparse(32)
    for call in (lambda: sp.sample_paths(S, F), lambda: sp.paths_eval(Zraw), lambda: sp.rollout_paths(x0, u, S=S, F=F)):
        try:
            call()
        except RuntimeError as e:
            assert 'FITC' in str(e)
        else:
            raise AssertionError('a sparse object did not refuse')
    sp.close()
    gp.close()
