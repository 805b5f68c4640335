"""Gates of the predictive variance var = sf^2 - |L^-1 ks|^2 against an extended-precision value, shared by the emulator
tier (tests/test_emu_variance.py) and the GPU tier (tests/test_gpu_variance.py).

Why: near the training data the variance is 1e-4 ... 1e-5 of the two terms that are subtracted, and the suite's bar
|var - oracle| <= 1e-10 sf^2 is ~2000 times the error of a correctly rounded fp64 evaluation there: a route that loses a few
digits (a slab summed in lower precision, a partial sum rounded through a narrower type) passes it.

Yardstick: parity_cases.longdouble_variance (longdouble kernel by direct differences, K^-1 ks refined with longdouble
residuals), evaluated once per model and output and shared by every route.  It certifies itself: 4 and 5 refinement steps must
agree to 1/100 of numpy's own error on the same probes.

Probes (256 per model): 64 training points, 64 points at 1e-3 ell from training points, 128 points of the generator's Z.  Two
outputs with different length scales, sn = 1e-2 and 0.1.

Gate, per route and output, E_dev = |device - truth| against E_np = |numpy - truth| (numpy: the oracle's fp64 evaluation of the
same formula, gp_oracle.mean_var_jac / mean_var_sens):
    max E_dev <= K_SET max E_np,   rms E_dev <= K_SET rms E_np    (E_dev over the probes the route was given, E_np over all)
    E_dev[i]  <= K_POINT max(E_np[i], floor[i]),   floor = eps (sf^2 + |L^-1 ks|^2)   (the size of the summands)
K_SET and K_POINT come from numpy against ITSELF with the training points in another order -- the same formula, an equally
good evaluation: twice the worst ratio over 32 orders at the test shapes, rounded up (tools/var_error_scale.py,
profiles/var_error_scale.txt).  They are not tuned to the device.  The suite's 1e-10 sf^2 bar is asserted next to them."""
import numpy as np
from scipy.linalg import solve_triangular

import gp_oracle as go
import parity_cases as pc
from gp_mpc_amd._lib import Handle
from gp_mpc_amd.synthetic import synthetic_problem

EPS = float(np.finfo(np.float64).eps)
NY = 2
N_TRAIN, N_NEAR, N_Z = 64, 64, 128
YARDSTICK_SHARE = 0.01        # the yardstick's 4- and 5-step values may differ by this share of numpy's error
# Twice the worst ratio of a reordered numpy evaluation to the unpermuted one over the shapes of both tiers, rounded up
# (profiles/var_error_scale.txt; worst ratios 2.96 / 1.97 / 2.69 on the maximum and rms, 68.5 / 5280 / 27.3 per probe).  The
# per-probe ratios have a heavy tail: at sn = 1e-2 numpy's typical error, cond(K) eps, is 100 times the floor eps x summands, so
# where numpy's own sum happens to land on the truth a reordered evaluation is that far beyond max(E_np, floor).
K_SET = {'var': 6.0, 'dvar': 4.0, 'cov': 6.0}
K_POINT = {'var': 137.0, 'dvar': 10560.0, 'cov': 55.0}
COVAR_PROBES = np.r_[0:24, 64:88, 128:150]        # 70 probes of the three kinds: beyond one 64-column block

RECORD = []                   # (label, what, max ratio, rms ratio, per-probe ratio) of every gate of this process


def make_probes(X, Z, ell, seed=99):
    """The probe set of a model: rows of X, rows of X displaced by 1e-3 ell in a random direction, rows of Z."""
    rng = np.random.default_rng(seed)
    N, d = X.shape
    at = rng.choice(N, N_TRAIN, replace=False)
    near = rng.choice(N, N_NEAR, replace=False)
    u = rng.standard_normal((N_NEAR, d))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return np.vstack([X[at], X[near] + 1e-3 * ell * u, Z[:N_Z]])


def numpy_covar(X, H, chol, P):
    """sf^2 - V^T V, V = L^-1 ks: what gpmpc_covar returns (gp_class.py:353-381), numpy's fp64 evaluation."""
    d = X.shape[1]
    out = np.zeros((len(H), len(P), len(P)))
    for a in range(len(H)):
        V = solve_triangular(chol[a], go.cov_se_ard_direct(X, P, H[a, :d], H[a, d] ** 2), lower=True)
        out[a] = H[a, d] ** 2 - V.T @ V
    return out


def f64(a):
    return np.asarray(a, dtype=np.float64)


def dist(value, truth):
    """|value - truth| with the difference formed in longdouble."""
    return f64(np.abs(np.asarray(value, dtype=np.float64).astype(np.longdouble) - truth))


def rms(e):
    return float(np.sqrt(np.mean(np.square(e))))


class Truth:
    """Extended-precision values of one output at the probes, and the floors of the per-probe gate."""

    def __init__(self, X, hyper_row, P):
        d = X.shape[1]
        t4, t5 = pc.longdouble_variance(X, hyper_row, P, iters=(4, 5))
        self.t4, self.t5 = t4, t5
        sf2 = float(hyper_row[d]) ** 2
        q = f64(np.diag(t4['quad']))                               # |L^-1 ks|^2 = ks^T K^-1 ks
        self.var, self.dvar = t4['var'], t4['dvar']
        self.covar = np.longdouble(sf2) - t4['quad']               # the quantity gpmpc_covar defines (kss = sf^2 for every pair)
        self.floor = {'var': EPS * (sf2 + q), 'dvar': EPS * f64(t4['dvar_abs']),
                      'cov': EPS * (sf2 + np.sqrt(np.outer(q, q)))}

    def certify(self, label, e_np_var, e_np_dvar, e_np_cov):
        """4 against 5 refinement steps: at most YARDSTICK_SHARE of numpy's own error on the same probes."""
        for what, key, e_np in (('var', 'var', e_np_var), ('dvar', 'dvar', e_np_dvar), ('cov', 'quad', e_np_cov)):
            spread = f64(np.abs(self.t4[key] - self.t5[key]))
            rel = lambda e: float(np.max(e / np.abs(f64(self.var)))) if what == 'var' else float('nan')
            print(f'[yardstick {label}] {what}: 4 vs 5 steps max {spread.max():.2e} (rel. to var {rel(spread):.1e}); '
                  f'numpy max error {e_np.max():.2e} (rel. to var {rel(e_np):.1e})')
            assert spread.max() <= YARDSTICK_SHARE * e_np.max(), ('yardstick too coarse', label, what, spread.max(), e_np.max())
            if what == 'var':
                assert rel(spread) <= YARDSTICK_SHARE * rel(e_np), ('yardstick too coarse (relative)', label, rel(spread), rel(e_np))


class Model:
    """One synthetic data set (N, d, sn, seed), its probes, numpy's evaluation and the truth, for NY outputs."""

    def __init__(self, N, d, sn, seed=1234):
        pc._longdouble_or_skip()
        self.N, self.d, self.sn = N, d, sn
        p = synthetic_problem(N, d, NY, N_Z, seed=seed, sn=sn)
        self.X, self.Y, self.H = p['X'], p['Y'], p['hyper']
        self.sf2 = self.H[:, d] ** 2
        self.P = make_probes(self.X, p['Z'], self.H[0, :d])
        self.B = len(self.P)
        o = go.fit(self.X, self.Y, self.H, want_invK=False)
        self.chol, self.alpha = o['chol'], o['alpha']
        _, self.np_var, _ = go.mean_var_jac(self.P, self.X, self.H, o['alpha'], o['chol'], False)
        _, self.np_dvar = go.mean_var_sens(self.P, self.X, self.H, o['alpha'], o['chol'])
        self.np_cov = numpy_covar(self.X, self.H, o['chol'], self.P[COVAR_PROBES])
        self.truth = [Truth(self.X, self.H[a], self.P) for a in range(NY)]
        ix = np.ix_(COVAR_PROBES, COVAR_PROBES)
        for a, t in enumerate(self.truth):
            t.certify(f'N={N} d={d} sn={sn} output {a}', dist(self.np_var[:, a], t.var), dist(self.np_dvar[:, a], t.dvar),
                      dist(self.np_cov[a], t.covar[ix]))
            lo, hi = f64(t.var[:N_TRAIN]).min() / self.sf2[a], f64(t.var[:N_TRAIN]).max() / self.sf2[a]
            print(f'[model N={N} d={d} sn={sn} output {a}] var/sf^2 at training points {lo:.1e} ... {hi:.1e}')

    def handle(self, lib, outputs=None):
        h = Handle(lib, self.X, self.Y if outputs is None else np.ascontiguousarray(self.Y[:, outputs]))
        assert np.all(h.fit(self.H if outputs is None else self.H[outputs]) == 0)
        return h


_MODELS = {}


def model(N, d, sn, seed=1234):
    key = (N, d, sn, seed)
    if key not in _MODELS:
        _MODELS[key] = Model(*key)
    return _MODELS[key]


# ------------------------------------------------------------------------------------------------ the gate
def gate(label, what, dev, ref_np, truth, floor, sf2=None, e_np_set=None):
    """The three measures of the module docstring for one route and output; dev, ref_np, truth, floor of one shape.  With sf2,
    the suite's bar |dev - numpy| <= 1e-10 sf^2 is asserted as well.  e_np_set: numpy's errors at ALL probes of the model, for
    a route that was given a part of them -- the maximum and rms of numpy are always those of the whole probe set (numpy's
    largest error on a handful of probes is a draw, not a scale).  Returns the three ratios."""
    e_dev, e_np = dist(dev, truth).ravel(), dist(ref_np, truth).ravel()
    floor = np.broadcast_to(f64(floor), np.shape(dev)).ravel()
    e_set = e_np if e_np_set is None else np.ravel(e_np_set)
    r_max, r_rms = e_dev.max() / e_set.max(), rms(e_dev) / rms(e_set)
    r_pt = float(np.max(e_dev / np.maximum(e_np, floor)))
    old = float(np.max(np.abs(f64(dev) - f64(ref_np)))) / sf2 if sf2 is not None else float('nan')
    RECORD.append((label, what, float(r_max), float(r_rms), r_pt))
    print(f'[{what} vs longdouble] {label}: max E_dev {e_dev.max():.2e} E_np {e_set.max():.2e} (ratio {r_max:.2f}, bar {K_SET[what]:g})  '
          f'rms {rms(e_dev):.2e} / {rms(e_set):.2e} (ratio {r_rms:.2f})  per probe <= {r_pt:.2f} x max(E_np, floor) '
          f'(bar {K_POINT[what]:g})  |dev - numpy|/sf^2 {old:.1e}')
    if sf2 is not None:
        assert old <= 1e-10, (label, what, old)
    assert r_max <= K_SET[what], ('maximum over the probes', label, what, r_max)
    assert r_rms <= K_SET[what], ('rms over the probes', label, what, r_rms)
    assert r_pt <= K_POINT[what], ('per probe', label, what, r_pt)
    return float(r_max), float(r_rms), r_pt


def gate_var(m, label, var, rows=None, outputs=None):
    """var[len(rows), outputs] of a route against the truth at the probes `rows` (default: all), every output on its own."""
    rows = np.arange(m.B) if rows is None else np.asarray(rows)
    outs = range(NY) if outputs is None else outputs
    assert var.shape == (len(rows), len(outs)), (label, var.shape)
    for k, a in enumerate(outs):
        t = m.truth[a]
        gate(f'{label} output {a}', 'var', var[:, k], m.np_var[rows, a], t.var[rows], t.floor['var'][rows], m.sf2[a],
             e_np_set=dist(m.np_var[:, a], t.var))


def windows(n, B):
    """Starts of consecutive windows of B of n items; the last one is moved back so that it is a full window."""
    s = list(range(0, n - B + 1, B))
    if n % B:
        s.append(n - B)
    return s


# ------------------------------------------------------------------------------------------------ checks
def check_batch_size(lib, B, stride=1, **size):
    """gpmpc_predict_mean_var with B points per call -- B = 1: var_small_kernel<1>; 5, 32: the small-batch DMA GEMM, 32
    columns; 33, 64: 64 columns; 65: the tile GEMM -- every probe through that route, B at a time (stride: every stride-th
    window only, where a call is slow)."""
    m = model(**size)
    h = m.handle(lib)
    var, rows = by_windows(lambda P: h.predict_mean_var(P)[1], m, B, stride)
    h.close()
    gate_var(m, f'predict_mean_var B={B}', var, rows=rows)


def check_large_batch(lib, **size):
    """All probes in one call with 128 x 128 tiles: one tile per workgroup + var_finish_kernel ('vargemm_persist' 0) and
    vargemm_persist_kernel (2: at any size)."""
    m = model(**size)
    h = Handle(lib, m.X, m.Y)
    try:
        lib.set_tuning('gemm_tile', 128)
        assert np.all(h.fit(m.H) == 0)
        lib.set_tuning('vargemm_persist', 0)
        v0 = h.predict_mean_var(m.P)[1]
        assert h.counter('persistent_variance_products') == 0
        lib.set_tuning('vargemm_persist', 2)
        v2 = h.predict_mean_var(m.P)[1]
        assert h.counter('persistent_variance_products') >= 1
    finally:
        lib.set_tuning('gemm_tile', 0)
        lib.set_tuning('vargemm_persist', -1)
        h.close()
    gate_var(m, 'tile GEMM 128 + var_finish', v0)
    gate_var(m, 'vargemm_persist', v2)


def check_chunked(lib, **size):
    """'predict_chunk' = 64: the probes span four scratch chunks."""
    m = model(**size)
    try:
        lib.set_tuning('predict_chunk', 64)
        h = m.handle(lib)
        var = h.predict_mean_var(m.P)[1]
        h.close()
    finally:
        lib.set_tuning('predict_chunk', 0)
    gate_var(m, 'predict_chunk 64', var)


def check_fused_fit_predict(lib, **size):
    """gpmpc_fit_predict_mean_var with device pointers (the fused route: 'fused_fit_predicts' goes up)."""
    m = model(**size)
    h = Handle(lib, m.X, m.Y)
    h.set_pointer_mode(True)
    z, mean, var = pc.DevArray(lib, m.P), pc.DevArray(lib, shape=(m.B, NY)), pc.DevArray(lib, shape=(m.B, NY))
    n0 = h.counter('fused_fit_predicts')
    assert np.all(h.fit_predict_mean_var_dev(m.H, m.B, z.ptr, mean.ptr, var.ptr) == 0)
    h.synchronize()
    assert h.counter('fused_fit_predicts') == n0 + 1
    v = var.numpy()
    for a in (z, mean, var):
        a.free()
    h.close()
    gate_var(m, 'fit_predict_mean_var', v)


def check_behind_tail(lib, outputs=(0,), **size):
    """The first prediction behind a fit, device pointers ('predictions_behind_tail' goes up).  Only a one-output fit returns at
    the end of its chain kernel (tile-owner workers need a batch of one matrix): the model is output 0 of the shared data set,
    whose truth it reuses."""
    m = model(**size)
    outputs = list(outputs)
    h = Handle(lib, m.X, np.ascontiguousarray(m.Y[:, outputs]))
    h.set_pointer_mode(True)
    z, var = pc.DevArray(lib, m.P), pc.DevArray(lib, shape=(m.B, len(outputs)))
    mean = pc.DevArray(lib, shape=(m.B, len(outputs)))
    n0 = h.counter('predictions_behind_tail')
    assert np.all(h.fit(m.H[outputs]) == 0)
    h.predict_mean_var_dev(m.B, z.ptr, mean.ptr, var.ptr)
    h.synchronize()
    n1 = h.counter('predictions_behind_tail')
    v = var.numpy()
    for a in (z, mean, var):
        a.free()
    h.close()
    assert n1 == n0 + 1, ('the prediction did not take the route behind the fit\'s tail', n0, n1)
    gate_var(m, 'behind the tail', v, outputs=outputs)


def check_moment_methods(lib, **size):
    """gpmpc_predict: the diagonals of 'ME' and of 'TA' with Sigma = 0 (cov = diag(var) + J 0 J^T)."""
    m = model(**size)
    h = m.handle(lib)
    _, c_me = h.predict('ME', m.P)
    _, c_ta = h.predict('TA', m.P, np.zeros((m.B, m.d, m.d)))
    h.close()
    for name, c in (('ME', c_me), ('TA, Sigma = 0', c_ta)):
        gate_var(m, f'predict {name}', np.stack([c[:, a, a] for a in range(NY)], axis=1))
        off = c[:, ~np.eye(NY, dtype=bool)]
        assert np.all(off == 0.0), (name, np.abs(off).max())


def check_sens(lib, sizes=(33, 256), **size):
    """gpmpc_predict_sens: var (the VT route: V^T is kept for the derivative) and dvar = -2 (d ks/dz)^T K^-1 ks against the
    longdouble derivative, numpy's distance from the oracle's analytic dvar; `sizes` probes per call."""
    m = model(**size)
    h = m.handle(lib)
    for B in sizes:
        var, dvar = np.zeros((m.B, NY)), np.zeros((m.B, NY, m.d))
        for s in windows(m.B, B):
            _, v, _, _, dv = h.predict_sens(m.P[s:s + B])
            var[s:s + B], dvar[s:s + B] = v, dv
        gate_var(m, f'predict_sens B={B}', var)
        for a in range(NY):
            t = m.truth[a]
            gate(f'predict_sens B={B} output {a}', 'dvar', dvar[:, a], m.np_dvar[:, a], t.dvar, t.floor['dvar'])
    h.close()


def check_covar(lib, **size):
    """gpmpc_covar on 70 probes (two 64-column blocks): the diagonal under the variance gate, the off-diagonal entries
    sf^2 - v_i^T v_j (gp_class.py:353-381) with the floor eps (sf^2 + |v_i| |v_j|)."""
    m = model(**size)
    h = m.handle(lib)
    cv = h.covar(m.P[COVAR_PROBES])
    h.close()
    ix = np.ix_(COVAR_PROBES, COVAR_PROBES)
    gate_var(m, 'covar diagonal', np.stack([np.diag(cv[a]) for a in range(NY)], axis=1), rows=COVAR_PROBES)
    offd = ~np.eye(len(COVAR_PROBES), dtype=bool)
    for a in range(NY):
        t = m.truth[a]
        gate(f'covar off-diagonal output {a}', 'cov', cv[a][offd], m.np_cov[a][offd], t.covar[ix][offd], t.floor['cov'][ix][offd],
             m.sf2[a])


def by_windows(call, m, B, stride=1):
    """var[B, NY] of call(points) over the windows of B probes (every stride-th window); returns (var of the probes served,
    their indices)."""
    var, got = np.zeros((m.B, NY)), np.zeros(m.B, dtype=bool)
    for s in windows(m.B, B)[::stride]:
        var[s:s + B] = call(m.P[s:s + B])
        got[s:s + B] = True
    return var[got], np.flatnonzero(got)


def check_after_append(lib, N0, stride=1, **size):
    """gpmpc_append of the last N - N0 points onto a fit of the first N0: the truth is that of the whole data set.  All probes
    at once, and 33 and one at a time.  (At N = 330, Np = 384, the strip update serves at most Np / 4 = 96 re-factored rows
    counted from row 64 floor(N0 / 64): N0 = 320 takes it, N0 = 300 and 250 are refits -- api_fit.inl.)"""
    m = model(**size)
    h = Handle(lib, m.X[:N0], m.Y[:N0])
    assert np.all(h.fit(m.H) == 0)
    assert np.all(h.append(m.X[N0:], m.Y[N0:]) == 0) and h.N == m.N
    var = h.predict_mean_var(m.P)[1]
    v33, r33 = by_windows(lambda P: h.predict_mean_var(P)[1], m, 33, stride)
    v1, r1 = by_windows(lambda P: h.predict_mean_var(P)[1], m, 1, 4 * stride)
    h.close()
    gate_var(m, f'after append {N0} + {m.N - N0}', var)
    gate_var(m, f'after append {N0} + {m.N - N0}, B=33', v33, rows=r33)
    gate_var(m, f'after append {N0} + {m.N - N0}, B=1', v1, rows=r1)


def check_after_set_factors(lib, stride=1, **size):
    """gpmpc_set_factors with numpy's factor: L^-1 comes from the inverse-only factor_blocked."""
    m = model(**size)
    h = Handle(lib, m.X, m.Y)
    h.set_factors(m.H, m.chol, m.alpha)
    var = h.predict_mean_var(m.P)[1]
    v1, r1 = by_windows(lambda P: h.predict_mean_var(P)[1], m, 1, 4 * stride)
    h.close()
    gate_var(m, 'after set_factors', var)
    gate_var(m, 'after set_factors, B=1', v1, rows=r1)


def check_rollouts(lib, stride=1, **size):
    """The first-step variance of 'ME' trajectories started at probe points: gpmpc_rollout and gpmpc_rollout_multi with one
    trajectory (the one-column kernel), three and 33 trajectories (the two widths of the batched product)."""
    m = model(**size)
    h = m.handle(lib)
    S0 = np.zeros((m.d, m.d))
    diag = lambda c: np.array([c[a, a] for a in range(NY)])
    v, r = by_windows(lambda P: diag(h.rollout('ME', P[0], P[:, NY:], S0)[1][0])[None, :], m, 1, 4 * stride)
    gate_var(m, 'rollout ME', v, rows=r)
    for M, st in ((1, 4 * stride), (3, stride), (33, 1)):
        v, r = by_windows(lambda P: np.array([diag(c[0]) for c in h.rollout_multi(['ME'] * M, P, P[:, None, NY:], S0)[1]]), m, M, st)
        gate_var(m, f'rollout_multi M={M}', v, rows=r)
    h.close()
