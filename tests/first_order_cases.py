"""Gates of the predictive mean ks^T alpha, its Jacobian J = d mean / dz, its Hessian Hm and the off-diagonal 'TA' covariance
J_a Sigma J_b^T against extended-precision values, per route; shared by the emulator tier (tests/test_emu_first_order.py) and the
GPU tier (tests/test_gpu_first_order.py).  docs/first_order_gates.md has the table of cases, routes and bars.

Why: the suite holds these outputs to 1e-10 x (sum_i |alpha_i ks_i|) [/ ell_min, / ell_min^2], which is ~4.5e5 times the error of
a correctly rounded fp64 evaluation: a route that loses four or five digits (a truncated polynomial in the table exponential, a
partial sum through a narrower type, a chunk partial added twice) passes it.

Yardstick (host, longdouble; fixed input): alpha is the DEVICE's own, read back with get_factors() after the fit and taken as
exact fp64 numbers -- the factor gates (factor_cases.py) answer for alpha itself, this gate measures the predict kernels alone and
needs no N x N longdouble matrix.  With ks_i the longdouble kernel by direct differences (parity_cases.longdouble_kernel) and
r_ip = (X_ip - z_p) / ell_p^2:
    mean = sum_i alpha_i ks_i,   J_p = sum_i alpha_i ks_i r_ip,   Hm_pq = sum_i alpha_i ks_i r_ip r_iq - delta_pq mean / ell_p^2,
    TAoff_ab = J_a Sigma J_b^T (a != b; the diagonals are gated by variance_cases.check_moment_methods).
Floors, with y_i = 1/2 sum_k (x_ik - z_k)^2 / ell_k^2:  eps sum_i |summand_i| (1 + y_i)  -- the size of the summands times the
conditioning of exp at its argument; Hm's diagonal adds eps sum_i |alpha_i ks_i| / ell_p^2; TAoff: eps sum_pq |J_a,p| |S_pq| |J_b,q|
plus the J floors propagated through Sigma; a prior mean function adds eps x the absolute values of its own terms.
The yardstick certifies itself: evaluated with the training points in reversed order (and another summation tree) it agrees
with itself to YARDSTICK_SHARE of the floor at every probe.

Numpy's own evaluation (gp_oracle.mean_var_jac / mean_var_sens / ta_cov on the same device alpha) gives E_np.

Gate, per route, output and quantity q in {mean, J, Hm, TAoff}, E_dev = |device - truth|:
    max E_dev <= K_SET[q] max E_np,   rms E_dev <= K_SET[q] rms E_np    (E_np over ALL probes of the model)
    E_dev[i]  <= K_POINT[q] max(E_np[i], floor[i])
and the suite's old bar next to them.  K_SET / K_POINT are measured with numpy against itself (tools/first_order_error_scale.py,
profiles/first_order_error_scale.txt): the same formula with the training points in 32 other orders and with every ks entry moved
by +-2 ulp at random (the accuracy the table exponential documents for itself), over every shape of both tiers; twice the worst
ratio, rounded up.  They are not tuned to the device.

The mean taken from the persistent variance product's fused sums (sum_i V_ij w_i, another formula whose error is bounded by
cond(K) against either alpha) gets the full-truth yardstick instead: parity_cases.longdouble_alpha + longdouble_mean, numpy's
gp_oracle.fit alpha as E_np, the maximum and the rms only ('fused_mean')."""
import time

import numpy as np

import gp_oracle as go
import parity_cases as pc
import variance_cases as vc
from gp_mpc_amd._lib import Handle
from gp_mpc_amd.synthetic import synthetic_problem

LD = np.longdouble
EPS = vc.EPS
NY = vc.NY
NPROBE = vc.N_TRAIN + vc.N_NEAR + vc.N_Z
YARDSTICK_SHARE = 0.01        # the yardstick in another summation order may differ from itself by this share of the floor
# Twice the worst ratio of a reordered / +-2 ulp numpy evaluation to the plain one over the shapes of both tiers, rounded up:
# profiles/first_order_error_scale.txt (tools/first_order_error_scale.py), last lines -- worst ratios 4.58 / 4.06 / 3.72 / 4.37 on
# the maximum and rms (mean / J / Hm / TAoff; fused_mean 4.68), 0.57 / 1.32 / 1.55 / 0.86 per probe.  (The per-probe ratios are
# near 1 because the floor's factor 1 + y_i already covers what an fp64 evaluation of the exponent loses.)
K_SET = {'mean': 10.0, 'J': 9.0, 'Hm': 8.0, 'TAoff': 9.0, 'fused_mean': 10.0}
K_POINT = {'mean': 2.0, 'J': 3.0, 'Hm': 4.0, 'TAoff': 2.0}

# the models of cases 7 and 8 (parity_cases.check_wide_inputs / check_mean_functions: seeds, stretched length scales, N)
EDGE_SIZES = {d: dict(N=130, d=d, sn=0.1, seed=77 + d, stretch=True) for d in (1, 9, 16)}
PRIOR_SIZES = {f: dict(N=150, d=3, sn=0.1, seed=31, mean_func=f) for f in ('const', 'linear', 'polynomial')}

RECORD = []                   # (label, what, max ratio, rms ratio, per-probe ratio) of every gate of this process
f64, dist, rms, windows = vc.f64, vc.dist, vc.rms, vc.windows


def _sum(A, other_order=False):
    """Row sums of A[B, N] (longdouble, contiguous: numpy's pairwise tree).  other_order: the columns reversed and cut at a third
    -- other partial sums, another tree (a mirrored tree alone would repeat the same additions at N = 2^k)."""
    if not other_order:
        return A.sum(axis=1)
    Ar = np.ascontiguousarray(A[:, ::-1])
    k = A.shape[1] // 3
    return Ar[:, :k].sum(axis=1) + Ar[:, k:].sum(axis=1)


def mean_function_longdouble(hyper_row, Z, d, func):
    """m(z), dm/dz, diag d2m/dz2 in longdouble, and the sums of the absolute values of their terms (gp_oracle.mean_function)."""
    B = len(Z)
    Zl, hp = Z.astype(LD), np.asarray(hyper_row, dtype=np.float64).astype(LD)
    m, dm, d2 = np.zeros(B, dtype=LD), np.zeros((B, d), dtype=LD), np.zeros((B, d), dtype=LD)
    am, adm, ad2 = np.zeros(B), np.zeros((B, d)), np.zeros((B, d))
    if func == 'const':
        m += hp[-1]
        am += abs(float(hp[-1]))
    elif func == 'linear':
        a, c = hp[-d - 1:-1], hp[-1]
        m = Zl @ a + c
        am = f64(np.abs(Zl * a).sum(axis=1)) + abs(float(c))
        dm += a
        adm += f64(np.abs(a))
    elif func == 'polynomial':
        a, b, c = hp[-2 * d - 1:-d - 1], hp[-d - 1:-1], hp[-1]
        m = (Zl * Zl) @ a + Zl @ b + c
        am = f64((np.abs(Zl * Zl * a) + np.abs(Zl * b)).sum(axis=1)) + abs(float(c))
        dm = 2 * Zl * a + b
        adm = f64(np.abs(2 * Zl * a) + np.abs(b))
        d2 += 2 * a
        ad2 += f64(np.abs(2 * a))
    return m, dm, d2, am, adm, ad2


class Reference:
    """Truth, floors and numpy's evaluation of one model at one (device) alpha[len(outputs), N]: mean[B, n], J[B, n, d],
    Hm[B, n, d, d] (with want_hm), TA[B, n, n] -- truths longdouble, floors / numpy / mean_scale fp64."""


class Model:
    """One synthetic data set, its 256 probes with the generator's Sigma, and the longdouble parts every alpha shares."""

    def __init__(self, N, d, sn, seed=1234, stretch=False, mean_func='zero'):
        pc._longdouble_or_skip()
        self.N, self.d, self.sn, self.mean_func = N, d, sn, mean_func
        p = synthetic_problem(N, d, NY, NPROBE, seed=seed, sn=sn)       # (its first 128 Z are those of a 128-point call)
        self.X, self.Y, H = p['X'], p['Y'], p['hyper'].copy()
        if stretch:                                                     # parity_cases.check_wide_inputs
            H[:, :d] *= np.linspace(1.5, 3.0, d)[None, :]
        if mean_func != 'zero':                                         # parity_cases.check_mean_functions
            self.Y = self.Y + 0.4 + 0.3 * self.X[:, :1]
            H = np.hstack([H, np.random.default_rng(seed).uniform(-0.3, 0.3, (NY, go.mean_param_count(mean_func, d)))])
        self.H, self.Hk = H, np.ascontiguousarray(H[:, :d + 2])
        self.P = vc.make_probes(self.X, p['Z'], H[0, :d])
        self.S = p['Sigma']
        self.B = len(self.P)
        assert self.B == NPROBE == len(self.S)
        self.ell_min = self.Hk[:, :d].min(axis=1)
        t0 = time.time()
        self.ks, self.R, self.cond = [], [], []
        for a in range(NY):
            ell2 = self.Hk[a, :d].astype(LD) ** 2
            self.ks.append(np.ascontiguousarray(pc.longdouble_kernel(self.X, self.P, self.Hk[a]).T))            # [B, N]
            R = [(self.X[:, k].astype(LD)[None, :] - self.P[:, k].astype(LD)[:, None]) / ell2[k] for k in range(d)]
            self.R.append(R)
            self.cond.append(1.0 + f64(sum(R[k] * R[k] * (ell2[k] / 2) for k in range(d))))                      # 1 + y_i
        self.host_seconds = time.time() - t0
        self._cache, self._certified = {}, set()
        self.label = f'N={N} d={d} sn={sn:g}' + (' stretched' if stretch else '') + ('' if mean_func == 'zero' else f' {mean_func}')

    # -- one output at one alpha
    def _output(self, a, alpha_a, want_hm, other_order=False):
        d, ell2 = self.d, self.Hk[a, :self.d].astype(LD) ** 2
        w = self.ks[a] * alpha_a.astype(LD)[None, :]
        aw, cond, R = f64(np.abs(w)), self.cond[a], self.R[a]
        o = dict(mean=_sum(w, other_order), ms=aw.sum(axis=1), f_mean=EPS * (aw * cond).sum(axis=1))
        o['J'], o['f_J'] = np.zeros((self.B, d), dtype=LD), np.zeros((self.B, d))
        if want_hm:
            o['Hm'], o['f_Hm'] = np.zeros((self.B, d, d), dtype=LD), np.zeros((self.B, d, d))
        for p in range(d):
            wr = w * R[p]
            o['J'][:, p], o['f_J'][:, p] = _sum(wr, other_order), EPS * (f64(np.abs(wr)) * cond).sum(axis=1)
            if want_hm:
                for q in range(p + 1):
                    wrr = wr * R[q]
                    o['Hm'][:, p, q] = o['Hm'][:, q, p] = _sum(wrr, other_order)
                    o['f_Hm'][:, p, q] = o['f_Hm'][:, q, p] = EPS * (f64(np.abs(wrr)) * cond).sum(axis=1)
                o['Hm'][:, p, p] -= o['mean'] / ell2[p]
                o['f_Hm'][:, p, p] += EPS * o['ms'] / float(ell2[p])
        if self.mean_func != 'zero':
            m, dm, d2, am, adm, ad2 = mean_function_longdouble(self.H[a], self.P, d, self.mean_func)
            o['mean'], o['f_mean'] = o['mean'] + m, o['f_mean'] + EPS * am
            o['J'], o['f_J'] = o['J'] + dm, o['f_J'] + EPS * adm
            if want_hm:
                ii = np.arange(d)
                o['Hm'][:, ii, ii] += d2
                o['f_Hm'][:, ii, ii] += EPS * ad2
        return o

    def _certify(self, a, alpha_a, o, want_hm):
        """The yardstick in another summation order: within YARDSTICK_SHARE of the floor at every probe."""
        o2 = self._output(a, alpha_a, want_hm, other_order=True)
        for q in ('mean', 'J') + (('Hm',) if want_hm else ()):
            share = float(np.max(f64(np.abs(o[q] - o2[q])) / o['f_' + q]))
            print(f'[yardstick {self.label} output {a}] {q}: two summation orders differ by {share:.1e} of the floor')
            assert share <= YARDSTICK_SHARE, ('yardstick too coarse', self.label, a, q, share)

    def reference(self, alpha, outputs=None, want_hm=False):
        outs = list(range(NY)) if outputs is None else list(outputs)
        alpha = np.asarray(alpha, dtype=np.float64).reshape(len(outs), self.N)
        key = (tuple(outs), alpha.tobytes(), want_hm)
        if key in self._cache:
            return self._cache[key]
        t0 = time.time()
        r, per = Reference(), []
        for k, a in enumerate(outs):
            o = self._output(a, alpha[k], want_hm)
            if (a, want_hm) not in self._certified:
                self._certify(a, alpha[k], o, want_hm)
                self._certified.add((a, want_hm))
            per.append(o)
        st = lambda name: np.stack([o[name] for o in per], axis=1)
        r.outs = outs
        r.mean, r.J, r.ms, r.f_mean, r.f_J = st('mean'), st('J'), st('ms'), st('f_mean'), st('f_J')
        if want_hm:
            r.Hm, r.f_Hm = st('Hm'), st('f_Hm')
        # J_a Sigma J_b^T and its floor: eps sum |J_a,p| |S_pq| |J_b,q| + the J floors through |Sigma|
        S, aS, aJ = self.S.astype(LD), np.abs(self.S), f64(np.abs(r.J))
        r.TA = np.einsum('bad,bde,bce->bac', r.J, S, r.J)
        r.f_TA = (EPS * np.einsum('bad,bde,bce->bac', aJ, aS, aJ) + np.einsum('bad,bde,bce->bac', r.f_J, aS, aJ)
                  + np.einsum('bad,bde,bce->bac', aJ, aS, r.f_J))
        # numpy on the same alpha (var is not asked for: an identity stands in for the factor)
        eye = np.broadcast_to(np.eye(self.N), (len(outs), self.N, self.N))
        H = self.H[outs]
        r.np_mean, _, r.np_J = go.mean_var_jac(self.P, self.X, H, alpha, eye, True, mean_func=self.mean_func)
        r.np_TA = go.ta_cov(np.zeros((self.B, len(outs))), r.np_J, self.S)
        if want_hm:
            r.np_Hm, _ = go.mean_var_sens(self.P, self.X, self.Hk[outs], alpha, eye)
            if self.mean_func == 'polynomial':
                for k in range(len(outs)):
                    r.np_Hm[:, k] += np.diag(2 * H[k, self.d + 2:2 * self.d + 2])
        r.host_seconds = time.time() - t0
        print(f'[yardstick {self.label}] outputs {outs}{" with Hm" if want_hm else ""}: {r.host_seconds:.1f} s of host time '
              f'(+ {self.host_seconds:.1f} s for the longdouble kernel, once per model)')
        self._cache[key] = r
        return r

    def handle(self, lib, outputs=None):
        """A fitted handle on the model's data (prior mean function added to the prediction)."""
        h = Handle(lib, self.X, self.Y if outputs is None else np.ascontiguousarray(self.Y[:, outputs]))
        if self.mean_func != 'zero':
            h.set_mean_func(self.mean_func, True)
        assert np.all(h.fit(self.H if outputs is None else self.H[outputs]) == 0)
        return h


_MODELS = {}


def model(N, d, sn, seed=1234, stretch=False, mean_func='zero'):
    key = (N, d, sn, seed, stretch, mean_func)
    if key not in _MODELS:
        _MODELS[key] = Model(*key)
    return _MODELS[key]


def device_alpha(h):
    return h.get_factors(chol=False)['alpha']


# ------------------------------------------------------------------------------------------------ the gate
def measures(dev, ref_np, truth, floor, e_np_set=None):
    """(max ratio, rms ratio, per-probe ratio, E_dev max, E_np max) of the module docstring."""
    e_dev, e_np = dist(dev, truth).ravel(), dist(ref_np, truth).ravel()
    e_set = e_np if e_np_set is None else np.ravel(e_np_set)
    r_pt = float('nan')
    if floor is not None:
        r_pt = float(np.max(e_dev / np.maximum(e_np, np.broadcast_to(f64(floor), np.shape(dev)).ravel())))
    return float(e_dev.max() / e_set.max()), float(rms(e_dev) / rms(e_set)), r_pt, float(e_dev.max()), float(e_set.max())


def gate(label, what, dev, ref_np, truth, floor, old_scale, e_np_set=None, per_probe=True):
    """One route, output and quantity: the three measures against K_SET / K_POINT, and the suite's old bar
    |dev - numpy| <= 1e-10 old_scale (old_scale broadcasts against dev)."""
    r_max, r_rms, r_pt, e_dev, e_np = measures(dev, ref_np, truth, floor if per_probe else None, e_np_set)
    old = float(np.max(np.abs(f64(dev) - f64(ref_np)) / old_scale))
    RECORD.append((label, what, r_max, r_rms, r_pt))
    print(f'[{what} vs longdouble] {label}: max E_dev {e_dev:.2e} E_np {e_np:.2e} (ratio {r_max:.2f}, bar {K_SET[what]:g})  rms ratio '
          f'{r_rms:.2f}' + (f'  per probe <= {r_pt:.2f} x max(E_np, floor) (bar {K_POINT[what]:g})' if per_probe else '')
          + f'  old bar: {old:.1e} of its scale')
    assert old <= 1e-10, ('the old bar', label, what, old)
    assert r_max <= K_SET[what], ('maximum over the probes', label, what, r_max)
    assert r_rms <= K_SET[what], ('rms over the probes', label, what, r_rms)
    if per_probe:
        assert r_pt <= K_POINT[what], ('per probe', label, what, r_pt)
    return r_max, r_rms, r_pt


def gate_outputs(m, r, label, rows=None, mean=None, J=None, Hm=None, cov=None):
    """Whatever a route returned -- mean[n, outs], J[n, outs, d], Hm[n, outs, d, d], cov[n, outs, outs] ('TA': its off-diagonal
    entries) -- at the probes `rows` (default: all), every output on its own."""
    rows = np.arange(m.B) if rows is None else np.asarray(rows)
    n = len(r.outs)
    for k, a in enumerate(r.outs):
        lab = f'{label} output {a}'
        # (the old bar of a model with a prior mean is |d mean| <= 1e-10 (mean_scale + 1): check_mean_functions)
        ms = r.ms[rows, k] + (0.0 if m.mean_func == 'zero' else 1.0)
        if mean is not None:
            assert mean.shape == (len(rows), n), (label, mean.shape)
            gate(lab, 'mean', mean[:, k], r.np_mean[rows, k], r.mean[rows, k], r.f_mean[rows, k], ms,
                 e_np_set=dist(r.np_mean[:, k], r.mean[:, k]))
        if J is not None:
            assert J.shape == (len(rows), n, m.d), (label, J.shape)
            gate(lab, 'J', J[:, k], r.np_J[rows, k], r.J[rows, k], r.f_J[rows, k], (ms / m.ell_min[a])[:, None],
                 e_np_set=dist(r.np_J[:, k], r.J[:, k]))
        if Hm is not None:
            assert Hm.shape == (len(rows), n, m.d, m.d), (label, Hm.shape)
            gate(lab, 'Hm', Hm[:, k], r.np_Hm[rows, k], r.Hm[rows, k], r.f_Hm[rows, k], (ms / m.ell_min[a] ** 2)[:, None, None],
                 e_np_set=dist(r.np_Hm[:, k], r.Hm[:, k]))
    if cov is not None and n > 1:
        assert cov.shape == (len(rows), n, n), (label, cov.shape)
        off = ~np.eye(n, dtype=bool)
        sf2 = float(np.max(m.Hk[r.outs, m.d] ** 2))
        gate(f'{label} off-diagonal', 'TAoff', cov[:, off], r.np_TA[rows][:, off], r.TA[rows][:, off], r.f_TA[rows][:, off],
             max(1.0, sf2), e_np_set=dist(r.np_TA[:, off], r.TA[:, off]))


def by_windows(call, m, B, stride=1):
    """call(probe indices of one window) -> tuple of arrays [B, ...], over the windows of B probes (every stride-th): the
    tuple of the stacked results of the probes served, and their indices."""
    out, got = None, np.zeros(m.B, dtype=bool)
    for s in windows(m.B, B)[::stride]:
        res = call(np.arange(s, s + B))
        if out is None:
            out = [np.zeros((m.B,) + np.shape(x)[1:]) for x in res]
        for o, x in zip(out, res):
            o[s:s + B] = x
        got[s:s + B] = True
    return tuple(o[got] for o in out), np.flatnonzero(got)


def no_fused_mean(h):
    """The fixed-input gates are for ks^T alpha: the mean must not have come from the persistent variance product."""
    assert h.counter('persistent_variance_products') == 0


# ------------------------------------------------------------------------------------------------ checks
def check_mean_batch(lib, B, stride=1, **size):
    """Case 1.  gpmpc_predict_mean_var, B probes per call: crosscov_kernel<D, 8, false>, one launch -- partial blocks of eight
    test points (B = 1, 5, 9, 33, 65) and the padding of Bp = 32 k."""
    m = model(**size)
    h = m.handle(lib)
    (mean,), rows = by_windows(lambda ix: (h.predict_mean_var(m.P[ix])[0],), m, B, stride)
    r = m.reference(device_alpha(h))
    no_fused_mean(h)
    h.close()
    gate_outputs(m, r, f'predict_mean_var B={B}', rows=rows, mean=mean)


def check_jac_batch(lib, B, stride=1, **size):
    """Case 2.  gpmpc_mean_jac and gpmpc_predict_jac('TA'), B probes per call: crosscov_kernel<D, 4, true>.  Mean, J, TAoff; the
    mean has the bits of the kernel without the Jacobian (gp_kernels.hpp: 'the same mean bits with and without the Jacobian')."""
    m = model(**size)
    h = m.handle(lib)
    (mean, J), rows = by_windows(lambda ix: h.mean_jac(m.P[ix]), m, B, stride)
    (mean_ta, cov, J_ta), rows_ta = by_windows(lambda ix: h.predict_jac('TA', m.P[ix], m.S[ix]), m, B, stride)
    plain = np.vstack([h.predict_mean_var(m.P[s:s + 64])[0] for s in range(0, m.B, 64)])
    r = m.reference(device_alpha(h))
    no_fused_mean(h)
    h.close()
    assert np.array_equal(mean, plain[rows]) and np.array_equal(mean_ta, plain[rows_ta]), 'mean bits differ with the Jacobian'
    assert np.array_equal(J, J_ta)
    gate_outputs(m, r, f'mean_jac B={B}', rows=rows, mean=mean, J=J)
    gate_outputs(m, r, f"predict_jac('TA') B={B}", rows=rows_ta, mean=mean_ta, J=J_ta, cov=cov)


def check_chunk_route(lib, B, stride=1, **size):
    """Case 3.  Np >= CROSSCOV_CHUNK_MIN_NP and Bp <= 64: the training points in gridDim.z = 8 chunks, partials in cpart,
    crosscov_finish_kernel; without (mean alone) and with J.  The same probes through B = 65 at the same N (one launch, Bp = 96)
    are gated as the comparison; how far the two routes are apart is printed in units of the floor."""
    m = model(**size)
    h = m.handle(lib)

    def mean_only(ix):
        out = np.zeros((len(ix), NY))
        h.predict_mean_var_dev(len(ix), np.ascontiguousarray(m.P[ix]), out, None)
        return (out,)
    (mean,), rows = by_windows(mean_only, m, B, stride)
    (mean_j, J), rows_j = by_windows(lambda ix: h.mean_jac(m.P[ix]), m, B, stride)
    (mean1,), rows1 = by_windows(mean_only, m, 65, stride)
    (mean1_j, J1), _ = by_windows(lambda ix: h.mean_jac(m.P[ix]), m, 65, stride)
    r = m.reference(device_alpha(h))
    no_fused_mean(h)
    h.close()
    assert np.array_equal(mean, mean_j), 'chunk route: mean bits differ with the Jacobian'
    gate_outputs(m, r, f'chunk route B={B}', rows=rows, mean=mean)
    gate_outputs(m, r, f'chunk route B={B} with J', rows=rows_j, mean=mean_j, J=J)
    gate_outputs(m, r, 'one launch B=65', rows=rows1, mean=mean1)
    gate_outputs(m, r, 'one launch B=65 with J', rows=rows1, mean=mean1_j, J=J1)
    both = np.intersect1d(rows, rows1)
    apart = np.abs(mean[np.searchsorted(rows, both)] - mean1[np.searchsorted(rows1, both)]) / r.f_mean[both]
    print(f'[chunk route {m.label} B={B}] eight chunks vs one launch: the means are at most {apart.max():.2f} floors apart')


def check_behind_tail(lib, repeat=5, **size):
    """Case 4a.  The first prediction behind a one-output fit, device pointers, the probe set `repeat` times: the throttled
    alpha-less crosscov launch (B = 1280 > 8 x half the CU count: workgroups walk a second block) + mean_dot_kernel."""
    m = model(**size)
    Z = np.tile(m.P, (repeat, 1))
    B = len(Z)
    h = Handle(lib, m.X, np.ascontiguousarray(m.Y[:, [0]]))
    h.set_pointer_mode(True)
    z, mean, var = pc.DevArray(lib, Z), pc.DevArray(lib, shape=(B, 1)), pc.DevArray(lib, shape=(B, 1))
    n0 = h.counter('predictions_behind_tail')
    assert np.all(h.fit(m.H[[0]]) == 0)
    h.predict_mean_var_dev(B, z.ptr, mean.ptr, var.ptr)
    h.synchronize()
    n1 = h.counter('predictions_behind_tail')
    got = mean.numpy()
    alpha = device_alpha(h)
    no_fused_mean(h)
    for a in (z, mean, var):
        a.free()
    h.close()
    assert n1 == n0 + 1, ('the prediction did not take the route behind the fit\'s tail', n0, n1)
    r = m.reference(alpha, outputs=[0])
    for k in range(repeat):
        gate_outputs(m, r, f'behind the tail, rows {k * m.B}..', mean=got[k * m.B:(k + 1) * m.B])
    assert np.array_equal(got, np.tile(got[:m.B], (repeat, 1))), 'the same probe gave other bits in another block'


def check_fused_fit_predict(lib, repeat=5, **size):
    """Case 4b.  gpmpc_fit_predict_mean_var with device pointers ('fused_fit_predicts' goes up), both outputs."""
    m = model(**size)
    Z = np.tile(m.P, (repeat, 1))
    B = len(Z)
    h = Handle(lib, m.X, m.Y)
    h.set_pointer_mode(True)
    z, mean, var = pc.DevArray(lib, Z), pc.DevArray(lib, shape=(B, NY)), pc.DevArray(lib, shape=(B, NY))
    n0 = h.counter('fused_fit_predicts')
    assert np.all(h.fit_predict_mean_var_dev(m.H, B, z.ptr, mean.ptr, var.ptr) == 0)
    h.synchronize()
    assert h.counter('fused_fit_predicts') == n0 + 1
    got = mean.numpy()
    alpha = device_alpha(h)
    no_fused_mean(h)
    for a in (z, mean, var):
        a.free()
    h.close()
    r = m.reference(alpha)
    for k in range(repeat):
        gate_outputs(m, r, f'fit_predict_mean_var, rows {k * m.B}..', mean=got[k * m.B:(k + 1) * m.B])


_FULL = {}


def full_truth(m):
    """The full-truth yardstick of the mean (alpha refined in longdouble) and numpy's own fit, per output: for the fused mean."""
    if m.label not in _FULL:
        t0 = time.time()
        o = go.fit(m.X, m.Y, m.H, want_invK=False)
        np_mean, _, _ = go.mean_var_jac(m.P, m.X, m.H, o['alpha'], o['chol'], False)
        truth = np.stack([pc.longdouble_mean(m.X, m.H[a], pc.longdouble_alpha(m.X, m.Y[:, a], m.H[a])[0], m.P) for a in range(NY)], axis=1)
        print(f'[full-truth yardstick {m.label}] {time.time() - t0:.1f} s of host time')
        _FULL[m.label] = (truth, np_mean, pc.mean_scale(m.X, m.P, m.H, o['alpha']))
    return _FULL[m.label]


def check_fused_mean(lib, **size):
    """Case 5.  128 x 128 tiles; 'vargemm_persist' 0: the mean of crosscov_kernel (fixed-input gate), then 2: the mean from the
    persistent variance product's fused sums sum_i V_ij w_i -- full-truth yardstick, maximum and rms, both outputs."""
    m = model(**size)
    h = Handle(lib, m.X, m.Y)
    try:
        lib.set_tuning('gemm_tile', 128)
        assert np.all(h.fit(m.H) == 0)
        lib.set_tuning('vargemm_persist', 0)
        m0 = h.predict_mean_var(m.P)[0]
        assert h.counter('persistent_variance_products') == 0
        lib.set_tuning('vargemm_persist', 2)
        m2 = h.predict_mean_var(m.P)[0]
        assert h.counter('persistent_variance_products') >= 1
        alpha = device_alpha(h)
    finally:
        lib.set_tuning('gemm_tile', 0)
        lib.set_tuning('vargemm_persist', -1)
        h.close()
    gate_outputs(m, m.reference(alpha), 'tile GEMM 128, mean of crosscov', mean=m0)
    truth, np_mean, ms = full_truth(m)
    for a in range(NY):
        gate(f'fused mean of vargemm_persist output {a}', 'fused_mean', m2[:, a], np_mean[:, a], truth[:, a], None, ms[:, a], per_probe=False)


def check_sens(lib, B, stride=1, **size):
    """Case 6.  gpmpc_predict_sens, B probes per call: Hm of sens_kernel<D>, and the mean and J it returns."""
    m = model(**size)
    h = m.handle(lib)

    def call(ix):
        mean, _, J, Hm, _ = h.predict_sens(m.P[ix])
        return mean, J, Hm
    (mean, J, Hm), rows = by_windows(call, m, B, stride)
    r = m.reference(device_alpha(h), want_hm=True)
    no_fused_mean(h)
    h.close()
    gate_outputs(m, r, f'predict_sens B={B}', rows=rows, mean=mean, J=J, Hm=Hm)


def check_edges(lib, B=9, stride=1, **size):
    """Cases 7 and 8.  predict_jac('TA') and predict_sens, B probes per call: mean, J, TAoff, Hm -- at the first, a middle and
    the last instantiated input dimension with stretched length scales, or with a prior mean function added (mean_add_kernel)."""
    m = model(**size)
    h = m.handle(lib)
    (mean, cov, J), rows = by_windows(lambda ix: h.predict_jac('TA', m.P[ix], m.S[ix]), m, B, stride)

    def sens(ix):
        mean, _, J, Hm, _ = h.predict_sens(m.P[ix])
        return mean, J, Hm
    (mean_s, J_s, Hm), rows_s = by_windows(sens, m, B, stride)
    r = m.reference(device_alpha(h), want_hm=True)
    no_fused_mean(h)
    h.close()
    gate_outputs(m, r, f"predict_jac('TA') B={B}", rows=rows, mean=mean, J=J, cov=cov)
    gate_outputs(m, r, f'predict_sens B={B}', rows=rows_s, mean=mean_s, J=J_s, Hm=Hm)


def check_rollouts(lib, stride=4, **size):
    """Case 9.  Step 0 of 'TA' roll-outs started at probes with the probe's Sigma: gpmpc_rollout (predict_chunk with one point)
    and gpmpc_rollout_multi with three and 33 trajectories (several points); mean and TAoff."""
    m = model(**size)
    h = m.handle(lib)

    def single(ix):
        mean, cov = h.rollout('TA', m.P[ix[0]], m.P[ix, NY:], m.S[ix[0]])
        return mean[:1], cov[:1]

    def multi(ix):
        mean, cov = h.rollout_multi(['TA'] * len(ix), m.P[ix], m.P[ix][:, None, NY:], m.S[ix])
        return mean[:, 0], cov[:, 0]
    res = [('rollout TA', by_windows(single, m, 1, stride))]
    res += [(f'rollout_multi TA M={M}', by_windows(multi, m, M, st)) for M, st in ((3, stride), (33, max(1, stride // 4)))]
    r = m.reference(device_alpha(h))
    no_fused_mean(h)
    h.close()
    for label, ((mean, cov), rows) in res:
        gate_outputs(m, r, label, rows=rows, mean=mean, cov=cov)
