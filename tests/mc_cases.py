"""Checks of gpmpc_rollout_mc / gpmpc_randn (Monte Carlo roll-outs: S particles through the GP on the device) and of
GP.rollout_mc / predict_compare(mc=...), shared by the emulator tier (tests/test_emu_mc.py) and the GPU tier
(tests/test_gpu_mc.py).

Yardsticks: an independent numpy Philox-4x32-10 + Box-Muller (below) for the generator; oracle.gp_oracle.mean_var_jac, fed
with the device's OWN particle inputs step by step (teacher forcing: nothing is amplified through the dynamics), for the
propagation; numpy.mean / numpy.cov for the moments; gpmpc_predict('EM') for one step's distribution.  The replay bars are
the ones the mean / variance parity checks apply to gpmpc_predict_mean_var (parity_cases: |dmean| <= 1e-10 sum_i |ks_i alpha_i|,
+ 1e-10 with a mean function added; |dvar| <= 1e-10 sf^2), carried through y = m + sqrt(v) eps to first order:
|dy| <= b_m + |eps| b_v / (2 sqrt(max(v + noise sn^2, b_v)))."""
import ctypes

import numpy as np

import gp_oracle as go
from gp_mpc_amd._lib import EINVAL, GpmpcError, Handle
from parity_cases import mean_scale

# ---------------------------------------------------------------------------------------------------------------------
# the generator, restated: Philox-4x32-10 (Salmon et al., SC'11), key = halves of the seed, counter = (row, pair, stream, 0)
# ---------------------------------------------------------------------------------------------------------------------
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Arrays (or scalars) of 32-bit words -> the four output words, as uint64 arrays holding 32-bit values."""
    c = [np.asarray(x, dtype=np.uint64) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c


def randn_ref(seed, stream, rows, cols):
    pairs = (cols + 1) // 2
    r, j = np.meshgrid(np.arange(rows, dtype=np.uint64), np.arange(pairs, dtype=np.uint64), indexing='ij')
    w = philox4x32_10(r, j, np.uint64(stream), np.uint64(0), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    sh5, sh6 = np.uint64(5), np.uint64(6)
    u1 = ((w[0] >> sh5).astype(np.float64) * 67108864.0 + (w[1] >> sh6).astype(np.float64) + 1.0) * 2.0 ** -53
    u2 = ((w[2] >> sh5).astype(np.float64) * 67108864.0 + (w[3] >> sh6).astype(np.float64) + 1.0) * 2.0 ** -53
    rad, ang = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
    out = np.zeros((rows, 2 * pairs))
    out[:, 0::2], out[:, 1::2] = rad * np.cos(ang), rad * np.sin(ang)
    return np.ascontiguousarray(out[:, :cols])


SEEDS = (0, 12345, 0xDEADBEEFCAFEF00D)


def check_generator(lib):
    """1. gpmpc_randn against the numpy restatement: three seeds, two streams, odd cols, rows 1 and 1000; rtol 1e-13 (the
    integers are exact, only log / sqrt / sin / cos differ by ulps).  The restatement reproduces the Random123 known-answer
    vector for counter 0, key 0.  A sub-block equals the same entries of a larger call bitwise."""
    kat = [int(x) for x in philox4x32_10(0, 0, 0, 0, 0, 0)]
    assert kat == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8], [hex(x) for x in kat]
    worst = 0.0
    for seed in SEEDS:
        for stream in (0, 3):
            for rows in (1, 1000):
                got, ref = lib.randn(seed, stream, rows, 5), randn_ref(seed, stream, rows, 5)
                worst = max(worst, np.max(np.abs(got - ref) / np.abs(ref)))
                assert np.allclose(got, ref, rtol=1e-13, atol=0), (seed, stream, rows, np.max(np.abs(got - ref) / np.abs(ref)))
    print(f'[generator] worst relative difference to numpy {worst:.2e} (bar 1e-13)')
    big = lib.randn(SEEDS[1], 2, 1000, 7)
    assert abs(big.mean()) < 0.05 and abs(big.std() - 1.0) < 0.05
    assert np.array_equal(lib.randn(SEEDS[1], 2, 300, 4), big[:300, :4])          # (row, column) only: not rows, cols, geometry
    assert np.array_equal(lib.randn(SEEDS[1], 2, 1, 7), big[:1])
    assert not np.array_equal(lib.randn(SEEDS[1], 1, 300, 4), big[:300, :4])      # another stream, other numbers


# ---------------------------------------------------------------------------------------------------------------------
# a fitted model with its oracle factors, shared by the checks of one tier
# ---------------------------------------------------------------------------------------------------------------------
class Model:
    """Synthetic model (sn = 0.1) on a handle, the oracle's factors of it, and roll-out inputs: start z0 = [x_0, u_0], controls
    U, small gains (0.05 N(0, 1), as rollout_feedback_cases), a non-trivial re-standardisation sa / sb and three initial
    covariances: 'full' (full rank, small), 'wide' (full rank: the spread of the 'EM' comparison) and 'semi' (the roll-outs'
    eye * 1e-6 with the state block diag(sn^2) and a ZERO control block: semidefinite).  mean_func 'const': the prior mean is
    added to the prediction (gpmpc_set_mean_func(..., add_to_prediction))."""

    def __init__(self, lib, N, Ny, d, T, seed=33, mean_func='zero'):
        p = go.synthetic_problem(N, d, Ny, 4, seed=seed, sn=0.1)
        self.N, self.Ny, self.d, self.T, self.Nu, self.mean_func = N, Ny, d, T, d - Ny, mean_func
        self.X, self.Y, self.Hk = p['X'], p['Y'], p['hyper']
        rng = np.random.default_rng(seed + 1)
        if mean_func == 'zero':
            self.H = self.Hk
            o = go.fit(self.X, self.Y, self.H, want_invK=False)
            self.h = Handle(lib, self.X, self.Y)
        else:
            self.Y = self.Y + 0.4                              # something for a mean function to explain
            self.H = np.hstack([self.Hk, rng.uniform(0.2, 0.5, (Ny, go.mean_param_count(mean_func, d)))])
            o = go.fit_mean(self.X, self.Y, self.H, mean_func, want_invK=False)
            self.h = Handle(lib, self.X, self.Y)
            self.h.set_mean_func(mean_func, True)
        assert np.all(self.h.fit(self.H) == 0)
        self.alpha, self.chol = o['alpha'], o['chol']
        Nu = self.Nu
        self.z0 = p['Z'][0].copy()
        self.U = 0.3 * rng.standard_normal((T, Nu))
        self.Kz, self.k0 = 0.05 * rng.standard_normal((Nu, Ny)), 0.05 * rng.standard_normal(Nu)
        self.sa, self.sb = 1.0 - 0.05 * rng.random(Ny), 0.02 * rng.standard_normal(Ny)
        semi = np.zeros((d, d))
        semi[:Ny, :Ny] = np.diag(self.H[:, d + 1] ** 2)
        self.Sigma = {'full': p['Sigma'][0], 'wide': 20.0 * p['Sigma'][1], 'semi': semi}
        self.sf2, self.sn2 = self.H[:, d] ** 2, self.H[:, d + 1] ** 2

    def factor(self, which):
        """Lower-triangular factor of an initial covariance (zero rows / columns where it is singular)."""
        S0, d = self.Sigma[which], self.d
        if which != 'semi':
            return np.linalg.cholesky(S0)
        L = np.zeros((d, d))
        L[:self.Ny, :self.Ny] = np.diag(np.sqrt(np.diag(S0)[:self.Ny]))
        return L

    def oracle(self, Z):
        return go.mean_var_jac(Z, self.X, self.H, self.alpha, self.chol, want_jac=False, mean_func=self.mean_func)[:2]

    def bars(self, Z):
        """(b_m[B, Ny], b_v[Ny]) of parity_cases' gpmpc_predict_mean_var checks at the points Z."""
        ms = mean_scale(self.X, Z, self.Hk, self.alpha)
        return 1e-10 * (ms + (0.0 if self.mean_func == 'zero' else 1.0)), 1e-10 * self.sf2

    def run(self, S, closed=False, noise=False, sigma='full', T=None, eps0=None, eps=None, seed=0, particles=True):
        T = self.T if T is None else T
        kw = dict(Kz=self.Kz, k0=self.k0) if closed else dict(U=self.U[:T])
        return self.h.rollout_mc(S, T, self.z0, self.Sigma[sigma], sa=self.sa, sb=self.sb, seed=seed, noise=noise, eps0=eps0,
                                 eps=eps, return_particles=particles, **kw)

    def close(self):
        self.h.close()


_MODELS = {}


def model(lib, mean_func='zero', **size):
    key = (id(lib), mean_func, tuple(sorted(size.items())))
    if key not in _MODELS:
        _MODELS[key] = Model(lib, mean_func=mean_func, **size)
    return _MODELS[key]


def close_models():
    for m in _MODELS.values():
        m.close()
    _MODELS.clear()


# ---------------------------------------------------------------------------------------------------------------------
# 2. step-by-step replay against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def replay_bound(md, Zt, eps_t, noise):
    """Oracle draw y_ref[S, Ny] at the inputs Zt with the normals eps_t, and the bar on |y_dev - y_ref|."""
    m, v = md.oracle(Zt)
    b_m, b_v = md.bars(Zt)
    nz = md.sn2 if noise else 0.0
    y_ref = m + np.sqrt(np.maximum(v, 0.0) + nz) * eps_t
    return y_ref, b_m + np.abs(eps_t) * b_v / (2.0 * np.sqrt(np.maximum(v + nz, b_v)))


def next_inputs(md, Y, t, closed):
    """The device's inputs of step t + 1, rebuilt from its step-t particles Y[S, Ny]."""
    u = Y @ md.Kz.T + md.k0 if closed else np.tile(md.U[t + 1], (Y.shape[0], 1))
    return np.hstack([md.sa * Y + md.sb, u])


def replay(md, S, closed, noise, sigma, rng_seed=5, label=''):
    rng = np.random.default_rng(rng_seed)
    T, d, Ny = md.T, md.d, md.Ny
    eps0, eps = rng.standard_normal((S, d)), rng.standard_normal((T, S, Ny))
    mean, cov, P = md.run(S, closed=closed, noise=noise, sigma=sigma, eps0=eps0, eps=eps)
    Zt = md.z0 + eps0 @ md.factor(sigma).T
    worst = 0.0
    for t in range(T):
        y_ref, bar = replay_bound(md, Zt, eps[t], noise)
        r = np.max(np.abs(P[t] - y_ref) / bar)
        worst = max(worst, r)
        assert r <= 1.0, (label, t, r)
        if t + 1 < T:
            Zt = next_inputs(md, P[t], t, closed)
    print(f'[replay {label} S={S} closed={closed} noise={noise} Sigma0={sigma}] worst |dy| / bar {worst:.2e}')
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(cov))
    return eps0, eps, P


VARIANTS = ((False, False, 'full'), (True, True, 'full'), (False, True, 'semi'), (True, False, 'semi'))


def check_replay(lib, S, chunk=None, variants=VARIANTS, **size):
    """Open and closed loop, noise 0 and 1, a full-rank and a semidefinite Sigma0 (zero control block); `chunk` sets
    "predict_chunk" for the call (S = 200 at 64: three chunks and a ragged fourth)."""
    md = model(lib, **size)
    if chunk:
        lib.set_tuning('predict_chunk', chunk)
    try:
        for closed, noise, sigma in variants:
            replay(md, S, closed, noise, sigma, label=f'N={md.N} chunk={chunk}')
    finally:
        if chunk:
            lib.set_tuning('predict_chunk', 0)


def check_replay_mean_function(lib, S, **size):
    """A 'const' prior mean added to the prediction: the particles follow ks^T alpha + c."""
    md = model(lib, mean_func='const', **size)
    replay(md, S, False, True, 'full', label=f'N={md.N} const mean')
    replay(md, S, True, False, 'semi', label=f'N={md.N} const mean')


def check_replay_sparse(lib, N=300, M=64, Ny=3, d=5, T=4, S=200):
    """GP.sparse(M): the FITC handle runs the same call; yardstick: the oracle's functions on its exported factors
    (fitc_cases.check_ordinary_model), bars as above."""
    from gp_mpc_amd.gp import GP
    p = go.synthetic_problem(N, d, Ny, 4, seed=21, sn=0.1)
    o = go.fit(p['X'], p['Y'], p['hyper'])
    gp = GP(p['X'], p['Y'], hyper=dict(hyper=p['hyper'], chol=o['chol'], alpha=o['alpha'], invK=o['invK']), normalize=False,
            gp_method='ME', lib=lib)
    sp = gp.sparse(M)
    s = sp.handle
    f = s.get_factors()
    Xu = sp._GP__X
    rng = np.random.default_rng(9)
    U = 0.3 * rng.standard_normal((T, d - Ny))
    S0 = np.eye(d) * 1e-6
    S0[:Ny, :Ny] = np.diag(p['hyper'][:, d + 1] ** 2)
    eps0, eps = rng.standard_normal((S, d)), rng.standard_normal((T, S, Ny))
    z0 = p['Z'][0]
    mean, cov, P = s.rollout_mc(S, T, z0, S0, U=U, noise=True, eps0=eps0, eps=eps, return_particles=True)
    Zt = z0 + eps0 @ np.linalg.cholesky(S0).T
    sf2, sn2 = p['hyper'][:, d] ** 2, p['hyper'][:, d + 1] ** 2
    for t in range(T):
        m, v, _ = go.mean_var_jac(Zt, Xu, p['hyper'], f['alpha'], f['chol'], want_jac=False)
        b_m, b_v = 1e-10 * mean_scale(Xu, Zt, p['hyper'], f['alpha']), 1e-10 * sf2
        y_ref = m + np.sqrt(np.maximum(v, 0.0) + sn2) * eps[t]
        bar = b_m + np.abs(eps[t]) * b_v / (2.0 * np.sqrt(np.maximum(v + sn2, b_v)))
        r = np.max(np.abs(P[t] - y_ref) / bar)
        print(f'[replay FITC M={M} of N={N}] step {t}: worst |dy| / bar {r:.2e}')
        assert r <= 1.0, (t, r)
        if t + 1 < T:
            Zt = np.hstack([P[t], np.tile(U[t + 1], (S, 1))])
    assert np.allclose(mean, P.mean(axis=1), rtol=0, atol=1e-12 * np.abs(P).max())
    sp.close()
    gp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. - 5. moments, generator path = array path, reproducibility
# ---------------------------------------------------------------------------------------------------------------------
def check_moments(lib, S_list=(1, 2, 96, 257, 2500), **size):
    """mean / cov = numpy.mean / numpy.cov(ddof=1) of the returned particles to 1e-12 max|.|; S = 1: cov exactly 0.  Two
    steps (one at S = 2500: ten blocks of partial sums either way); up to S = 257 also without the particle record."""
    md = model(lib, **size)
    for S in S_list:
        steps = 2 if S <= 257 else 1
        mean, cov, P = md.run(S, noise=True, sigma='wide', T=steps, seed=7)
        for t in range(steps):
            rm = P[t].mean(axis=0)
            rc = np.cov(P[t], rowvar=False, ddof=1).reshape(md.Ny, md.Ny) if S > 1 else np.zeros((md.Ny, md.Ny))
            em, ec = np.abs(mean[t] - rm).max(), np.abs(cov[t] - rc).max()
            assert em <= 1e-12 * np.abs(rm).max(), (S, t, em)
            assert ec <= 1e-12 * max(np.abs(rc).max(), np.finfo(float).tiny), (S, t, ec)
            assert np.array_equal(cov[t], cov[t].T)
        if S == 1:
            assert np.all(cov == 0.0)
        else:
            assert np.all(np.einsum('tii->ti', cov) > 0)
        if S <= 257:                     # without the particle record the moments are the same bits
            m2, c2 = md.run(S, noise=True, sigma='wide', T=steps, seed=7, particles=False)
            assert np.array_equal(m2, mean) and np.array_equal(c2, cov), S


def check_generator_path_equals_array_path(lib, S, closed=False, **size):
    """4. A call with `seed` and no arrays = bitwise a call handed gpmpc_randn's arrays for streams 0 and 1 .. T."""
    md = model(lib, **size)
    seed = SEEDS[2]
    a = md.run(S, closed=closed, noise=True, seed=seed)
    eps0 = lib.randn(seed, 0, S, md.d)
    eps = np.stack([lib.randn(seed, 1 + t, S, md.Ny) for t in range(md.T)])
    b = md.run(S, closed=closed, noise=True, eps0=eps0, eps=eps, seed=99)           # (seed unused with both arrays)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = md.run(S, closed=closed, noise=True, seed=seed + 1)
    assert not np.array_equal(a[2], c[2])


def check_reproducible(lib, S, chunk=64, **size):
    """5. The same call twice: the same bits.  Chunked ("predict_chunk" 64) against unchunked: every particle of every step
    within the replay bar of check 2 around the unchunked run (another variance kernel serves another batch width)."""
    md = model(lib, **size)
    a = md.run(S, noise=True, seed=3)
    b = md.run(S, noise=True, seed=3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    lib.set_tuning('predict_chunk', chunk)
    try:
        c = md.run(S, noise=True, seed=3)
        c2 = md.run(S, noise=True, seed=3)
    finally:
        lib.set_tuning('predict_chunk', 0)
    assert all(np.array_equal(x, y) for x, y in zip(c, c2))
    eps0 = lib.randn(3, 0, S, md.d)
    Zt = md.z0 + eps0 @ md.factor('full').T
    worst = 0.0
    for t in range(md.T):
        eps_t = lib.randn(3, 1 + t, S, md.Ny)
        _, bar = replay_bound(md, Zt, eps_t, True)
        worst = max(worst, np.max(np.abs(c[2][t] - a[2][t]) / bar))
        if t + 1 < md.T:
            Zt = next_inputs(md, a[2][t], t, False)
    print(f'[chunked vs unchunked S={S}] worst |dy| / bar {worst:.2e}')
    assert worst <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------------
# 6. one step against 'EM'
# ---------------------------------------------------------------------------------------------------------------------
def moment_ratios(Y, m_ref, c_ref):
    """|sample moment - reference| in standard errors: the mean's is sqrt(c_aa / S), a covariance entry's comes from the
    particles' own fourth moments, sqrt((m_aabb - c_ab^2) / S)."""
    S = Y.shape[0]
    ym = Y.mean(axis=0)
    D = Y - ym
    c = D.T @ D / (S - 1)
    m4 = np.einsum('sa,sb->ab', D * D, D * D) / S
    rm = np.abs(ym - m_ref) / np.sqrt(np.diag(c) / S)
    rc = np.abs(c - c_ref) / np.sqrt((m4 - c * c) / S)
    return rm.max(), rc.max()


EM_SEED = 2024


def check_one_step_vs_em(lib, S, **size):
    """T = 1, noise 0, the full-rank 'wide' Sigma0, seed EM_SEED: sample mean and covariance within 5 standard errors of
    gpmpc_predict('EM') on the same z0, Sigma0 (the tier's test names the ratios seen in a pure numpy replay)."""
    md = model(lib, **size)
    mean, cov, P = md.run(S, noise=False, sigma='wide', T=1, seed=EM_SEED)
    em_m, em_c = md.h.predict('EM', md.z0[None], md.Sigma['wide'][None])
    rm, rc = moment_ratios(P[0], em_m[0], em_c[0])
    # (the call's own mean / cov are those of the particles: check 3)
    print(f'[one step vs EM, N={md.N} S={S}] mean within {rm:.2f}, covariance within {rc:.2f} standard errors (bar 5)')
    assert rm <= 5.0 and rc <= 5.0, (rm, rc)


def numpy_one_step_ratios(S, seed=EM_SEED, **size):
    """The CPU pre-check of check_one_step_vs_em's seed: oracle predictions at z0 + L0 eps0 with the restated generator's
    normals, against the oracle's exact_moment.  No library involved."""
    p = go.synthetic_problem(size['N'], size['d'], size['Ny'], 4, seed=33, sn=0.1)
    o = go.fit(p['X'], p['Y'], p['hyper'])
    S0 = 20.0 * p['Sigma'][1]
    Z = p['Z'][0] + randn_ref(seed, 0, S, size['d']) @ np.linalg.cholesky(S0).T
    m, v, _ = go.mean_var_jac(Z, p['X'], p['hyper'], o['alpha'], o['chol'], want_jac=False)
    Y = m + np.sqrt(np.maximum(v, 0.0)) * randn_ref(seed, 1, S, size['Ny'])
    em_m, em_c = go.exact_moment(o['invK'], p['X'], p['Y'], p['hyper'], p['Z'][0], S0)
    return moment_ratios(Y, em_m, em_c)


# ---------------------------------------------------------------------------------------------------------------------
# 7. Python surface, 8. argument errors
# ---------------------------------------------------------------------------------------------------------------------
def check_python_surface(lib, tank, Nt=5):
    """GP.rollout_mc with S = 1, noise=False and eps = 0 follows the mean recursion: the mean trajectory of
    GP.rollout(methods=['ME']), on the normalised tank model and an un-normalised synthetic one; predict_compare(mc=None)
    returns today's keys, mc=64 adds 'mc_mean' / 'mc_var'."""
    from gp_mpc_amd.gp import GP
    g = tank
    hyper = dict(hyper=g['hyper'], chol=g['chol'], alpha=g['alpha'], invK=g['invK'])
    gp = GP(g['X'], g['Y'], hyper=hyper, gp_method='ME', normalize=True, lib=lib, meta=g['meta'], xlb=g['xlb'], xub=g['xub'],
            ulb=g['ulb'], uub=g['uub'])
    N, Ny, Nu = gp.get_size()
    x0 = g['meta']['meanX'] + 0.3 * g['meta']['stdX']
    u = np.tile(g['meta']['meanU'] - 0.2 * g['meta']['stdU'], (Nt, 1)) * (1.0 + 0.05 * np.arange(Nt))[:, None]
    zero0, zero = np.zeros((1, Ny + Nu)), np.zeros((Nt, 1, Ny))
    ref_m, _ = gp.rollout(x0, u, methods=['ME'])
    m, v, P = gp.rollout_mc(x0, u, S=1, noise=False, eps0=zero0, eps=zero, return_particles=True)
    assert m.shape == (Nt + 1, Ny) and v.shape == (Nt + 1, Ny) and P.shape == (Nt, 1, Ny)
    e = np.abs(m - ref_m[0]).max()
    print(f'[python, tank] eps = 0 particle against the ME mean recursion: {e:.2e}')
    assert e <= 1e-12 * max(1.0, np.abs(ref_m).max()), e
    assert np.array_equal(m[0], x0) and np.all(v == 0.0) and np.array_equal(P[:, 0], m[1:])
    K = 0.05 * np.random.default_rng(2).standard_normal((Nu, Ny))
    ref_c, _ = gp.rollout(x0, u, methods=['ME'], feedback=True, K=K, x_ref=0.9 * x0)
    mc_c, _ = gp.rollout_mc(x0, u, S=1, feedback=True, K=K, x_ref=0.9 * x0, eps0=zero0, eps=zero)
    e = np.abs(mc_c - ref_c[0]).max()
    print(f'[python, tank] closed loop, eps = 0: {e:.2e}')
    assert e <= 1e-12 * max(1.0, np.abs(ref_c).max()), e
    base = gp.predict_compare(x0, u, methods=['TA', 'ME'])
    assert sorted(base) == ['mean', 'methods', 't', 'var', 'y_sim']
    assert sorted(gp.predict_compare(x0, u, methods=['TA', 'ME'], mc=None)) == sorted(base)
    both = gp.predict_compare(x0, u, methods=['TA', 'ME'], mc=64)
    assert sorted(both) == sorted(list(base) + ['mc_mean', 'mc_var'])
    assert both['mc_mean'].shape == (Nt + 1, Ny) and both['mc_var'].shape == (Nt + 1, Ny)
    assert np.array_equal(both['mean'], base['mean']) and np.array_equal(both['var'], base['var'])
    assert np.all(np.isfinite(both['mc_mean'])) and np.all(both['mc_var'][1:] > 0) and np.all(both['mc_var'][0] == 0)
    gp.close()
    p = go.synthetic_problem(120, 5, 3, Nt + 3, seed=21, sn=0.1)
    o = go.fit(p['X'], p['Y'], p['hyper'])
    gp = GP(p['X'], p['Y'], hyper=dict(hyper=p['hyper'], chol=o['chol'], alpha=o['alpha'], invK=o['invK']), normalize=False,
            gp_method='TA', lib=lib)
    x0, u = p['Z'][0, :3], 0.3 * p['Z'][:Nt, 3:]
    ref_m, _ = gp.rollout(x0, u, methods=['ME'])
    m, v = gp.rollout_mc(x0, u, S=1, eps0=np.zeros((1, 5)), eps=np.zeros((Nt, 1, 3)))
    e = np.abs(m - ref_m[0]).max()
    print(f'[python, synthetic] eps = 0 particle against the ME mean recursion: {e:.2e}')
    assert e <= 1e-12 * max(1.0, np.abs(ref_m).max()), e
    gp.close()


def check_argument_errors(lib, **size):
    """8. GPMPC_EINVAL for S = 0, S = 2^20 + 1, NULL z0, an indefinite Sigma0, a closed loop on a model without controls;
    the following valid call is correct (the bits of the call before)."""
    md = model(lib, **size)
    S, T, d, Ny = 96, md.T, md.d, md.Ny
    good = md.run(S, noise=True, seed=11)
    h = md.h
    indef = md.Sigma['full'].copy()
    indef[1, 1] = -1e-3
    mean, cov = np.zeros((T, Ny)), np.zeros((T, Ny, Ny))
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    S0 = np.ascontiguousarray(md.Sigma['full'])
    U = np.ascontiguousarray(md.U)
    bad_calls = {
        'S = 0': lambda: h.rollout_mc(0, T, md.z0, S0, U=U),
        'S = 2^20 + 1': lambda: h.rollout_mc((1 << 20) + 1, T, md.z0, S0, U=U),
        'T = 0': lambda: h.rollout_mc(S, 0, md.z0, S0, U=np.zeros((0, md.Nu))),
        'indefinite Sigma0': lambda: h.rollout_mc(S, T, md.z0, indef, U=U),
        'open loop, NULL U': lambda: h.rollout_mc(S, T, md.z0, S0),
        'closed loop, NULL k0': lambda: h.rollout_mc(S, T, md.z0, S0, Kz=md.Kz),
        'NULL z0': lambda: lib.check(lib.dll.gpmpc_rollout_mc(h.h, S, T, 0, 0, None, vp(S0), vp(U), None, None, None, None, None,
                                                              None, vp(mean), vp(cov), None)),
    }
    for label, call in bad_calls.items():
        try:
            call()
        except GpmpcError as e:
            assert e.code == EINVAL, (label, e)
        else:
            raise AssertionError(f'{label}: no error')
        again = md.run(S, noise=True, seed=11)
        assert all(np.array_equal(x, y) for x, y in zip(again, good)), label
    # a model without controls (d == Ny): an open-loop call runs (U ignored), a closed one is refused
    q = go.synthetic_problem(100, Ny, Ny, 2, seed=5, sn=0.1)
    h2 = Handle(lib, q['X'], q['Y'])
    assert np.all(h2.fit(q['hyper']) == 0)
    Sq = np.eye(Ny) * 1e-4
    dummy = np.zeros((1, Ny))
    m2, c2 = np.zeros((T, Ny)), np.zeros((T, Ny, Ny))
    z0 = np.ascontiguousarray(q['Z'][0])
    raw = lambda Kz, k0: lib.dll.gpmpc_rollout_mc(h2.h, 32, T, 5, 0, vp(z0), vp(Sq), None, None, None, Kz, k0, None, None, vp(m2),
                                                  vp(c2), None)
    assert raw(vp(dummy), vp(dummy)) == EINVAL
    assert raw(None, None) == 0
    ref = h2.rollout_mc(32, T, z0, Sq, seed=5)
    assert np.array_equal(m2, ref[0]) and np.array_equal(c2, ref[1]) and np.all(np.isfinite(m2))
    h3 = Handle(lib, q['X'], q['Y'])                       # no factors yet
    try:
        h3.rollout_mc(32, T, z0, Sq)
    except GpmpcError as e:
        assert e.code == -3, e
    else:
        raise AssertionError('no GPMPC_ENOTFIT')
    h3.close()
    h2.close()
