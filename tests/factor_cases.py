"""Gates of the fit's factors -- L, alpha, the NLL, K^-1 and gpmpc_cholesky's L^-1 -- per 64 x 64 tile against an
extended-precision value, per execution of the factorisation; shared by the emulator tier (tests/test_emu_factor.py) and the GPU
tier (tests/test_gpu_factor.py).

Why: what held L so far is ||L - numpy||_F / ||L||_F <= 1e-10 over the whole matrix (and normwise residuals at N = 4096 and on
the two fixtures).  One off-diagonal tile of L multiplied by 1 + 1e-13 randn moves that figure by 5e-15 -- 20 000 times below the
bar -- and raises that tile's residual ||(L L^T - K)_tile||_F to 5.3 times numpy's.  A worker that skips one slab of one tile's
update, a hand-off tile read one step stale, a slab summed through a narrower type: each loses 3 to 4 digits in a few tiles and
passes every normwise bar.

Yardstick (host, longdouble; skipped where longdouble is not the x87 80-bit type), per model (X, y, hyper row), cached for the
life of the process:
    K_t      parity_cases.longdouble_kernel by direct differences + sn^2 on the diagonal (+ 1e-8 in the jitter case)
    L_t      a right-looking blocked Cholesky of K_t carried in longdouble (N <= 1024 only)
    alpha_t  parity_cases.longdouble_alpha (the jitter case: the same refinement on K_t + 1e-8 I)
    nll_t    0.5 y^T alpha_t + sum log diag L_t      (gp_oracle.nll's constant: no N/2 log 2 pi term)
    K_t^-1   the columns invk_columns(N, cuts): one per 64-block and both neighbours of every block boundary the case names, by the
             refinement of longdouble_alpha with unit vectors as right-hand sides
It certifies itself (certify): 4 against 5 refinement steps within 1/100 of numpy's error on the same quantity, and
||L_t L_t^T - K_t|| per tile within 1/100 of numpy's tile residual.

numpy is gp_oracle.gram -> np.linalg.cholesky -> Li = solve_triangular(L, I); alpha = Li^T (Li y), K^-1 = Li^T Li, the NLL as above
-- the explicit-inverse formulas of the library, in fp64.

Measures, per execution and output (device value against numpy's value of the same measure):
    rho        ||(L L^T - K_t)[tile i, j]||_F, product and difference in longdouble.  Not amplified by cond(K), needs no L_t.
               N <= 600: every lower tile; above: the block rows the case names.
    fwd        ||(L - L_t)[tile]||_F (N <= 1024), every lower tile; the strict upper triangle of L must be exactly zero.
    alpha      ||alpha - alpha_t||_2;   alpha_res  ||K_t alpha - y||_2, both formed in longdouble
    nll        |gpmpc_nll(fitted row) - nll_t|
    invK       ||(K^-1 - K_t^-1)[rows of block i, column c]||_2 on the truth's columns; the exported matrix exactly symmetric
    LiL        gpmpc_cholesky: ||(L^-1 L - I)[tile]||_F in longdouble (with rho and fwd of its L against the longdouble factor
               of the matrix it was given)
Every measure X takes the three conditions of the variance gate:
    max X_dev <= K_SET max X_np,   rms X_dev <= K_SET rms X_np,   X_dev <= K_POINT max(X_np, median X_np) per tile / block.
K_SET and K_POINT are NOT tuned to the device: they are twice the worst ratio, rounded up, of equally good fp64 evaluations to
numpy's own -- a 64- and a 32-column blocked Cholesky, the same with the library's explicit-inverse panel formula, K rounded
from K_t, K moved by +-1 ulp per entry, the training points in 8 other orders -- over every shape of both tiers (tools/factor_error_scale.py, profiles/factor_error_scale.txt).  The suite's old
bar relF(L, numpy) <= 1e-10 is asserted next to them.

Executions and the cases that reach them (factor_chain and its caller, api_factor.inl / api_fit.inl; confirmed once with
GPMPC_VERBOSE and the counters; `cut` = first block of a later worker launch / super-panel):

GPU tier (SEGR = 512, 256 CUs -> 224 workers; d = 6)
    case                          Np    blocks  route                                    launches  cuts
    N=60                          64    1       single queue (Np < 128: factor_chain refuses)   -   -
    N=520 GPMPC_CHAIN=0           576   9       single queue (factor_blocked)             -         -
    N=150                         192   3       chain + tile-owner workers                1         -
    N=520 (sn 1e-2 and 1e-3)      576   9       chain + workers, ragged last block        1         -
    N=1000 (+ no courier, + release-fence hand-offs)
                                  1024  16      chain + workers, inverse by row panels    2         8
    N=2000                        2048  32      chain + workers, inverse by row panels    3         16, 24
    N=520 Ny=2                    576   9       chain + flagged GEMM launches             -         -
    N=900 cu_count=8              960   15      chain + flagged GEMMs, inverse pipelined (104 tiles > 6 owners x 10)
    N=1000 Ny=2                   1024  16      two-level, width 8                        -         8
    N=1100 Ny=2                   1152  18      two-level, width 8, ragged third panel    -         8, 16
    N=1800 Ny=2                   1856  29      two-level, width 14                       -         14, 28
    N=520, N=1000 want_invK       as above                + K^-1 = L^-T L^-1
    N=520 Ny=2 want_invK          as above
    gpmpc_cholesky n=520, n=1000  576/1024      single queue (factor_blocked), exports L^-1
    N=330 jitter (sf = 1, sn = 1e-8, 8 rows twice: numpy's Cholesky fails at sn <= 1e-8 and succeeds with + 1e-8)
                                  384   6       chain + workers, twice (info = 1)         1         -
    N=512+8 append                576   9       fit: workers; append: strip update on the single queue.  (500 + 20 is a
                                                refit on the GPU: the strip's 128 x 448 panel exceeds the 64 x 512 scratch slot of
                                                Np = 576 at SEGR = 512, api_fit.inl; 512 + 8 is the strip that fits.)
Emulator tier (SEGR = 128, 8 CUs -> 7 workers, two-level width 2; d = 4)
    N=60  64/1 single queue;  N=150  192/3 workers, 1 launch;  N=330  384/6 workers, 1 launch;  N=560  576/9 workers, 2 launches
    (cut 4);  N=700  704/11 workers, 2 launches (cut 8);  N=950 cu_count=16  960/15 workers, 3 launches (cuts 8, 12);
    N=150 Ny=2  192/3 flagged GEMMs;  N=330 Ny=2  384/6 two-level (cuts 2, 4);  N=560 Ny=2  576/9 two-level, ragged (cuts 2 .. 8);
    N=560 GPMPC_CHAIN=0  single queue;  want_invK N=330;  gpmpc_cholesky n=330;  jitter N=330 (d = 6);  append 320+10.
(The counters: a fit that ran with the chained mode on counts as `chained_factorisations` even at Np = 64, where factor_chain
hands it to factor_blocked at once; `single_queue_factorisations` counts fits with the mode off.)

Host seconds per model: in the docstrings of the two tiers."""
import hashlib
import os
import time

import numpy as np
from scipy.linalg import cho_factor, cho_solve, solve_triangular

import gp_oracle as go
import parity_cases as pc
from gp_mpc_amd._lib import Handle
from gp_mpc_amd.synthetic import synthetic_problem

LD = np.longdouble
TILE = 64
JITTER = 1e-8
L_T_MAX_N = 1024              # the longdouble factor is formed up to here (1.7 s at 1024, 15 s at 2048)
ALL_TILES_MAX_N = 600         # rho over every lower tile up to here, over the named block rows above
YARDSTICK_SHARE = 0.01

# Twice the worst ratio variant / numpy over the variants and shapes of tools/factor_error_scale.py, rounded up
# (profiles/factor_error_scale.txt holds the raw ratios: worst 6.97 / 2.09 / 3.17 / 7.26 / 56.27 / 1.47 / 1.19 on the maximum and
# rms, 8.15 / 2.34 / 3.17 / 7.26 / 56.27 / 4.10 / 1.22 per tile).  rho's ratios are those of the library's own panel formula
# L21 = A21 L11^-1^T evaluated in numpy: its residual in the panel's first block columns grows with cond(L11), 3 to 8 times
# LAPACK's at these shapes, and every execution shows exactly that (the other variants stay below 1.5).  alpha's residual and
# the NLL are one number per model: where numpy's own value happens to land on the truth an equally good evaluation is far
# beyond it (N = 520, d = 6: numpy's NLL error 3e-11 against 1e-9 typical), hence the wide bars of those two.
K_SET = {'rho': 14.0, 'fwd': 5.0, 'alpha': 7.0, 'alpha_res': 15.0, 'nll': 113.0, 'invK': 3.0, 'LiL': 3.0}
K_POINT = {'rho': 17.0, 'fwd': 5.0, 'alpha': 7.0, 'alpha_res': 15.0, 'nll': 113.0, 'invK': 9.0, 'LiL': 3.0}

RECORD = []                   # (label, what, max ratio, rms ratio, per-tile ratio) of every gate of this process
_BEYOND = []                  # what the gates of the running check found beyond a bar: every gate prints first, the check fails last


def beyond(*what):
    _BEYOND.append(what)


def verdict():
    """Fails the check if any of its gates was beyond its bar -- after every gate has printed its line."""
    found = list(_BEYOND)
    _BEYOND.clear()
    assert not found, found


def f64(a):
    return np.asarray(a, dtype=np.float64)


def rms(e):
    return float(np.sqrt(np.mean(np.square(e))))


def nblocks(n):
    return (n + TILE - 1) // TILE


def lower_tiles(n, rows=None):
    """(i, j) of the lower 64 x 64 tiles of an n x n matrix, of the block rows `rows` (default: all)."""
    rows = range(nblocks(n)) if rows is None else sorted(set(rows))
    return [(i, j) for i in rows for j in range(i + 1)]


def blocked_cholesky(K, nb=TILE, inverse_panel=False):
    """Right-looking blocked Cholesky (lower) in the type of K: the diagonal block column by column, the panel by a
    triangular solve, the trailing update by block columns of the lower triangle.  longdouble: the yardstick's L_t; float64
    with nb = 64 / 32: two of the equally good evaluations that scale the gates.  inverse_panel (fp64): the formula of the
    library's panels instead, L21 = A21 I^T with I = L11^-1 formed explicitly (LAPACK's factor of the diagonal block,
    solve_triangular for its inverse)."""
    A = np.array(K, copy=True)
    n = len(A)
    for k in range(0, n, nb):
        e = min(n, k + nb)
        D = A[k:e, k:e]
        P = A[e:, k:e]
        if inverse_panel:
            D[:] = np.linalg.cholesky(D)
            P[:] = P @ solve_triangular(D, np.eye(e - k), lower=True).T
        else:
            for j in range(e - k):
                D[j, j] = np.sqrt(D[j, j] - D[j, :j] @ D[j, :j])
                D[j + 1:, j] = (D[j + 1:, j] - D[j + 1:, :j] @ D[j, :j]) / D[j, j]
            for j in range(e - k):
                P[:, j] = (P[:, j] - P[:, :j] @ D[j, :j]) / D[j, j]
        for c in range(e, n, nb):
            A[c:, c:c + nb] -= P[c - e:] @ P[c - e:c - e + nb].T
    return np.tril(A)


def refine(K_t, cf, B, iters):
    """K_t^-1 B by the refinement of parity_cases.longdouble_alpha: the fp64 Cholesky cf of the rounded K_t as the
    preconditioner, the residual B - K_t V formed in longdouble.  iters: increasing step counts -> one solution per count."""
    Bl = np.asarray(B).astype(LD)
    V = cho_solve(cf, f64(B)).astype(LD)
    out, done = [], 0
    for n in iters:
        for _ in range(n - done):
            V = V + cho_solve(cf, f64(Bl - K_t @ V)).astype(LD)
        done = n
        out.append(V)
    return out


def tile_residual(L, K_t, tiles):
    """rho(i, j) = ||(L L^T - K_t)[tile i, j]||_F with L promoted to longdouble and the product formed in longdouble (only the
    columns a lower tile needs: L is lower triangular)."""
    Ll = np.asarray(L).astype(LD)
    n = len(Ll)
    out = np.zeros(len(tiles))
    byrow = {}
    for t, (i, j) in enumerate(tiles):
        byrow.setdefault(i, []).append((t, j))
    for i, lst in byrow.items():
        r0, r1 = TILE * i, min(n, TILE * i + TILE)
        R = Ll[r0:r1, :r1] @ Ll[:r1, :r1].T - K_t[r0:r1, :r1]
        for t, j in lst:
            out[t] = float(np.sqrt(np.sum(np.square(R[:, TILE * j:TILE * j + TILE]))))
    return out


def tile_norms(D, tiles):
    """||D[tile]||_F of a longdouble matrix D per tile."""
    return np.array([float(np.sqrt(np.sum(np.square(D[TILE * i:TILE * i + TILE, TILE * j:TILE * j + TILE])))) for i, j in tiles])


def invk_columns(n, cuts=()):
    """The columns of K^-1 the truth holds: the middle of every 64-block, and both neighbours of every block boundary in `cuts`
    (block numbers)."""
    cols = {min(n - 1, TILE * b + TILE // 2) for b in range(nblocks(n))}
    for c in cuts:
        if 0 < TILE * c < n:
            cols |= {TILE * c - 1, TILE * c}
    return np.array(sorted(cols))


def numpy_factors(K, y):
    """numpy's fp64 evaluation of the library's formulas from a gram matrix K."""
    L = np.linalg.cholesky(K)
    return factors_from_L(L, y)


def factors_from_L(L, y):
    Li = solve_triangular(L, np.eye(len(L)), lower=True)
    return dict(L=L, Li=Li, alpha=Li.T @ (Li @ y), invK=Li.T @ Li,
                nll=float(0.5 * y @ (Li.T @ (Li @ y)) + np.sum(np.log(np.diag(L)))))


class Truth:
    """The extended-precision values of one output (X, y, hyper row): see the module docstring.  The parts are formed when
    first asked for."""

    def __init__(self, X, y, hyper_row, jitter=False, cuts=(), K_t=None):
        t0 = time.time()
        d = X.shape[1]
        self.N, self.y, self.jitter = len(X), y, jitter
        self.X, self.hyper_row, self.cuts = X, hyper_row, tuple(cuts)
        if K_t is not None:                                       # gpmpc_cholesky: the matrix it is given IS the truth
            self.K_t = K_t
        else:
            self.K_t = pc.longdouble_kernel(X, X, hyper_row)
            self.K_t[np.diag_indices(self.N)] += LD(hyper_row[d + 1]) ** 2 + (LD(JITTER) if jitter else LD(0))
        self._L = self._alpha = self._cols = None
        self.seconds = time.time() - t0

    @property
    def cf(self):
        if not hasattr(self, '_cf'):
            self._cf = cho_factor(f64(self.K_t), lower=True)
        return self._cf

    @property
    def L_t(self):
        assert self.N <= L_T_MAX_N
        if self._L is None:
            t0 = time.time()
            self._L = blocked_cholesky(self.K_t)
            self.seconds += time.time() - t0
        return self._L

    @property
    def alpha45(self):
        if self._alpha is None:
            t0 = time.time()
            if self.jitter:
                self._alpha = refine(self.K_t, self.cf, self.y, (4, 5))
            else:
                self._alpha = [pc.longdouble_alpha(self.X, self.y, self.hyper_row, iters=n)[0] for n in (4, 5)]
            self.seconds += time.time() - t0
        return self._alpha

    @property
    def alpha_t(self):
        return self.alpha45[0]

    @property
    def nll_t(self):
        return LD(0.5) * (self.y.astype(LD) @ self.alpha_t) + np.sum(np.log(np.diag(self.L_t)))

    def invk(self, cuts=()):
        """(columns, K_t^-1[:, columns] at 4 steps, at 5 steps)"""
        if self._cols is None or self._cols[0] != tuple(cuts):
            t0 = time.time()
            cols = invk_columns(self.N, cuts)
            E = np.zeros((self.N, len(cols)))
            E[cols, np.arange(len(cols))] = 1.0
            self._cols = (tuple(cuts), cols) + tuple(refine(self.K_t, self.cf, E, (4, 5)))
            self.seconds += time.time() - t0
        return self._cols[1:]


_TRUTHS = {}


def truth(X, y, hyper_row, jitter=False):
    key = hashlib.sha1(X.tobytes() + y.tobytes() + f64(hyper_row).tobytes() + bytes([jitter])).hexdigest()
    if key not in _TRUTHS:
        _TRUTHS[key] = Truth(X, y, hyper_row, jitter)
    return _TRUTHS[key]


class Model:
    """One data set, numpy's factors of every output and the outputs' truths.  kind: 'plain' | 'jitter' (sf = 1, sn as given,
    the first 8 rows repeated as the last 8: the first factorisation fails, the one with + 1e-8 succeeds)."""

    def __init__(self, N, d, Ny, sn, kind='plain', seed=1234):
        pc._longdouble_or_skip()
        self.N, self.d, self.Ny, self.sn, self.kind = N, d, Ny, sn, kind
        p = synthetic_problem(N, d, Ny, 1, seed=seed, sn=sn)
        self.X, self.Y, self.H = p['X'], p['Y'], p['hyper']
        self.jitter = kind == 'jitter'
        if self.jitter:
            self.X[-8:], self.Y[-8:] = self.X[:8], self.Y[:8]
            self.H[:, d] = 1.0
        self.K = [go.gram(self.X, self.H[a, :d], self.H[a, d] ** 2, self.H[a, d + 1] ** 2) for a in range(Ny)]
        if self.jitter:
            for a in range(Ny):
                check_jitter_premise(self.X, self.Y[:, a], self.H[a], self.K[a])
            self.K = [K + JITTER * np.eye(N) for K in self.K]
        self.np = [numpy_factors(self.K[a], self.Y[:, a]) for a in range(Ny)]
        self.truth = [truth(self.X, self.Y[:, a], self.H[a], self.jitter) for a in range(Ny)]
        self.label = f'N={N} d={d} Ny={Ny} sn={sn:g}' + (' jitter' if self.jitter else '')
        self._certified = set()


def check_jitter_premise(X, y, hyper_row, K):
    """numpy's Cholesky fails on K and succeeds on K + 1e-8 I, and gp_oracle.nll takes that branch."""
    try:
        np.linalg.cholesky(K)
        failed = False
    except np.linalg.LinAlgError:
        failed = True
    assert failed, 'the jitter case is positive definite in fp64 without the jitter'
    L = np.linalg.cholesky(K + JITTER * np.eye(len(K)))
    want = 0.5 * y @ np.linalg.solve(L.T, np.linalg.solve(L, y)) + np.sum(np.log(np.diag(L)))
    got = go.nll(hyper_row, X, y)
    assert abs(got - want) <= 1e-9 * (abs(want) + len(K)), ('gp_oracle.nll did not take the jitter branch', got, want)


_MODELS = {}


def model(N, d, Ny=1, sn=1e-2, kind='plain', seed=1234):
    key = (N, d, Ny, sn, kind, seed)
    if key not in _MODELS:
        _MODELS[key] = Model(*key)
    return _MODELS[key]


def named_rows(n, cuts=()):
    """The block rows measured above ALL_TILES_MAX_N: 0, 1, the last two, and both sides of every cut."""
    nb = nblocks(n)
    rows = {0, 1, nb - 2, nb - 1}
    for c in cuts:
        rows |= {c - 1, c}
    return sorted(r for r in rows if 0 <= r < nb)


def rho_tiles(n, cuts=(), rows=None, all_tiles=False):
    if rows is not None:
        return lower_tiles(n, rows)
    return lower_tiles(n) if (n <= ALL_TILES_MAX_N or all_tiles) else lower_tiles(n, named_rows(n, cuts))


# ------------------------------------------------------------------------------------------------ measures
def measure_L(L, t, tiles, want_fwd):
    """{'rho': per tile, 'fwd': per lower tile} of a factor L against the truth t."""
    out = {'rho': tile_residual(L, t.K_t, tiles)}
    if want_fwd:
        out['fwd'] = tile_norms(np.asarray(L).astype(LD) - t.L_t, lower_tiles(t.N))
    return out


def measure_alpha(alpha, t, want_err=True):
    al = np.asarray(alpha).astype(LD)
    out = {'alpha_res': np.array([float(np.sqrt(np.sum(np.square(t.K_t @ al - t.y.astype(LD)))))])}
    if want_err:
        out['alpha'] = np.array([float(np.sqrt(np.sum(np.square(al - t.alpha_t))))])
    return out


def measure_nll(v, t):
    return {'nll': np.array([float(abs(LD(v) - t.nll_t))])}


def measure_invK(invK, t, cuts=()):
    cols, V4, _ = t.invk(cuts)
    D = np.asarray(invK)[:, cols].astype(LD) - V4
    nb = nblocks(t.N)
    return {'invK': np.array([[float(np.sqrt(np.sum(np.square(D[TILE * i:TILE * i + TILE, c])))) for c in range(len(cols))]
                              for i in range(nb)]).ravel()}


def measure_LiL(Li, L):
    """||(Li L - I)[tile]||_F per lower tile, the product in longdouble (block row by block row: both are lower triangular)."""
    n = len(L)
    Lil, Ll = np.asarray(Li).astype(LD), np.asarray(L).astype(LD)
    out = []
    for i in range(nblocks(n)):
        r0, r1 = TILE * i, min(n, TILE * i + TILE)
        D = Lil[r0:r1, :r1] @ Ll[:r1, :r1]
        D[np.arange(r1 - r0), np.arange(r0, r1)] -= 1
        out += [float(np.sqrt(np.sum(np.square(D[:, TILE * j:TILE * j + TILE])))) for j in range(i + 1)]
    return {'LiL': np.array(out)}


def ratios(x, x_np):
    """The three ratios of a measure x against numpy's x_np (same tiles)."""
    x, x_np = f64(x).ravel(), f64(x_np).ravel()
    floor = float(np.median(x_np))
    return float(x.max() / x_np.max()), rms(x) / rms(x_np), float(np.max(x / np.maximum(x_np, floor)))


def gate(label, what, x_dev, x_np):
    r_max, r_rms, r_pt = ratios(x_dev, x_np)
    worst = int(np.argmax(f64(x_dev).ravel() / np.maximum(f64(x_np).ravel(), float(np.median(x_np)))))
    RECORD.append((label, what, r_max, r_rms, r_pt))
    print(f'[{what} vs longdouble] {label}: max X_dev {np.max(x_dev):.2e} X_np {np.max(x_np):.2e} (ratio {r_max:.2f}, bar {K_SET[what]:g})  '
          f'rms {rms(x_dev):.2e} / {rms(x_np):.2e} (ratio {r_rms:.2f})  per tile <= {r_pt:.2f} x max(X_np, median) at #{worst} '
          f'(bar {K_POINT[what]:g})  over {np.size(x_dev)}')
    if r_max > K_SET[what]:
        beyond('maximum over the tiles', label, what, round(r_max, 2), K_SET[what])
    if r_rms > K_SET[what]:
        beyond('rms over the tiles', label, what, round(r_rms, 2), K_SET[what])
    if r_pt > K_POINT[what]:
        beyond('per tile', label, what, round(r_pt, 2), K_POINT[what], f'tile #{worst}')


def gate_all(label, dev, ref):
    for what in dev:
        gate(label, what, dev[what], ref[what])


def certify(m, a, tiles, parts, cuts=()):
    """The yardstick of output a against numpy's own error, once per (model, output, parts)."""
    key = (a, tuple(tiles), tuple(parts), tuple(cuts))
    if key in m._certified:
        return
    t, ref = m.truth[a], m.np[a]

    def share(what, mine, theirs):
        print(f'[yardstick {m.label} output {a}] {what}: yardstick {mine:.2e}, numpy {theirs:.2e}')
        assert mine <= YARDSTICK_SHARE * theirs, ('yardstick too coarse', m.label, a, what, mine, theirs)
    if 'fwd' in parts:
        own, theirs = tile_residual(t.L_t, t.K_t, tiles), tile_residual(ref['L'], t.K_t, tiles)
        share('tile residual of L_t (worst ratio to numpy\'s on the same tile)', float(np.max(own / theirs)), 1.0)
    if 'alpha' in parts:
        a4, a5 = t.alpha45
        share('alpha, 4 vs 5 steps', float(np.sqrt(np.sum(np.square(a4 - a5)))), measure_alpha(ref['alpha'], t)['alpha'][0])
    if 'invK' in parts:
        cols, V4, V5 = t.invk(cuts)
        share('K^-1 columns, 4 vs 5 steps', float(np.max(np.sqrt(np.sum(np.square(V4 - V5), axis=0)))),
              float(np.max(np.sqrt(np.sum(np.square(ref['invK'][:, cols].astype(LD) - V4), axis=0)))))
    m._certified.add(key)


# ------------------------------------------------------------------------------------------------ checks
class tunings:
    """set_tuning(name, value) for the body, the restoring value in every case on the way out."""

    def __init__(self, lib, *triples):
        self.lib, self.triples = lib, triples

    def __enter__(self):
        done = []
        try:
            for name, value, _ in self.triples:
                done.append(name)
                self.lib.set_tuning(name, value)
        except Exception:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        for name, _, restore in self.triples:
            self.lib.set_tuning(name, restore)


def make_handle(lib, X, Y, chain=True):
    """A handle; chain = False: created under GPMPC_CHAIN=0 (set and restored around the creation: the variable is read
    there), i.e. every factorisation of it on the single queue."""
    if chain:
        return Handle(lib, X, Y)
    old = os.environ.get('GPMPC_CHAIN')
    os.environ['GPMPC_CHAIN'] = '0'
    try:
        return Handle(lib, X, Y)
    finally:
        if old is None:
            del os.environ['GPMPC_CHAIN']
        else:
            os.environ['GPMPC_CHAIN'] = old


def check_route_counters(h, chain, fits):
    """The execution the handle's fits took: no hand-off time-out, and the chained mode on / off as the case says."""
    assert h.counter('handoff_timeouts') == 0, h.counter('handoff_timeouts')
    if chain:
        assert h.counter('chained_factorisations') == fits and h.counter('single_queue_factorisations') == 0
    else:
        assert h.counter('single_queue_factorisations') == fits and h.counter('chained_factorisations') == 0


def gate_factors(m, label, f, nll, cuts=(), rows=None, all_tiles=False, want_invK=False):
    """The measures of the factors f (get_factors) and the NLL values nll[a] of a model against the truth, per output; which
    measures: by the size, see the module docstring."""
    N = m.N
    big = N > L_T_MAX_N
    tiles = rho_tiles(N, cuts, rows, all_tiles)
    for a in range(m.Ny):
        t, ref = m.truth[a], m.np[a]
        L = f['chol'][a]
        lab = f'{label} output {a}' if m.Ny > 1 else label
        old = pc.relF(L, ref['L'])
        print(f'[old bar] {lab}: relF(L, numpy) {old:.2e}')
        if not old <= 1e-10:
            beyond('old bar relF(L, numpy) <= 1e-10', lab, float(old))
        if not np.all(np.triu(L, 1) == 0.0):
            beyond('strict upper triangle of L is not zero', lab)
        certify(m, a, tiles, (() if big else ('fwd', 'alpha')) + (('invK',) if want_invK else ()), cuts)
        gate_all(lab, measure_L(L, t, tiles, not big), measure_L(ref['L'], t, tiles, not big))
        gate_all(lab, measure_alpha(f['alpha'][a], t, not big), measure_alpha(ref['alpha'], t, not big))
        if not big and nll is not None:
            gate_all(lab, measure_nll(nll[a], t), measure_nll(ref['nll'], t))
        if want_invK:
            iK = f['invK'][a]
            if not np.array_equal(iK, iK.T):
                beyond('K^-1 is not exactly symmetric', lab)
            gate_all(lab, measure_invK(iK, t, cuts), measure_invK(ref['invK'], t, cuts))


def check_fit(lib, label, N, d, Ny=1, sn=1e-2, kind='plain', chain=True, tune=(), cuts=(), rows=None, all_tiles=False,
              want_invK=False):
    """gpmpc_fit on the model, get_factors and gpmpc_nll at the fitted rows -> gate_factors.  tune: (name, value, restore)
    triples of set_tuning in force while the handle exists."""
    m = model(N, d, Ny, sn, kind)
    _BEYOND.clear()
    with tunings(lib, *tune):
        h = make_handle(lib, m.X, m.Y, chain)
        try:
            info = h.fit(m.H, want_invK=want_invK)
            assert np.all(info == (1 if m.jitter else 0)), info
            check_route_counters(h, chain, 2 if m.jitter else 1)
            f = h.get_factors(invK=want_invK)
            nll = None
            if N <= L_T_MAX_N:
                nll = [h.nll(a, m.H[a]) for a in range(Ny)]
                assert h.last_jitter == (1 if m.jitter else 0)
                assert h.counter('handoff_timeouts') == 0
        finally:
            h.close()
    gate_factors(m, f'{label} {m.label}', f, nll, cuts, rows, all_tiles, want_invK)
    verdict()


def check_append(lib, N0, n, d, sn=1e-2, all_tiles=False):
    """Fit N0 points, gpmpc_append n more (the strip route: the one factor update that never runs a Cholesky over the whole
    matrix): rho, fwd, alpha and the NLL of the extended model against the truth of all N0 + n points."""
    m = model(N0 + n, d, 1, sn)
    h = Handle(lib, m.X[:N0], m.Y[:N0])
    try:
        assert np.all(h.fit(m.H) == 0)
        assert np.all(h.append(m.X[N0:], m.Y[N0:]) == 0) and h.N == m.N
        assert h.counter('handoff_timeouts') == 0
        fits = h.counter('chained_factorisations') + h.counter('single_queue_factorisations')
        assert fits == 1, ('the append refitted instead of extending the factors', fits)
        f = h.get_factors()
        nll = [h.nll(0, m.H[0])]
    finally:
        h.close()
    gate_factors(m, f'append {N0} + {n} {m.label}', f, nll, all_tiles=all_tiles)
    verdict()


_CHOL = {}


def check_cholesky(lib, n, d, sn=1e-2):
    """gpmpc_cholesky (factor_blocked; the one place L^-1 itself is exported) on the fp64 rounding A of the model's longdouble
    gram: rho and fwd of L against the longdouble factor of A, and (L^-1 L - I) per tile against numpy's solve_triangular."""
    m = model(n, d, 1, sn)
    if (n, d, sn) not in _CHOL:
        A = f64(m.truth[0].K_t)
        t = Truth(m.X, m.Y[:, 0], m.H[0], K_t=A.astype(LD))
        L = np.linalg.cholesky(A)
        _CHOL[n, d, sn] = (A, t, L, solve_triangular(L, np.eye(n), lower=True))
    A, t, L_np, Li_np = _CHOL[n, d, sn]
    L, Li, info = lib.cholesky(A, want_inverse=True)
    assert info == 0
    label = f'gpmpc_cholesky n={n} d={d} sn={sn:g}'
    old = pc.relF(L, L_np)
    print(f'[old bar] {label}: relF(L, numpy) {old:.2e}')
    if not old <= 1e-10:
        beyond('old bar relF(L, numpy) <= 1e-10', label, float(old))
    if not (np.all(np.triu(L, 1) == 0.0) and np.all(np.triu(Li, 1) == 0.0)):
        beyond('strict upper triangles are not zero', label)
    tiles = lower_tiles(n)
    own, theirs = tile_residual(t.L_t, t.K_t, tiles), tile_residual(L_np, t.K_t, tiles)
    assert np.max(own / theirs) <= YARDSTICK_SHARE, ('yardstick too coarse', label, float(np.max(own / theirs)))
    gate_all(label, measure_L(L, t, tiles, True), measure_L(L_np, t, tiles, True))
    gate_all(label, measure_LiL(Li, L), measure_LiL(Li_np, L_np))
    verdict()


# ------------------------------------------------------------------------------------------------ the cases of the two tiers
def real_cu_count(lib):
    """The device's compute units (what 'cu_count' is restored to): the library names the admissible range when it refuses."""
    import re
    from gp_mpc_amd._lib import GpmpcError
    try:
        lib.set_tuning('cu_count', 1 << 20)
    except GpmpcError as e:
        return int(re.search(r'cu_count must be in \[8, (\d+)\]', str(e)).group(1))
    raise AssertionError('cu_count = 2^20 was accepted')


def fit_case(N, Ny=1, sn=1e-2, **kw):
    return dict(check='fit', N=N, Ny=Ny, sn=sn, **kw)


GPU_D, EMU_D = 6, 4
NO_COURIER = (('worker_courier', 0, -1),)
RELEASE_FENCE = (('handoff_write_through', 0, -1),)
# id -> case.  cuts: the block boundaries (worker-launch cuts, super-panel edges) whose two sides are measured; rows: the block
# rows of rho where the issue names them.  'cu': the emulated / pretended CU count (restored to the tier's own).  'd': input
# dimensions other than the tier's (the jitter model at d = 4 has numpy's own factor 1.7e-10 from the longdouble one and its
# variants 2e-10 from numpy: the old bar 1e-10 means nothing there; at d = 6 they are at 3e-13).
CASES = {
    'gpu': {
        'single_queue_N60': fit_case(60, label='single queue (Np = 64)'),
        'single_queue_chain_off_N520': fit_case(520, chain=False, label='single queue (GPMPC_CHAIN=0)'),
        'workers_N150': fit_case(150, label='workers, 1 launch'),
        'workers_N520': fit_case(520, label='workers, 1 launch, ragged'),
        'workers_N520_sn1e-3': fit_case(520, sn=1e-3, label='workers, 1 launch, ragged'),
        'workers_two_launches_N1000': fit_case(1000, cuts=(8,), label='workers, 2 launches'),
        'workers_two_launches_no_courier_N1000': fit_case(1000, cuts=(8,), tune=NO_COURIER, label='workers, 2 launches, no courier'),
        'workers_two_launches_release_fence_N1000': fit_case(1000, cuts=(8,), tune=RELEASE_FENCE, label='workers, 2 launches, release fence'),
        'workers_three_launches_N2000': fit_case(2000, cuts=(16, 24), rows=(0, 1, 15, 16, 23, 24, 30, 31), label='workers, 3 launches'),
        'flagged_Ny2_N520': fit_case(520, Ny=2, label='flagged GEMMs'),
        'flagged_cu8_N900': fit_case(900, cu=8, label='flagged GEMMs (8 CUs)'),
        'twolevel_Ny2_N1000': fit_case(1000, Ny=2, cuts=(8,), label='two-level, 2 panels'),
        'twolevel_ragged_Ny2_N1100': fit_case(1100, Ny=2, cuts=(8, 16), label='two-level, ragged third panel'),
        'twolevel_width14_Ny2_N1800': fit_case(1800, Ny=2, cuts=(14, 28), rows=(0, 13, 14, 27, 28), label='two-level, width 14'),
        'invK_N520': fit_case(520, want_invK=True, label='K^-1'),
        'invK_N1000': fit_case(1000, want_invK=True, cuts=(8,), label='K^-1'),
        'invK_Ny2_N520': fit_case(520, Ny=2, want_invK=True, label='K^-1'),
        'cholesky_n520': dict(check='cholesky', N=520),
        'cholesky_n1000': dict(check='cholesky', N=1000),
        'jitter_N330': fit_case(330, sn=1e-8, kind='jitter', label='jitter'),
        'append_512_8': dict(check='append', N0=512, n=8),
    },
    'emu': {
        'single_queue_N60': fit_case(60, label='single queue (Np = 64)'),
        'single_queue_chain_off_N560': fit_case(560, chain=False, label='single queue (GPMPC_CHAIN=0)'),
        'workers_N150': fit_case(150, label='workers, 1 launch'),
        'workers_N330': fit_case(330, label='workers, 1 launch, ragged'),
        'workers_N330_sn1e-3': fit_case(330, sn=1e-3, label='workers, 1 launch, ragged'),
        'workers_two_launches_N560': fit_case(560, cuts=(4,), label='workers, 2 launches'),
        'workers_two_launches_N700': fit_case(700, cuts=(8,), all_tiles=True, label='workers, 2 launches'),
        'workers_two_launches_no_courier_N700': fit_case(700, cuts=(8,), all_tiles=True, tune=NO_COURIER, label='workers, 2 launches, no courier'),
        'workers_two_launches_release_fence_N700': fit_case(700, cuts=(8,), all_tiles=True, tune=RELEASE_FENCE,
                                                            label='workers, 2 launches, release fence'),
        'workers_three_launches_cu16_N950': fit_case(950, cuts=(8, 12), all_tiles=True, cu=16, label='workers, 3 launches'),
        'flagged_Ny2_N150': fit_case(150, Ny=2, label='flagged GEMMs'),
        'twolevel_Ny2_N330': fit_case(330, Ny=2, cuts=(2, 4), label='two-level, 3 panels'),
        'twolevel_ragged_Ny2_N560': fit_case(560, Ny=2, cuts=(2, 4, 6, 8), label='two-level, ragged fifth panel'),
        'invK_N330': fit_case(330, want_invK=True, label='K^-1'),
        'cholesky_n330': dict(check='cholesky', N=330),
        'jitter_N330': fit_case(330, sn=1e-8, kind='jitter', d=6, label='jitter'),
        'append_320_10': dict(check='append', N0=320, n=10, all_tiles=True),
    },
}


def run_case(lib, tier, name):
    c = dict(CASES[tier][name])
    d = c.pop('d', GPU_D if tier == 'gpu' else EMU_D)
    kind = c.pop('check')
    if kind == 'cholesky':
        return check_cholesky(lib, c['N'], d)
    if kind == 'append':
        return check_append(lib, c['N0'], c['n'], d, all_tiles=c.get('all_tiles', False))
    tune = tuple(c.pop('tune', ()))
    cu = c.pop('cu', None)
    if cu is not None:
        tune += (('cu_count', cu, real_cu_count(lib) if tier == 'gpu' else 8),)
    check_fit(lib, c.pop('label'), c.pop('N'), d, tune=tune, **c)
