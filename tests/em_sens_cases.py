"""Gates of the exact-moment Jacobians (gpmpc_predict_em_sens: d mean/d z, d mean/d Sigma, d cov/d z, d cov/d Sigma) against
a longdouble value on FIXED inputs, and the routes of that entry point no other test reaches; shared by the emulator tier
(tests/test_emu_em_sens.py) and the GPU tier (tests/test_gpu_em_sens.py).

Why: parity_cases.check_em_sens bars d cov at 1e-9 of the pair sums' cancellation scale over ell, which is 1e-4 ... 0.3 of
the largest entry at the shapes it runs -- a row tile dropped at the ragged end, the (a, c) / (c, a) strips swapped, the
cross term symmetrised or a padded point in a moment need not show under it.  fp64 achieves 1e-11 ... 1e-15 there.

Yardstick: em_sens_fixed_input_longdouble -- the formulas of gp_oracle.exact_moment_sens on the device's own K^-1
(gpmpc_get_factors), beta = K^-1 y formed in longdouble from it, the pair sums in row blocks whose partial sums are added
exactly; evaluated twice by independent routes, whose spread is its own error, and with the 2-norm of the summands of every
entry (one fp64 rounding of every summand moves a sum by about eps times that norm, whatever the order).

Gate, per array, per output (d mean) or output pair of the lower triangle (d cov), entry by entry:
    E_dev <= EM_SENS_GATE_RATIO max(E_np, eps ||summands||) + EM_GATE_FLOOR max|ref over that block|
with E_np the distance of gp_oracle.exact_moment_sens (fp64, the same K^-1) from the yardstick.  Before the device's
Jacobians are looked at, the references alone must show that the yardstick is fine enough (spread <= EM_YARDSTICK_SHARE
of what it judges) and that the gate is no wider than 1e-6 of the block's largest entry.
profiles/em_sens_fixed_input_digits.txt holds the measured ratios of both tiers, profiles/em_sens_fixed_input_mutations.txt
what the gate catches."""
import numpy as np

import gp_oracle as go
from parity_cases import (_solve_ld, _det_ld, _ld_words, _fsum_ld, _longdouble_or_skip, clustered_problem, Handle, DevArray,
                          EM_GATE_RATIO, EM_GATE_FLOOR, EM_YARDSTICK_SHARE)

EPS = float(np.finfo(np.float64).eps)
ARRAYS = ('dm_dz', 'dm_dS', 'dc_dz', 'dc_dS')
# Twice the values' ratio (parity_cases.EM_GATE_RATIO = 8), and at most twice the largest per-entry ratio measured: 8.29 on the
# emulated build and 6.93 on the MI355X, both d cov at N = 600, d = 8, Ny = 6; every other case below 4.6
# (profiles/em_sens_fixed_input_digits.txt).  No step of the device accounts for the excess over 8 (exp_lean, the Gauss-Jordan
# eliminations, beta and the order of the sums were each checked, same file): an fp64 evaluation of these sums is a few
# eps ||summands|| from the exact value, not one (an error in a row's or column's operand is carried by N summands at once), the
# entries of a pair share their moments and so their draw, and numpy against ITSELF with the training points in another order
# reaches 7.1 at that shape.  A dropped tile, swapped strips or a symmetrised cross term is off by 1e7 ... 1e13 gate widths
# (profiles/em_sens_fixed_input_mutations.txt).
EM_SENS_GATE_RATIO = 2 * EM_GATE_RATIO
EM_SENS_GATE_WIDTH = 1e-6     # the widest the gate may be, as a share of the block's largest entry (from the references alone)

RECORD = []                   # (label, input, array, largest per-entry ratio, gate width / max|block|) of every gate of this process


def _exact_total(parts):
    """Entry by entry, the exact sum of the blocks' partial sums (longdouble arrays of one shape), rounded to longdouble:
    every partial sum is split into two fp64 words and the words are added exactly."""
    shape = np.shape(parts[0])
    P = np.stack([np.asarray(p, dtype=np.longdouble).ravel() for p in parts])
    out = np.array([_fsum_ld(_ld_words(P[:, e])) for e in range(P.shape[1])], dtype=np.longdouble)
    return out.reshape(shape)


def em_sens_fixed_input_longdouble(invK, X, Y, H, mu, Sigma, rows=(256, 173)):
    """The formulas in the docstring of gp_oracle.exact_moment_sens on FIXED fp64 inputs -- K^-1 as given (the device's
    own), X, Y, hyper, mu, Sigma -- evaluated in longdouble (TEST ONLY).  beta = K^-1 y is formed in longdouble from that
    K^-1; no N^3 step: per output pair the moments
        s0 = sum W,  sum W v_i,  sum W v_j,  sum W v_i v_i^T,  sum W v_j v_j^T,  sum W v_i v_j^T      (W = A o Q, over i, j)
    are formed in row blocks, every block's partial sums split into fp64 words and the words added exactly.
    Everything is done TWICE, independently: row blocks of rows[0] over (i, j), the exponent's cross term as
    (2 ii_i S') . ij_j, G = R^-T from _solve_ld(R, I), S' = R^-1 Sigma / 2 solved directly; and row blocks of rows[1] over
    the transposed (j, i), the cross term as ii_i . (2 ij_j S'^T), G = I - (I + Lab Sigma)^-1 Lab Sigma (the identity the
    reference uses for its inverses) and S' = Sigma G / 2.  The mean's moments once as one pairwise sum with
    P = (Sigma + Lambda)^-1 from that identity, once as block words with P solved directly.
    Returns a dict: dm_dz[Ny,d], dm_dS[Ny,d,d], dc_dz[Ny,Ny,d], dc_dS[Ny,Ny,d,d] (longdouble), the same with suffix '2'
    (the second evaluation) and with suffix '_l2' (fp64): the 2-norm of the summands of every entry -- for d mean its N
    summands w_i g_i, for d cov  t ||W o g|| + |mean_c| ||summands of d mean_a|| + |mean_a| ||summands of d mean_c||
    (every entry is t sum_ij W_ij g_ij - mean_c d mean_a - mean_a d mean_c).  invK: sequence of Ny [N, N] matrices."""
    ld = np.longdouble
    half = ld(0.5)
    Ny, (N, d) = len(H), X.shape
    Hl = np.asarray(H, dtype=np.float64).astype(ld)
    v = X.astype(ld) - np.asarray(mu, dtype=np.float64).astype(ld).reshape(1, d)
    vf = v.astype(np.float64)
    S = np.asarray(Sigma, dtype=np.float64).astype(ld)
    eye = np.eye(d, dtype=ld)
    ell2 = Hl[:, :d] ** 2
    sf2 = Hl[:, d] ** 2
    beta = []
    for a in range(Ny):
        y = Y[:, a].astype(ld)
        beta.append(np.concatenate([np.sum(invK[a][r0:r0 + 256].astype(ld) * y[None, :], axis=1) for r0 in range(0, N, 256)]))
    log_k = [np.log(sf2[a]) - half * np.sum(v * v / ell2[a][None, :], axis=1) for a in range(Ny)]

    # ---- the mean and its derivatives: d mean_a/d mu = P M1, d mean_a/d Sigma = -1/2 P mean_a + 1/2 P M2 P
    out = {}
    means = []
    dmz_l2, dmS_l2 = np.zeros((Ny, d)), np.zeros((Ny, d, d))
    for form in (0, 1):
        m, dmz, dmS = np.zeros(Ny, dtype=ld), np.zeros((Ny, d), dtype=ld), np.zeros((Ny, d, d), dtype=ld)
        for a in range(Ny):
            R = S + np.diag(ell2[a])
            if form == 0:
                iLam = np.diag(1 / ell2[a])
                P = iLam @ (eye - _solve_ld(eye + S @ iLam, S @ iLam))
            else:
                P = _solve_ld(R, eye)
            c = sf2[a] / np.sqrt(_det_ld(R)) * np.prod(Hl[a, :d])
            w = c * np.exp(-half * np.sum((v @ P) * v, axis=1)) * beta[a]
            wv = w[:, None] * v
            if form == 0:
                M0, M1, M2 = np.sum(w), np.sum(wv, axis=0), wv.T @ v
                wf, Pv, Pf = w.astype(np.float64), (v @ P).astype(np.float64), P.astype(np.float64)
                dmz_l2[a] = np.sqrt(np.sum((wf[:, None] * Pv) ** 2, axis=0))
                g = -0.5 * Pf[None, :, :] + 0.5 * Pv[:, :, None] * Pv[:, None, :]
                dmS_l2[a] = np.sqrt(np.sum((wf[:, None, None] * g) ** 2, axis=0))
            else:
                blocks = [slice(r0, r0 + 97) for r0 in range(0, N, 97)]
                M0 = _exact_total([np.sum(w[s]) for s in blocks])
                M1 = _exact_total([np.sum(wv[s], axis=0) for s in blocks])
                M2 = _exact_total([wv[s].T @ v[s] for s in blocks])
            m[a], dmz[a], dmS[a] = M0, P @ M1, -half * P * M0 + half * P @ M2 @ P
        means.append(m)
        sfx = '' if form == 0 else '2'
        out['mean' + sfx], out['dm_dz' + sfx], out['dm_dS' + sfx] = m, dmz, dmS
    out['dm_dz_l2'], out['dm_dS_l2'] = dmz_l2, dmS_l2

    # ---- the pair sums
    dcz_l2, dcS_l2 = np.zeros((Ny, Ny, d)), np.zeros((Ny, Ny, d, d))
    for form, bs in enumerate(rows):
        sfx = '' if form == 0 else '2'
        m, dmz, dmS = means[form], out['dm_dz' + sfx], out['dm_dS' + sfx]
        dcz, dcS = np.zeros((Ny, Ny, d), dtype=ld), np.zeros((Ny, Ny, d, d), dtype=ld)
        for a in range(Ny):
            ila = 1 / ell2[a]
            for b in range(a + 1):
                ilb = 1 / ell2[b]
                lab = ila + ilb
                R = S * lab[None, :] + eye                        # Sigma Lab + I
                if form == 0:
                    t = 1 / np.sqrt(_det_ld(R))
                    G = _solve_ld(R, eye).T
                    Q1 = _solve_ld(R, S * half)
                else:
                    t = 1 / np.sqrt(_det_ld(R.T))
                    LS = lab[:, None] * S                         # Lab Sigma;  G = (I + Lab Sigma)^-1
                    G = eye - _solve_ld(eye + LS, LS)
                    Q1 = half * (S @ G)
                ii, ij = v * ila[None, :], v * ilb[None, :]
                ra = log_k[a] + np.sum((ii @ Q1) * ii, axis=1)
                rb = log_k[b] + np.sum((ij @ Q1) * ij, axis=1)
                if form == 0:                    # row index i (output a), column index j (output b)
                    rw, cw = (ra, 2 * (ii @ Q1), beta[a]), (rb, ij, beta[b])
                else:                            # row index j, column index i
                    rw, cw = (rb, 2 * (ij @ Q1.T), beta[b]), (ra, ii, beta[a])
                if form == 0:                    # fp64 is enough for the norms: p_i = G ii_i, u_j = G ij_j
                    pf, uf = (ii @ G.T).astype(np.float64), (ij @ G.T).astype(np.float64)
                    GLf = (G * lab[None, :]).astype(np.float64)
                    sqz, sqS = np.zeros(d), np.zeros((d, d))
                parts = [[] for _ in range(6)]
                for r0 in range(0, N, bs):
                    r1 = min(N, r0 + bs)
                    E = rw[0][r0:r1, None] + cw[0][None, :]
                    for k in range(d):
                        E += rw[1][r0:r1, k:k + 1] * cw[1][:, k][None, :]
                    A = rw[2][r0:r1, None] * cw[2][None, :]
                    if a == b:
                        A -= (invK[a][r0:r1] if form == 0 else invK[a][:, r0:r1].T).astype(ld)
                    W = A * np.exp(E)
                    vr = v[r0:r1]
                    rs, cs = np.sum(W, axis=1), np.sum(W, axis=0)
                    for lst, val in zip(parts, (np.sum(W), vr.T @ rs, v.T @ cs, (vr * rs[:, None]).T @ vr, (v * cs[:, None]).T @ v,
                                                vr.T @ (W @ v))):
                        lst.append(val)
                    if form == 0:
                        W2 = W.astype(np.float64) ** 2
                        for k in range(d):
                            sqz[k] += np.sum(W2 * (pf[r0:r1, k][:, None] + uf[:, k][None, :]) ** 2)
                            for q in range(d):
                                g = (-0.5 * GLf[k, q] + 0.5 * (pf[r0:r1, k] * pf[r0:r1, q])[:, None] + 0.5 * (uf[:, k] * uf[:, q])[None, :]
                                     + pf[r0:r1, k][:, None] * uf[:, q][None, :])
                                sqS[k, q] += np.sum(W2 * g * g)
                s0, R1, C1, R2, C2, Xrc = [_exact_total(p) for p in parts]
                if form == 0:
                    Mi1, Mj1, Mi2, Mj2, Xij = R1, C1, R2, C2, Xrc          # sum W v_i, sum W v_j, ..., sum W v_i v_j^T
                else:
                    Mi1, Mj1, Mi2, Mj2, Xij = C1, R1, C2, R2, Xrc.T
                z1 = ila * Mi1 + ilb * Mj1
                # maha's cross term is not symmetrised: 2 ii_i ij_j^T, not ii_i ij_j^T + ij_j ii_i^T
                ZZ = ila[:, None] * Mi2 * ila[None, :] + ilb[:, None] * Mj2 * ilb[None, :] + 2 * ila[:, None] * Xij * ilb[None, :]
                dz = t * (G @ z1) - m[b] * dmz[a] - m[a] * dmz[b]
                dS = t * (-half * (G * lab[None, :]) * s0 + half * G @ ZZ @ G.T) - m[b] * dmS[a] - m[a] * dmS[b]
                dcz[a, b] = dcz[b, a] = dz
                dcS[a, b] = dcS[b, a] = dS
                if form == 0:
                    ma, mb = abs(float(m[a])), abs(float(m[b]))
                    dcz_l2[a, b] = dcz_l2[b, a] = float(t) * np.sqrt(sqz) + mb * dmz_l2[a] + ma * dmz_l2[b]
                    dcS_l2[a, b] = dcS_l2[b, a] = float(t) * np.sqrt(sqS) + mb * dmS_l2[a] + ma * dmS_l2[b]
        out['dc_dz' + sfx], out['dc_dS' + sfx] = dcz, dcS
    out['dc_dz_l2'], out['dc_dS_l2'] = dcz_l2, dcS_l2
    return out


# ------------------------------------------------------------------------------------------------ the gate
def _blocks(name, Ny):
    """The index of every gated block of an array: an output (d mean) or an output pair of the lower triangle (d cov)."""
    return [(a,) for a in range(Ny)] if name.startswith('dm') else [(a, c) for a in range(Ny) for c in range(a + 1)]


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _dist(value, truth):
    return _f64(np.abs(_f64(value).astype(np.longdouble) - truth))


class Reference:
    """The yardstick and numpy's evaluation for one input of one case; certifies the yardstick and the gate's width from
    the two alone (no device value is involved)."""

    def __init__(self, label, invK, X, Y, H, z, S):
        self.label, self.Ny = label, len(H)
        self.ref = em_sens_fixed_input_longdouble(invK, X, Y, H, z, S)
        self.np = dict(zip(ARRAYS, go.exact_moment_sens(invK, X, Y, H, z, S)))
        self.width = {}
        for name in ARRAYS:
            worst = 0.0
            for blk in _blocks(name, self.Ny):
                rv, rv2 = self.ref[name][blk], self.ref[name + '2'][blk]
                e_np = np.maximum(_dist(self.np[name][blk], rv), EPS * self.ref[name + '_l2'][blk])
                top = float(np.max(np.abs(rv)))
                floor = EM_GATE_FLOOR * top
                spread = _f64(np.abs(rv - rv2))
                assert np.all(spread <= EM_YARDSTICK_SHARE * np.maximum(e_np, floor)), ('yardstick too coarse', label, name, blk, spread, e_np, floor)
                width = float(np.max(EM_SENS_GATE_RATIO * e_np + floor))
                assert width <= EM_SENS_GATE_WIDTH * top, ('the gate would be vacuous', label, name, blk, width, top)
                worst = max(worst, width / top)
            self.width[name] = worst

    def gate(self, tag, dev):
        """dev: dict of the four arrays of this input (fp64, the reference's shapes).  One digits line per array: the
        largest errors over the array as shares of its largest entry, and the largest per-entry ratio
        (E_dev - floor) / max(E_np, eps ||summands||) -- the gate asks that it stay below EM_SENS_GATE_RATIO."""
        bad = []
        for name in ARRAYS:
            ratio, e_dev_max, e_np_max, e_num_max, spread_max, top_all = 0.0, 0.0, 0.0, 0.0, 0.0, float(np.max(np.abs(self.ref[name])))
            for blk in _blocks(name, self.Ny):
                rv = self.ref[name][blk]
                e_dev, e_num = _dist(dev[name][blk], rv), _dist(self.np[name][blk], rv)
                e_np = np.maximum(e_num, EPS * self.ref[name + '_l2'][blk])
                floor = EM_GATE_FLOOR * float(np.max(np.abs(rv)))
                ratio = max(ratio, float(np.max(np.maximum(e_dev - floor, 0.0) / e_np)))
                e_dev_max, e_np_max, e_num_max = max(e_dev_max, e_dev.max()), max(e_np_max, e_np.max()), max(e_num_max, e_num.max())
                spread_max = max(spread_max, float(np.max(np.abs(rv - self.ref[name + '2'][blk]))))
                if not np.all(e_dev <= EM_SENS_GATE_RATIO * e_np + floor):
                    bad.append((name, blk, float(np.max(e_dev / (EM_SENS_GATE_RATIO * e_np + floor))), float(e_dev.max())))
            RECORD.append((tag, name, ratio, self.width[name]))
            print(f'[EM sens fixed input] {tag} {name}: max|ref| {top_all:.3e}  E_dev/max {e_dev_max / top_all:.2e}  E_np/max {e_np_max / top_all:.2e} '
                  f'(numpy {e_num_max / top_all:.2e})  ratio per entry <= {ratio:.2f}  gate width/max|block| <= {self.width[name]:.1e}  '
                  f'yardstick spread/max {spread_max / top_all:.1e}')
        assert not bad, ('EM Jacobian', tag, 'blocks beyond the gate (array, block, E_dev / gate, E_dev)', bad)


# ------------------------------------------------------------------------------------------------ cases
SF = (0.7, 1.0, 1.9, 1.3, 0.85, 1.5)              # rows of every H differ in ell (the generators), sf and sn
SN = (0.1, 0.12, 0.15, 0.11, 0.13, 0.14)           # (no row below the generators' 0.1: cond(K), and with it the gate's width, stays theirs)


def _rows_differ(H, d):
    H = H.copy()
    H[:, d], H[:, d + 1] = SF[:len(H)], SN[:len(H)]
    return H


def clustered(N, d, Ny, B=1):
    """parity_cases.clustered_problem: Q = O(1) in every 64 x 64 tile, so no tile of the sweeps is idle."""
    X, Y, H, Z, S = clustered_problem(N, d, Ny, B=B)
    return X, Y, _rows_differ(H, d), Z, S


def wide_sigma(N, d, Ny, B, seed, take=None):
    """The inputs of parity_cases.check_em_sens: Z x 0.5, Sigma x 40 (G far from the identity), stretched length scales."""
    p = go.synthetic_problem(N, d, Ny, B, seed=seed, sn=0.1)
    H = p['hyper'].copy()
    H[:, :d] *= np.linspace(0.6, 1.3, d)[None, :]
    take = B if take is None else take
    return p['X'], p['Y'], _rows_differ(H, d), p['Z'][:take] * 0.5, p['Sigma'][:take] * 40


# label -> (inputs, the outputs whose pairs are gated (None: all), the 'em_sens_chunk' settings to run under)
CASES = {
    # tiles == 1: no prefetch, no second LDS buffer
    'one tile': (lambda: clustered(64, 3, 2), None, (0,)),
    # one real row in tile 2: 63 padded rows / columns; the full 8-deep cross term (9 of 16 feature columns live)
    'one real row in tile 2': (lambda: clustered(65, 8, 2), None, (0,)),
    # six row tiles, all nine ordered pairs, distinct length scales: (a, c) != (c, a) and 2 X' != X' + X'^T
    'ragged, Ny = 3, d = 1': (lambda: clustered(333, 1, 3), None, (0,)),
    # bl against b0 + bl indexing, in one pass and with one input per pass
    'two inputs': (lambda: clustered(555, 4, 2, B=2), None, (0, 1)),
    # KD = 16: c_j on the VALU plus the cross-lane sums, eight passes of em_mean_sens_kernel
    '16-deep': (lambda: clustered(200, 9, 2), None, (0,)),
    # the largest d, every tile live
    '16-deep, full': (lambda: clustered(200, 16, 2), None, (0,)),
    # 18 tiles, only the K^-1-streaming instantiation; N > 4 x 256 for the strided loop of the mean kernel
    'DIAG only': (lambda: clustered(1100, 3, 1), None, (0,)),
    # G far from the identity
    'wide Sigma': (lambda: wide_sigma(150, 4, 3, 5, 13, take=2), None, (0,)),
    # the shape at which check_em_sens's bar is a quarter of the largest entry; three of the 21 pairs (host time)
    "C3's dimensions": (lambda: wide_sigma(600, 8, 6, 3, 4, take=1), (1, 4), (0,)),
}


def check_case(lib, label):
    """The four Jacobian arrays of one case against the yardstick on the device's own K^-1, every input, under every
    'em_sens_chunk' setting of the case; the values must be those of gpmpc_predict('EM')."""
    _longdouble_or_skip()
    make, outs, chunks = CASES[label]
    X, Y, H, Z, S = make()
    d = X.shape[1]
    outs = list(range(len(H))) if outs is None else list(outs)
    h = Handle(lib, X, Y)
    try:
        assert np.all(h.fit(H, want_invK=True) == 0), label
        iK = h.get_factors(chol=False, alpha=False, invK=True)['invK']
        iK = [iK[a].copy() for a in outs]
        name = f'{label} N={len(X)} d={d} Ny={len(H)}' + (f' outputs {tuple(outs)}' if len(outs) < len(H) else '')
        refs = [Reference(f'{name} input {b}', iK, X, Y[:, outs], H[outs], Z[b], S[b]) for b in range(len(Z))]
        m0, c0 = h.predict('EM', Z, S)
        ix = np.ix_(outs, outs)
        for chunk in chunks:
            lib.set_tuning('em_sens_chunk', chunk)
            mean, cov, dm_dz, dm_dS, dc_dz, dc_dS = h.predict_em_sens(Z, S)
            assert np.array_equal(mean, m0) and np.array_equal(cov, c0), (label, chunk)
            for b, ref in enumerate(refs):
                tag = f'{name}' + (f' [em_sens_chunk {chunk}]' if chunk else '') + f' input {b}'
                ref.gate(tag, dict(dm_dz=dm_dz[b][outs], dm_dS=dm_dS[b][outs], dc_dz=dc_dz[b][ix], dc_dS=dc_dS[b][ix]))
    finally:
        lib.set_tuning('em_sens_chunk', 0)
        h.close()


# ------------------------------------------------------------------------------------------------ the routes
def _same_bits(tag, got, want):
    assert len(got) == len(want)
    for nm, g, w in zip(Handle.EM_SENS_OUTPUTS, got, want):
        if g is None:
            continue
        assert np.array_equal(g, w), (tag, nm, np.argwhere(g != w)[:4].tolist())


def check_unpacked_host(lib, N=100, d=8, Ny=6, B=12, seed=21):
    """gpmpc_predict_em_sens with host pointers beyond the packed block: at Ny = 6, d = 8 an input carries 3066 output
    doubles, so B = 12 exceeds the 32768 doubles of the pinned block and every array goes up and comes down in a copy of
    its own; calls of 5 + 5 + 2 inputs go packed.  Every output carries the bits of the packed calls -- with all six
    outputs, without cov, and with dcov_dS alone (every other output NULL)."""
    X, Y, H, Z, S = wide_sigma(N, d, Ny, B, seed)
    per_in = Ny + Ny * Ny + Ny * d + Ny * d * d + Ny * Ny * d + Ny * Ny * d * d
    assert B * per_in > 32768 >= 5 * max(per_in, d + d * d)
    h = Handle(lib, X, Y)
    try:
        assert np.all(h.fit(H, want_invK=True) == 0)
        parts = [h.predict_em_sens(Z[s], S[s]) for s in (slice(0, 5), slice(5, 10), slice(10, 12))]
        packed = [np.concatenate([p[i] for p in parts]) for i in range(6)]
        assert all(np.all(np.isfinite(a)) for a in packed)
        assert np.abs(packed[4]).max() > 0 and np.abs(packed[5]).max() > 0
        _same_bits('all six outputs', h.predict_em_sens(Z, S), packed)
        nv = h.predict_em_sens(Z, S, want_cov=False)
        assert nv[1] is None and all(a is not None for i, a in enumerate(nv) if i != 1)
        _same_bits('without cov', nv, packed)
        only = h.predict_em_sens(Z, S, outputs=('dcov_dS',))
        assert only[5] is not None and all(a is None for a in only[:5])
        _same_bits('dcov_dS alone', only, packed)
    finally:
        h.close()


def check_device_pointers(lib, N=100, d=4, Ny=3, B=5, seed=13, fill=-7.25):
    """gpmpc_predict_em_sens in device-pointer mode, two inputs per pass ('em_sens_chunk' = 2, B = 5: the b0 offsets into the
    caller's arrays): all six outputs, then without cov, then dmean_dz alone -- the kernels write all of them, so those left
    out land in the handle's scratch.  Outputs are two inputs too long and pre-filled: the head holds the bits of the
    host-pointer call, the tail is untouched."""
    X, Y, H, Z, S = wide_sigma(N, d, Ny, B, seed)
    names = Handle.EM_SENS_OUTPUTS
    shapes = ((Ny,), (Ny, Ny), (Ny, d), (Ny, d, d), (Ny, Ny, d), (Ny, Ny, d, d))
    h = Handle(lib, X, Y)
    z, s = DevArray(lib, Z), DevArray(lib, S)
    made = []
    try:
        assert np.all(h.fit(H, want_invK=True) == 0)
        lib.set_tuning('em_sens_chunk', 2)
        host = h.predict_em_sens(Z, S)
        h.set_pointer_mode(True)
        for want in (names, tuple(n for n in names if n != 'cov'), ('dmean_dz',)):
            outs = [DevArray(lib, np.full((B + 2,) + sh, fill)) if nm in want else None for nm, sh in zip(names, shapes)]
            made += [o for o in outs if o is not None]
            h.predict_em_sens_dev(B, z.ptr, s.ptr, *[None if o is None else o.ptr for o in outs])
            h.synchronize()
            for nm, o, ref in zip(names, outs, host):
                if o is None:
                    continue
                got = o.numpy()
                assert np.all(got[B:] == fill), (want, nm, 'wrote past the end')
                assert np.array_equal(got[:B], ref), (want, nm, np.argwhere(got[:B] != ref)[:4].tolist())
    finally:
        h.set_pointer_mode(False)
        lib.set_tuning('em_sens_chunk', 0)
        for a in [z, s] + made:
            a.free()
        h.close()


def check_far_inputs(lib, N=150, d=3, Ny=2, seed=9):
    """The model of parity_cases.check_far_points, B = 4: input 0 at 1e3, then at 1e5 length scales from every training
    point and input 2 at 3e8, near inputs in between.  Every Q and every mean weight of a far input is an exact zero (the
    Jacobian kernels' exp has no clamp route): all six outputs finite, the far inputs' four Jacobian arrays exact zeros,
    the near inputs the bits of their own B = 1 calls."""
    p = go.synthetic_problem(N, d, Ny, 80, seed=seed, sn=0.1)
    X, Y, H = p['X'], p['Y'], p['hyper']
    h = Handle(lib, X, Y)
    try:
        assert np.all(h.fit(H, want_invK=True) == 0)
        S = p['Sigma'][:4] * 1e-3
        for scale in (1e3, 1e5):
            Z = p['Z'][:4].copy()
            Z[0] = Z[0] + scale * H[0, :d].max() * np.array([1.0, -1.0, 1.0][:d])
            Z[2] = 3e8
            out = h.predict_em_sens(Z, S)
            for nm, a in zip(Handle.EM_SENS_OUTPUTS, out):
                assert np.all(np.isfinite(a)), (scale, nm, np.argwhere(~np.isfinite(a))[:4].tolist())
            for b in (0, 2):
                assert np.all(out[0][b] == 0.0) and np.array_equal(out[1][b], np.diag(H[:, d] ** 2)), (scale, b)
                for nm, a in zip(Handle.EM_SENS_OUTPUTS[2:], out[2:]):
                    assert np.all(a[b] == 0.0), (scale, b, nm, np.abs(a[b]).max())
            for b in (1, 3):
                assert np.abs(out[4][b]).max() > 0 and np.abs(out[5][b]).max() > 0, (scale, b)
                _same_bits(f'near input {b} beside far ones at {scale:g}', [a[b:b + 1] for a in out], h.predict_em_sens(Z[b:b + 1], S[b:b + 1]))
    finally:
        h.close()
