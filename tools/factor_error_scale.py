"""How far equally good fp64 evaluations of the fit's factors land from numpy's own, in the measures of tests/factor_cases.py
(per 64 x 64 tile against the longdouble yardstick), at every shape of the emulator and the GPU tier.  The variants:
    a64, a32   a 64- and a 32-column right-looking blocked fp64 Cholesky in place of LAPACK's
    i64, iW    the same with the library's panel formula L21 = A21 I^T, I = L11^-1 formed explicitly (chol_chain.hpp, factor_twolevel),
               at the library's panel widths: 64 columns, and in the two-level cases the super-panel (emulator 128; GPU 512 or 896)
    b          K rounded from the longdouble K_t instead of built by gp_oracle.gram
    c          gp_oracle.gram's K with every entry moved by a random +-1 ulp (another exp of the same class)
    d0 .. d7   the training points in 8 other orders, mapped back (alpha, alpha's residual, the NLL, the K^-1 columns)
    t          gpmpc_cholesky's shapes only: L^-1 by a column-oriented triangular solve (of L^T) instead of the row-oriented one
Per measure the worst ratio variant / numpy of the three gated figures -- the maximum and the rms over the tiles, and per tile
against max(numpy's, numpy's median) -- and the bars that follow: twice the worst ratio, rounded up.  CPU only.

--lib PATH (tests/emu/_build/libgpmpc_emu.so, or the product library on an MI355X) adds the ratios device / numpy of every gate of
that tier's cases under the heading "measured on the device"; they do not set the bars.  Output: profiles/factor_error_scale.txt."""
import argparse
import math
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')]

import numpy as np                                   # noqa: E402
from scipy.linalg import solve_triangular            # noqa: E402
import gp_oracle as go                               # noqa: E402
import factor_cases as fc                            # noqa: E402



def inverse_panels(tier, N, Ny):
    """The widths of the library's explicit-inverse panels in this case: the 64-column tile, and the two-level super-panel
    where the case takes that route -- more than one output and at least two super-panels (factor_chain; twolevel_width:
    emulator 2 block columns; GPU 8, from 28 blocks on 14)."""
    nb = fc.nblocks(N)
    W = 2 if tier == 'emu' else (14 if nb >= 28 else 8)
    return (64, 64 * W) if Ny > 1 and nb >= 2 * W else (64,)


WHATS = ('rho', 'fwd', 'alpha', 'alpha_res', 'nll', 'invK', 'LiL')
ORDERS = 8


def ulp_moved(K, rng):
    """K with every entry of the lower triangle moved one ulp up or down, mirrored."""
    s = np.tril(rng.integers(0, 2, K.shape) * 2 - 1)
    s = s + np.tril(s, -1).T
    return np.where(s > 0, np.nextafter(K, np.inf), np.nextafter(K, -np.inf))


def measures(f, t, tiles, big, cuts, want_invK):
    out = fc.measure_L(f['L'], t, tiles, not big)
    out.update(fc.measure_alpha(f['alpha'], t, not big))
    if not big:
        out.update(fc.measure_nll(f['nll'], t))
    if want_invK:
        out.update(fc.measure_invK(f['invK'], t, cuts))
    return out


def shape_variants(tier, spec, rng):
    """{variant: {what: (max, rms, per tile)}} of one fit case, worst over its outputs."""
    d = spec.get('d', fc.GPU_D if tier == 'gpu' else fc.EMU_D)
    N, Ny, sn, kind = spec['N'], spec.get('Ny', 1), spec.get('sn', 1e-2), spec.get('kind', 'plain')
    cuts, want_invK = spec.get('cuts', ()), spec.get('want_invK', False)
    m = fc.model(N, d, Ny, sn, kind)
    big = N > fc.L_T_MAX_N
    tiles = fc.rho_tiles(N, cuts, spec.get('rows'), spec.get('all_tiles', False))
    worst = {}

    def note(variant, got, base):
        w = worst.setdefault(variant, {})
        for what in got:
            w[what] = np.maximum(w.get(what, np.zeros(3)), fc.ratios(got[what], base[what]))
    for a in range(Ny):
        t, y = m.truth[a], m.Y[:, a]
        base = measures(m.np[a], t, tiles, big, cuts, want_invK)
        K = m.K[a]
        note('a64', measures(fc.factors_from_L(fc.blocked_cholesky(K, 64), y), t, tiles, big, cuts, want_invK), base)
        note('a32', measures(fc.factors_from_L(fc.blocked_cholesky(K, 32), y), t, tiles, big, cuts, want_invK), base)
        for nb in inverse_panels(tier, N, Ny):
            if nb < N:
                note(f'i{nb}', measures(fc.factors_from_L(fc.blocked_cholesky(K, nb, True), y), t, tiles, big, cuts, want_invK), base)
        note('b', measures(fc.numpy_factors(fc.f64(t.K_t), y), t, tiles, big, cuts, want_invK), base)
        note('c', measures(fc.numpy_factors(ulp_moved(K, rng), y), t, tiles, big, cuts, want_invK), base)
        for o in range(ORDERS):
            perm = rng.permutation(N)
            inv = np.argsort(perm)
            Kp = go.gram(m.X[perm], m.H[a, :d], m.H[a, d] ** 2, m.H[a, d + 1] ** 2) + (fc.JITTER * np.eye(N) if m.jitter else 0.0)
            f = fc.numpy_factors(Kp, y[perm])
            got = fc.measure_alpha(f['alpha'][inv], t, not big)
            if not big:
                got.update(fc.measure_nll(f['nll'], t))
            if want_invK:
                got.update(fc.measure_invK(f['invK'][np.ix_(inv, inv)], t, cuts))
            note(f'd{o}', got, base)
    return worst


def cholesky_variants(tier, spec):
    d = fc.GPU_D if tier == 'gpu' else fc.EMU_D
    n = spec['N']

    class Recorder:                                   # the matrix, its truth and numpy's factors as check_cholesky makes them
        def cholesky(self, A, want_inverse=True):
            L = np.linalg.cholesky(A)
            return L, solve_triangular(L, np.eye(n), lower=True), 0
    fc.check_cholesky(Recorder(), n, d)
    A, t, L_np, Li_np = fc._CHOL[n, d, 1e-2]
    tiles = fc.lower_tiles(n)
    base = dict(fc.measure_L(L_np, t, tiles, True), **fc.measure_LiL(Li_np, L_np))
    worst = {}
    for variant, nb, inv in (('a64', 64, False), ('a32', 32, False), ('i64', 64, True)):
        L = fc.blocked_cholesky(A, nb, inv)
        got = dict(fc.measure_L(L, t, tiles, True), **fc.measure_LiL(solve_triangular(L, np.eye(n), lower=True), L))
        worst[variant] = {what: np.array(fc.ratios(got[what], base[what])) for what in got}
    got = fc.measure_LiL(solve_triangular(L_np.T, np.eye(n), lower=False).T, L_np)
    worst['t'] = {'LiL': np.array(fc.ratios(got['LiL'], base['LiL']))}
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiers', default='emu,gpu')
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--lib', default=None, help='also report the ratios of this build of the library (device / numpy), first tier of --tiers')
    args = ap.parse_args()
    if np.finfo(np.longdouble).nmant < 63:
        sys.exit('longdouble is no wider than fp64 here: no yardstick')
    rng = np.random.default_rng(args.seed)
    tiers = args.tiers.split(',')
    lines, overall, seen = [], {w: np.zeros(3) for w in WHATS}, set()
    if not args.lib:
        for tier in tiers:
            for name, spec in fc.CASES[tier].items():
                key = (tier, spec['check'], spec.get('N', spec.get('N0')), spec.get('n'), spec.get('Ny', 1), spec.get('sn', 1e-2),
                       spec.get('kind'), spec.get('want_invK', False), tuple(spec.get('cuts', ())), spec.get('d'))
                if key in seen:                              # (the same model and measures under another tuning)
                    continue
                seen.add(key)
                if spec['check'] == 'append':
                    spec = dict(N=spec['N0'] + spec['n'], all_tiles=spec.get('all_tiles', False))
                    key2 = (tier, 'fit', spec['N'], None, 1, 1e-2, None, False, (), None)
                    if key2 in seen:
                        continue
                    seen.add(key2)
                worst = cholesky_variants(tier, spec) if spec.get('check') == 'cholesky' else shape_variants(tier, spec, rng)
                for variant in sorted(worst):
                    if variant.startswith('d') and variant != 'd0':
                        continue
                    w = worst[variant]
                    if variant == 'd0':                      # the 8 orders as one line: the worst of them
                        for o in range(1, ORDERS):
                            for what in w:
                                w[what] = np.maximum(w[what], worst[f'd{o}'][what])
                    lines.append(f'{tier} {name:42s} {"d (8 orders)" if variant == "d0" else variant:12s} ' +
                                 '  '.join(f'{what} {r[0]:.2f}/{r[1]:.2f}/{r[2]:.2f}' for what, r in w.items()))
                    for what, r in w.items():
                        overall[what] = np.maximum(overall[what], r)
                print(tier, name, flush=True)
    print()
    print('tools/factor_error_scale.py' + (f' --tiers {args.tiers}' if args.tiers != 'emu,gpu' else '') +
          (f' --lib {os.path.relpath(args.lib, ROOT)}' if args.lib else ''))
    if not args.lib:
        print('variant / numpy, worst over the outputs: measure max/rms/per-tile')
        for line in lines:
            print(line)
        for what, w in overall.items():
            print(f'{what:9s}: worst ratio max / rms {max(w[0], w[1]):.2f} -> K_SET = {math.ceil(2 * max(w[0], w[1]))};  '
                  f'per tile {w[2]:.2f} -> K_POINT = {math.ceil(2 * w[2])}')
        return
    from gp_mpc_amd._lib import GpmpcLib
    lib = GpmpcLib(args.lib)
    print('measured on the device: device / numpy per gate, max / rms / per tile')
    for name in fc.CASES[tiers[0]]:
        fc.RECORD.clear()
        try:
            fc.run_case(lib, tiers[0], name)
        except AssertionError as e:                      # a figure beyond a bar is reported, not hidden
            print(f'{tiers[0]} {name}: BEYOND A BAR: {str(e)[:200]}')
        for label, what, r_max, r_rms, r_pt in fc.RECORD:
            print(f'{tiers[0]} {name:42s} {what:9s} {r_max:.2f} / {r_rms:.2f} / {r_pt:.2f}   ({label})')


if __name__ == '__main__':
    main()
