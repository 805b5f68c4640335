"""How far fp64 evaluations of the exact-moment covariance land from its longdouble value on FIXED inputs, in units of
eps ||summands|| (tests/parity_cases.py: em_fixed_input_longdouble, cov_l2), per output pair: the device (by default the
CPU emulator build of the kernels, tests/emu/_build/libgpmpc_emu.so; --lib for another build), numpy (gp_oracle), and
numpy on the same inputs with the training points in another order (the same sums, an equally accurate evaluation).
Prints how often each exceeds 2 x numpy's own distance.  Output: profiles/em_fixed_input_error_scale.txt."""
import argparse
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')]

import numpy as np                                   # noqa: E402
import gp_oracle as go                               # noqa: E402
import parity_cases as pc                            # noqa: E402
from gp_mpc_amd._lib import GpmpcLib, Handle         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=os.path.join(ROOT, 'tests', 'emu', '_build', 'libgpmpc_emu.so'))
    ap.add_argument('--cases', type=int, default=24)
    ap.add_argument('--seed', type=int, default=11)
    args = ap.parse_args()
    lib = GpmpcLib(args.lib)
    eps = np.finfo(float).eps
    rng = np.random.default_rng(args.seed)
    rows = []
    for case in range(args.cases):
        N, d, Ny = int(rng.integers(100, 600)), int(rng.integers(1, 9)), int(rng.integers(1, 4))
        p = go.synthetic_problem(N, d, Ny, 1, seed=case, sn=(1e-2, 0.1)[case % 2])
        X, Y, H, Z, S = p['X'], p['Y'], p['hyper'], p['Z'], p['Sigma'] * 30
        h = Handle(lib, X, Y)
        h.fit(H, want_invK=True)
        iK = h.get_factors(chol=False, alpha=False, invK=True)['invK']
        _, c = h.predict('EM', Z, S)
        h.close()
        ref = pc.em_fixed_input_longdouble(iK, X, Y, H, Z[0], S[0])
        _, nc = go.exact_moment(iK, X, Y, H, Z[0], S[0])
        P = rng.permutation(N)
        _, pcv = go.exact_moment([k[P][:, P] for k in iK], X[P], Y[P], H, Z[0], S[0])
        sig = eps * ref['cov_l2']
        for a in range(Ny):
            for b in range(a + 1):
                r = ref['cov'][a, b]
                e = [float(abs(np.longdouble(x[a, b]) - r)) for x in (c[0], nc, pcv)]
                rows.append((e[0], e[1], e[2], sig[a, b]))
    R = np.array(rows)

    def rat(num, den):
        return num / np.maximum(den, 1e-300)
    print(f'{len(R)} output pairs of {args.cases} random shapes (N 100..600, d 1..8, Ny 1..3, sn 1e-2 / 0.1)')
    for name, i in (('device', 0), ('numpy, points in another order', 2)):
        r_plain, r_floor, r_sig = rat(R[:, i], R[:, 1]), rat(R[:, i], np.maximum(R[:, 1], R[:, 3])), rat(R[:, i], R[:, 3])
        print(f'{name}: > 2 x numpy in {np.mean(r_plain > 2):.0%} of the pairs (max {r_plain.max():.1f} x); > 2 x max(numpy, '
              f'eps ||summands||) in {np.mean(r_floor > 2):.0%} (max {r_floor.max():.2f} x); distance / (eps ||summands||) '
              f'median {np.median(r_sig):.2f} max {r_sig.max():.2f}')
    r_sig = rat(R[:, 1], R[:, 3])
    print(f'numpy: distance / (eps ||summands||) median {np.median(r_sig):.2f} max {r_sig.max():.2f}')


if __name__ == '__main__':
    main()
