"""How far equally good fp64 evaluations of the predictive variance land from each other, measured against its longdouble
value (tests/parity_cases.py: longdouble_variance) at the shapes and probes of tests/variance_cases.py: numpy (gp_oracle) on the
data as given, and numpy with the training points in --orders other orders (the same formula, the same sums in another
order).  Per quantity (var, dvar, off-diagonal covar) the worst ratio reordered / unpermuted of the three gated measures -- the
maximum and the rms over the probes, and per probe against max(numpy's error, eps x summands) -- and the bars that follow: twice
the worst ratio, rounded up (a finite sample of orders underestimates the tail).  CPU only.

--lib PATH (e.g. tests/emu/_build/libgpmpc_emu.so, or the product library on an MI355X) adds the same three ratios of every
route the tests gate, device / numpy; they do not set the bars.  Output: profiles/var_error_scale.txt."""
import argparse
import math
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')]

import numpy as np                                   # noqa: E402
import gp_oracle as go                               # noqa: E402
import variance_cases as vc                          # noqa: E402

SHAPES = {'emu': [(330, 4)], 'gpu': [(330, 6), (1024, 6)]}


def measures(value, ref_np, truth, floor):
    e, e0 = vc.dist(value, truth).ravel(), vc.dist(ref_np, truth).ravel()
    return np.array([e.max() / e0.max(), vc.rms(e) / vc.rms(e0), np.max(e / np.maximum(e0, np.ravel(floor)))])


def reorder_ratios(m, orders, rng):
    """Worst ratios over `orders` permutations of the training points, per quantity: {what: [max, rms, per probe]}."""
    worst = {w: np.zeros(3) for w in ('var', 'dvar', 'cov')}
    ix = np.ix_(vc.COVAR_PROBES, vc.COVAR_PROBES)
    offd = ~np.eye(len(vc.COVAR_PROBES), dtype=bool)
    for _ in range(orders):
        perm = rng.permutation(m.N)
        X, Y = m.X[perm], m.Y[perm]
        o = go.fit(X, Y, m.H, want_invK=False)
        _, var, _ = go.mean_var_jac(m.P, X, m.H, o['alpha'], o['chol'], False)
        _, dvar = go.mean_var_sens(m.P, X, m.H, o['alpha'], o['chol'])
        cov = vc.numpy_covar(X, m.H, o['chol'], m.P[vc.COVAR_PROBES])
        for a, t in enumerate(m.truth):
            for what, r in (('var', measures(var[:, a], m.np_var[:, a], t.var, t.floor['var'])),
                            ('dvar', measures(dvar[:, a], m.np_dvar[:, a], t.dvar, t.floor['dvar'])),
                            ('cov', measures(cov[a][offd], m.np_cov[a][offd], t.covar[ix][offd], t.floor['cov'][ix][offd]))):
                worst[what] = np.maximum(worst[what], r)
    return worst


def device_ratios(lib, size):
    vc.RECORD.clear()
    checks = [(lambda B=B: vc.check_batch_size(lib, B, **size)) for B in (1, 5, 32, 33, 64, 65)]
    checks += [lambda: vc.check_large_batch(lib, **size), lambda: vc.check_chunked(lib, **size),
               lambda: vc.check_fused_fit_predict(lib, **size), lambda: vc.check_moment_methods(lib, **size),
               lambda: vc.check_sens(lib, **size), lambda: vc.check_covar(lib, **size),
               lambda: vc.check_after_append(lib, 320, **size), lambda: vc.check_after_append(lib, 300, **size),
               lambda: vc.check_after_append(lib, 250, **size), lambda: vc.check_after_set_factors(lib, **size),
               lambda: vc.check_rollouts(lib, **size)]
    failed = []
    for c in checks:
        try:
            c()
        except AssertionError as e:                  # a figure beyond a bar is reported, not hidden
            failed.append(str(e)[:200])
    return list(vc.RECORD), failed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', choices=sorted(SHAPES), default='emu', help="'emu': N = 330, d = 4; 'gpu': N = 330 and 1024, d = 6")
    ap.add_argument('--orders', type=int, default=32)
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--lib', default=None, help='also report the ratios of this build of the library (device / numpy)')
    args = ap.parse_args()
    if np.finfo(np.longdouble).nmant < 63:
        sys.exit('longdouble is no wider than fp64 here: no yardstick')
    rng = np.random.default_rng(args.seed)
    lib = None
    if args.lib:
        from gp_mpc_amd._lib import GpmpcLib
        lib = GpmpcLib(args.lib)
    overall = {w: np.zeros(3) for w in ('var', 'dvar', 'cov')}
    lines = []
    for N, d in SHAPES[args.shapes]:
        for sn in (1e-2, 0.1):
            m = vc.model(N, d, sn)
            w = reorder_ratios(m, args.orders, rng)
            for what in overall:
                overall[what] = np.maximum(overall[what], w[what])
                lines.append(f'N={N} d={d} sn={sn:g} {what:4s}: numpy reordered / numpy, worst of {args.orders} orders x {vc.NY} outputs: '
                             f'max {w[what][0]:.2f}  rms {w[what][1]:.2f}  per probe {w[what][2]:.2f}')
            if lib is not None:
                rec, failed = device_ratios(lib, dict(N=N, d=d, sn=sn))
                for what in overall:
                    r = np.array([x[2:] for x in rec if x[1] == what])
                    k = int(np.argmax(r[:, 2]))
                    names = [x[0] for x in rec if x[1] == what]
                    lines.append(f'N={N} d={d} sn={sn:g} {what:4s}: device / numpy, worst of {len(r)} gates: max {r[:, 0].max():.2f}  '
                                 f'rms {r[:, 1].max():.2f}  per probe {r[:, 2].max():.2f} ({names[k]})')
                for f in failed:
                    lines.append(f'N={N} d={d} sn={sn:g} BEYOND A BAR: {f}')
    print()
    print(f"tools/var_error_scale.py --shapes {args.shapes} --orders {args.orders}" + (f' --lib {os.path.relpath(args.lib, ROOT)}' if args.lib else ''))
    for line in lines:
        print(line)
    for what, w in overall.items():
        print(f'{what:4s}: worst reorder ratio max / rms {max(w[0], w[1]):.2f} -> K_SET = {math.ceil(2 * max(w[0], w[1]))};  '
              f'per probe {w[2]:.2f} -> K_POINT = {math.ceil(2 * w[2])}')


if __name__ == '__main__':
    main()
