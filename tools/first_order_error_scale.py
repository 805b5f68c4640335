"""How far equally good fp64 evaluations of the predictive mean, its Jacobian J, its Hessian Hm and the off-diagonal 'TA'
covariance land from each other, measured against their longdouble values on fixed alpha (tests/first_order_cases.py) at every
shape of both test tiers.  numpy (gp_oracle) on the data as given is the unit; against it
  * numpy with the training points (and alpha with them) in --orders other orders: the same sums in another order, and
  * the same with every ks entry moved by +-2 ulp at random: the accuracy the table exponential of the cross-covariance kernel
    documents for itself (<= 1 ulp of the table entry + 0.6 ulp + the reduction; gp_kernels.hpp, exp_tab32).
Per quantity the worst ratio of the three gated measures -- the maximum and the rms over the probes, and per probe against
max(numpy's error, floor) -- and the bars that follow: twice the worst ratio, rounded up.  alpha is numpy's own
(gp_oracle.fit / fit_mean), held fixed.  'fused_mean' (the mean from sum_i V_ij w_i, full-truth yardstick): numpy's whole fit on
the reordered data against numpy's fit on the data as given, maximum and rms.  CPU only; nothing here reads a device.

Output: profiles/first_order_error_scale.txt (and stdout)."""
import argparse
import math
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')]

import numpy as np                                   # noqa: E402
import gp_oracle as go                               # noqa: E402
import first_order_cases as fc                       # noqa: E402

# every model of tests/test_emu_first_order.py and tests/test_gpu_first_order.py
EDGE, PRIOR = list(fc.EDGE_SIZES.values()), list(fc.PRIOR_SIZES.values())
SHAPES = {'emu': [dict(N=330, d=4, sn=1e-2), dict(N=330, d=4, sn=0.1), dict(N=520, d=4, sn=1e-2)],
          'gpu': [dict(N=330, d=6, sn=1e-2), dict(N=330, d=6, sn=0.1), dict(N=1024, d=6, sn=1e-2), dict(N=1024, d=6, sn=0.1),
                  dict(N=2048, d=6, sn=1e-2), dict(N=2050, d=6, sn=1e-2)],
          'both': EDGE + PRIOR}
FUSED = {'emu': [dict(N=330, d=4, sn=1e-2), dict(N=330, d=4, sn=0.1)],
         'gpu': [dict(N=330, d=6, sn=1e-2), dict(N=330, d=6, sn=0.1), dict(N=1024, d=6, sn=1e-2), dict(N=1024, d=6, sn=0.1)]}
WHAT = ('mean', 'J', 'Hm', 'TAoff')
_plain_kernel = go.cov_se_ard_direct


def moved_kernel(rng):
    def ks(X, Z, ell, sf2):
        k = _plain_kernel(X, Z, ell, sf2)
        return k + rng.choice([-2.0, 2.0], size=k.shape) * np.spacing(k)
    return ks


def evaluate(m, X, alpha, kernel):
    """numpy's mean, J, Hm and off-diagonal TA covariance of model m with the training points X / alpha as given."""
    go.cov_se_ard_direct = kernel
    try:
        eye = np.broadcast_to(np.eye(m.N), (fc.NY, m.N, m.N))
        mean, _, J = go.mean_var_jac(m.P, X, m.H, alpha, eye, True, mean_func=m.mean_func)
        Hm, _ = go.mean_var_sens(m.P, X, m.Hk, alpha, eye)
        if m.mean_func == 'polynomial':
            for a in range(fc.NY):
                Hm[:, a] += np.diag(2 * m.H[a, m.d + 2:2 * m.d + 2])
    finally:
        go.cov_se_ard_direct = _plain_kernel
    return mean, J, Hm, go.ta_cov(np.zeros((m.B, fc.NY)), J, m.S)


def ratios(m, r, value):
    """{what: [max, rms, per probe]}, the worst over the outputs, of one evaluation against numpy's plain one."""
    mean, J, Hm, TA = value
    off = ~np.eye(fc.NY, dtype=bool)
    out = {w: np.zeros(3) for w in WHAT}
    for a in range(fc.NY):
        for w, v, ref, t, f in (('mean', mean[:, a], r.np_mean[:, a], r.mean[:, a], r.f_mean[:, a]),
                                ('J', J[:, a], r.np_J[:, a], r.J[:, a], r.f_J[:, a]),
                                ('Hm', Hm[:, a], r.np_Hm[:, a], r.Hm[:, a], r.f_Hm[:, a])):
            out[w] = np.maximum(out[w], fc.measures(v, ref, t, f)[:3])
    out['TAoff'] = np.array(fc.measures(TA[:, off], r.np_TA[:, off], r.TA[:, off], r.f_TA[:, off])[:3])
    return out


def model_ratios(size, orders, rng):
    m = fc.model(**size)
    fit = go.fit_mean(m.X, m.Y, m.H, m.mean_func, want_invK=False) if m.mean_func != 'zero' else go.fit(m.X, m.Y, m.H, want_invK=False)
    alpha = fit['alpha']
    r = m.reference(alpha, want_hm=True)
    worst = {kind: {w: np.zeros(3) for w in WHAT} for kind in ('reordered', 'moved')}
    for _ in range(orders):
        perm = rng.permutation(m.N)
        for kind, kernel in (('reordered', _plain_kernel), ('moved', moved_kernel(rng))):
            got = ratios(m, r, evaluate(m, m.X[perm], np.ascontiguousarray(alpha[:, perm]), kernel))
            for w in WHAT:
                worst[kind][w] = np.maximum(worst[kind][w], got[w])
    return m, worst


def fused_ratios(size, orders, rng):
    """numpy's whole fit + mean on reordered data (plain and +-2 ulp kernel) against numpy's on the data as given: [max, rms]."""
    m = fc.model(**size)
    truth, np_mean, _ = fc.full_truth(m)
    worst = np.zeros(2)
    eye = np.broadcast_to(np.eye(m.N), (fc.NY, m.N, m.N))
    for _ in range(orders):
        perm = rng.permutation(m.N)
        X, Y = m.X[perm], m.Y[perm]
        alpha = go.fit(X, Y, m.H, want_invK=False)['alpha']
        for kernel in (_plain_kernel, moved_kernel(rng)):
            go.cov_se_ard_direct = kernel
            try:
                mean, _, _ = go.mean_var_jac(m.P, X, m.H, alpha, eye, False)
            finally:
                go.cov_se_ard_direct = _plain_kernel
            for a in range(fc.NY):
                worst = np.maximum(worst, fc.measures(mean[:, a], np_mean[:, a], truth[:, a], None)[:2])
    return m, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--orders', type=int, default=32)
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'first_order_error_scale.txt'))
    args = ap.parse_args()
    if np.finfo(np.longdouble).nmant < 63:
        sys.exit('longdouble is no wider than fp64 here: no yardstick')
    rng = np.random.default_rng(args.seed)
    t0 = time.time()
    overall = {w: np.zeros(3) for w in WHAT}
    lines = [f'tools/first_order_error_scale.py --orders {args.orders} --seed {args.seed}',
             'ratio of numpy with the training points in another order ("reordered") and with every ks entry moved by +-2 ulp as',
             'well ("moved") to numpy on the data as given, each against the longdouble value on the same alpha;',
             f'worst of {args.orders} orders x {fc.NY} outputs: maximum / rms over the 256 probes / per probe against max(E_np, floor)', '']
    for tier in ('emu', 'gpu', 'both'):
        for size in SHAPES[tier]:
            m, worst = model_ratios(size, args.orders, rng)
            for kind in ('reordered', 'moved'):
                for w in WHAT:
                    v = worst[kind][w]
                    overall[w] = np.maximum(overall[w], v)
                    lines.append(f'[{tier:4s}] {m.label:32s} {w:5s} {kind:9s}: max {v[0]:6.2f}  rms {v[1]:6.2f}  per probe {v[2]:6.2f}')
            print('\n'.join(lines[-8:]), flush=True)
    fused = np.zeros(2)
    for tier in ('emu', 'gpu'):
        for size in FUSED[tier]:
            m, v = fused_ratios(size, args.orders, rng)
            fused = np.maximum(fused, v)
            lines.append(f'[{tier:4s}] {m.label:32s} fused_mean (whole fit reordered, plain and moved): max {v[0]:6.2f}  rms {v[1]:6.2f}')
            print(lines[-1], flush=True)
    lines.append('')
    for w in WHAT:
        v = overall[w]
        lines.append(f'{w:10s}: worst ratio max / rms {max(v[0], v[1]):.2f} -> K_SET = {math.ceil(2 * max(v[0], v[1]))};  '
                     f'per probe {v[2]:.2f} -> K_POINT = {math.ceil(2 * v[2])}')
    lines.append(f'fused_mean: worst ratio max / rms {fused.max():.2f} -> K_SET = {math.ceil(2 * fused.max())}')
    lines.append(f'({time.time() - t0:.0f} s)')
    print('\n'.join(lines[-6:]))
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
