"""How far equally good fp64 evaluations of the pathwise samples land from each other, measured against their longdouble
values (tests/paths_cases.py) at every model of both test tiers: the constants K_W, K_F, K_P of the paths gates, and the
feature-count table of the method's own error.  numpy on the data as given is the unit; against it
  * path weights v = alpha - K^-1 (Phi w + sn xi): the explicit-inverse route L^-T (L^-1 r) the library takes, cho_solve with
    every feature value moved by +-2 ulp at random, and numpy's whole computation on the training points in other orders (each
    against the longdouble value on its own factor);
  * evaluation f_s(z_s) and the grid evaluation: the kernel sum with the training points in --orders other orders and every
    kernel value moved by +-2 ulp at random (the accuracy the table exponential documents for itself, gp_kernels.hpp).
Per gate the worst ratio of numpy-variant error to numpy error (maximum, rms, and per point against max(E_np, floor)), and the
constant that follows: twice the worst ratio, rounded up.
Method error (numpy only, no gate): |C~ - exact posterior covariance| at model A for F = 64 .. 4096, in units of sf^2 and of the
largest posterior variance, so that users can choose F.  CPU only; nothing here reads a device.

Output: profiles/paths_error_scale.txt (and stdout)."""
import argparse
import math
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')]

import numpy as np                                   # noqa: E402
import gp_oracle as go                               # noqa: E402
import paths_cases as pc                             # noqa: E402

LD = pc.LD
# (model, S, F, paths whose weights are checked) of tests/test_emu_paths.py and tests/test_gpu_paths.py
CASES = [(pc.A, 96, 6, None), (pc.A, 300, 64, None), (pc.A, 601, 6, None), (pc.B1, 96, 64, None), (pc.B2, 96, 64, None), (pc.C1, 96, 64, None),
         (pc.C16, 96, 64, None), (pc.BIG, 512, 256, None)]
GRID_B = (1, 33, 65)


def moves(rng, shape):
    return rng.choice([-2.0, 2.0], size=shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--orders', type=int, default=32)
    ap.add_argument('--weight-orders', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'paths_error_scale.txt'))
    args = ap.parse_args()
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)
    worst = dict(W=0.0, F=0.0, P=0.0)
    say(f'# paths error scale: numpy against numpy, {args.orders} orders x +-2 ulp (evaluation), '
        f'{args.weight_orders} orders + inverse route + moved features (weights)')
    for size, S, F, ncols in CASES:
        rng = np.random.default_rng(S + F)
        p = go.synthetic_problem(size['N'], size['d'], size['Ny'], 8, seed=33, sn=size['sn'])
        X, Y, H, d, N = p['X'], p['Y'], p['hyper'], size['d'], size['N']
        o = go.fit(X, Y, H, want_invK=False)
        label = f"N={N} d={d} Ny={size['Ny']} sn={size['sn']:g} S={S} F={F}"
        cols = np.arange(S) if ncols is None else np.linspace(0, S - 1, ncols).astype(int)
        for a in range(size['Ny']):
            hk = H[a]
            om = rng.standard_normal((F // 2, d)) / hk[:d]
            w, xi = rng.standard_normal((S, F)), rng.standard_normal((S, N))
            base = (X, hk, o['chol'][a], o['alpha'][a], om, w[cols], xi[cols])
            truth = pc.weights(*base, dtype=LD)
            v_np = pc.weights(*base)
            e_np = pc.f64(np.abs(v_np.astype(LD) - truth))
            rw = []
            for v_var, t_var in ([(pc.weights(*base, route='inv'), truth), (pc.weights(*base, ulp=moves(rng, (N, F))), truth)]):
                e = pc.f64(np.abs(v_var.astype(LD) - t_var))
                rw.append(max(e.max() / e_np.max(), np.sqrt((e ** 2).mean() / (e_np ** 2).mean())))
            for _ in range(args.weight_orders):
                pm = rng.permutation(N)
                Xp, yp = X[pm], Y[pm, a]
                Kp = go.cov_se_ard_direct(Xp, Xp, hk[:d], hk[d] ** 2) + hk[d + 1] ** 2 * np.eye(N)
                Lp = np.linalg.cholesky(Kp)
                ap_ = pc.cho_solve((Lp, True), yp)
                perm_args = (Xp, hk, Lp, ap_, om, w[cols], xi[cols][:, pm])
                e = pc.f64(np.abs(pc.weights(*perm_args).astype(LD) - pc.weights(*perm_args, dtype=LD)))
                rw.append(max(e.max() / e_np.max(), np.sqrt((e ** 2).mean() / (e_np ** 2).mean())))
            worst['W'] = max(worst['W'], max(rw))
            # evaluation at the numpy weights of all S paths
            v_all = v_np if ncols is None else pc.weights(X, hk, o['chol'][a], o['alpha'][a], om, w, xi)
            Z = rng.standard_normal((S, d))
            ev = (X, hk, om, w, v_all, Z)
            t_f, floor, _ = pc.eval_own(*ev, dtype=LD)
            e0 = pc.f64(np.abs(pc.eval_own(*ev).astype(LD) - t_f))
            rf, rp = 0.0, 0.0
            for _ in range(args.orders):
                e = pc.f64(np.abs(pc.eval_own(*ev, perm=rng.permutation(N), ulp=moves(rng, (S, N))).astype(LD) - t_f))
                rf = max(rf, e.max() / e0.max(), np.sqrt((e ** 2).mean() / (e0 ** 2).mean()))
                rp = max(rp, float(np.max(e / np.maximum(e0, floor))))
            worst['F'], worst['P'] = max(worst['F'], rf), max(worst['P'], rp)
            say(f'{label} output {a}: weights E_np max {e_np.max():.2e} variants {max(rw):.2f} x | eval E_np max {e0.max():.2e} '
                f'(|f| ~ {float(np.abs(pc.f64(t_f)).mean()):.2f}) variants {rf:.2f} x, per point {rp:.2f} x max(E_np, floor)')
            if size is pc.A and F == 64:
                for B in GRID_B:
                    Zg = rng.standard_normal((B, d))
                    gv = (X, hk, om, w, v_all, Zg)
                    t_g, fl_g, _ = pc.eval_grid(*gv, dtype=LD)
                    g0 = pc.f64(np.abs(pc.eval_grid(*gv).astype(LD) - t_g))
                    ks, _ = pc.kernel_and_exponent(X, Zg, hk)
                    phi, _ = pc.features(Zg, om, hk[d])
                    rg, rgp = 0.0, 0.0
                    for _ in range(args.orders):
                        pm = rng.permutation(N)
                        km = ks * (1.0 + moves(rng, ks.shape) * pc.EPS)
                        f_var = (v_all[:, None, pm] * km[None, :, pm]).sum(axis=2) + w @ phi.T
                        e = pc.f64(np.abs(f_var.astype(LD) - t_g))
                        rg = max(rg, e.max() / g0.max(), np.sqrt((e ** 2).mean() / (g0 ** 2).mean()))
                        rgp = max(rgp, float(np.max(e / np.maximum(g0, fl_g))))
                    worst['F'], worst['P'] = max(worst['F'], rg), max(worst['P'], rgp)
                    say(f'    grid B={B}: E_np max {g0.max():.2e} variants {rg:.2f} x, per point {rgp:.2f} x')
    say()
    for k, name in (('W', 'K_W (weights, max and rms)'), ('F', 'K_F (evaluation, max and rms)'), ('P', 'K_P (evaluation, per point)')):
        say(f'{name}: worst ratio {worst[k]:.2f} -> constant {math.ceil(2.0 * worst[k])}')
    # ---- the method's own error: the prior's F features
    say()
    say('# method error at model A (40 probes drawn like the training inputs): |C~ - exact posterior covariance|, worst entry')
    p = go.synthetic_problem(pc.A['N'], pc.A['d'], pc.A['Ny'], 8, seed=33, sn=pc.A['sn'])
    X, H, d = p['X'], p['hyper'], pc.A['d']
    P = np.random.default_rng(5).standard_normal((40, d))
    for a in range(pc.A['Ny']):
        hk = H[a]
        K = go.cov_se_ard_direct(X, X, hk[:d], hk[d] ** 2) + hk[d + 1] ** 2 * np.eye(len(X))
        ks = go.cov_se_ard_direct(X, P, hk[:d], hk[d] ** 2)
        exact = go.cov_se_ard_direct(P, P, hk[:d], hk[d] ** 2) - ks.T @ np.linalg.solve(K, ks)
        vmax = float(np.diag(exact).max())
        for F in (64, 256, 1024, 4096):
            errs = []
            for rep in range(5):
                om = np.random.default_rng(100 * F + rep).standard_normal((F // 2, d)) / hk[:d]
                errs.append(float(np.abs(pc.corr_cov(X, hk, om, P)[0] - exact).max()))
            say(f'output {a} F={F:5d}: {min(errs) / hk[d] ** 2:.1e} .. {max(errs) / hk[d] ** 2:.1e} sf^2 = '
                f'{min(errs) / vmax:.2f} .. {max(errs) / vmax:.2f} of the largest posterior variance ({vmax / hk[d] ** 2:.1e} sf^2)')
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
