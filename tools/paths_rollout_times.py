#!/usr/bin/env python3
"""Whole-call times of the consistent Monte Carlo roll-out (gpmpc_paths_draw + gpmpc_rollout_paths) next to gpmpc_rollout_mc,
from the same run on the same box, and the evaluation kernel's share of the machine.

Cases: the C2 size (N = 4096, d = 6, Ny = 1) with S = 10 000 particles and T = 30 steps, and C3 (N = 8192, Ny = 6, d = 8) with
S = 4096; open loop, noise on, no particle record, generator path, F = 1024 features.  Wall clock around synchronised calls,
best of --reps.
  rollout_mc:     the whole call (the yardstick; independent draws per step).
  paths_draw:     the whole setup (features, three matrix products per block of 512 paths).
  rollout_paths:  the whole call (one upload, T x (evaluation + second pass + moments), one download).
  kernel 3 alone: the GPMPC_PH_MC bracket of gpmpc_paths_eval, which holds paths_eval_kernel only (its second pass,
      paths_finish_kernel, is bracketed as 'finish' and given next to it), best of the repetitions, one phase profiled at a
      time.  Two roofline fractions of the kernel, per the least time either resource allows:
        HBM: the bytes it must read, the weight streams V (Ny Np S x 8) and W (Ny F S x 8), over 8 TB/s;
        exp: the kernel values it forms, Ny N S exponentials of 2 d + 18 fp64 VALU instructions each (a subtraction and an fma
             per dimension, exp_tab32_neg's 17, the accumulating fma: counted in the source, not measured) and Ny F/2 S
             sine-cosine pairs (not counted: their instruction count is the math library's), over the chip's fp64 VALU
             issue rate 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3 T lane-instructions/s.
Records, not gates.  Writes profiles/paths_rollout.txt (or --out)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
from gp_mpc_amd.synthetic import synthetic_problem
from gp_mpc_amd._lib import Handle, get_lib

CASES = [dict(name='C2', N=4096, d=6, Ny=1, S=10000, T=30), dict(name='C3', N=8192, d=8, Ny=6, S=4096, T=30)]
HBM_PEAK = 8.0e12
VALU_F64_PEAK = 256 * 4 * 16 * 2.4e9          # fp64 lane-instructions per second, full-rate instructions


def timed(f, h, reps):
    best = float('inf')
    for _ in range(reps):
        h.synchronize()
        t0 = time.perf_counter()
        f()
        h.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'paths_rollout.txt'))
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--features', type=int, default=1024)
    ap.add_argument('--cases', nargs='+', default=[c['name'] for c in CASES])
    a = ap.parse_args()
    lib = get_lib()
    assert lib.device_count() >= 1
    F = a.features
    lines = [f'tools/paths_rollout_times.py on {lib.device_name()}',
             f'wall clock around synchronised calls, best of {a.reps}; open loop, noise on, no particle record, seed 1, F = {F}']
    for c in CASES:
        if c['name'] not in a.cases:
            continue
        N, d, Ny, S, T = c['N'], c['d'], c['Ny'], c['S'], c['T']
        p = synthetic_problem(N, d, Ny, B=4, seed=1234, sn=1e-2)
        h = Handle(lib, p['X'], p['Y'])
        assert np.all(h.fit(p['hyper']) == 0)
        rng = np.random.default_rng(5)
        z0, U = p['Z'][0], 0.3 * rng.standard_normal((T, d - Ny))
        S0 = np.eye(d) * 1e-6
        S0[:Ny, :Ny] = np.diag(p['hyper'][:, d + 1] ** 2)
        run_mc = lambda: h.rollout_mc(S, T, z0, S0, U=U, seed=1, noise=True)
        draw = lambda: h.paths_draw(S, F, seed=1)
        run_paths = lambda: h.rollout_paths(T, z0, S0, U=U, seed=1, noise=True)
        mean, cov = run_mc()                                       # warm-up: scratch, code objects
        assert np.all(np.isfinite(mean)) and np.all(np.isfinite(cov))
        draw()
        mean_p, cov_p = run_paths()
        assert np.all(np.isfinite(mean_p)) and np.all(np.isfinite(cov_p))
        t_mc = timed(run_mc, h, a.reps)
        t_draw = timed(draw, h, a.reps)
        t_paths = timed(run_paths, h, a.reps)
        Z = z0 + 0.1 * rng.standard_normal((S, d))
        h.paths_eval(Z)
        best, best_fin = float('inf'), float('inf')
        for _ in range(max(a.reps, 5)):
            for phase in ('mc', 'finish'):
                h.profile_enable(True, [phase])
                h.paths_eval(Z)
                ms = h.profile_read()[phase][0]
                h.profile_enable(False)
                if phase == 'mc':
                    best = min(best, ms)
                else:
                    best_fin = min(best_fin, ms)
        Np = (N + 63) // 64 * 64
        bytes_v, bytes_w = 8.0 * Ny * Np * S, 8.0 * Ny * F * S
        exps, pairs = float(Ny) * N * S, float(Ny) * (F // 2) * S
        h.close()
        lines += [f"{c['name']}: N={N} d={d} Ny={Ny}  S={S} particles, T={T} steps",
                  f'  gpmpc_rollout_mc (whole call)                 {t_mc:10.3f} ms',
                  f'  gpmpc_paths_draw (whole call)                 {t_draw:10.3f} ms',
                  f'  gpmpc_rollout_paths (whole call)              {t_paths:10.3f} ms',
                  f'  draw + roll-out against rollout_mc            {t_draw + t_paths:10.3f} ms  ({t_mc / (t_draw + t_paths):.2f} x)',
                  f'  kernel 3 alone (paths_eval_kernel, events)    {best:10.3f} ms   second pass {best_fin:.3f} ms',
                  f'    HBM: V {bytes_v / 1e9:.3f} GB + W {bytes_w / 1e9:.3f} GB at {(bytes_v + bytes_w) / (best * 1e-3) / 1e12:.2f} TB/s = '
                  f'{100.0 * (bytes_v + bytes_w) / (best * 1e-3) / HBM_PEAK:.0f} % of 8 TB/s',
                  f'    exp: {exps / (best * 1e-3) / 1e9:.0f} G exponentials/s x {2 * d + 18} instructions = '
                  f'{100.0 * exps * (2 * d + 18) / (best * 1e-3) / VALU_F64_PEAK:.0f} % of {VALU_F64_PEAK / 1e12:.1f} T fp64 lane-instructions/s '
                  f'(+ {pairs / (best * 1e-3) / 1e9:.1f} G sine-cosine pairs/s, not counted)']
    with open(a.out, 'w') as out:
        for ln in lines:
            print(ln, flush=True)
            out.write(ln + '\n')


if __name__ == '__main__':
    main()
