#!/usr/bin/env python3
"""Whole-call times of gpmpc_rollout_mc next to what the library could already do for the same arithmetic: T times one
device-pointer gpmpc_predict_mean_var of B = S points, from the same run on the same box.

Cases: the C2 size (N = 4096, d = 6, Ny = 1) with S = 10 000 particles and T = 30 steps, and C3 (N = 8192, Ny = 6, d = 8) with
S = 4096; open loop, no particle record, generator path.  Wall clock around synchronised calls, best of --reps.
  rollout_mc: the whole call (one upload, T x (prediction + hand-over + moments), one download).
  T x predict: T times the best time of one gpmpc_predict_mean_var of S points with device pointers (no copies).
  new kernels: the GPMPC_PH_MC brackets of one more call with only that phase profiled (particle init, T hand-overs, 4 T
               moment launches), summed.
Records, not gates.  Writes profiles/mc_rollout.txt (or --out)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
from gp_mpc_amd.synthetic import synthetic_problem
from gp_mpc_amd._lib import Handle, get_lib

CASES = [dict(name='C2', N=4096, d=6, Ny=1, S=10000, T=30), dict(name='C3', N=8192, d=8, Ny=6, S=4096, T=30)]


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mc_rollout.txt'))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cases', nargs='+', default=[c['name'] for c in CASES])
    a = ap.parse_args()
    lib = get_lib()
    assert lib.device_count() >= 1
    lines = [f'tools/mc_rollout_times.py on {lib.device_name()}',
             f'wall clock around synchronised calls, best of {a.reps}; open loop, noise on, no particle record, seed 1']
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
        run = lambda: h.rollout_mc(S, T, z0, S0, U=U, seed=1, noise=True)
        mean, cov = run()                                          # warm-up: scratch, code objects
        assert np.all(np.isfinite(mean)) and np.all(np.isfinite(cov))
        t_mc = timed(run, h, a.reps)
        h.profile_enable(True, ['mc'])
        run()
        ms_new, launches = h.profile_read()['mc']
        h.profile_enable(False)
        Z = torch.from_numpy(z0 + 0.1 * rng.standard_normal((S, d))).cuda()
        m, v = torch.zeros(S, Ny, dtype=torch.float64, device='cuda'), torch.zeros(S, Ny, dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        h.set_pointer_mode(True)
        pred = lambda: h.predict_mean_var_dev(S, Z.data_ptr(), m.data_ptr(), v.data_ptr())
        pred()
        t_pred = timed(pred, h, max(a.reps, 10))
        h.set_pointer_mode(False)
        h.close()
        over = 100.0 * (t_mc - T * t_pred) / (T * t_pred)
        lines += [f"{c['name']}: N={N} d={d} Ny={Ny}  S={S} particles, T={T} steps",
                  f'  gpmpc_rollout_mc (whole call)               {t_mc:10.3f} ms',
                  f'  T x gpmpc_predict_mean_var(B = S), device   {T * t_pred:10.3f} ms  ({t_pred:.3f} ms each)',
                  f'  on top of the T predictions                 {t_mc - T * t_pred:10.3f} ms  ({over:+.1f} %)',
                  f'  new kernels (init, hand-over, moments)      {ms_new:10.3f} ms in {launches} brackets']
    with open(a.out, 'w') as out:
        for ln in lines:
            print(ln, flush=True)
            out.write(ln + '\n')


if __name__ == '__main__':
    main()
