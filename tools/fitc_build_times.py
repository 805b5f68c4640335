#!/usr/bin/env python3
"""Whole-call times of gpmpc_sparse_fitc and what a prediction on the sparse handle costs, next to the exact model's figures
from the same run on the same box.

N = 8192, Ny = 6, d = 8, M = 512 and 1024 inducing points (a seeded random subset), wall clock around synchronised calls,
best of --reps.
  build:   gpmpc_sparse_fitc on a source handle that was never fitted (hyper given: nothing N x N is allocated).
  update:  the rank updates B += Vs Vs^T alone -- the GPMPC_PH_VARGEMM bracket of the new handle (the build inherits the
           source's profiling switch) -- as TFLOP/s of the lower tiles actually computed, against gpmpc_mfma_selftest's
           issue-bound rate of the fp64 matrix instruction.
  predict: one 'TA' prediction with B = 1 (host pointers) on the sparse handle.
  exact:   gpmpc_fit at that N and the same B = 1 prediction on the exact model.
Records, not gates.  Writes profiles/fitc_build.txt (or --out)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
from gp_mpc_amd.synthetic import synthetic_problem
from gp_mpc_amd._lib import Handle, get_lib


def timed(f, h, reps):
    best = float('inf')
    r = None
    for _ in range(reps):
        h.synchronize()
        t0 = time.perf_counter()
        r = f()
        h.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fitc_build.txt'))
    ap.add_argument('--N', type=int, default=8192)
    ap.add_argument('--Ny', type=int, default=6)
    ap.add_argument('--d', type=int, default=8)
    ap.add_argument('--M', type=int, nargs='+', default=[512, 1024])
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    lib = get_lib()
    assert lib.device_count() >= 1
    layout, peak = lib.mfma_selftest(0)
    p = synthetic_problem(a.N, a.d, a.Ny, B=4, seed=1234, sn=1e-2)
    X, Y, H, Z, S = p['X'], p['Y'], p['hyper'], p['Z'][:1], p['Sigma'][:1]
    lines = [f'tools/fitc_build_times.py on {lib.device_name()}',
             f'N={a.N} d={a.d} Ny={a.Ny}  (wall clock around synchronised calls, best of {a.reps}); '
             f'fp64 MFMA issue-bound rate (gpmpc_mfma_selftest): {peak:.1f} TFLOP/s']
    src = Handle(lib, X, Y)                                   # never fitted: the build gets the hyper-parameters
    rng = np.random.default_rng(97)
    for M in a.M:
        Xu = np.ascontiguousarray(X[np.sort(rng.choice(a.N, M, replace=False))])
        src.sparse_fitc(Xu, H).close()                        # warm-up: code objects
        held = []

        def build():
            s = src.sparse_fitc(Xu, H)
            held.append(s)
            return s
        t_build, s = timed(build, src, a.reps)
        for x in held[:-1]:
            x.close()
        src.profile_enable(True, ['vargemm'])
        sp = src.sparse_fitc(Xu, H)
        src.profile_enable(False)
        ms_upd, launches = sp.profile_read()['vargemm']
        sp.close()
        Mp = (M + 63) // 64 * 64
        T = Mp // 64
        Np = (a.N + 63) // 64 * 64                            # (rows of the chunks, padded per chunk: a lower bound on the work done)
        flop = 2.0 * a.Ny * (T * (T + 1) / 2) * 64 * 64 * Np
        s.predict('TA', Z, S)
        t_pred, _ = timed(lambda: s.predict('TA', Z, S), s, max(a.reps, 20))
        lines += [f'M={M}:',
                  f'  gpmpc_sparse_fitc (whole call)     {t_build:10.2f} ms',
                  f'  rank updates B += Vs Vs^T          {ms_upd:10.3f} ms in {launches} launches: {flop / (ms_upd * 1e-3) * 1e-12:.2f} TFLOP/s '
                  f'({100.0 * flop / (ms_upd * 1e-3) * 1e-12 / peak:.0f} % of the issue-bound rate)',
                  f"  'TA' prediction, B = 1, sparse     {t_pred * 1e3:10.1f} us"]
        s.close()
    src.close()
    h = Handle(lib, X, Y)
    h.fit(H)                                                  # warm-up (allocates the N x N blocks)
    t_fit, _ = timed(lambda: h.fit(H), h, a.reps)
    h.predict('TA', Z, S)
    t_pe, _ = timed(lambda: h.predict('TA', Z, S), h, max(a.reps, 20))
    h.close()
    lines += ['exact model, same run:',
              f'  gpmpc_fit                          {t_fit:10.2f} ms',
              f"  'TA' prediction, B = 1, exact      {t_pe * 1e3:10.1f} us"]
    with open(a.out, 'w') as out:
        for ln in lines:
            print(ln, flush=True)
            out.write(ln + '\n')


if __name__ == '__main__':
    main()
