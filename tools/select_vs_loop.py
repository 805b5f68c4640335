#!/usr/bin/env python3
"""gpmpc_append_select against the same greedy selection written as the loop the older API allows.

N = 4096, d = 6, n = 1024 candidates, k = 128 picks, Ny = 1 and Ny = 3, wall clock around synchronised calls.
  new:  one gpmpc_append_select call.  Its phases by differences of whole calls (no brackets inside the call):
        Schur GEMMs ~ a selection-only call with k = 1 (upload, cross-covariances, two GEMMs, one step, download),
        selection steps ~ selection-only with k = 128 minus that, append ~ the full call minus selection-only.
  loop: per pick gpmpc_covar of the remaining candidates (two GEMMs of depth N and an n x n download), the arg-max of the
        summed diagonals on the host, gpmpc_append of the one row.
Both must give the same picks.  Also printed: the bytes the step kernels move on the pivot columns G (step t reads t
columns of Bp doubles per output and writes one) over the time of the steps -- the figure a faster step kernel would raise.
Writes profiles/select_vs_loop.txt (or --out)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
from gp_mpc_amd.synthetic import synthetic_problem
from gp_mpc_amd._lib import Handle, get_lib


def timed(f, h):
    h.synchronize()
    t0 = time.perf_counter()
    r = f()
    h.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def run(lib, N, d, Ny, n, k, reps, out):
    p = synthetic_problem(N, d, Ny, B=n, seed=1234, sn=1e-2)
    X, Y, H, C = p['X'], p['Y'], p['hyper'], p['Z']
    Yc = np.random.default_rng(4321).standard_normal((n, Ny))

    def fresh():
        h = Handle(lib, X, Y)
        assert np.all(h.fit(H) == 0)
        return h
    h = fresh()
    h.append_select(C, None, k)                                            # warm-up: code objects, scratch
    t_one = min(timed(lambda: h.append_select(C, None, 1), h)[0] for _ in range(reps))
    t_sel = min(timed(lambda: h.append_select(C, None, k), h)[0] for _ in range(reps))
    h.close()
    t_full = []
    for _ in range(reps):
        h = fresh()
        h.append_select(C, None, 1)
        ms, (sel, gain) = timed(lambda: h.append_select(C, Yc, k), h)
        t_full.append(ms)
        h.close()
    t_full = min(t_full)
    # the loop of the older API, once (it is the slow side)
    h = fresh()
    h.covar(C[:64])
    left = np.arange(n)
    picks = []
    h.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        cov = h.covar(C[left])
        j = int(np.argmax(np.einsum('aii->i', cov)))
        picks.append(int(left[j]))
        h.append(C[left[j]:left[j] + 1], Yc[left[j]:left[j] + 1])
        left = np.delete(left, j)
    h.synchronize()
    t_loop = (time.perf_counter() - t0) * 1e3
    h.close()
    picks = np.array(picks)
    same = np.array_equal(picks, sel)
    first = -1 if same else int(np.argmax(picks != sel))
    Bp = (n + 63) // 64 * 64
    t_steps = max(t_sel - t_one, 1e-6)
    g_bytes = 8.0 * Ny * Bp * (k * (k - 1) / 2 + k)
    lines = [f'N={N} d={d} Ny={Ny} n={n} k={k}  (wall clock, best of {reps}; the loop once)',
             f'  gpmpc_append_select        {t_full:10.2f} ms',
             f'    Schur GEMMs (k=1 call)   {t_one:10.2f} ms',
             f'    selection steps          {t_steps:10.2f} ms   ({t_steps / max(k - 1, 1) * 1e3:.1f} us per step; G traffic {g_bytes / 1e6:.1f} MB '
             f'-> {g_bytes / t_steps / 1e6:.1f} GB/s)',
             f'    append of {k} rows       {t_full - t_sel:10.2f} ms',
             f'  covar + arg-max + append loop {t_loop:8.2f} ms   ({t_loop / t_full:.1f} x)',
             f'  same picks: {same}' + ('' if same else f' (first difference at step {first}: loop {picks[first]}, call {sel[first]})'),
             f'  dominant phase of the new call: {"selection steps" if t_steps > max(t_one, t_full - t_sel) else ("Schur GEMMs" if t_one > t_full - t_sel else "append")}']
    for ln in lines:
        print(ln, flush=True)
        out.write(ln + '\n')
    out.flush()
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'select_vs_loop.txt'))
    ap.add_argument('--N', type=int, default=4096)
    ap.add_argument('--n', type=int, default=1024)
    ap.add_argument('--k', type=int, default=128)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    lib = get_lib()
    assert lib.device_count() >= 1
    ok = True
    with open(a.out, 'w') as out:
        out.write(f'tools/select_vs_loop.py on {lib.device_name()}\n')
        for Ny in (1, 3):
            ok &= run(lib, a.N, 6, Ny, a.n, a.k, a.reps, out)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
