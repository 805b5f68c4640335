#!/usr/bin/env python3
"""gpmpc_remove against what a user does without it: a fit on the remaining rows.

Per grid point (N, Ny, n, which points) three whole calls, wall clock around synchronised calls (gpmpc_remove and gpmpc_fit
block until their results are there, and the removal's host side -- the data buffers, the new workspace -- belongs to the
call), best of --reps after one untimed call of each kind on a model of the same size:
  downdate  gpmpc_remove with remove_mode 1 (Householder downdate of L and L^-1, remove_kernels.hpp)
  refit     gpmpc_remove with remove_mode 2 (new buffers + gpmpc_fit inside the call)
  fit       gpmpc_fit on a model that holds the remaining rows already: the yardstick, code the removal does not touch
and the branch the automatic rule (remove_mode 0) takes.  d = 6.  Removed points: the n oldest (every panel is reflected:
the worst case) and n scattered ones.  Every timed removal starts from a freshly fitted model of N points.
Writes profiles/remove_vs_refit.txt (or --out); exits 1 if the automatic rule takes the slower measured branch anywhere."""
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
    f()
    h.synchronize()
    return (time.perf_counter() - t0) * 1e3


def run(lib, p, N, Ny, n, kind, reps, out):
    X, Y, H = p['X'], p['Y'], p['hyper']
    if kind == 'oldest':
        idx = np.arange(n)
    else:
        idx = np.sort(np.random.default_rng(7).choice(N, size=n, replace=False))
    keep = np.ones(N, dtype=bool)
    keep[idx] = False

    def removal(mode):
        h = Handle(lib, X, Y)
        assert np.all(h.fit(H) == 0)
        lib.set_tuning('remove_mode', mode)
        try:
            ms = timed(lambda: h.remove(idx), h)
            took = 'downdate' if h.counter('remove_downdates') else 'refit'
        finally:
            lib.set_tuning('remove_mode', -1)
        h.close()
        return ms, took

    t = {}
    for name, mode in (('downdate', 1), ('refit', 2)):
        removal(mode)                                          # warm-up: code objects, the block list
        t[name] = min(removal(mode)[0] for _ in range(reps))
    h = Handle(lib, X[keep], Y[keep])
    assert np.all(h.fit(H) == 0)
    t['fit'] = min(timed(lambda: h.fit(H), h) for _ in range(reps))
    h.close()
    auto = removal(0)[1]
    faster = 'downdate' if t['downdate'] < t['refit'] else 'refit'
    ok = auto == faster or abs(t['downdate'] - t['refit']) <= 0.05 * min(t['downdate'], t['refit'])
    ln = (f'N={N:5d} Ny={Ny} n={n:3d} {kind:9s}  downdate {t["downdate"]:8.2f} ms   refit {t["refit"]:8.2f} ms   fit {t["fit"]:8.2f} ms   '
          f'automatic: {auto}' + ('' if ok else '   <-- the slower branch'))
    print(ln, flush=True)
    out.write(ln + '\n')
    out.flush()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'remove_vs_refit.txt'))
    ap.add_argument('--N', type=int, nargs='+', default=[1024, 4096, 8192])
    ap.add_argument('--Ny', type=int, nargs='+', default=[1, 6])
    ap.add_argument('--n', type=int, nargs='+', default=[1, 64, 256])
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    lib = get_lib()
    assert lib.device_count() >= 1
    ok = True
    with open(a.out, 'w') as out:
        out.write(f'tools/remove_vs_refit.py on {lib.device_name()}: whole calls, wall clock, best of {a.reps} (ties within 5 % count as either branch)\n')
        for N in a.N:
            for Ny in a.Ny:
                p = synthetic_problem(N, 6, Ny, B=1, seed=1234, sn=1e-2)
                for n in a.n:
                    for kind in ('oldest', 'scattered'):
                        ok &= run(lib, p, N, Ny, n, kind, a.reps, out)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
