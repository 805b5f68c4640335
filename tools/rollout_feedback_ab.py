#!/usr/bin/env python3
"""Closed-loop roll-outs: one lock-step call (gpmpc_rollout_multi_feedback) against the same trajectories as consecutive
gpmpc_rollout_feedback calls, in ONE process on one GPU, the two variants interleaved round by round.

    python tools/rollout_feedback_ab.py [--N 8192 --Ny 6 --d 8 --T 30] [--rounds 5] [--commit TEXT] [--out FILE]

Default model: the C3 size (N = 8192, Ny = 6, d = 8, T = 30, inputs from gp_mpc_amd/synthetic.py).  Cases: 2, 8 and 32 closed
'TA' trajectories (different starts and gains), and ['ME', 'TA', 'EM'] closed from one start.  A time is a host clock around a
call that ends in the library's own synchronise (results are back on the host); every case is warmed with two calls of each
variant.  Prints the table (ms per call: mean and min over the rounds, ratio sequential / lock-step of the means), the largest
difference between the two variants' results, and one JSON line; --out writes the same text."""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gp_mpc_amd._lib import Handle, get_lib            # noqa: E402
from gp_mpc_amd.synthetic import synthetic_problem     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--N', type=int, default=8192)
    ap.add_argument('--Ny', type=int, default=6)
    ap.add_argument('--d', type=int, default=8)
    ap.add_argument('--T', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    N, Ny, d, T, Nu = a.N, a.Ny, a.d, a.T, a.d - a.Ny
    lib = get_lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    p = synthetic_problem(N, d, Ny, 64, seed=1234, sn=0.1)
    h = Handle(lib, p['X'], p['Y'])
    t0 = time.perf_counter()
    assert np.all(h.fit(p['hyper'], want_invK=True) == 0)
    say(f'box: {socket.gethostname()} / {lib.device_name(0)}   commit: {a.commit}')
    say(f'model: N={N} Ny={Ny} d={d} T={T} (fit with K^-1: {time.perf_counter() - t0:.1f} s)   rounds: {a.rounds}, interleaved')
    rng = np.random.default_rng(7)
    S0 = np.eye(d) * 1e-6
    S0[:Ny, :Ny] = np.diag(p['hyper'][:, d + 1] ** 2)
    Z = p['Z'][:32]
    Kz = 0.05 * rng.standard_normal((32, Nu, Ny))
    k0 = 0.05 * rng.standard_normal((32, Nu))
    Kc = 0.05 * rng.standard_normal((32, Nu, Ny))
    sf2 = (p['hyper'][:, d] ** 2).max()
    cases = [(f"{M} x 'TA'", ['TA'] * M, list(range(M))) for M in (2, 8, 32)]
    cases.append(("'ME','TA','EM' one start", ['ME', 'TA', 'EM'], [0, 0, 0]))
    say('%-28s %12s %12s %12s %12s %8s' % ('case', 'lockstep ms', '(min)', 'sequential', '(min)', 'ratio'))
    result = {}
    for label, methods, idx in cases:
        def lockstep():
            return h.rollout_multi_feedback(methods, Z[idx], S0, Kz[idx], k0[idx], Kc[idx], T=T)

        def sequential():
            out = [h.rollout_feedback(m, T, Z[i], S0, Kz[i], k0[i], Kc[i]) for m, i in zip(methods, idx)]
            return tuple(np.stack([o[k] for o in out]) for k in range(3))
        for _ in range(2):
            a_res, b_res = lockstep(), sequential()
        diff = [float(np.abs(x - y).max()) for x, y in zip(a_res, b_res)]
        tl, ts = [], []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            lockstep()
            t1 = time.perf_counter()
            sequential()
            t2 = time.perf_counter()
            tl.append((t1 - t0) * 1e3)
            ts.append((t2 - t1) * 1e3)
        ml, ms = float(np.mean(tl)), float(np.mean(ts))
        say('%-28s %12.3f %12.3f %12.3f %12.3f %8.2f' % (label, ml, min(tl), ms, min(ts), ms / ml))
        say('%-28s   max |lock-step - sequential|: mean %.1e  cov %.1e (sf^2 = %.2g)  controls %.1e' % ('', diff[0], diff[1], sf2, diff[2]))
        result[label] = dict(lockstep_ms=ml, lockstep_min_ms=min(tl), sequential_ms=ms, sequential_min_ms=min(ts), ratio=ms / ml,
                             max_diff_mean=diff[0], max_diff_cov=diff[1], max_diff_controls=diff[2])
    h.close()
    print(json.dumps(dict(N=N, Ny=Ny, d=d, T=T, rounds=a.rounds, cases=result)), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
