"""Pairs per second of the batched quantum Chernoff bound (fbx_chernoff_bound) on one GPU, against the host function
quantum_chernoff_bound (one fbx_eigh call and a scipy scalar search per pair) and against fbx_state_measures(fidelity), which also
does two eigendecompositions per item.  Also the certified share and the p50 / p99 of the evaluations per pair.

    python scripts/chernoff_time.py [--tol 1e-10] [--host-pairs 200]

2^16 random pairs at 1-3 qubits, 4096 at 4-5 qubits; half
full-rank, a quarter low-rank, a quarter nearly commuting (tests/chernoff_cases.py).  One JSON line per size."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "forest-benchmarking_amd"), os.path.join(ROOT, "tests")]

import chernoff_cases as cc  # noqa: E402
from fbx import _lib, distance_measures as dm  # noqa: E402


def pairs(nq, count, seed=1):
    """`count` pairs built from 64 distinct ones (generation on the host is not what is measured)"""
    rng = np.random.default_rng([seed, nq])
    d = 2 ** nq
    kinds = ["full", "full", "lowrank", "near"]
    base = [cc.golden_pair(kinds[k % 4], d, rng) for k in range(64)]
    idx = np.arange(count) % 64
    return np.array([b[0] for b in base])[idx], np.array([b[1] for b in base])[idx]


def timed(fn, reps=3):
    fn()                                                             # warm-up: code objects, workspaces
    best = np.inf
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        best = min(best, time.perf_counter() - t)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--host-pairs", type=int, default=200)
    args = ap.parse_args()
    _lib.set_device(0)
    for nq in (1, 2, 3, 4, 5):
        B = 1 << 16 if nq <= 3 else 4096
        rho, sigma = pairs(nq, B)
        t, (q, s, lower, iters) = timed(lambda: dm.quantum_chernoff_bound_batch(rho, sigma, tol=args.tol, return_bounds=True))
        tf, _ = timed(lambda: dm.state_measures_batch(rho, sigma, ("fidelity",)))
        nh = min(args.host_pairs, B)
        dm.quantum_chernoff_bound(rho[0], sigma[0])                  # warm-up: scipy import, eigensolver code objects
        th = time.perf_counter()
        for b in range(nh):
            dm.quantum_chernoff_bound(rho[b], sigma[b])
        th = (time.perf_counter() - th) / nh
        cert = iters >= 0
        ev = np.abs(iters)
        print(json.dumps({"n_qubits": nq, "pairs": B, "tol": args.tol, "seconds": round(t, 5),
                          "pairs_per_s": round(B / t, 1), "fidelity_items_per_s": round(B / tf, 1),
                          "host_pairs_per_s": round(1 / th, 2), "speedup_vs_host": round(B / t * th, 1),
                          "certified": round(float(cert.mean()), 5),
                          "max_rel_gap_uncertified": float(np.max(((q - lower) / np.maximum(q, 1e-12))[~cert]))
                          if (~cert).any() else 0.0,
                          "iters_p50": float(np.percentile(ev, 50)), "iters_p99": float(np.percentile(ev, 99))}),
              flush=True)


if __name__ == "__main__":
    main()
