"""Items per second of the fused 4- and 5-qubit state kernels (fbx_state_measures, fbx_proj_state_physical) on one GPU, against
the composition of generic primitives they replace (distance_measures._state_measures_large: fbx_eigh / fbx_matmul with numpy
in between; project_state_matrix._project_general) on the same inputs in the same run.  Both through the host-pointer entries,
copies included.

    python scripts/state_measures_time.py [--items 4096] [--reps 7] [--qubits 4 5]

Fidelity only and projection only.  The two paths are timed alternately, `reps` times each after a warm-up of both; the rates are
those of the median time, `spread` is (slowest - fastest) / median over the repetitions.  The largest difference of the two
paths' outputs on these inputs is reported beside the rates.  One JSON line per size."""
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
from fbx.operator_tools import project_state_matrix as psm  # noqa: E402


def pairs(nq, count, seed=1):
    """`count` full-rank pairs built from 64 distinct ones (generation on the host is not what is measured)"""
    rng = np.random.default_rng([seed, nq])
    d = 2 ** nq
    base = [cc.golden_pair("full", d, rng) for _ in range(64)]
    idx = np.arange(count) % 64
    return np.array([b[0] for b in base])[idx], np.array([b[1] for b in base])[idx]


def indefinite(nq, count, seed=2):
    """`count` Hermitian trace-one matrices with negative eigenvalues, built from 64 distinct ones"""
    rng = np.random.default_rng([seed, nq])
    d = 2 ** nq
    h = rng.standard_normal((64, d, d)) + 1j * rng.standard_normal((64, d, d))
    h = h + h.conj().transpose(0, 2, 1)
    h = h / np.trace(h, axis1=1, axis2=2).real[:, None, None]
    return h[np.arange(count) % 64]


def alternate(fns, reps):
    """every function once as warm-up, then `reps` rounds of all of them in turn: per function (times, last output)"""
    outs = [fn() for fn in fns]
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            t = time.perf_counter()
            outs[k] = fn()                                           # the host-pointer entries synchronise before they return
            times[k].append(time.perf_counter() - t)
    return [np.array(t) for t in times], outs


def rate(B, t):
    med = float(np.median(t))
    return {"items_per_s": round(B / med, 1), "seconds": round(med, 5), "spread": round(float((t.max() - t.min()) / med), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--qubits", type=int, nargs="+", default=[4, 5])
    args = ap.parse_args()
    _lib.set_device(0)
    B = args.items
    for nq in args.qubits:
        rho, sigma = pairs(nq, B)
        (tf, tc), (f, fc) = alternate([lambda: dm.state_measures_batch(rho, sigma, ("fidelity",))["fidelity"],
                                       lambda: dm._state_measures_large(rho, sigma, ("fidelity",))["fidelity"]], args.reps)
        h = indefinite(nq, B)
        (tp, tg), (p, pg) = alternate([lambda: psm.project_state_matrix_to_physical_batch(h),
                                       lambda: psm._project_general(h)], args.reps)
        print(json.dumps({"n_qubits": nq, "items": B, "reps": args.reps,
                          "fidelity_fused": rate(B, tf), "fidelity_composed": rate(B, tc),
                          "fidelity_ratio": round(float(np.median(tc) / np.median(tf)), 2),
                          "fidelity_max_abs_diff": float(np.abs(f - fc).max()),
                          "projection_fused": rate(B, tp), "projection_composed": rate(B, tg),
                          "projection_ratio": round(float(np.median(tg) / np.median(tp)), 2),
                          "projection_max_abs_diff": float(np.abs(p - pg).max())}), flush=True)


if __name__ == "__main__":
    main()
