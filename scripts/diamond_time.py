"""Device rate of the batched diamond-norm distance (fbx_diamond_norm_dev) against the host solver.

    python scripts/diamond_time.py [--n2 65536] [--n3 4096] [--host-sample 8]

Times 2-qubit pairs against one shared target (the identity channel) and 3-qubit pairs with explicit targets, inputs and outputs
resident in HBM (one warm-up launch of a small batch first), and reports pairs/s, the distribution of iters_out (negative = tol not
reached) and the host solver's (distance_measures.diamond_norm_distance) per-pair rate on a sample.  One JSON line per size."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "forest-benchmarking_amd"))
from fbx import _lib, distance_measures as dm  # noqa: E402


def kraus_choi(k):                       # [B, r, d, d] Kraus operators -> [B, d^2, d^2] Choi (column-stacking vec)
    B, r, d, _ = k.shape
    v = k.transpose(0, 1, 3, 2).reshape(B, r, d * d)
    return np.einsum("bri,brj->bij", v, v.conj())


def channels(B, d, rs):
    """Half random rank-2 channels, half near-unitary channels (small random rotation plus a little depolarising)."""
    rank = 2
    g = rs.randn(B, d * rank, d) + 1j * rs.randn(B, d * rank, d)
    q, _ = np.linalg.qr(g)
    c = kraus_choi(q.reshape(B, rank, d, d))
    h = rs.randn(B, d, d) + 1j * rs.randn(B, d, d)
    h = 1e-2 * (h + h.conj().transpose(0, 2, 1))
    w, v = np.linalg.eigh(h)
    u = np.einsum("bij,bj,bkj->bik", v, np.exp(-1j * w), v.conj())
    p = 1e-2 * rs.rand(B)
    cu = (1 - p)[:, None, None] * kraus_choi(u[:, None]) + p[:, None, None] * np.eye(d * d) / d
    c[1::2] = cu[1::2]
    return np.ascontiguousarray(c)


def run(nq, B, shared, host_sample, rs, reps=3):
    d = 2 ** nq
    c0 = channels(B, d, rs)
    c1 = kraus_choi(np.eye(d, dtype=complex)[None, None]) if shared else channels(B, d, rs)
    DB, lib = _lib.DeviceBuffer, _lib.lib()
    d0, d1 = DB.from_array(c0), DB.from_array(c1)
    dd, du, di = DB(B * 8), DB(B * 8), DB(B * 4)
    args = lambda n: (nq, n, d0.ptr, d1.ptr, int(shared), 1e-7, 200, dd.ptr, du.ptr, None, di.ptr)   # noqa: E731
    _lib.check(lib.fbx_diamond_norm_dev(*args(min(B, 256))))                      # warm-up (workspace, code objects)
    _lib.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        _lib.check(lib.fbx_diamond_norm_dev(*args(B)))
        _lib.synchronize()
        times.append(time.perf_counter() - t0)
    dist = dd.to_array(np.float64, (B,))
    upper = du.to_array(np.float64, (B,))
    iters = di.to_array(np.int32, (B,))
    t = min(times)
    host_t = []
    for b in range(min(host_sample, B)):
        t0 = time.perf_counter()
        h = dm.diamond_norm_distance(c0[b], c1[0] if shared else c1[b])
        host_t.append(time.perf_counter() - t0)
        assert dist[b] >= h - 1e-9 * max(1.0, h) and upper[b] >= h - 1e-12, (b, dist[b], upper[b], h)
    host_rate = len(host_t) / sum(host_t) if host_t else None
    conv = iters >= 0
    rel_gap = (upper - dist) / np.maximum(dist, 1e-12)
    out = {"n_qubits": nq, "pairs": B, "shared_target": bool(shared), "seconds": t, "times": times, "pairs_per_s": B / t,
           "converged_fraction": float(conv.mean()),
           "iters_percentiles_converged": np.percentile(iters[conv], [0, 50, 90, 99, 100]).tolist() if conv.any() else None,
           "iters_not_converged_max": int(-iters[~conv].min()) if (~conv).any() else 0,
           "rel_gap_max": float(rel_gap.max()), "host_pairs_per_s": host_rate,
           "speedup_vs_one_host_process": (B / t) / host_rate if host_rate else None}
    for buf in (d0, d1, dd, du, di):
        buf.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n2", type=int, default=65536)
    ap.add_argument("--n3", type=int, default=4096)
    ap.add_argument("--host-sample", type=int, default=8)
    a = ap.parse_args()
    _lib.set_device(0)
    rs = np.random.RandomState(2026)
    if a.n2:
        print(json.dumps(run(2, a.n2, True, a.host_sample, rs)), flush=True)
    if a.n3:
        print(json.dumps(run(3, a.n3, False, a.host_sample, rs)), flush=True)


if __name__ == "__main__":
    main()
