"""Sequences per second of fbx_rb_simulate_dev (and of fbx_rb_sequences_dev, which feeds it) on one GPU, buffers resident, timed with
device events, next to the dense numpy loop (a d^2 x d^2 product per step) on one core.

    python scripts/rb_sim_time.py [--qubits 1 2] [--depths 10 100 500] [--batches 10000 1000000] [--reps 7] [--cpu-sequences 200]

Every configuration runs once as warm-up and then `reps` times; the rate is that of the median time, `spread` is
(slowest - fastest) / median.  All sequences of a configuration have the same length and share one noise PTM (a wave-uniform noise
id: the broadcast case).  The numpy loop runs `--cpu-sequences` sequences and is scaled.  A configuration whose element words would
need more than --max-bytes of HBM is skipped and says so.  One JSON line per configuration."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "forest-benchmarking_amd")]

from fbx import _lib, clifford  # noqa: E402


def timed_dev(launch, reps):
    lib = _lib.lib()
    launch(); _lib.synchronize()
    out = []
    ms = C.c_double(0.0)
    for _ in range(reps):
        _lib.check(lib.fbx_timer_begin())
        launch()
        _lib.check(lib.fbx_timer_end(C.byref(ms)))
        out.append(ms.value * 1e-3)
    t = np.asarray(out)
    med = float(np.median(t))
    return med, round(float((t.max() - t.min()) / med), 3)


def numpy_loop(n, elems, depth, count, lam):
    tables = {}
    D = 4 ** n
    prep = np.zeros(D)
    prep[0] = prep[3] = 1.0
    t0 = time.perf_counter()
    for b in range(count):
        v = prep
        for e in elems[b * depth:(b + 1) * depth]:
            p = tables.get(e)
            if p is None:
                p = tables[e] = clifford.to_ptm(int(e), n)
            v = lam @ (p @ v)
    return (time.perf_counter() - t0) / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--depths", type=int, nargs="+", default=[10, 100, 500])
    ap.add_argument("--batches", type=int, nargs="+", default=[10000, 1000000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-sequences", type=int, default=200)
    ap.add_argument("--max-bytes", type=float, default=8e9)
    args = ap.parse_args()
    _lib.set_device(0)
    lib, DB = _lib.lib(), _lib.DeviceBuffer
    for n in args.qubits:
        D = 4 ** n
        lam = np.diag([1.0] + [0.99] * (D - 1)) + 1e-3 * np.random.default_rng(0).normal(size=(D, D))
        lam[0] = np.eye(D)[0]
        for depth in args.depths:
            for B in args.batches:
                total = B * depth
                row = {"what": "fbx_rb_simulate_dev", "n_qubits": n, "depth": depth, "batch": B, "reps": args.reps}
                if 5 * total > args.max_bytes:
                    print(json.dumps(dict(row, skipped="element words exceed --max-bytes")), flush=True)
                    continue
                off = np.arange(B + 1, dtype=np.int64) * depth
                d_off, d_e, d_i = DB.from_array(off), DB(4 * total), DB(total)
                d_l, d_out = DB.from_array(lam), DB(8 * B * D)
                gen = timed_dev(lambda: _lib.check(lib.fbx_rb_sequences_dev(n, B, d_off.ptr, 1, _lib.CLIFFORD_NONE, 1, d_e.ptr, d_i.ptr)),
                                args.reps)
                sim = timed_dev(lambda: _lib.check(lib.fbx_rb_simulate_dev(n, B, d_off.ptr, d_e.ptr, d_i.ptr, 1, d_l.ptr, None, d_out.ptr)),
                                args.reps)
                _lib.synchronize()
                count = min(args.cpu_sequences, B)
                elems = d_e.to_array(np.uint32, (count * depth,))
                cpu = numpy_loop(n, elems.tolist(), depth, count, lam)
                for b in (d_off, d_e, d_i, d_l, d_out):
                    b.free()
                print(json.dumps(dict(row, seconds=round(sim[0], 6), spread=sim[1], sequences_per_s=round(B / sim[0], 1),
                                      steps_per_s=round(total / sim[0], 1), fp64_flops_per_s=round(2.0 * D * D * total / sim[0], 1),
                                      generate_seconds=round(gen[0], 6), generate_spread=gen[1],
                                      generate_sequences_per_s=round(B / gen[0], 1),
                                      numpy_one_core_sequences_per_s=round(1.0 / cpu, 1), numpy_sequences_timed=count,
                                      speedup_over_numpy_one_core=round(cpu * B / sim[0], 1))), flush=True)


if __name__ == "__main__":
    main()
