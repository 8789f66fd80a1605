"""Time of fbx_rb_acquire on one GPU next to the composition it fuses, fbx_rb_sequences -> fbx_rb_simulate, in the same run, all
in device-pointer form on resident buffers.

    python scripts/rb_acquire_time.py [--reps 7] [--configs 2:10000:32:0 2:10000:32:500 2:100000:32:0 2:100000:32:500]

A config is n_qubits:experiments:sequences_per_depth:shots; the depths are 2, 4, 8, 16, 32, 64.  The fused call draws, simulates
and measures E experiments, each under its own noise matrix and readout error, and writes the expectations and standard errors of
every sequence ([E, S K, 2^n - 1] each).  The composition is the two calls of the existing entry points on the same number of
sequences of the same lengths: element words and noise ids to memory, then the final vectors [E S K, 4^n].  Those entry points take
one seed and one shared set of noise matrices per call, so the composition runs all E S K sequences as ONE batch under one
matrix -- per-experiment noise would need E calls of each -- and draws no shots: it is the least the unfused route can cost, and
it stops short of the measurement.  Each side is timed with device events around each of `reps` separate launches after one
warm-up; the two sides alternate, so that a drift of the clock meets both; the time is the median, `spread` is (slowest -
fastest) / median, and the ratio fused / composition is formed per repetition.  One JSON line per configuration."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "forest-benchmarking_amd")]

from fbx import _lib  # noqa: E402

DEPTHS = (2, 4, 8, 16, 32, 64)


def summary(times):
    t = np.asarray(times)
    med = float(np.median(t))
    return round(med, 6), round(float((t.max() - t.min()) / med), 3)


def timed_alternating(launches, reps):
    """seconds per launch of every entry of `launches`, from the library's device timer around each of `reps` launches (after one
    warm-up each); the entries take turns"""
    lib = _lib.lib()
    for launch in launches:
        launch()
    _lib.synchronize()
    out = [[] for _ in launches]
    ms = C.c_double(0.0)
    for _ in range(reps):
        for times, launch in zip(out, launches):
            _lib.check(lib.fbx_timer_begin())
            launch()
            _lib.check(lib.fbx_timer_end(C.byref(ms)))
            times.append(ms.value * 1e-3)
    return out


def noise(n, E):
    """[E, 1, D, D]: 16 distinct channels, repeated -- depolarizing of 0.2 .. 1.7 % with a little amplitude damping on qubit 0"""
    D = 4 ** n
    out = np.empty((16, D, D))
    for i in range(16):
        m = np.eye(D) * (1.0 - 0.002 - 0.001 * i)
        m[0, 0] = 1.0
        m[3 << (2 * (n - 1)), 0] = 0.001 * (i + 1)
        out[i] = m
    return np.ascontiguousarray(out[np.arange(E) % 16][:, None])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--configs", nargs="+", default=["2:10000:32:0", "2:10000:32:500", "2:100000:32:0", "2:100000:32:500"])
    args = ap.parse_args()
    _lib.set_device(0)
    lib, DB = _lib.lib(), _lib.DeviceBuffer
    depths = np.array(DEPTHS, dtype=np.int32)
    S = depths.size
    for cfg in args.configs:
        n, E, K, shots = (int(x) for x in cfg.split(":"))
        D, Cn = 4 ** n, 2 ** n - 1
        seqs = E * S * K
        ptms = noise(n, E)
        flips = np.random.default_rng(7).uniform(0.0, 0.05, size=(n, 2))
        d_l = DB.from_array(ptms)
        d_f = DB.from_array(np.ascontiguousarray(np.broadcast_to(flips, (E, n, 2))))
        d_e, d_s, d_st = DB(8 * seqs * Cn), DB(8 * seqs * Cn), DB(4 * E)
        lengths = np.tile(np.repeat(depths.astype(np.int64), K), E)           # self-inverting, plain: `depth` elements
        offsets = np.zeros(seqs + 1, dtype=np.int64)
        np.cumsum(lengths, out=offsets[1:])
        total = int(offsets[-1])
        d_off, d_one = DB.from_array(offsets), DB.from_array(ptms[0])
        d_el, d_id, d_vec = DB(4 * total), DB(total), DB(8 * seqs * D)

        def fused():
            _lib.check(lib.fbx_rb_acquire_dev(n, E, S, _lib.iptr(depths), K, _lib.RB_STANDARD, _lib.CLIFFORD_NONE, 1, d_l.ptr, None,
                                              d_f.ptr, shots, 1234, 0, None, None, None, d_e.ptr, d_s.ptr, d_st.ptr))

        def composition():
            _lib.check(lib.fbx_rb_sequences_dev(n, seqs, d_off.ptr, 1234, _lib.CLIFFORD_NONE, 1, d_el.ptr, d_id.ptr))
            _lib.check(lib.fbx_rb_simulate_dev(n, seqs, d_off.ptr, d_el.ptr, d_id.ptr, 1, d_one.ptr, None, d_vec.ptr))
        tf, tc = timed_alternating((fused, composition), args.reps)
        assert not d_st.to_array(np.int32, (E,)).any()
        (fm, fs), (cm, cs) = summary(tf), summary(tc)
        ratio = np.asarray(tf) / np.asarray(tc)
        print(json.dumps({
            "what": "rb_acquire", "n_qubits": n, "experiments": E, "depths": list(DEPTHS), "sequences_per_depth": K, "shots": shots,
            "sequences": seqs, "elements": total, "reps": args.reps,
            "rb_acquire_dev": {"seconds": fm, "spread": fs, "experiments_per_s": round(E / fm, 1), "sequences_per_s": round(seqs / fm, 1)},
            "sequences_then_simulate_dev": {"seconds": cm, "spread": cs, "element_bytes": 5 * total},
            "fused_over_composition": round(float(np.median(ratio)), 4),
            "ratio_per_repetition": {"min": round(float(ratio.min()), 4), "max": round(float(ratio.max()), 4),
                                     "spread": round(float((ratio.max() - ratio.min()) / np.median(ratio)), 3)}}), flush=True)
        for buf in (d_l, d_f, d_e, d_s, d_st, d_off, d_one, d_el, d_id, d_vec):
            buf.free()


if __name__ == "__main__":
    main()
