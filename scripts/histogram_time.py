"""Bytes per second of fbx_bit_histogram_dev on one GPU, with fbx_shots_to_moments_dev on the SAME buffers as the yardstick (both
read every byte of the records once; the histogram adds one LDS table read and one LDS add per shot).

    python scripts/histogram_time.py [--reps 9] [--out profiles/r08/histogram_time.jsonl]

Configurations: the joint kind at k = 1, 2, 3 and 10 and the weight kind at k = 5 and 17 (n_cols = k, all columns selected; the weight
kind with a random expected pattern), each on 1000-shot records (a wavefront per record; 4096 records) and on 10^6-shot records (a
workgroup per record; 64 records).  Buffers stay resident; every configuration runs once as warm-up and then `reps` times between
device events (fbx_timer_*); the rate is that of the median time, `spread` is (slowest - fastest) / median.  One JSON line per
configuration; nothing here is a pass criterion."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "forest-benchmarking_amd")]

from fbx import _lib  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, MI355X


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.set_device(0)
    lib = _lib.lib()
    sink = open(args.out, "w") if args.out else None
    # (scripts/ab_shot_records.py times these sizes too: keep its copy in step)
    for kind, k in ((0, 1), (0, 2), (0, 3), (0, 10), (1, 5), (1, 17)):
        for shots, B in ((1000, 4096), (10 ** 6, 64)):
            rng = np.random.default_rng([kind, k, shots])
            bits = rng.integers(0, 2, size=(B, shots, k), dtype=np.uint8)
            bins = (1 << k) if kind == 0 else k + 1
            expected = rng.integers(0, 2, size=(B, k), dtype=np.uint8) if kind == 1 else None
            d_bits = _lib.DeviceBuffer.from_array(bits)
            d_exp = _lib.DeviceBuffer.from_array(expected) if expected is not None else None
            d_counts = _lib.DeviceBuffer(B * bins * 8)
            d_mask = _lib.DeviceBuffer.from_array(np.ones((B, k), dtype=np.uint8))
            d_mean, d_var = _lib.DeviceBuffer(B * 8), _lib.DeviceBuffer(B * 8)
            hist = timed_dev(lambda: _lib.check(lib.fbx_bit_histogram_dev(k, B, shots, d_bits.ptr, k, None, 1, d_exp.ptr if d_exp else None,
                                                                          kind, d_counts.ptr)), args.reps)
            yard = timed_dev(lambda: _lib.check(lib.fbx_shots_to_moments_dev(k, B, shots, d_bits.ptr, d_mask.ptr, None, 0, d_mean.ptr,
                                                                             d_var.ptr)), args.reps)
            counts = d_counts.to_array(np.int64, (B, bins))
            assert (counts.sum(axis=1) == shots).all()
            line = json.dumps({"what": "bit_histogram", "kind": "joint" if kind == 0 else "weight", "k": k, "n_cols": k, "batch": B,
                               "shots": shots, "bytes": int(bits.nbytes), "reps": args.reps,
                               "histogram": {"seconds": round(hist[0], 7), "spread": hist[1], "bytes_per_s": round(bits.nbytes / hist[0], 1),
                                             "fraction_of_hbm_peak": round(bits.nbytes / hist[0] / HBM_PEAK, 4)},
                               "shots_to_moments": {"seconds": round(yard[0], 7), "spread": yard[1],
                                                    "bytes_per_s": round(bits.nbytes / yard[0], 1),
                                                    "fraction_of_hbm_peak": round(bits.nbytes / yard[0] / HBM_PEAK, 4)},
                               "histogram_over_yardstick_time": round(hist[0] / yard[0], 2)})
            print(line, flush=True)
            if sink:
                sink.write(line + "\n"); sink.flush()
            for buf in (d_bits, d_exp, d_counts, d_mask, d_mean, d_var):
                if buf is not None:
                    buf.free()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
