"""Estimates and bytes per second of fbx_rpe_from_shots on one GPU, next to the composed path on the same bits
(fbx_shots_to_moments_dev for the X and the Y records, then fbx_rpe_phase_dev), buffers resident, timed with device events.

    python scripts/rpe_time.py [--batch 100000] [--depths 10] [--shots 500] [--qubits 2] [--reps 7] [--zcol]

The yardstick is the shot -> moment reduction, recorded at 3.9-5.8 TB/s on an MI355X: both paths read the same
2 x batch x depths x shots x qubits bytes once.  Every configuration runs once as warm-up and then `reps` times; the rate is that
of the median time, `spread` is (slowest - fastest) / median.  One JSON line per path."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "forest-benchmarking_amd")]

from fbx import _lib  # noqa: E402

HBM_PEAK = 8.0e12                       # bytes / s, MI355X
SHOTS_TO_MOMENTS_RECORDED = "3.9-5.8 TB/s"


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
    # (scripts/ab_shot_records.py times these sizes too: keep its copy in step)
    ap.add_argument("--batch", type=int, default=100000)
    ap.add_argument("--depths", type=int, default=10)
    ap.add_argument("--shots", type=int, default=500)
    ap.add_argument("--qubits", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--zcol", action="store_true", help="post-select on column 1 (needs --qubits >= 2)")
    args = ap.parse_args()
    B, K, shots, n = args.batch, args.depths, args.shots, args.qubits
    _lib.set_device(0)
    lib, DB = _lib.lib(), _lib.DeviceBuffer
    rng = np.random.default_rng(0)
    zcol = 1 if args.zcol else -1
    # records from 64 distinct estimates with a visibility that keeps every item running (generation is not what is measured)
    depth = 2.0 ** np.arange(K)
    phases = rng.uniform(0, 2 * np.pi, 64)
    bits = []
    for fn in (np.cos, np.sin):
        b = rng.integers(0, 2, size=(64, K, shots, n), dtype=np.uint8)
        b[..., 0] = rng.random((64, K, shots)) < (1 - 0.9 * fn(depth[None, :, None] * phases[:, None, None])) / 2
        bits.append(np.ascontiguousarray(b[np.arange(B) % 64]))
    nbytes = bits[0].nbytes + bits[1].nbytes
    d_x, d_y = DB.from_array(bits[0]), DB.from_array(bits[1])
    d_phase, d_depth = DB(B * 8), DB(B * 4)
    fused = timed_dev(lambda: _lib.check(lib.fbx_rpe_from_shots_dev(n, B, K, shots, d_x.ptr, d_y.ptr, 0, zcol, 0, d_phase.ptr,
                                                                    d_depth.ptr, None, None)), args.reps)
    _lib.synchronize()
    reached = d_depth.to_array(np.int32, (B,))
    masks = np.zeros((2, B * K, n), dtype=np.uint8)
    masks[:, :, 0] = 1
    if args.zcol:
        masks[1, :, 1] = 1
    d_masks = [DB.from_array(masks[0]), DB.from_array(masks[1])]
    mom = [(DB(B * K * 8), DB(B * K * 8)) for _ in range(4 if args.zcol else 2)]

    def composed():
        for which in range(2 if args.zcol else 1):
            for i, d_bits in enumerate((d_x, d_y)):
                m, v = mom[2 * which + i]
                _lib.check(lib.fbx_shots_to_moments_dev(n, B * K, shots, d_bits.ptr, d_masks[which].ptr, None, 0, m.ptr, v.ptr))
        part = [mom[2][0].ptr, mom[3][0].ptr, mom[2][1].ptr, mom[3][1].ptr] if args.zcol else [None] * 4
        _lib.check(lib.fbx_rpe_phase_dev(B, K, mom[0][0].ptr, mom[1][0].ptr, mom[0][1].ptr, mom[1][1].ptr, 1, part[0], part[1],
                                         part[2], part[3], 0, d_phase.ptr, d_depth.ptr, None))
    comp = timed_dev(composed, args.reps)
    for name, (sec, spread), passes in (("fbx_rpe_from_shots_dev", fused, 1), ("shots_to_moments_dev -> rpe_phase_dev", comp,
                                                                               2 if args.zcol else 1)):
        print(json.dumps({"what": name, "batch": B, "depths": K, "shots": shots, "n_qubits": n, "zcol": zcol, "reps": args.reps,
                          "seconds": round(sec, 6), "spread": spread, "estimates_per_s": round(B / sec, 1),
                          "shot_bytes": nbytes, "shot_bytes_per_s": round(nbytes / sec, 1),
                          "fraction_of_hbm_peak": round(nbytes / sec / HBM_PEAK, 4), "passes_over_the_bits": passes,
                          "mean_depth_reached": round(float(reached.mean()), 2),
                          "yardstick_shots_to_moments_recorded": SHOTS_TO_MOMENTS_RECORDED}), flush=True)


if __name__ == "__main__":
    main()
