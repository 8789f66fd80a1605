"""Shots per second and output bytes per second of fbx_sample_bitstrings on one GPU, next to numpy's Generator.choice on one host
core (synthetic.qv_shots, what every example and timing script drew its shots with) and to fbx_qv_count_heavy on the bytes produced.

    python scripts/sample_time.py [--widths 5 10 13] [--reps 7] [--short 4096 1000] [--long 1 1000000 8 1000000]

Per width: many short records (B x shots = 4096 x 10^3) and few long ones (1 and 8 x 10^6, which the launcher cuts into shot ranges),
with and without readout flips, the _dev form (buffers resident, timed with device events around `reps` separate launches after one
warm-up) and, for the short shape, the host-pointer form (copies and synchronisation included).  Distributions are Porter-Thomas-like
(squared moduli of complex normals) with depolarizing 0.1.  The host baseline is timed on at most `--baseline-shots` shots in all
and scaled per shot.  The rate is that of the median time, `spread` is (slowest - fastest) / median.  One JSON line per configuration."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "forest-benchmarking_amd")]

from fbx import _lib, sampling, synthetic  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, MI355X


def summary(times):
    t = np.asarray(times)
    med = float(np.median(t))
    return med, round(float((t.max() - t.min()) / med), 3)


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return out


def timed_dev(launch, reps):
    """seconds per launch from the library's device timer around each of `reps` launches (after one warm-up)"""
    lib = _lib.lib()
    launch(); _lib.synchronize()
    out = []
    ms = C.c_double(0.0)
    for _ in range(reps):
        _lib.check(lib.fbx_timer_begin())
        launch()
        _lib.check(lib.fbx_timer_end(C.byref(ms)))
        out.append(ms.value * 1e-3)
    return out


def rates(seconds, spread, shots_total, nbytes):
    return {"seconds": round(seconds, 6), "spread": spread, "shots_per_s": round(shots_total / seconds, 1),
            "bytes_per_s": round(nbytes / seconds, 1), "fraction_of_hbm_peak": round(nbytes / seconds / HBM_PEAK, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", type=int, nargs="+", default=[5, 10, 13])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--short", type=int, nargs=2, default=[4096, 1000], metavar=("B", "SHOTS"))
    ap.add_argument("--long", type=int, nargs="+", default=[1, 1000000, 8, 1000000], metavar="B SHOTS")
    ap.add_argument("--baseline-shots", type=int, default=200000)
    args = ap.parse_args()
    _lib.set_device(0)
    lib = _lib.lib()
    shapes = [("short", args.short[0], args.short[1])] + [("long", args.long[i], args.long[i + 1]) for i in range(0, len(args.long), 2)]
    for n in args.widths:
        N, W = 1 << n, max(1, (1 << n) // 64)
        rng = np.random.default_rng([n, 4242])
        for kind, B, shots in shapes:
            z = rng.standard_normal((min(B, 16), N)) + 1j * rng.standard_normal((min(B, 16), N))
            p = np.ascontiguousarray((np.abs(z) ** 2)[np.arange(B) % len(z)])
            lam = np.full(B, 0.1)
            flips = np.ascontiguousarray(np.broadcast_to(rng.uniform(0.0, 0.05, size=(n, 2)), (B, n, 2)))
            nbytes = B * shots * n
            # host baseline: numpy's choice, one loop iteration per record, on one core
            bshots = max(1, min(shots, args.baseline_shots // min(B, 4)))
            t = time.perf_counter()
            synthetic.qv_shots(p[:min(B, 4)], bshots, depolarizing=0.1)
            base_per_shot = (time.perf_counter() - t) / (min(B, 4) * bshots)
            d_p, d_lam, d_flips = _lib.DeviceBuffer.from_array(p), _lib.DeviceBuffer.from_array(lam), _lib.DeviceBuffer.from_array(flips)
            d_bits, d_status = _lib.DeviceBuffer(nbytes), _lib.DeviceBuffer(4 * B)
            d_mask = _lib.DeviceBuffer.from_array(rng.integers(0, 2 ** 63, size=(B, W), dtype=np.uint64))
            d_counts = _lib.DeviceBuffer(8 * B)
            for with_flips in (False, True):
                dm, ds = summary(timed_dev(lambda: _lib.check(lib.fbx_sample_bitstrings_dev(
                    n, B, shots, d_p.ptr, d_lam.ptr, d_flips.ptr if with_flips else None, 1234, 0, d_bits.ptr, d_status.ptr)), args.reps))
                rec = {"what": "sample_bitstrings", "n_qubits": n, "shape": kind, "batch": B, "shots": shots, "flips": with_flips,
                       "reps": args.reps, "output_bytes": nbytes, "dev_form": rates(dm, ds, B * shots, nbytes),
                       "baseline_numpy_choice_shots_per_s": round(1.0 / base_per_shot, 1),
                       "ratio_dev_form": round(base_per_shot * B * shots / dm, 1)}
                if kind == "short":
                    hm, hs = summary(timed(lambda: sampling.sample_bitstrings_batch(
                        p, shots, depolarizing=lam, readout_flip=flips if with_flips else None, seed=1234), args.reps))
                    rec["host_form"] = rates(hm, hs, B * shots, nbytes)
                    rec["ratio_host_form"] = round(base_per_shot * B * shots / hm, 1)
                print(json.dumps(rec), flush=True)
            if n >= 2:                                   # the consumer on the bytes just produced
                cm, cs = summary(timed_dev(lambda: _lib.check(lib.fbx_qv_count_heavy_dev(n, B, shots, d_bits.ptr, d_mask.ptr, d_counts.ptr)),
                                           args.reps))
                print(json.dumps({"what": "count_heavy_on_sampled_bytes", "n_qubits": n, "shape": kind, "batch": B, "shots": shots,
                                  "reps": args.reps, "dev_form": rates(cm, cs, B * shots, nbytes)}), flush=True)
            assert not d_status.to_array(np.int32, (B,)).any()
            for buf in (d_p, d_lam, d_flips, d_bits, d_status, d_mask, d_counts):
                buf.free()


if __name__ == "__main__":
    main()
