"""Circuits per second of fbx_qv_heavy_outputs and bytes per second of fbx_qv_count_heavy on one GPU, against the numpy restatement
of collect_heavy_outputs (tests/qv_cases.py: tensordot over the two target axes, statistics.median, the heavy list) on one host core
in the same run.

    python scripts/qv_time.py [--widths 2 .. 13] [--batches 100 4096] [--reps 7] [--baseline-circuits 8]

Per (width, batch): the host-pointer form (copies and synchronisation included) and the _dev form (buffers resident, timed with
device events around `reps` separate launches), reference pairing, with and without probs_out.  Circuits are built from 16 distinct
ones (generation is not what is measured).  Every configuration runs once as warm-up and then `reps` times; the rate is that of
the median time, `spread` is (slowest - fastest) / median.  One JSON line per configuration."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "forest-benchmarking_amd"), os.path.join(ROOT, "tests")]

import qv_cases as qc  # noqa: E402
from fbx import _lib, quantum_volume as qv  # noqa: E402

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


def baseline(n, perms, gates, count):
    """seconds per circuit of the numpy restatement on this host, one core"""
    t = time.perf_counter()
    for b in range(count):
        p = qc.simulate(n, qc.pairs_of(perms[b % len(perms)]), gates[b % len(perms)].reshape(-1, 4, 4))
        med, heavy = qc.heavy_of(p)
        np.flatnonzero(heavy).tolist()
    return (time.perf_counter() - t) / count


def main():
    ap = argparse.ArgumentParser()
    # (scripts/ab_shot_records.py times these sizes too: keep its copy in step)
    ap.add_argument("--widths", type=int, nargs="+", default=list(range(2, 14)))
    ap.add_argument("--batches", type=int, nargs="+", default=[100, 4096])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline-circuits", type=int, default=8)
    ap.add_argument("--shots", type=int, nargs="+", default=[1000, 100000])
    args = ap.parse_args()
    _lib.set_device(0)
    lib = _lib.lib()
    for n in args.widths:
        perms, gates = qc.random_circuits(n, 16, seed=n, min_gap=0.0)
        L, N, W = n * (n // 2), 1 << n, max(1, (1 << n) // 64)
        base_s = baseline(n, perms, gates, max(1, args.baseline_circuits if n >= 10 else 8 * args.baseline_circuits))
        for B in args.batches:
            sel = np.arange(B) % 16
            pairs = np.ascontiguousarray(qv.layer_pairs(perms[sel]).reshape(B, L, 2))
            flat = np.ascontiguousarray(gates[sel].reshape(B, L, 4, 4))
            d_pairs, d_gates = _lib.DeviceBuffer.from_array(pairs), _lib.DeviceBuffer.from_array(flat)
            d_p, d_m, d_k = _lib.DeviceBuffer(B * N * 8), _lib.DeviceBuffer(B * 8), _lib.DeviceBuffer(B * W * 8)
            d_hp, d_hc = _lib.DeviceBuffer(B * 8), _lib.DeviceBuffer(B * 4)
            for with_probs in (False, True):
                host = timed(lambda: qv.heavy_outputs_flat(n, pairs, flat, probabilities=with_probs), args.reps)
                dev = timed_dev(lambda: _lib.check(lib.fbx_qv_heavy_outputs_dev(
                    n, B, L, d_pairs.ptr, d_gates.ptr, d_p.ptr if with_probs else None, d_m.ptr, d_k.ptr, d_hp.ptr, d_hc.ptr)), args.reps)
                (hm, hs), (dm, ds) = summary(host), summary(dev)
                print(json.dumps({"what": "heavy_outputs", "n_qubits": n, "gates": L, "batch": B, "probs_out": with_probs, "reps": args.reps,
                                  "host_form": {"circuits_per_s": round(B / hm, 1), "seconds": round(hm, 6), "spread": hs},
                                  "dev_form": {"circuits_per_s": round(B / dm, 1), "seconds": round(dm, 6), "spread": ds},
                                  "baseline_numpy_circuits_per_s": round(1.0 / base_s, 2),
                                  "ratio_host_form": round(base_s * B / hm, 1), "ratio_dev_form": round(base_s * B / dm, 1)}), flush=True)
            for buf in (d_pairs, d_gates, d_p, d_m, d_k, d_hp, d_hc):
                buf.free()
        # heavy counts: B circuits x shots x n bytes, resident
        for shots in args.shots:
            B = 100 if shots >= 100000 else 4096
            rng = np.random.default_rng([n, shots])
            bits = rng.integers(0, 2, size=(B, shots, n), dtype=np.uint8)
            mask = rng.integers(0, 2 ** 63, size=(B, W), dtype=np.uint64)
            d_bits, d_mask, d_c = _lib.DeviceBuffer.from_array(bits), _lib.DeviceBuffer.from_array(mask), _lib.DeviceBuffer(B * 8)
            dev = timed_dev(lambda: _lib.check(lib.fbx_qv_count_heavy_dev(n, B, shots, d_bits.ptr, d_mask.ptr, d_c.ptr)), args.reps)
            dm, ds = summary(dev)
            t = time.perf_counter()
            qc.count_heavy_direct(bits[:4], qv.unpack_heavy_mask(mask[:4], n))
            base = (time.perf_counter() - t) / 4
            print(json.dumps({"what": "count_heavy", "n_qubits": n, "batch": B, "shots": shots, "reps": args.reps,
                              "dev_form": {"circuits_per_s": round(B / dm, 1), "seconds": round(dm, 6), "spread": ds,
                                           "bytes_per_s": round(bits.nbytes / dm, 1), "fraction_of_hbm_peak": round(bits.nbytes / dm / HBM_PEAK, 4)},
                              "baseline_numpy_circuits_per_s": round(1.0 / base, 2), "ratio_dev_form": round(base * B / dm, 1)}), flush=True)
            for buf in (d_bits, d_mask, d_c):
                buf.free()


if __name__ == "__main__":
    main()
