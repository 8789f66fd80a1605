"""Trajectories per second of fbx_native_trajectories_dev on one GPU for the compiled ripple-carry adder, and its time per gate
against fbx_qv_noisy_trajectories_dev -- the sibling whose gate is a 4 x 4 product -- at the same width and on as many
trajectories in the same run.

    python scripts/native_time.py [--bits 2 3 4] [--items 4] [--trajectories 16] [--reps 9] [--window 0.05]

Per adder width n_bits (2 n_bits + 2 qubits): the circuit of ripple_carry_adder.compiled_adder_circuit, B = --items noise settings
(p_rx, p_rz, p_cz) = (0.001, 0, 0.01) x all 4^n_bits input words x T = --trajectories trajectories, device pointers, the mean
marginal on the answer qubits as the only output.  The partner: B 4^n_bits quantum-volume circuits of the same width (16 distinct
ones, repeated; n (n // 2) gates each, every gate with error p_cz) x T trajectories, probs_mean_out only.  The two are timed with
the library's device timer, each after a warm-up, ALTERNATING within every repetition so that drift of the shared machine hits
them alike; a timed window holds as many launches as bring it to about --window seconds.  The time is the median over the
repetitions, `spread` is (slowest - fastest) / median.  `lane_cycles_per_trajectory_gate` is the time x CUs x 4 SIMDs x 16 lanes
x the clock, over trajectories x gates; `per_gate_over_qv` is the ratio of the two times per (trajectory x gate).  One JSON line
per width."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "forest-benchmarking_amd"), os.path.join(ROOT, "tests")]

import qv_cases as qc  # noqa: E402
from fbx import _lib, quantum_volume as qv  # noqa: E402
from fbx.classical_logic import ripple_carry_adder as rca  # noqa: E402

CLOCK_HZ = 2.4e9


def summary(times):
    t = np.asarray(times)
    med = float(np.median(t))
    return med, round(float((t.max() - t.min()) / med), 3)


def window(launch, count):
    """seconds per launch from the library's device timer around `count` launches"""
    lib = _lib.lib()
    ms = C.c_double(0.0)
    _lib.check(lib.fbx_timer_begin())
    for _ in range(count):
        launch()
    _lib.check(lib.fbx_timer_end(C.byref(ms)))
    return ms.value * 1e-3 / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, nargs="+", default=[2, 3, 4])
    ap.add_argument("--items", type=int, default=4)
    ap.add_argument("--trajectories", type=int, default=16)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--window", type=float, default=0.05)
    ap.add_argument("--errors", type=float, nargs=3, default=[0.001, 0.0, 0.01])
    args = ap.parse_args()
    _lib.set_device(0)
    lib = _lib.lib()
    _, cus = _lib.device_name()
    B, T = args.items, args.trajectories
    for n_bits in args.bits:
        words, angles, n, out, cls = rca.compiled_adder_circuit(n_bits)
        G, P, m = int(words.size), 4 ** n_bits, n_bits + 1
        total = B * P * T
        ce = np.tile(np.asarray(args.errors, dtype=np.float64), (B, 1))
        perms, gates = qc.random_circuits(n, 16, seed=n, min_gap=0.0)
        L = n * (n // 2)
        sel = np.arange(B * P) % 16
        with _lib.DeviceScope() as dev:
            d_words, d_angles, d_cls = dev.upload(words), dev.upload(angles), dev.upload(cls)
            d_inputs, d_out, d_ce = dev.upload(np.arange(P, dtype=np.uint64)), dev.upload(out), dev.upload(ce)
            d_probs, d_status = dev.alloc(8 * B * P << m), dev.alloc(4 * B)
            d_pairs = dev.upload(np.ascontiguousarray(qv.layer_pairs(perms).reshape(16, L, 2)[sel]))
            d_gates = dev.upload(np.ascontiguousarray(gates.reshape(16, L, 4, 4)[sel]))
            d_ge = dev.upload(np.full((B * P, L), args.errors[2]))
            d_mean, d_qstatus = dev.alloc(8 * B * P << n), dev.alloc(4 * B * P)
            launches = {
                "native": lambda: _lib.check(lib.fbx_native_trajectories_dev(n, G, d_words.ptr, d_angles.ptr, d_cls.ptr, 3, P, d_inputs.ptr, m,
                                                                             d_out.ptr, B, T, d_ce.ptr, 1, 0, 0, d_probs.ptr, None, d_status.ptr)),
                "qv_noisy": lambda: _lib.check(lib.fbx_qv_noisy_trajectories_dev(n, B * P, L, T, d_pairs.ptr, d_gates.ptr, d_ge.ptr, None, 1, 0,
                                                                                 d_mean.ptr, None, None, d_qstatus.ptr)),
            }
            counts, times = {}, {k: [] for k in launches}
            for k, launch in launches.items():                            # warm-up, and the number of launches per window
                launch(); _lib.synchronize()
                counts[k] = int(min(200, max(1, np.ceil(args.window / window(launch, 1)))))
            for _ in range(args.reps):
                for k, launch in launches.items():
                    times[k].append(window(launch, counts[k]))
            probs = d_probs.to_array(np.float64, (B, P, 1 << m))
            assert not d_status.to_array(np.int32, (B,)).any() and not d_qstatus.to_array(np.int32, (B * P,)).any()
            assert np.abs(probs.sum(axis=2) - 1.0).max() < 1e-12
        res = {k: summary(v) for k, v in times.items()}
        line = {"what": "native_trajectories", "n_bits": n_bits, "n_qubits": n, "gates": G, "cz_gates": int((cls == 2).sum()),
                "items": B, "inputs": P, "trajectories": T, "class_error": list(args.errors), "qv_gates": L, "reps": args.reps,
                "launches_per_window": counts, "compute_units": cus}
        for k, (med, spread) in res.items():
            per_gate = med / (total * (G if k == "native" else L))
            line[k] = {"trajectories_per_s": round(total / med, 1), "seconds": round(med, 6), "spread": spread,
                       "lane_cycles_per_trajectory_gate": round(per_gate * cus * 4 * 16 * CLOCK_HZ, 1)}
        line["per_gate_over_qv"] = round((res["native"][0] / G) / (res["qv_noisy"][0] / L), 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
