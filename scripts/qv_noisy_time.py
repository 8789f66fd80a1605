"""Trajectories per second of fbx_qv_noisy_trajectories_dev on one GPU, against fbx_qv_heavy_outputs_dev on as many IDEAL circuits of
the same width (asked for heavy_prob only) in the same run, and against the numpy restatement of a trajectory
(synthetic.restate_qv_gate_errors + quantum_volume.fold_gate_errors + tests/qv_cases.simulate) on one host core.

    python scripts/qv_noisy_time.py [--widths 6 10 13] [--log2-trajectories 14] [--batch 128] [--gate-error 0.01] [--reps 7]

Per width: B circuits x T trajectories with B T = 2^log2-trajectories, device pointers, reference pairing; the circuits are built
from 16 distinct ones (generation is not what is measured).  Three configurations are timed with the library's device timer, each
after a warm-up, ALTERNATING within every repetition so that drift of the shared machine hits them alike: the ideal partner, the
trajectories with hprob_traj_out only (every trajectory a unit of work of its own), and the trajectories with probs_mean_out and
hprob_traj_out (units of four trajectories, partial sums, the mean kernel).  A timed window holds as many launches as bring it to
about --window seconds.  The time is the median over the repetitions, `spread` is (slowest - fastest) / median.  A trajectory runs
the gates of an ideal circuit, skips the radix select and adds one Philox block per two gates and a mask read:
`per_trajectory_over_per_circuit` is expected to stay below 1.15.  One JSON line per width."""
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
from fbx import _lib, quantum_volume as qv, synthetic  # noqa: E402


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


def baseline(n, pairs, flat, p, count):
    """seconds per trajectory of the numpy restatement on this host, one core"""
    L = pairs.shape[0]
    t = time.perf_counter()
    paulis = synthetic.restate_qv_gate_errors(1, count, L, p, 1)[0]
    folded = qv.fold_gate_errors(flat[None], paulis[None])[0]
    for k in range(count):
        qc.simulate(n, pairs, folded[k])
    return (time.perf_counter() - t) / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", type=int, nargs="+", default=[6, 10, 13])
    ap.add_argument("--log2-trajectories", type=int, default=14)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--gate-error", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.05)
    ap.add_argument("--baseline-trajectories", type=int, default=16)
    args = ap.parse_args()
    _lib.set_device(0)
    lib = _lib.lib()
    DB = _lib.DeviceBuffer
    total = 1 << args.log2_trajectories
    B = args.batch
    if B < 1 or total % B:
        raise SystemExit("--batch must divide 2^log2-trajectories")
    T = total // B
    for n in args.widths:
        perms, gates = qc.random_circuits(n, 16, seed=n, min_gap=0.0)
        L, N, W = n * (n // 2), 1 << n, max(1, (1 << n) // 64)
        all_pairs = qv.layer_pairs(perms).reshape(16, L, 2)
        all_flat = gates.reshape(16, L, 4, 4)
        base_s = baseline(n, all_pairs[0], all_flat[0], args.gate_error, max(1, args.baseline_trajectories if n >= 10
                                                                              else 8 * args.baseline_trajectories))
        bufs = []

        def dev(x):
            bufs.append(x)
            return x
        # the ideal partner: B T circuits, heavy_prob only
        sel = np.arange(total) % 16
        d_ipairs, d_igates = dev(DB.from_array(np.ascontiguousarray(all_pairs[sel]))), dev(DB.from_array(np.ascontiguousarray(all_flat[sel])))
        d_ihp = dev(DB(8 * total))
        # the trajectories: B circuits, T each; the heavy sets come from one ideal call outside the timed windows
        sel = np.arange(B) % 16
        d_pairs, d_gates = dev(DB.from_array(np.ascontiguousarray(all_pairs[sel]))), dev(DB.from_array(np.ascontiguousarray(all_flat[sel])))
        d_ge = dev(DB.from_array(np.full((B, L), args.gate_error)))
        d_mask, d_mean, d_hp, d_st = dev(DB(8 * B * W)), dev(DB(8 * B * N)), dev(DB(8 * total)), dev(DB(4 * B))
        _lib.check(lib.fbx_qv_heavy_outputs_dev(n, B, L, d_pairs.ptr, d_gates.ptr, None, None, d_mask.ptr, None, None))
        launches = {
            "ideal": lambda: _lib.check(lib.fbx_qv_heavy_outputs_dev(n, total, L, d_ipairs.ptr, d_igates.ptr, None, None, None, d_ihp.ptr, None)),
            "hprob": lambda: _lib.check(lib.fbx_qv_noisy_trajectories_dev(n, B, L, T, d_pairs.ptr, d_gates.ptr, d_ge.ptr, d_mask.ptr, 1, 0,
                                                                          None, d_hp.ptr, None, d_st.ptr)),
            "mean": lambda: _lib.check(lib.fbx_qv_noisy_trajectories_dev(n, B, L, T, d_pairs.ptr, d_gates.ptr, d_ge.ptr, d_mask.ptr, 1, 0,
                                                                         d_mean.ptr, d_hp.ptr, None, d_st.ptr)),
        }
        counts, times = {}, {k: [] for k in launches}
        for k, launch in launches.items():                                # warm-up, and the number of launches per window
            launch(); _lib.synchronize()
            counts[k] = int(min(200, max(1, np.ceil(args.window / window(launch, 1)))))
        for _ in range(args.reps):
            for k, launch in launches.items():
                times[k].append(window(launch, counts[k]))
        hp = d_hp.to_array(np.float64, (B, T))
        assert not d_st.to_array(np.int32, (B,)).any() and np.all((hp > 0) & (hp < 1 + 1e-12))
        res = {k: summary(v) for k, v in times.items()}
        line = {"what": "qv_noisy_trajectories", "n_qubits": n, "gates": L, "batch": B, "trajectories": T, "gate_error": args.gate_error,
                "reps": args.reps, "launches_per_window": counts}
        for k, (med, spread) in res.items():
            line[k] = {"per_s": round(total / med, 1), "seconds": round(med, 6), "spread": spread}
        line["per_trajectory_over_per_circuit"] = {"hprob": round(res["hprob"][0] / res["ideal"][0], 3),
                                                   "mean": round(res["mean"][0] / res["ideal"][0], 3)}
        line["baseline_numpy_trajectories_per_s"] = round(1.0 / base_s, 2)
        line["ratio_to_numpy"] = {"hprob": round(base_s * total / res["hprob"][0], 1), "mean": round(base_s * total / res["mean"][0], 1)}
        print(json.dumps(line), flush=True)
        for b in bufs:
            b.free()


if __name__ == "__main__":
    main()
