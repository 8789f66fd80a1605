"""Time per (shot x gate) of the reversible-circuit sampler (fbx_reversible_sample_shots_dev, csrc/fbx_reversible.hip) on one GPU,
next to its sibling, the Pauli-frame sampler (fbx_clifford_sample_shots_dev, csrc/fbx_frames.hip), in the same run.

    python scripts/adder_sim_time.py [--reps 9] [--bits 4] [--batch 256] [--shots 1000]

The workload is the adder benchmark's: the `bits`-bit ripple-carry adder in the Z basis (8 bits + 1 gates on 2 bits + 2 qubits), all
4^bits pairs of summands, `shots` shots each, `batch` noise settings -- without noise (class_error NULL: no Philox block) and with
it (three classes, error probabilities up to 0.03: a block per pair of gates).  Two forms are timed: the fused histogram alone
(weight_counts; what simulate_adder_statistics_batch launches: nothing per shot is written) and packed records (words_out).  The
sibling samples a CNOT-only circuit of the same gate count on the same number of qubits, batch x 4^bits items of `shots` shots,
packed records out, with and without noise of one class.  Buffers are resident; the library's device timer surrounds each launch;
in every repetition the calls run one after another, so each repetition gives its own ratio to the sibling.  Reported: the median
seconds and the (slowest - fastest) / median spread of each call, lane-cycles per (shot x gate) on 1024 SIMDs x 16 lanes x 2.4 GHz
(the scale of scripts/clifford_sample_time.py), and the median, smallest and largest per-repetition ratio.  One JSON line per
result.  The noiseless records are checked against the arithmetic and the noisy ones, on one unit, against the host restatement."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "forest-benchmarking_amd")]

from fbx import _lib, clifford_circuit as cc  # noqa: E402
from fbx.classical_logic import reversible as rev, ripple_carry_adder as rca  # noqa: E402

LANE_RATE = 1024 * 16 * 2.4e9                  # lane-cycles per second of the chip


def summary(times):
    t = np.asarray(times)
    med = float(np.median(t))
    return med, round(float((t.max() - t.min()) / med), 3)


def timed_once(launch):
    ms = C.c_double(0.0)
    _lib.check(_lib.lib().fbx_timer_begin())
    launch()
    _lib.check(_lib.lib().fbx_timer_end(C.byref(ms)))
    return ms.value * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--shots", type=int, default=1000)
    args = ap.parse_args()
    _lib.set_device(0)
    lib = _lib.lib()
    n_bits, B, shots, seed = args.bits, args.batch, args.shots, 2024
    gates, out_qubits = rca.adder(*rca.default_adder_registers(n_bits))
    n, m, P = 2 * n_bits + 2, n_bits + 1, 4 ** n_bits
    words = rev.encode_reversible(gates, n)
    G = int(words.size)
    classes = (rev.gate_arity(words) - 1).astype(np.uint8)
    rng = np.random.default_rng(7)
    errors = rng.uniform(0.001, 0.03, size=(B, 3))
    expected = rev.pack_records(rca.adder_expected_bits(n_bits))
    sibling_gates = [("CNOT", (g % (n - 1), g % (n - 1) + 1)) for g in range(G)]
    sibling_words = cc.encode_gates(sibling_gates, n)
    items, total = B * P, B * P * shots
    with _lib.DeviceScope() as dev:
        d_words, d_classes, d_inputs = dev.upload(words), dev.upload(classes), dev.upload(np.arange(P, dtype=np.uint64))
        d_out, d_expected, d_errors = dev.upload(np.array(out_qubits, dtype=np.uint8)), dev.upload(expected), dev.upload(errors)
        d_sib, d_sib_errors, d_ref = dev.upload(sibling_words), dev.upload(np.repeat(errors[:, 1], P)), dev.alloc(8)
        d_records, d_counts, d_status = dev.alloc(8 * total), dev.alloc(8 * items * (m + 1)), dev.alloc(4 * items)
        _lib.check(lib.fbx_clifford_reference_sample_dev(n, G, d_sib.ptr, d_ref.ptr))

        def reversible(noisy, records):
            return lambda: _lib.check(lib.fbx_reversible_sample_shots_dev(
                n, G, d_words.ptr, d_classes.ptr, 3, P, d_inputs.ptr, m, d_out.ptr, d_expected.ptr, B, shots,
                d_errors.ptr if noisy else None, None, seed, 0, 0, None, d_records.ptr if records else None,
                None if records else d_counts.ptr, d_status.ptr))

        def sibling(noisy):
            return lambda: _lib.check(lib.fbx_clifford_sample_shots_dev(
                n, G, d_sib.ptr, None, 1, d_ref.ptr, items, shots, d_sib_errors.ptr if noisy else None, None, seed, 0, None,
                d_records.ptr, d_status.ptr))

        # what is timed is also right: the noiseless records, and one unit of the noisy ones
        reversible(False, True)(); _lib.synchronize()
        assert np.array_equal(d_records.to_array(np.uint64, (P, shots)), np.broadcast_to(expected[:, None], (P, shots)))
        reversible(True, False)(); _lib.synchronize()
        want = rev.restate_reversible_shots(words, n, [P - 1], out_qubits, shots, errors[:1], classes, seed=seed, first_input=P - 1)
        assert np.array_equal(d_counts.to_array(np.int64, (P, m + 1))[P - 1], rev.weight_counts(want, expected[P - 1:], m)[0, 0])

        for noisy in (False, True):
            calls = {"reversible_counts": reversible(noisy, False), "reversible_words": reversible(noisy, True),
                     "clifford_words": sibling(noisy)}
            for launch in calls.values():
                launch()
            _lib.synchronize()
            times = {name: [] for name in calls}
            for _ in range(args.reps):
                for name, launch in calls.items():
                    times[name].append(timed_once(launch))
            for name in calls:
                med, spread = summary(times[name])
                line = {"what": name, "noise": noisy, "n_qubits": n, "gates": G, "batch": B, "pairs": P, "shots": shots, "reps": args.reps,
                        "seconds": round(med, 7), "spread": spread, "shot_gates_per_s": round(total * G / med, 1),
                        "lane_cycles_per_shot_gate": round(LANE_RATE * med / (total * G), 2)}
                if name != "clifford_words":
                    ratios = np.asarray(times[name]) / np.asarray(times["clifford_words"])
                    line["ratio_to_clifford"] = {"median": round(float(np.median(ratios)), 3), "min": round(float(ratios.min()), 3),
                                                 "max": round(float(ratios.max()), 3)}
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
