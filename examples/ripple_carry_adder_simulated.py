"""The ripple-carry adder benchmark with simulated shots: the circuit of ``forest.benchmarking.classical_logic`` as a gate list, its
measured answers under gate noise drawn on the device (a shot is one word of classical bits: CCNOT is not Clifford, but the adder
only ever holds Z or X eigenstates), and the statistics the reference computes from them.

1. For 1-4 bit adders in the Z and in the X basis: the success probability and the mean weight of the error, averaged over all
   4^n pairs of summands, against the two-qubit gate error -- simulated (``simulate_adder_statistics_batch``: one call per adder,
   no record leaves the device) next to predicted (``predicted_adder_statistics``: the exact outcome distribution, no sampling).
2. Where along the carry chain the errors fall: how often each answer bit of the 4-bit adder is wrong, from the records.
3. The reference's own path: ``simulate_n_bit_adder_results`` stands where ``get_n_bit_adder_results`` runs the programs, and
   its output goes through ``get_success_probabilities_from_results`` unchanged.

The noise is a depolarizing channel after every gate -- one-qubit gates err a tenth as often as two-qubit gates, the Toffoli
three times as often -- and an asymmetric readout flip per answer bit.

    python examples/ripple_carry_adder_simulated.py [--shots 2000]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "forest-benchmarking_amd"))

from fbx.classical_logic import ripple_carry_adder as rca  # noqa: E402

ERRORS = np.array([0.0, 0.001, 0.003, 0.01, 0.03])               # two-qubit gate error


def mean_weight(hamming):
    return (hamming * np.arange(hamming.shape[-1])).sum(axis=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=2000)
    args = ap.parse_args()
    shots, seed = args.shots, 2024
    class_error = np.stack([0.1 * ERRORS, ERRORS, 3.0 * ERRORS], axis=1)      # [B, 3]: one-, two-, three-qubit gates

    for in_x_basis in (False, True):
        print(f"{'X' if in_x_basis else 'Z'} basis: success probability (mean error weight), simulated | predicted, over all pairs")
        for n in (1, 2, 3, 4):
            flips = np.tile([0.002, 0.005], (n + 1, 1))                       # P(read 1 | 0), P(read 0 | 1)
            n_gates = len(rca.adder(*rca.default_adder_registers(n), in_x_basis=in_x_basis)[0])
            success, hamming = rca.simulate_adder_statistics_batch(n, class_error, in_x_basis=in_x_basis, num_shots=shots,
                                                                   readout_flip=flips, seed=seed)
            want_success, want_hamming = rca.predicted_adder_statistics(n, class_error, in_x_basis=in_x_basis, readout_flip=flips)
            print(f"  {n}-bit adder, {n_gates} gates, {4 ** n} pairs x {shots} shots")
            for b, p in enumerate(ERRORS):
                print(f"    two-qubit error {p:6.3f}   {success[b].mean():.4f} ({mean_weight(hamming[b]).mean():.4f})"
                      f" | {want_success[b].mean():.4f} ({mean_weight(want_hamming[b]).mean():.4f})")

    n = 4
    results = rca.simulate_n_bit_adder_results(n, num_shots=shots, gate_error=tuple(class_error[3]), seed=seed)
    wrong = (results != rca.adder_expected_bits(n)[:, None, :]).mean(axis=(0, 1))
    print(f"4-bit adder, Z basis, two-qubit error {ERRORS[3]}, no readout error: how often each answer bit is wrong, over all pairs")
    for j in range(n, -1, -1):                                                # column 0 is the most significant bit
        print(f"    bit {n - j}{' (final carry)' if j == 0 else '':14s}   {wrong[j]:.4f}")

    results = rca.simulate_n_bit_adder_results(2, num_shots=100, gate_error=tuple(class_error[3]), seed=seed)
    probabilities = rca.get_success_probabilities_from_results(results)
    print(f"2-bit adder, 100 shots per pair as in the reference's notebook: results {results.shape}, "
          f"success probabilities from {min(probabilities):.2f} to {max(probabilities):.2f}")


if __name__ == "__main__":
    main()
