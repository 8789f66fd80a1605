"""Simulated process tomography with grouped settings: settings that are diagonal in one tensor-product basis are read off the
same shots, as ``do_tomography(..., group_tpb_settings=True)`` of the reference acquires them (a two-qubit Pauli experiment is
324 runs, not 540).  One two-qubit channel is simulated ungrouped (every setting its own shots) and grouped, PGDB reconstructs
from both, and the fidelity of each estimate to the truth is printed (the reference's process fidelity is a fidelity when one
argument is unitary: for the default mixing channel it is below 1 even against itself, and what to compare is the two numbers).

What only the grouped data have is the correlation INSIDE a group.  From the outcome histogram of one ZZ-basis group the script
takes the IZ and ZI result of every shot and prints their sample correlation next to the value the group's outcome distribution
predicts; with independent shots per setting the two results would be uncorrelated whatever the state is.

    python examples/process_tomography_grouped.py [--shots 2000] [--kraus 2] [--seed 7]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "forest-benchmarking_amd"))

from fbx import distance_measures, synthetic, tomography  # noqa: E402
from fbx.design import group_design, process_design  # noqa: E402
from fbx.operator_tools.superoperator_transformations import convert_batch  # noqa: E402


def correlation(weights):
    """correlation of the IZ and ZI results (+-1) under the weights of the outcomes 00, 01, 10, 11: bit 0 of an outcome is
    qubit 1 (IZ), bit 1 is qubit 0 (ZI), bit value 1 = eigenvalue -1"""
    w = np.asarray(weights, dtype=np.float64) / np.sum(weights)
    iz, zi = np.array([1, -1, 1, -1.0]), np.array([1, 1, -1, -1.0])
    a, b, ab = w @ iz, w @ zi, w @ (iz * zi)
    return (ab - a * b) / np.sqrt((1 - a * a) * (1 - b * b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=2000)
    ap.add_argument("--kraus", type=int, default=2, help="Kraus operators of the random channel (1: a unitary)")
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    design = process_design(2, "pauli")
    grouping = group_design(design)                                       # the reference's greedy grouping
    channel = synthetic.kraus_batch(2, args.kraus, 1, seed=args.seed)
    truth = convert_batch("kraus", "pauli_liouville", channel).real.astype(np.complex128)
    print(f"one random two-qubit channel of {args.kraus} Kraus operator(s), {args.shots} shots per run")
    print(f"ungrouped: {design.m} runs; grouped: {grouping.n_groups} runs, the largest of {max(map(len, grouping.groups))} settings")

    e, c = tomography.simulate_process_tomography_batch(design, channel, args.shots, rep="kraus", seed=args.seed)
    eg, cg, prob, hist = tomography.simulate_grouped_process_tomography_batch(
        design, channel, args.shots, groups=grouping, rep="kraus", seed=args.seed, return_probabilities=True, return_histograms=True)
    for name, (x, n) in (("ungrouped", (e, c)), ("grouped", (eg, cg))):
        choi = tomography.pgdb_process_estimate_batch(design, x, n)
        f = distance_measures.process_fidelity_batch(truth, convert_batch("choi", "pauli_liouville", choi))
        print(f"PGDB on the {name:<9} data: process fidelity to the truth {f[0]:.5f}")

    zz = [i for i in range(grouping.n_groups) if np.all(grouping.basis[i] == 3)]
    i = max(zz, key=lambda g: abs(correlation(prob[0, g])))              # the input state that correlates the two qubits most
    state = "".join("XXYYZZ"[s] + "+-"[s % 2] for s in design.in_labels[grouping.groups[i][0]])
    print(f"ZZ-basis group {i} (input state {state}): outcomes 00 01 10 11 drawn {hist[0, i].tolist()}, "
          f"probabilities {np.round(prob[0, i], 4).tolist()}")
    print(f"correlation of the IZ and ZI results: {correlation(hist[0, i]):+.4f} in the shots, "
          f"{correlation(prob[0, i]):+.4f} predicted by the distribution")


if __name__ == "__main__":
    main()
