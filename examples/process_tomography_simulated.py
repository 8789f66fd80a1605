"""Simulated process tomography that never leaves the device: random channels -> noisy expectations of every setting, readout
errors included -> PGDB reconstruction -> process fidelity to the truth (``tomography.simulate_and_estimate_process_batch``).  Only
the fidelities (and the Choi matrices, unused here) come back.  The channels are Haar unitaries by default: the reference's process
fidelity is a fidelity when one of its arguments is unitary (for a mixing channel it is below 1 even against itself; try --kraus 2).

For every shot count the run is made twice: with a perfect readout, where the infidelity to the truth is the statistical error of
the estimator and shrinks with the shots, and with a small asymmetric readout error, where it settles at the bias the misread
bits put into the data.  The counterpart with data drawn on the host: examples/process_tomography_walkthrough.py.

    python examples/process_tomography_simulated.py [--qubits 2] [--channels 64] [--kraus 1]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "forest-benchmarking_amd"))

from fbx import synthetic, tomography  # noqa: E402
from fbx.design import process_design  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, default=2)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--kraus", type=int, default=1, help="Kraus operators per random channel (1: unitaries)")
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    design = process_design(args.qubits, "pauli")
    channels = synthetic.kraus_batch(args.qubits, args.kraus, args.channels, seed=args.seed)
    readout = np.broadcast_to(np.array([0.01, 0.03]), (args.qubits, 2))        # P(read 1 | 0), P(read 0 | 1) of every qubit
    print(f"{args.channels} random channels of {args.kraus} Kraus operators on {args.qubits} qubit(s), {design.m} settings each")
    print(f"{'shots':>8}  {'1 - F, perfect readout':>24}  {'1 - F, readout 1 % / 3 %':>26}")
    for shots in (100, 1000, 10_000, 100_000):
        row = []
        for flips in (None, readout):
            _, fidelity = tomography.simulate_and_estimate_process_batch(design, channels, shots, rep="kraus", readout_flip=flips,
                                                                         seed=args.seed, estimator="pgdb")
            row.append(f"{np.mean(1.0 - fidelity):.5f} +- {np.std(1.0 - fidelity) / np.sqrt(len(fidelity)):.5f}")
        print(f"{shots:>8}  {row[0]:>24}  {row[1]:>26}")


if __name__ == "__main__":
    main()
