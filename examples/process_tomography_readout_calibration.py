"""Simulated process tomography under an asymmetric, correlated readout error, with the two defaults of the reference's
``do_tomography`` that exist to undo such an error: exhaustive readout symmetrization (``symm_type=-1``) and the calibration of
every observable on its +1 eigenstate (``calibrate_observables=True``).  A two-qubit unitary is measured through a joint
confusion matrix -- a tensor product of asymmetric per-qubit flips mixed with a random row-stochastic matrix, so that what one
qubit reads depends on the other -- and PGDB reconstructs it three times on the device, truth -> shots -> estimate -> fidelity:

    raw                          symm_type = 0, no calibration: the plain readout error
    symmetrized                  symm_type = -1: the error is made symmetric, the expectations still shrink
    symmetrized and calibrated   ... and every expectation is divided by its observable's calibration

The fidelity of each estimate to the truth is printed.  What stays after the third is shot noise and the crosstalk on settings
that act on one qubit of a two-qubit group: the calibration flips only the observable's own qubits.

    python examples/process_tomography_readout_calibration.py [--shots 4000] [--batch 8] [--crosstalk 0.1] [--seed 7]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "forest-benchmarking_amd"))

from fbx import readout, synthetic, tomography  # noqa: E402
from fbx.design import group_design, process_design  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=4000, help="shots per group, and per calibration")
    ap.add_argument("--batch", type=int, default=8, help="number of random unitaries")
    ap.add_argument("--crosstalk", type=float, default=0.1, help="weight of the random row-stochastic part of the matrix")
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    design = process_design(2, "pauli")
    grouping = group_design(design)
    product = readout.confusion_from_flips([[0.03, 0.09], [0.05, 0.12]])        # P(read 1 | 0), P(read 0 | 1) per qubit
    r = rng.random((4, 4)) ** 3
    confusion = (1.0 - args.crosstalk) * product + args.crosstalk * r / r.sum(axis=1, keepdims=True)
    print("joint confusion matrix [drawn][read], bitstrings 00 01 10 11:")
    print(np.round(confusion, 4))
    us = np.array([synthetic.haar_unitary(4, np.random.RandomState(args.seed + b)) for b in range(args.batch)])
    cal_paulis, _ = tomography.calibration_list(design)
    print(f"{args.batch} Haar unitaries, {grouping.n_groups} groups of {args.shots} shots, {len(cal_paulis)} calibrations")
    kw = dict(rep="unitary", confusion=confusion, groups=grouping, seed=args.seed)
    for name, opts in (("raw", dict(symm_type=0, calibrate=False)),
                       ("symmetrized", dict(symm_type=-1, calibrate=False)),
                       ("symmetrized and calibrated", dict(symm_type=-1, calibrate=True))):
        _, fid = tomography.simulate_and_estimate_process_batch(design, us, args.shots, **kw, **opts)
        print(f"{name:<27} process fidelity to the truth: mean {fid.mean():.5f}, worst {fid.min():.5f}")


if __name__ == "__main__":
    main()
