"""Writes tests/golden/pgdb2q_onewave_slot_bits.npz: the exact bits the one-wave 2-qubit PGDB kernels produce on designs that
reach what pgdb2q_onewave_bits.npz does not -- lanes and whole outcome slots without a setting, observable coefficients other
than 1, and line searches with a listed / an overfull set of outcomes at the probability clip
(tests/test_pgdb_onewave_slots_gpu.py compares later builds against them).

    python tests/golden/make_pgdb_slot_bits.py COMMIT [OUT.npz]     (FBX_LIBRARY selects the build; default: the in-tree libfbx.so)

COMMIT is the commit the loaded build was compiled from; it is stored in the file.  Run it from the commit whose results are
the contract -- a scheduling change must not need it.

Every case is three items, two qubits, trace preserving, 100 fixed iterations, on a design made of settings of the 540-setting
Pauli design (36 input states x 15 Paulis):
    m512, m300   the first 512 / 300 settings: pgdb_kernel<2,9> with one empty slot / with four empty slots and a partial one
    m256         the first 256: pgdb_kernel<2,4>, every slot exactly full
    m577         all 540 and the first 37 again: pgdb_kernel<2,16>, one lane in slot 9, six empty slots
    nonunit      540 settings with coefficients -1 and 0.5 in a fixed pattern, the expectations scaled to match
    clip_few     540; Clifford channels, 5 % depolarised and sampled, with the exact +-1 written over six settings: a handful of
                 outcomes end at the clip (the listed set, 1..64)
    clip_many    540; the exact expectations of the Clifford channels: 108 outcomes at the clip (more than 64: full evaluations)
For the last two the number of outcomes whose model probability (the oracle's design matrix applied to the recorded Choi
matrices) is below 2e-6 is checked here, per item, against those ranges."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "forest-benchmarking_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

ITEMS = 3
CASES = ("m512", "m300", "m256", "m577", "nonunit", "clip_few", "clip_many")
INT_KEYS = ("iterations", "dykstra", "backtracks", "jacobi_sweeps", "eig_terms", "cost_evals", "power_sum_passes")
CLIP_RANGE = {"clip_few": (1, 64), "clip_many": (65, 1080)}       # outcomes below 2e-6, per item
NEAR_CLIP = 2e-6


def _clifford_unitaries():
    h = np.array([[1, 1], [1, -1]], dtype=complex) / np.sqrt(2)
    s = np.diag([1, 1j])
    eye = np.eye(2, dtype=complex)
    cnot = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]], dtype=complex)
    cz = np.diag([1, 1, 1, -1]).astype(complex)
    return np.array([cnot @ np.kron(h, s), cz @ np.kron(s @ h, h), np.kron(h, eye) @ cnot @ np.kron(s, h)])


def case_inputs(case):
    """(in_labels, paulis, coefs or None, expectations [3, m], counts [3, m]) of a case: host arithmetic only"""
    from fbx import synthetic
    base, _, e, c = synthetic.process_batch(2, "pauli", ITEMS)
    coefs = None
    idx = np.arange(base.m)
    if case in ("m512", "m300", "m256"):
        idx = idx[:int(case[1:])]
    elif case == "m577":
        idx = np.concatenate([idx, idx[:37]])
    elif case == "nonunit":
        coefs = np.where((7 * np.arange(base.m)) % 5 < 2, -1.0, 0.5)
        e = e * coefs[None, :]
    elif case in ("clip_few", "clip_many"):
        us = _clifford_unitaries()
        exact = synthetic.exact_process_expectations(base, us)
        if case == "clip_many":
            e, c = exact, np.full(exact.shape, 1000.0)
        else:
            e, c = synthetic.sample_expectations(synthetic.exact_process_expectations(base, us, 0.05), 1000)
            for b in range(ITEMS):
                ks = np.flatnonzero(np.abs(np.abs(exact[b]) - 1.0) < 1e-12)[::18][:6]
                e[b, ks] = exact[b, ks]
    else:
        raise ValueError(case)
    return (base.in_labels[idx], base.paulis[idx], coefs, np.ascontiguousarray(e[:, idx]), np.ascontiguousarray(c[:, idx]))


def run_case(case):
    """name -> array of everything the kernel reports for the case, on the loaded build"""
    from fbx import tomography
    from fbx.design import Design
    ins, paulis, coefs, e, c = case_inputs(case)
    design = Design(2, "process", ins, paulis, coefs)
    choi, st = tomography.pgdb_process_estimate_batch(design, e, c, trace_preserving=True, return_stats=True, mode="fixed", max_iters=100)
    out = {"choi": np.ascontiguousarray(choi).view(np.float64).reshape(ITEMS, 16, 16, 2).copy(),
           "cost": np.array(st["cost"], dtype=np.float64)}
    for k in INT_KEYS:
        out[k] = np.array(st[k], dtype=np.int32)
    return out


def outcomes_near_clip(case, choi):
    """per item: outcomes whose model probability under the recorded Choi matrix is below 2e-6 (CPU; the oracle's design matrix)"""
    from fbx_oracle import design as od, estimators as oe
    ins, paulis, coefs, _, _ = case_inputs(case)
    A = oe.design_matrix_A(od.Design(2, "process", ins, paulis, np.ones(len(paulis)) if coefs is None else coefs))
    est = choi[..., 0] + 1j * choi[..., 1]
    return [int((np.real(A @ oe.vec(est[b]))[:, 0] < NEAR_CLIP).sum()) for b in range(ITEMS)]


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    from fbx import _lib
    _lib.set_device(0)
    arrays = {"commit": np.array(sys.argv[1])}
    for case in CASES:
        got = run_case(case)
        for k, v in got.items():
            arrays[f"{case}/{k}"] = v
        print(case, "dykstra", got["dykstra"], "halvings", got["backtracks"], "cost evaluations", got["cost_evals"],
              "power-sum passes", got["power_sum_passes"], flush=True)
        if case in CLIP_RANGE:
            n, (lo, hi) = outcomes_near_clip(case, got["choi"]), CLIP_RANGE[case]
            print(case, "outcomes below 2e-6 per item:", n)
            if not all(lo <= x <= hi for x in n):
                sys.exit(f"{case}: {n} outcomes near the clip, want {lo}..{hi} for every item -- choose another input")
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "pgdb2q_onewave_slot_bits.npz")
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")
