"""Writes tests/golden/pgdb2q_onewave_bits.npz: the exact bits the one-wave 2-qubit PGDB kernels produce for three seeded
items, from the build it is run with on a GPU (tests/test_pgdb_onewave_bits_gpu.py compares later builds against them).

    python tests/golden/make_pgdb_bits.py [OUT.npz]         (FBX_LIBRARY selects the build; default: the in-tree libfbx.so)

Cases: in-basis pauli / sic (pgdb_kernel<2,9> / <2,4>), trace-preserving or not, 100 fixed iterations or to convergence.
Per case: the Choi matrices as raw float64 [3, 16, 16, 2], the costs, the iteration / Dykstra / halving counts and the four
work counters.  Run it from the commit whose results are the contract -- a scheduling change must not need it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "forest-benchmarking_amd"))

ITEMS = 3
BASES = ("pauli", "sic")
MODES = {"fixed": dict(mode="fixed", max_iters=100), "converge": dict(mode="converge")}
INT_KEYS = ("iterations", "dykstra", "backtracks", "jacobi_sweeps", "eig_terms", "cost_evals", "power_sum_passes")


def case_name(basis, tp, mode):
    return f"{basis}_{'tp' if tp else 'cp'}_{mode}"


def cases():
    for basis in BASES:
        for tp in (True, False):
            for mode in MODES:
                yield basis, tp, mode


def run_case(basis, tp, mode):
    """name -> array of everything the kernel reports for the case, on the loaded build"""
    from fbx import synthetic, tomography
    design, _, e, c = synthetic.process_batch(2, basis, ITEMS)
    choi, st = tomography.pgdb_process_estimate_batch(design, e, c, trace_preserving=tp, return_stats=True, **MODES[mode])
    out = {"choi": np.ascontiguousarray(choi).view(np.float64).reshape(ITEMS, 16, 16, 2).copy(),
           "cost": np.array(st["cost"], dtype=np.float64)}
    for k in INT_KEYS:
        out[k] = np.array(st[k], dtype=np.int32)
    return out


if __name__ == "__main__":
    from fbx import _lib
    _lib.set_device(0)
    arrays = {}
    for basis, tp, mode in cases():
        for k, v in run_case(basis, tp, mode).items():
            arrays[f"{case_name(basis, tp, mode)}/{k}"] = v
        n = case_name(basis, tp, mode)
        print(n, "iterations", arrays[n + "/iterations"], "dykstra", arrays[n + "/dykstra"], "halvings", arrays[n + "/backtracks"])
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "pgdb2q_onewave_bits.npz")
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")
