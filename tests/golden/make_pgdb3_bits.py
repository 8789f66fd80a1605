"""Writes tests/golden/pgdb3q_bits.npz: the exact bits the four kernels of the 3-qubit unit (csrc/fbx_pgdb3.hip) produce, from the
build it is run with on a GPU (tests/test_pgdb3_bits_gpu.py compares later builds against them).

    python tests/golden/make_pgdb3_bits.py [OUT.npz]         (FBX_LIBRARY selects the build; default: the in-tree libfbx.so)

PGDB cases -- the smallest that reach each instantiation of pgdb3_kernel and each path through it (seeded items of
synthetic.process_batch(3, basis, ...): 3 and 4 for the SIC in-basis -- item 3 converges without a halving, item 4 ends in a stalled
line search of some thirty halvings, the batched cost ladder --, 0 and 1 for the Pauli in-basis):
    sic_tp_fixed, sic_cp_fixed   <4>    2 items, 12 fixed iterations, trace-preserving and not
    sic_tp_converge              <4>    2 items, to convergence: small steps, stored bases, stalled line searches
    pauli_tp_fixed               <14>   2 items, 6 fixed iterations
    pad4_tp_fixed                <32>   1 item, the SIC design with 3 zero-count repetitions (16 128 settings), 3 iterations
    pad9_tp_fixed                <64>   1 item, ... with 8 zero-count repetitions (36 288 settings), 2 iterations
Per case: the Choi matrices as raw float64 [items, 64, 64, 2], the costs, the iteration / Dykstra / halving counts and the four
work counters.  In every design a (state, Pauli) cell of the gradient weights W receives one term with counts and otherwise exact
zeros, so the LDS atomics that fill W cannot depend on their order.

costgrad_sic, costgrad_pauli: fbx_pgdb_cost_grad at the maximally mixed estimate and at item 0 of sic_tp_fixed / pauli_tp_fixed
(a physical estimate a few iterations in): cost and gradient as raw float64.
proj_<kind>: fbx_proj_choi, every kind (CP, TP, TNI, physical with TP and with TNI), on two Hermitian non-physical 64 x 64 matrices and one with a NaN in it: iteration
counts and one sha256 digest per item of the output's bytes (raw arrays would take the file past the size a fixture may have).
linv_sic: fbx_linv_process, 2 items, one digest per item.

Run it from the commit whose results are the contract -- a change that only moves or reorders code must not need it."""
import functools
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "forest-benchmarking_amd"))

D = 64
FIRST_ITEM = {"sic": 3, "pauli": 0}
INT_KEYS = ("iterations", "dykstra", "backtracks", "jacobi_sweeps", "eig_terms", "cost_evals", "power_sum_passes")
# name -> (design, items, arguments of pgdb_process_estimate_batch)
PGDB_CASES = {
    "sic_tp_fixed": ("sic", 2, dict(trace_preserving=True, mode="fixed", max_iters=12)),
    "sic_cp_fixed": ("sic", 2, dict(trace_preserving=False, mode="fixed", max_iters=12)),
    "sic_tp_converge": ("sic", 2, dict(trace_preserving=True, mode="converge")),
    "pauli_tp_fixed": ("pauli", 2, dict(trace_preserving=True, mode="fixed", max_iters=6)),
    "pad4_tp_fixed": ("pad4", 1, dict(trace_preserving=True, mode="fixed", max_iters=3)),
    "pad9_tp_fixed": ("pad9", 1, dict(trace_preserving=True, mode="fixed", max_iters=2)),
}
COSTGRAD_CASES = {"costgrad_sic": ("sic", "sic_tp_fixed"), "costgrad_pauli": ("pauli", "pauli_tp_fixed")}   # name -> (design, PGDB case of the physical estimate)
PROJ_KINDS = (0, 1, 2, 3, 4)          # FBX_PROJ_CP, _TP, _TNI, _PHYSICAL_TP, _PHYSICAL_TNI (include/fbx.h)
PROJ_ITEMS = 3


def keys():
    """every key of the fixture"""
    out = {f"{n}/{k}" for n in PGDB_CASES for k in ("choi", "cost") + INT_KEYS}
    out |= {f"{n}/{k}" for n in COSTGRAD_CASES for k in ("cost", "grad")}
    out |= {f"proj_{kind}/{k}" for kind in PROJ_KINDS for k in ("sha256", "iters")}
    return out | {"linv_sic/sha256"}


@functools.lru_cache(maxsize=None)
def data(design):
    """(Design, expectations, counts) of two seeded items (FIRST_ITEM); pad<reps>: the SIC design followed by reps - 1 zero-count copies of itself
    (the same likelihood on a longer list, as tests/test_repeated_datasets.py builds it)"""
    from fbx import design as fd, synthetic
    if design in ("sic", "pauli"):
        d, _, e, c = synthetic.process_batch(3, design, 2, first_item=FIRST_ITEM[design])
        return d, e, c
    reps = int(design[3:])
    base, e, c = data("sic")
    big = fd.Design(3, "process", np.tile(base.in_labels, (reps, 1)), np.tile(base.paulis, (reps, 1)))
    return (big, np.concatenate([e] + [np.zeros_like(e)] * (reps - 1), axis=1),
            np.concatenate([c] + [np.zeros_like(c)] * (reps - 1), axis=1))


def raw(x):
    """complex [B, 64, 64] -> float64 [B, 64, 64, 2]"""
    x = np.ascontiguousarray(x)
    return x.view(np.float64).reshape(x.shape[0], D, D, 2).copy()


def digests(x):
    """one sha256 digest per item of a [B, ...] array's bytes, as uint8 [B, 32]"""
    return np.array([np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8) for a in x])


def run_pgdb(name):
    from fbx import tomography
    design, items, kw = PGDB_CASES[name]
    d, e, c = data(design)
    choi, st = tomography.pgdb_process_estimate_batch(d, e[:items], c[:items], return_stats=True, **kw)
    out = {"choi": raw(choi), "cost": np.array(st["cost"], dtype=np.float64)}
    for k in INT_KEYS:
        out[k] = np.array(st[k], dtype=np.int32)
    return out


def run_costgrad(name, physical):
    """`physical`: float64 [64, 64, 2], the estimate of item 0 a few PGDB iterations in (from the PGDB case COSTGRAD_CASES names)"""
    from fbx import tomography
    d, e, c = data(COSTGRAD_CASES[name][0])
    est = np.stack([np.eye(D, dtype=np.complex128) / 8, np.ascontiguousarray(physical).view(np.complex128).reshape(D, D)])
    n = np.repeat(tomography.normalised_counts(e[:1], c[:1]), 2, axis=0)
    cost, grad = tomography.cost_and_gradient_batch(d, n, est)
    return {"cost": np.array(cost, dtype=np.float64), "grad": raw(grad)}


def proj_inputs():
    """two Hermitian matrices with eigenvalues of both signs and a partial trace away from the identity; a third with one NaN"""
    r = np.random.RandomState(364)
    x = r.randn(PROJ_ITEMS, D, D) + 1j * r.randn(PROJ_ITEMS, D, D)
    x = (x + x.conj().transpose(0, 2, 1)) / 16 + np.eye(D) / 8
    x[2, 5, 7] = np.nan
    return x


def run_proj(kind):
    from fbx.operator_tools import project_superoperators as ps
    out, iters = ps.proj_choi_batch(kind, proj_inputs(), return_iters=True)
    return {"sha256": digests(out), "iters": np.array(iters, dtype=np.int32)}


def run_linv():
    from fbx import tomography
    d, e, _ = data("sic")
    return {"sha256": digests(tomography.linear_inv_process_estimate_batch(d, e))}


def run_all():
    arrays = {}
    for n in PGDB_CASES:
        for k, v in run_pgdb(n).items():
            arrays[f"{n}/{k}"] = v
        print(n, "iterations", arrays[n + "/iterations"], "dykstra", arrays[n + "/dykstra"], "halvings", arrays[n + "/backtracks"], flush=True)
    for n, (_, src) in COSTGRAD_CASES.items():
        for k, v in run_costgrad(n, arrays[src + "/choi"][0]).items():
            arrays[f"{n}/{k}"] = v
        print(n, "cost", arrays[n + "/cost"], flush=True)
    for kind in PROJ_KINDS:
        for k, v in run_proj(kind).items():
            arrays[f"proj_{kind}/{k}"] = v
        print("proj", kind, "iterations", arrays[f"proj_{kind}/iters"], flush=True)
    arrays["linv_sic/sha256"] = run_linv()["sha256"]
    return arrays


if __name__ == "__main__":
    from fbx import _lib
    _lib.set_device(0)
    arrays = run_all()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "pgdb3q_bits.npz")
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")
