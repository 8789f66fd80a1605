"""The table products of an outer PGDB iteration in the one-wave kernels, on designs that reach every path of their loops.

`predict_table` (T = R C, csrc/fbx_pgdb_body.hpp) walks a lane's states three per trip, then a pair, then a single one;
`grad_coefficients` (R^G = -(W C^T) / d^2) walks all states four per trip, then one by one.  With 64 / D = 4 lanes sharing the
states of a 2-qubit design, the number of input states S decides which of these run:

    S = 36 (Pauli)            9 states per lane: triples only                       36 = 9 x 4: no single steps
    S = 16 (SIC)              4 per lane: a triple and a single state               16 = 4 x 4
    S = 37 (Pauli + 1 state)  10 on the first quarter of the lanes, 9 on the rest   9 x 4 + 1
    S = 17 (SIC + 1 state)    5 on the first quarter (a triple and a PAIR), 4 else  4 x 4 + 1
    S = 6  (1 qubit, Pauli)   one state per lane (D = 4: 16 lanes per state slot), one output per lane: 4 + 1 + 1

Every design runs 5 fixed outer iterations on 4 items against the numpy oracle -- estimates, costs, outer / Dykstra / halving
counts per iteration, at the tolerances of tests/test_pgdb_gpu.py (five iterations from the starting point are nowhere near the
stalled iterations whose halvings are rounding-defined) -- and ONE cost and gradient (fbx_pgdb_cost_grad, the same device
functions) against the oracle's dense `A` at 1e-12 like tests/test_cost_grad_gpu.py."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHOI_TOL = 1e-9        # tests/test_pgdb_gpu.py
COST_TOL = 1e-10       # tests/test_pgdb_gpu.py
GRAD_TOL = 1e-12       # tests/test_cost_grad_gpu.py (relative to max(1, |.|))
ITEMS, ITERS = 4, 5
DESIGNS = ["2q-pauli", "2q-sic", "2q-pauli+1", "2q-sic+1", "1q-pauli"]
STATES = {"2q-pauli": 36, "2q-sic": 16, "2q-pauli+1": 37, "2q-sic+1": 17, "1q-pauli": 6}


def _design(name):
    from fbx.design import Design, process_design, traceless_pauli_codes
    n = int(name[0])
    base = process_design(n, name[3:].split("+")[0])
    if "+" not in name:
        return base
    # one more input state, measured in every Pauli: a SIC state beside the Pauli eigenstates, a Pauli eigenstate beside the SIC states
    extra = (7, 8) if "pauli" in name else (0, 3)
    p = traceless_pauli_codes(n)
    ins = np.concatenate([base.in_labels, np.tile(np.array(extra, dtype=np.uint8), (len(p), 1))])
    return Design(n, "process", ins, np.concatenate([base.paulis, p]))


@functools.lru_cache(maxsize=None)
def _case(name):
    """design, data and the oracle's answers for one design -- computed once, shared by both tests, never modified"""
    from fbx import synthetic
    from fbx_oracle import design as od, estimators as oe
    design = _design(name)
    assert design.n_states == STATES[name]
    us = np.array([synthetic.haar_unitary(design.dim, np.random.RandomState(1000 + b)) for b in range(ITEMS)])
    e, c = synthetic.sample_expectations(synthetic.exact_process_expectations(design, us), 1000)
    d = od.Design(design.n_qubits, design.kind, design.in_labels, design.paulis, design.coefs)
    A = oe.design_matrix_A(d)
    want, stats = [], []
    for b in range(ITEMS):
        est, st = oe.pgdb_process_estimate(d, e[b], c[b], A=A, return_stats=True, mode="fixed", max_iters=ITERS)
        want.append(est); stats.append(st)
    want = np.array(want)
    for a in (e, c, want):
        a.setflags(write=False)
    return design, e, c, A, want, stats


@pytest.mark.parametrize("name", DESIGNS)
def test_five_fixed_iterations_match_the_oracle(gpu, name):
    from fbx import tomography
    design, e, c, _, want, wst = _case(name)
    got, st = tomography.pgdb_process_estimate_batch(design, e, c, mode="fixed", max_iters=ITERS, return_stats=True,
                                                     trace_iters=ITERS)
    dev = np.abs(got - want).reshape(ITEMS, -1).max(axis=1)
    print(name, "S", design.n_states, "m", design.m, "max-abs per item", dev, "cost diff",
          [abs(st["cost"][b] - wst[b]["cost"]) for b in range(ITEMS)])
    assert dev.max() < CHOI_TOL
    for b in range(ITEMS):
        assert st["iterations"][b] == wst[b]["iterations"] == ITERS
        assert st["dykstra"][b] == wst[b]["dykstra"]
        wtr = np.array(wst[b]["trace"])
        assert np.array_equal(st["trace"][b, :, 0], wtr[:, 0])          # Dykstra iterations of every outer iteration
        assert np.array_equal(st["trace"][b, :, 1], wtr[:, 1])          # halvings of every outer iteration
        assert st["backtracks"][b] == wtr[:, 1].sum()
        assert abs(st["cost"][b] - wst[b]["cost"]) < COST_TOL


@pytest.mark.parametrize("name", DESIGNS)
def test_cost_and_gradient_match_the_dense_oracle(gpu, name):
    from fbx import tomography
    from fbx_oracle import estimators as oe
    design, e, c, A, want, _ = _case(name)
    D = design.dim ** 2
    rng = np.random.default_rng(11)
    h = rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D))
    ests = [want[0], want[1], np.eye(D) / design.dim, want[2] + 0.05 * (h + h.conj().T)]     # the last one: clipped probabilities
    items = [0, 1, 2, 2]
    nv = np.array([oe.counts_vector(e[b], c[b])[:, 0] for b in items])
    cost, grad = tomography.cost_and_gradient_batch(design, nv, np.array(ests))
    for k, est in enumerate(ests):
        want_c = oe.cost(A, nv[k][:, None], est).real.item()
        want_g = oe.grad_cost(A, nv[k][:, None], est)
        scale = max(1.0, float(np.abs(want_g).max()))
        print(name, k, "cost err", abs(cost[k] - want_c), "grad err / scale", np.abs(grad[k] - want_g).max() / scale)
        assert abs(cost[k] - want_c) <= GRAD_TOL * max(1.0, abs(want_c))
        assert np.abs(grad[k] - want_g).max() <= GRAD_TOL * scale
