"""The one-wave 2-qubit PGDB kernels reproduce recorded results BIT FOR BIT.

tests/golden/pgdb2q_onewave_bits.npz holds, for three seeded items (synthetic.process_batch(2, basis, 3)), what the build
before the hand-scheduled Jacobi round computed on an MI355X: in-basis pauli and sic (pgdb_kernel<2,9> and <2,4>),
trace-preserving and not, 100 fixed iterations and to convergence -- the smallest inputs that pass through a cold start, warm
starts from the previous iterate and from the stored bases, and stalled iterations.  Per case: Choi matrices as raw float64,
costs, iteration / Dykstra / halving counts and the four work counters.  Changes that only reorder instructions (scheduling,
register allocation, load placement) must keep every one of them.

A change that alters the arithmetic ON PURPOSE (another rotation formula, tolerance, summation order) regenerates the fixture
from its own build on the GPU and says so in its description:
    python tests/golden/make_pgdb_bits.py
after the oracle-parity tests (test_pgdb_gpu.py and the golden-file tests) pass with it."""
import os

import numpy as np
import pytest

import make_pgdb_bits as mk

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pgdb2q_onewave_bits.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in g.files}


def test_fixture_is_complete(golden):
    want = {f"{mk.case_name(*c)}/{k}" for c in mk.cases() for k in ("choi", "cost") + mk.INT_KEYS}
    assert set(golden) == want
    for c in mk.cases():
        n = mk.case_name(*c)
        assert golden[n + "/choi"].shape == (mk.ITEMS, 16, 16, 2) and golden[n + "/choi"].dtype == np.float64
        assert np.isfinite(golden[n + "/choi"]).all()
    # the fixed runs do all 100 iterations, the others stop by themselves; at least one item stalls (halvings) in a fixed run
    assert all((golden[f"{mk.case_name(b, tp, 'fixed')}/iterations"] == 100).all() for b in mk.BASES for tp in (True, False))
    assert all((golden[f"{mk.case_name(b, tp, 'converge')}/iterations"] < 100).all() for b in mk.BASES for tp in (True, False))
    assert any((golden[f"{mk.case_name(b, tp, 'fixed')}/backtracks"] > 0).any() for b in mk.BASES for tp in (True, False))


@pytest.mark.gpu
@pytest.mark.parametrize("basis,tp,mode", list(mk.cases()), ids=[mk.case_name(*c) for c in mk.cases()])
def test_bits(gpu, golden, basis, tp, mode):
    got = mk.run_case(basis, tp, mode)
    name = mk.case_name(basis, tp, mode)
    for k, v in got.items():
        want = golden[f"{name}/{k}"]
        assert v.dtype == want.dtype and v.shape == want.shape, k
        if v.dtype == np.float64:              # raw bits: -0.0 and 0.0, or two NaNs, are not the same result
            v, want = v.view(np.uint64), want.view(np.uint64)
        bad = np.argwhere(v != want)
        assert bad.size == 0, f"{name}/{k}: {len(bad)} of {v.size} entries differ, first at {bad[0].tolist()}"
