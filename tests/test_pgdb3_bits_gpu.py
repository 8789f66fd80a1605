"""The four kernels of the 3-qubit unit (csrc/fbx_pgdb3.hip) reproduce recorded results BIT FOR BIT.

tests/golden/pgdb3q_bits.npz holds what the build before the unit's clean-up (dead paths removed, twice-written code folded)
computed on an MI355X, recorded twice there with byte-identical arrays: pgdb3_kernel<4 | 14 | 32 | 64> on the smallest
designs that reach each instantiation -- fixed iteration counts, trace-preserving and not, and a run to convergence that passes
through small steps, stored bases and a stalled line search --, fbx_pgdb_cost_grad on the SIC and the Pauli design, every kind of
fbx_proj_choi including an item with a NaN, and fbx_linv_process (tests/golden/make_pgdb3_bits.py lists the cases).  Changes
that only move, fold or reorder code must keep every one of them.

A change that alters the arithmetic ON PURPOSE regenerates the fixture from its own build on the GPU and says so in its
description:
    python tests/golden/make_pgdb3_bits.py
after the oracle-parity tests (test_pgdb3_gpu.py, test_cost_grad_gpu.py and the golden-file tests) pass with it."""
import os

import numpy as np
import pytest

import make_pgdb3_bits as mk

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pgdb3q_bits.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in g.files}


def same_bits(got, golden, name):
    for k, v in got.items():
        want = golden[f"{name}/{k}"]
        assert v.dtype == want.dtype and v.shape == want.shape, k
        if v.dtype == np.float64:              # raw bits: -0.0 and 0.0, or two NaNs, are not the same result
            v, want = v.view(np.uint64), want.view(np.uint64)
        bad = np.argwhere(v != want)
        assert bad.size == 0, f"{name}/{k}: {len(bad)} of {v.size} entries differ, first at {bad[0].tolist()}"


def test_fixture_is_complete(golden):
    assert set(golden) == mk.keys()
    for n, (_, items, kw) in mk.PGDB_CASES.items():
        assert golden[n + "/choi"].shape == (items, 64, 64, 2) and golden[n + "/choi"].dtype == np.float64
        assert np.isfinite(golden[n + "/choi"]).all() and np.isfinite(golden[n + "/cost"]).all()
        if kw["mode"] == "fixed":              # the fixed runs did all their iterations
            assert (golden[n + "/iterations"] == kw["max_iters"]).all()
    # the run to convergence went past the fixed runs' 12 iterations; at least one item stalls (halvings)
    assert (golden["sic_tp_converge/iterations"] > 12).all()
    assert any((golden[n + "/backtracks"] > 0).any() for n in mk.PGDB_CASES)
    for n in mk.COSTGRAD_CASES:
        assert golden[n + "/grad"].shape == (2, 64, 64, 2) and np.isfinite(golden[n + "/grad"]).all() and np.isfinite(golden[n + "/cost"]).all()
    for kind in mk.PROJ_KINDS:                 # the Dykstra kinds iterate on the finite items and report 1 for the NaN item
        assert golden[f"proj_{kind}/sha256"].shape == (mk.PROJ_ITEMS, 32)
        assert (golden[f"proj_{kind}/iters"] == [0, 0, 0]).all() if kind < 3 else \
            ((golden[f"proj_{kind}/iters"][:2] > 1).all() and golden[f"proj_{kind}/iters"][2] == 1)
    assert golden["linv_sic/sha256"].shape == (2, 32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(mk.PGDB_CASES))
def test_pgdb_bits(gpu, golden, name):
    same_bits(mk.run_pgdb(name), golden, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(mk.COSTGRAD_CASES))
def test_cost_grad_bits(gpu, golden, name):
    """at the maximally mixed estimate and at the recorded estimate of item 0 of the design's fixed PGDB case"""
    same_bits(mk.run_costgrad(name, golden[mk.COSTGRAD_CASES[name][1] + "/choi"][0]), golden, name)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", mk.PROJ_KINDS)
def test_projection_bits(gpu, golden, kind):
    same_bits(mk.run_proj(kind), golden, f"proj_{kind}")


@pytest.mark.gpu
def test_linear_inversion_bits(gpu, golden):
    same_bits(mk.run_linv(), golden, "linv_sic")
