"""The one-wave 2-qubit PGDB kernels reproduce recorded results BIT FOR BIT where a lane's outcome slots are not all in use.

tests/golden/pgdb2q_onewave_bits.npz (test_pgdb_onewave_bits_gpu.py) holds the full 540- and 240-setting designs with unit
coefficients.  tests/golden/pgdb2q_onewave_slot_bits.npz adds what the passes over a lane's outcome slots do beyond those:
lanes and whole slots without a setting (m = 512, 300 in pgdb_kernel<2,9>, m = 577 in <2,16>), every slot exactly full (m = 256
in <2,4>), observable coefficients other than 1, and line searches with a listed (1..64) and an overfull (> 64) set of outcomes
at the probability clip.  Every case is three items, trace preserving, 100 fixed iterations
(tests/golden/make_pgdb_slot_bits.py describes the inputs).  The file was written by the build of the commit stored in it, before
the slot passes of the one-wave kernel became straight-line code; per case it holds the Choi matrices as raw float64, the costs,
the iteration / Dykstra / halving counts and the four work counters, and a later build must keep every one of them."""
import os

import numpy as np
import pytest

import make_pgdb_slot_bits as mk

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pgdb2q_onewave_slot_bits.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in g.files}


def test_fixture_is_complete(golden):
    want = {f"{c}/{k}" for c in mk.CASES for k in ("choi", "cost") + mk.INT_KEYS} | {"commit"}
    assert set(golden) == want
    assert len(str(golden["commit"])) == 40 and int(str(golden["commit"]), 16) >= 0
    for c in mk.CASES:
        assert golden[c + "/choi"].shape == (mk.ITEMS, 16, 16, 2) and golden[c + "/choi"].dtype == np.float64
        assert np.isfinite(golden[c + "/choi"]).all() and np.isfinite(golden[c + "/cost"]).all()
        assert golden[c + "/cost"].shape == (mk.ITEMS,) and golden[c + "/cost"].dtype == np.float64
        for k in mk.INT_KEYS:
            assert golden[f"{c}/{k}"].shape == (mk.ITEMS,) and golden[f"{c}/{k}"].dtype == np.int32
        assert (golden[c + "/iterations"] == 100).all()
    # the designs are what the cases say: sizes on either side of the slot counts of the three instantiations
    assert [mk.case_inputs(c)[1].shape[0] for c in mk.CASES] == [512, 300, 256, 577, 540, 540, 540]
    coefs = mk.case_inputs("nonunit")[2]
    assert set(np.unique(coefs)) == {-1.0, 0.5}
    # the clip cases ended where they were meant to: outcomes below 2e-6 under the recorded estimates (CPU, the oracle's design matrix)
    for c, (lo, hi) in mk.CLIP_RANGE.items():
        n = mk.outcomes_near_clip(c, golden[c + "/choi"])
        assert all(lo <= x <= hi for x in n), (c, n)
    # a listed clip set goes through the power sums, an overfull one through full evaluations only
    assert (golden["clip_few/power_sum_passes"] > 0).all()
    assert (golden["clip_many/power_sum_passes"] == 0).all() and (golden["clip_many/cost_evals"] > 100).all()
    # at least one item of every other case stalls (long halving runs: the one-pass ladder)
    assert all((golden[c + "/backtracks"] > 0).any() for c in mk.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", mk.CASES)
def test_bits(gpu, golden, case):
    got = mk.run_case(case)
    for k, v in got.items():
        want = golden[f"{case}/{k}"]
        assert v.dtype == want.dtype and v.shape == want.shape, k
        if v.dtype == np.float64:              # raw bits: -0.0 and 0.0, or two NaNs, are not the same result
            v, want = v.view(np.uint64), want.view(np.uint64)
        bad = np.argwhere(v != want)
        assert bad.size == 0, f"{case}/{k}: {len(bad)} of {v.size} entries differ, first at {bad[0].tolist()}"
