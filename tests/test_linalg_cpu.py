"""The fixture of tests/test_linalg_gpu.py checked without a GPU: the builders of tests/linalg_cases.py still produce the
matrices whose hashes tests/golden/linalg_cases.npz records; numpy.linalg.eigh meets every bound the device is held to, on
every case (so a failure on the device is the device's, not the reference's or the bound's); and on the Gaussian cases the new
eigenvalue tolerance is at most the 1e-12 N max(1, |A|max) of the tests beside it (tests/test_extras_gpu.py)."""
import os

import numpy as np
import pytest

import linalg_cases as lc

GOLD = os.path.join(os.path.dirname(__file__), "golden", "linalg_cases.npz")
SIZES = lc.DIRECT_SIZES + lc.PADDED_SIZES


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _row(gold, k):
    return [str(x) for x in gold["keys"]].index(k)


def test_fixture_lists_every_case_once(gold):
    assert [str(k) for k in gold["keys"]] == lc.all_keys()
    assert float(gold["c_w"]) >= 1.0
    for N in lc.DIRECT_SIZES:
        assert tuple(lc.cases(N)) == lc.DIRECT_FAMILIES
    for N in lc.PADDED_SIZES:
        missing = set(lc.PADDED_FAMILIES) - set(lc.cases(N))
        assert missing <= ({"rep_zero", "mixed_zero", "oplus0"} if N < 3 else set()), (N, missing)


@pytest.mark.parametrize("N", SIZES)
def test_hashes_match_the_builders(gold, N):
    for name, a in lc.cases(N).items():
        assert lc.sha256(a) == str(gold["sha256"][_row(gold, lc.key(name, N))]), lc.key(name, N)
        h = lc.hermitian(a)
        assert np.isfinite(h).all() and np.array_equal(h, h.conj().T)
        if name != "upper_garbage":
            assert np.array_equal(h, a), lc.key(name, N)
        else:
            assert not np.isfinite(a[np.triu_indices(N, 1)]).all()


@pytest.mark.parametrize("N", SIZES)
def test_numpy_eigh_meets_every_bound(gold, N):
    c_w = float(gold["c_w"])
    for name, a in lc.cases(N).items():
        k = lc.key(name, N)
        row = _row(gold, k)
        norm2, normF, w_ref = float(gold["norm2"][row]), float(gold["normF"][row]), gold["w_" + k]
        assert w_ref.shape == (N,) and (np.diff(w_ref) >= 0).all()
        assert norm2 == np.abs(w_ref).max() and norm2 <= normF * (1 + 1e-15)
        w, v = np.linalg.eigh(lc.hermitian(a))
        assert np.abs(w - w_ref).max() <= lc.eigenvalue_tol(N, norm2, normF, c_w), k
        assert lc.residual(a, w, v) <= lc.residual_tol(N, normF, c_w), k
        assert lc.orthogonality(v) <= lc.orthogonality_tol(N), k


@pytest.mark.parametrize("N", SIZES)
def test_new_tolerance_is_no_wider_than_the_old_one_on_gaussian_input(gold, N):
    row = _row(gold, lc.key("gaussian", N))
    a = lc.cases(N)["gaussian"]
    new = lc.eigenvalue_tol(N, float(gold["norm2"][row]), float(gold["normF"][row]), float(gold["c_w"]))
    assert new <= 1e-12 * N * max(1.0, np.abs(a).max())
