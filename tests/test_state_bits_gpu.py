"""The state-tomography kernels (csrc/fbx_state.hip, csrc/fbx_state_measures.hip) reproduce recorded results BIT FOR BIT.

tests/golden/state_bits.npz holds what the build before the two units were split and their repeated code folded computed on an
MI355X, recorded twice there with byte-identical arrays: every instantiation of the iterative-MLE kernels and every path through
them (several items per wavefront, a setting per lane, settings staged in LDS and streamed, hedging and the entropy penalty, the
4- and 5-qubit workgroup kernels), the R operator, the log-likelihood and linear inversion, the physical projection with an item
that is kept, one that is rebuilt and one with a NaN, the four state measures, and the Pauli vector
(tests/golden/make_state_bits.py lists the cases).  Changes that only move, fold or reorder code must keep every one of them.

A change that alters the arithmetic ON PURPOSE regenerates the fixture from its own build on the GPU and says so in its
description:
    python tests/golden/make_state_bits.py
after the oracle-parity tests (test_state_gpu.py, test_state_big_gpu.py, test_state_dispatch_gpu.py, the state-measures tests and
test_repeated_datasets.py) pass with it."""
import hashlib
import os

import numpy as np
import pytest

import make_state_bits as mk

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "state_bits.npz")


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


def matrix_shape(items, n):
    """what make_state_bits.stored keeps of `items` d x d matrices"""
    return (items, 2 ** n, 2 ** n, 2) if n <= mk.RAW_QUBITS else (items, 32)


def all_nan(stored_item, n):
    """the stored form of a d x d matrix with NaN in every entry"""
    if n <= mk.RAW_QUBITS:
        return bool(np.isnan(stored_item).all())
    nan = np.full((2 ** n, 2 ** n), complex(np.nan, np.nan))
    return bytes(stored_item) == hashlib.sha256(nan.tobytes()).digest()


def test_fixture_is_complete(golden):
    assert set(golden) == mk.keys()
    for name, (n, _, _, items, mode, _) in mk.MLE_CASES.items():
        rho, it, hit = golden[name + "/rho"], golden[name + "/iterations"], golden[name + "/hit_max"]
        assert rho.shape == matrix_shape(items, n) and rho.dtype == (np.float64 if n <= mk.RAW_QUBITS else np.uint8)
        assert it.shape == hit.shape == (items,) and it.dtype == np.int32 and hit.dtype == np.uint8
        if n <= mk.RAW_QUBITS:
            assert np.isfinite(rho).all()
        maxiter = mk.mle_kwargs(name)["maxiter"]
        if mode == "converge":                 # stopped on tol, before the cap
            assert (it < maxiter).all() and (it > 1).all() and not hit.any()
        else:                                  # maxiter - 1 updates, then the cap (tomography.py:244-246)
            assert (it == maxiter).all() and hit.all()
    for name in ("packed1_unit", "packed1_signed", "packed2_unit", "packed2_signed"):
        assert len(set(golden[name + "/iterations"].tolist())) > 1       # the groups of a wavefront stop at different iterations
    for name, (n, _, linv_only) in mk.OTHER_CASES.items():
        for k in ("linv",) if linv_only else ("linv", "r"):
            assert golden[f"{name}/{k}"].shape == matrix_shape(mk.OTHER_ITEMS, n)
        if not linv_only:
            ll = golden[name + "/ll"]
            assert ll.shape == (mk.OTHER_ITEMS,) and ll.dtype == np.float64 and np.isfinite(ll).all()
    for n in mk.POST_QUBITS:
        out = golden[f"proj{n}/out"]
        assert out.shape == matrix_shape(3, n)
        assert not all_nan(out[0], n) and not all_nan(out[1], n) and all_nan(out[2], n)
        for k in mk.MEASURES:
            v = golden[f"measures{n}/{k}"]
            assert v.shape == (3,) and v.dtype == np.float64 and np.isfinite(v[:2]).all() and np.isnan(v[2])
    for n in mk.PAULI_QUBITS:
        assert golden[f"pauli{n}/out"].shape == ((2, 4 ** n) if n <= mk.RAW_QUBITS else (2, 32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(mk.MLE_CASES))
def test_mle_bits(gpu, golden, name):
    same_bits(mk.run_mle(name), golden, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(mk.OTHER_CASES))
def test_r_operator_likelihood_and_linear_inversion_bits(gpu, golden, name):
    same_bits(mk.run_other(name), golden, name)


@pytest.mark.gpu
@pytest.mark.parametrize("n", mk.POST_QUBITS)
def test_projection_bits(gpu, golden, n):
    same_bits(mk.run_proj(n), golden, f"proj{n}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", mk.POST_QUBITS)
def test_measures_bits(gpu, golden, n):
    same_bits(mk.run_measures(n), golden, f"measures{n}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", mk.PAULI_QUBITS)
def test_pauli_vector_bits(gpu, golden, n):
    same_bits(mk.run_pauli(n), golden, f"pauli{n}")
