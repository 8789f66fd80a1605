"""The conversion cases (tests/convert_cases.py) without a GPU: the reference that tests/test_convert_exact_gpu.py holds the
kernels to with np.array_equal is itself exact -- the oracle's output on gaussian integers is integral after the route's
power-of-two scale with deviation exactly 0.0 (1-4 qubits, every route), and for one and two qubits equal to an evaluation in
int64 written from the definitions -- and the closed form of the spectra family is the oracle's choi2chi."""
import numpy as np
import pytest

import convert_cases as cc
from fbx_oracle import superops as so

ALL_ROUTES = cc.LINEAR_ROUTES + cc.KRAUS_ROUTES


def test_the_route_tables_are_complete():
    assert len(cc.LINEAR_ROUTES) == 9 and len(set(cc.LINEAR_ROUTES)) == 9
    assert all(s != d and d != "chi" and s in cc.MATRIX_REPS and d in cc.MATRIX_REPS for s, d in cc.LINEAR_ROUTES)
    assert set(cc.SCALE_POWER) == set(ALL_ROUTES)
    assert set(cc.FIVE_QUBIT_ROUTES) <= set(cc.LINEAR_ROUTES)


def test_inputs_are_gaussian_integers_without_structure():
    for D in (4, 16, 64):
        x = cc.int_matrices(D, 3)
        assert np.array_equal(x, np.rint(x.real) + 1j * np.rint(x.imag))
        assert np.abs(x.real).max() == 9 and np.abs(x.imag).max() == 9
        assert not np.array_equal(x, x.conj().transpose(0, 2, 1)) and np.abs(x.imag).max() > 0
        assert not np.array_equal(x[0], x[1])
        assert np.array_equal(x, cc.int_matrices(D, 3))                     # seeded
    k = cc.int_kraus(4, 3, 2)
    assert k.shape == (2, 3, 4, 4) and np.abs(k.real).max() == 3 and np.abs(k.imag).max() == 3


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_the_oracle_is_exact_on_gaussian_integers(n):
    d = 2 ** n
    B = 2 if n < 4 else 1
    for src, dst in ALL_ROUTES:
        for K in ((1, 3) if src == "kraus" else (0,)):
            x, want = cc.exact_case(src, dst, n, B, K)
            assert cc.is_integral(want, d ** cc.SCALE_POWER[(src, dst)]) == 0.0, (src, dst, K)
            assert np.abs(want).max() > 0
            if n <= 2:
                for b in range(B):
                    re, im = cc.int64_route(src, dst, x[b])
                    got = want[b] * d ** cc.SCALE_POWER[(src, dst)]
                    assert np.array_equal(got.real, re) and np.array_equal(got.imag, im), (src, dst, K, b)


def test_the_int64_evaluation_notices_a_wrong_entry():
    x, want = cc.exact_case("choi", "pauli_liouville", 2, 2)
    y = np.array(x[0])
    y[3, 5] += 1
    re, im = cc.int64_route("choi", "pauli_liouville", y)
    assert not (np.array_equal(want[0].real * 4, re) and np.array_equal(want[0].imag * 4, im))


@pytest.mark.parametrize("n", [1, 2, 3])
def test_apply_choi_from_the_definition_is_the_oracle(n):
    d = 2 ** n
    choi, rho = cc.int_matrices(d * d, 3, tag=7), cc.int_states(d, 3, tag=7)
    want = cc.apply_choi_exact(choi, rho)
    assert cc.is_integral(want, 1) == 0.0
    for b in range(3):
        assert np.array_equal(so.apply_choi_matrix_2_state(choi[b], rho[b]), want[b])


@pytest.mark.parametrize("n", [1, 2, 3])
def test_pauli_diagonal_spectra_have_the_closed_form_chi(n):
    """float64 rounding of the oracle's eigh and products on entries of at most 0.4: D eps 0.4 = 6e-15 at three qubits"""
    d, D = 2 ** n, 4 ** n
    lam = cc.spectrum(n)
    assert len(lam) == D and (lam < 0).any() and (np.abs(lam) > cc.CUT).sum() < D
    if n >= 2:
        assert {2e-9, -2e-9, 5e-10, -5e-10, 0.0} <= set(lam)
    choi, chi = cc.spectra_cases(n)["diag"]
    for c, x in zip(choi, chi):
        assert np.abs(c - c.conj().T).max() < 1e-17
        assert np.abs(np.linalg.eigvalsh(c) - np.sort(lam)).max() < 1e-14
        assert np.abs(so.choi2chi(c) - x).max() < 1e-14
        assert np.count_nonzero(x) == (np.abs(lam) > cc.CUT).sum()
        # the cut is visible at the GPU test's 1e-11: the dropped +-5e-10 would contribute 5e-10 / d
        assert 5e-10 / d > 5e-11
    cb, xb = cc.spectra_cases(n)["basis"]
    for c, x in zip(cb, xb):
        assert np.abs(np.linalg.eigvalsh(c) - np.sort(lam)).max() < 1e-14
        assert np.abs(x - x.conj().T).max() < 1e-14 and abs(np.trace(x).real - np.abs(lam)[np.abs(lam) > cc.CUT].sum() / d) < 1e-14


def test_the_sources_of_a_spectrum_are_the_oracles_maps():
    choi, chi = cc.spectra_cases(2)["diag"]
    assert np.abs(cc.oracle_batch("superop", "chi", cc.as_source("superop", choi)) - chi).max() < 1e-14
    assert np.abs(cc.oracle_batch("pauli_liouville", "chi", cc.as_source("pauli_liouville", choi)) - chi).max() < 1e-14


def test_diagonal_integer_choi_matrices():
    choi, chi = cc.diagonal_int_choi(2, 5)
    assert cc.is_integral(chi, 16) == 0.0
    assert not np.array_equal(choi[0], choi[1]) and (choi.real < 0).any()
    for b in range(5):
        assert np.abs(so.choi2chi(choi[b]) - chi[b]).max() < 1e-14
