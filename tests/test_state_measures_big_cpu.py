"""tomography.state_measure_variance_batch refuses bad arguments before it touches the library (no device needed), and the
exact families of tests/state_measure_cases.py are what they claim to be (numpy / scipy on the host)."""
import types

import numpy as np
import pytest

import state_measure_cases as sc


class Untouchable:
    """stands in for a design: the sizes are there, the device handle must not be asked for"""
    n_qubits, dim, m = 4, 16, 255

    @property
    def handle(self):
        raise AssertionError("the library was touched before the arguments were checked")


@pytest.fixture()
def no_library(monkeypatch):
    from fbx import _lib

    def refuse(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "DeviceBuffer", types.SimpleNamespace(from_array=refuse))


def test_bad_arguments_are_refused_before_the_library(no_library):
    from fbx import tomography as T
    design = Untouchable()
    e, c = np.zeros((2, 255)), np.full((2, 255), 100.0)
    rho = np.eye(16, dtype=complex) / 16
    with pytest.raises(ValueError, match="measure"):
        T.state_measure_variance_batch(design, e, c, rho, measure="bures")
    for measure in ("fidelity", "infidelity", "trace_distance", "hs_ip"):
        with pytest.raises(ValueError, match="target"):
            T.state_measure_variance_batch(design, e, c, None, measure=measure)
    for bad in (np.eye(8) / 8, np.zeros((3, 16, 16)), np.zeros((2, 16, 8)), np.zeros(16), np.zeros((1, 2, 16, 16))):
        with pytest.raises(ValueError, match="target_state"):
            T.state_measure_variance_batch(design, e, c, bad, measure="fidelity")
    for r in (0, -3):
        with pytest.raises(ValueError, match="n_resamples"):
            T.state_measure_variance_batch(design, e, c, rho, n_resamples=r)
        with pytest.raises(ValueError, match="n_resamples"):
            T.state_measure_variance_batch(design, e, c, measure="purity", n_resamples=r)
    with pytest.raises(ValueError, match="estimator"):
        T.state_measure_variance_batch(design, e, c, rho, estimator="pgdb")
    with pytest.raises(ValueError, match="expectations"):
        T.state_measure_variance_batch(design, np.zeros((2, 7)), c, rho)
    with pytest.raises(AssertionError, match="touched"):             # good arguments do reach the library
        T.state_measure_variance_batch(design, e, c, rho)


@pytest.mark.parametrize("nq", [2, 3, 4])
@pytest.mark.parametrize("name", sorted(sc.FAMILIES))
def test_exact_families_on_the_host(name, nq):
    """the closed forms against scipy's sqrtm route, where that route is well conditioned (full rank), and against the plain
    sums everywhere"""
    from scipy.linalg import sqrtm
    rho, sigma, exact = sc.family(name, nq, 4)
    sums = sc.host_sums(rho, sigma)
    for key in ("purity", "hs_ip"):
        if key in exact:
            assert np.abs(sums[key] - exact[key]).max() < 1e-13
    for b in range(4):
        assert abs(np.trace(rho[b]) - 1) < 1e-13 and abs(np.trace(sigma[b]) - 1) < 1e-13
        assert np.abs(rho[b] - rho[b].conj().T).max() < 1e-15 and np.linalg.eigvalsh(rho[b]).min() > -1e-15
        if name in ("commuting", "identical"):
            root = sqrtm(rho[b])
            f = np.real(np.trace(sqrtm(root @ sigma[b] @ root))) ** 2
            assert abs(f - exact["fidelity"][b]) < 1e-9
