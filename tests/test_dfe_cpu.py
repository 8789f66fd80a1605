"""The host mirror of the DFE kernels (fbx/clifford_circuit.py) and the restatements the GPU tests compare against, checked on
the CPU against dense matrices and against the reference's loops written out with itertools.  No GPU needed."""
import numpy as np
import pytest

import dfe_cases as dc
from fbx import clifford, clifford_circuit as cc, direct_fidelity_estimation as dfe, synthetic
from fbx.observable_estimation import PauliTerm


def check_against_dense(gates, n):
    """U P U^+ of every Pauli on n qubits: the mirror's (x, z, sign) against the dense product."""
    labels = dc.all_labels(n)
    x, z = cc.paulis_from_labels(labels)
    xo, zo, so = cc.conjugate_paulis(gates, n, x, z)
    u = dc.dense_circuit(gates, n)
    for lab, out, s in zip(labels, cc.labels_from_paulis(n, xo, zo), so):
        want = u @ dc.dense_pauli(lab) @ u.conj().T
        assert np.abs(want - dc.dense_pauli(out, s)).max() < 1e-12, (gates, lab, out, int(s))


def test_every_gate_against_dense_matrices():
    for name in dc.ONE_QUBIT:
        check_against_dense([(name, (0,))], 1)
        for q in range(3):
            check_against_dense([(name, (q,))], 3)
    for name in dc.TWO_QUBIT:
        for pair in ((0, 1), (1, 0)):
            check_against_dense([(name, pair)], 2)
        for pair in ((0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)):
            check_against_dense([(name, pair)], 3)


@pytest.mark.parametrize("n", [3, 4])
def test_random_circuits_against_dense(n):
    rng = np.random.default_rng(100 + n)
    for _ in range(3):
        check_against_dense(dc.random_circuit(rng, n, 40), n)


@pytest.mark.parametrize("n", [1, 5, 33, 64])
def test_inverse_after_forward_is_the_identity(n):
    rng = np.random.default_rng(7 * n)
    gates = dc.random_circuit(rng, n, 200)
    x, z, s = dc.random_paulis(rng, n, 50)
    back = cc.conjugate_paulis(gates, n, *cc.conjugate_paulis(gates, n, x, z, s), inverse=True)
    for got, want in zip(back, (x, z, s)):
        assert np.array_equal(got, want)


def test_words_round_trip_and_bad_words_are_refused():
    rng = np.random.default_rng(3)
    gates = dc.random_circuit(rng, 64, 100, pairs=[(0, 63), (31, 32)])
    words = cc.encode_gates(gates, 64)
    assert words.dtype == np.uint32 and cc.decode_gates(words) == gates
    assert np.array_equal(cc.encode_gates(words, 64), words)
    for bad in ([("T", (0,))], [("H", (2,))], [("CNOT", (1, 1))], [("CZ", (0,))], [("H", (0, 1))], [("X", (-1,))]):
        with pytest.raises(ValueError):
            cc.encode_gates(bad, 2)
    for word in (15, 0 | (2 << 8), 12 | (1 << 8) | (1 << 16), 1 << 24, 0 | (1 << 16)):
        with pytest.raises(ValueError):
            cc.encode_gates(np.array([word], dtype=np.uint32), 2)
    for n in (0, 65):
        with pytest.raises(ValueError):
            cc.encode_gates([], n)


def test_compiled_clifford_elements_conjugate_like_the_group_code():
    """apply_clifford_to_pauli on the gate word of clifford.to_gates equals clifford.apply_to_pauli, for all 24 one-qubit elements
    and 150 two-qubit ones, on every Pauli."""
    rng = np.random.default_rng(11)
    for n, indices in ((1, range(24)), (2, rng.choice(11520, size=150, replace=False))):
        labels = dc.all_labels(n)
        for elem in clifford.from_index(n, list(indices)):
            gates = clifford.to_gates(int(elem), n)
            for k, lab in enumerate(labels):
                got = cc.apply_clifford_to_pauli(gates, PauliTerm({q: c for q, c in enumerate(lab)}), n)
                idx, sign = clifford.apply_to_pauli(int(elem), k, n)
                assert "".join(got[q] for q in range(n)) == labels[idx] and got.coefficient == sign, (n, int(elem), lab)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("kind", ["state", "process"])
def test_exhaustive_settings_equal_the_reference_loops(kind, n):
    gates = dc.random_circuit(np.random.default_rng(20 + n), n, 25)
    got = dc.settings_as_tuples(n, cc.restate_dfe_settings(n, kind, 0, 0, gates))
    assert got == dc.reference_settings(kind, n, gates)
    assert len(got) == ((4 ** n - 1) * 2 ** n if kind == "process" else 2 ** n - 1)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("kind", ["state", "process"])
def test_monte_carlo_settings_equal_a_setting_by_setting_loop(kind, n):
    """The documented stream, drawn setting by setting on the tests' own scalar Philox, through the reference's loop."""
    gates = dc.random_circuit(np.random.default_rng(30 + n), n, 25)
    seed = 0x9E3779B97F4A7C15 + n
    labels, eigs, rejected = dc.monte_carlo_inputs(kind, n, 60, seed)
    if n == 1:
        assert rejected > 10          # half (state) or a quarter (process) of the attempts are the identity
    got = dc.settings_as_tuples(n, cc.restate_dfe_settings(n, kind, 60, seed, gates))
    assert got == dc.reference_settings(kind, n, gates, labels, eigs)


def test_exhaustive_sizes_are_refused_from_2_31_on():
    assert cc.exhaustive_size(31, "state") == 2 ** 31 - 1 and cc.exhaustive_size(10, "process") == (4 ** 10 - 1) * 2 ** 10
    for n, kind in ((32, "state"), (64, "state"), (11, "process")):
        with pytest.raises(ValueError):
            cc.exhaustive_size(n, kind)


@pytest.mark.parametrize("n", [2, 3, 4])
def test_propagation_mirror_against_dense(n):
    """touches and sigma of the mirror against the dense answers of dfe_cases.propagation_case: process settings give sigma
    +-1, and settings with a wrong in-state label give 0 when the arriving Pauli is not the identity there."""
    gates, classes, s, wrong, sigma, touches = dc.propagation_case(n)
    got_sigma, got_touches = cc.propagate_settings(gates, n, s["in_x"], s["in_z"], s["in_minus"], s["obs_x"], s["obs_z"], classes, 3)
    assert np.array_equal(got_touches, touches)
    assert np.abs(got_sigma - sigma).max() < 1e-12
    assert set(got_sigma[~wrong].tolist()) <= {-1, 1} and (got_sigma[wrong] == 0).sum() > 0


def test_dfe_counts_are_the_tomography_counts_under_another_tag():
    rng = np.random.default_rng(5)
    exact = rng.uniform(-1, 1, size=(2, 7))
    coefs = np.where(rng.random(7) < 0.5, -1.0, 1.0)
    exact *= coefs
    tomo = synthetic.restate_tomography_counts(exact, coefs, 37, 1234, first_item=3)
    same = synthetic.restate_dfe_counts(exact, coefs, 37, 1234, first_item=3, key_tag=synthetic.TOMO_KEY_TAG)
    for a, b in zip(tomo, same):
        assert np.array_equal(a, b)
    plain = synthetic.restate_dfe_counts(exact, coefs, 37, 1234, first_item=3)
    cal = synthetic.restate_dfe_counts(exact, coefs, 37, 1234, first_item=3, key_tag=synthetic.DFE_CALIBRATION_KEY_TAG)
    assert not np.array_equal(plain[3], tomo[3]) and not np.array_equal(plain[3], cal[3])


def test_wrappers_refuse_bad_arguments_before_touching_the_library(monkeypatch):
    from fbx import _lib

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    gates = dc.ghz_circuit(3)
    expt = dfe.DfeExperiment("state", [4, 5, 6], gates, cc.restate_dfe_settings(3, "state", 0, 0, gates))
    assert expt.m == 7 and str(expt.settings()[0]) == "Z+_4 * Z+_5 * Z+_6→(1+0j)*Z5Z6"
    p = np.full((2, 2), 0.01)
    bad_calls = [
        lambda: dfe.generate_exhaustive_state_dfe_experiment(None, [("H", (3,))], [0, 1, 2]),
        lambda: dfe.generate_exhaustive_state_dfe_experiment(None, [("T", (0,))], [0]),
        lambda: dfe.generate_exhaustive_state_dfe_experiment(None, [], list(range(32))),
        lambda: dfe.generate_exhaustive_process_dfe_experiment(None, [], list(range(11))),
        lambda: dfe.generate_exhaustive_state_dfe_experiment(None, [], list(range(65))),
        lambda: dfe.generate_monte_carlo_state_dfe_experiment(None, gates, [0, 1, 2], n_terms=0),
        lambda: dfe.generate_monte_carlo_process_dfe_experiment(None, gates, [0, 1, 2], n_terms=-5),
        lambda: dfe.simulate_dfe_batch(expt, p, 2 ** 32),
        lambda: dfe.simulate_dfe_batch(expt, p, -1),
        lambda: dfe.simulate_dfe_batch(expt, p, 10, first_item=-1),
        lambda: dfe.simulate_dfe_batch(expt, np.zeros((2, 17)), 10),
        lambda: dfe.simulate_dfe_batch(expt, np.zeros((2, 2, 2)), 10),
        lambda: dfe.simulate_dfe_batch(expt, p, 10, noise_class=[0, 1]),
        lambda: dfe.simulate_dfe_batch(expt, p, 10, noise_class=[0, 1, 2]),
        lambda: dfe.simulate_dfe_batch(expt, p, 10, readout_flip=np.zeros((3, 3))),
        lambda: dfe.simulate_and_estimate_dfe_batch(expt, p, 0),
        lambda: dfe.simulate_dfe_results(expt, p, 10),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} was accepted")
