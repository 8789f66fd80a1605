"""The host formulas of fbx.randomized_benchmarking and fbx.utils against results recorded from the reference
(golden/rb_cases.npz, tests/golden/make_rb_goldens.py)."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rb_cases.npz")
TOL = 1e-15


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert (np.abs(got - want) <= TOL * np.maximum(1.0, np.abs(want))).all(), np.abs(got - want).max()


def test_conversion_and_bound_formulas(gold):
    from fbx import randomized_benchmarking as rb
    d, rbd, irb, uni, err = (gold[k] for k in ("f_dim", "f_rb", "f_irb", "f_unitarity", "f_error"))
    _close(rb.unitarity_to_rb_decay(uni, d), gold["f_unitarity_to_rb_decay"])
    _close(rb.coherence_angle(rbd, uni), gold["f_coherence_angle"])
    _close(rb.gamma(irb, uni), gold["f_gamma"])
    _close(np.stack(rb.interleaved_gate_fidelity_bounds(irb, rbd, d), axis=1), gold["f_bounds"])
    _close(np.stack(rb.interleaved_gate_fidelity_bounds(irb, rbd, d, uni), axis=1), gold["f_bounds_unitarity"])
    _close(rb.gate_error_to_irb_decay(err, rbd, d), gold["f_gate_error_to_irb_decay"])
    _close(rb.irb_decay_to_gate_error(irb, rbd, d), gold["f_irb_decay_to_gate_error"])
    _close(rb.average_gate_error_to_rb_decay(err, d), gold["f_average_gate_error_to_rb_decay"])
    _close(rb.rb_decay_to_gate_error(rbd, d), gold["f_rb_decay_to_gate_error"])
    # scalars as in the reference
    i = 3
    lo, hi = rb.interleaved_gate_fidelity_bounds(float(irb[i]), float(rbd[i]), int(d[i]))
    _close([lo, hi], gold["f_bounds"][i])
    assert rb.rb_decay_to_gate_error(rb.average_gate_error_to_rb_decay(0.01, 4), 4) == pytest.approx(0.01, abs=1e-15)
    assert rb.irb_decay_to_gate_error(rb.gate_error_to_irb_decay(0.02, 0.97, 2), 0.97, 2) == pytest.approx(0.02, abs=1e-15)


@pytest.mark.parametrize("dim", [4, 8, 16, 32])
def test_covariance_sum(gold, dim):
    from fbx import randomized_benchmarking as rb
    e, shots = gold[f"surv{dim}_e"], int(gold["shots"])
    _close([rb.covariances_of_all_iz_obs(row, shots) for row in e], gold[f"surv{dim}_cov"])


@pytest.mark.parametrize("dim", [2, 4, 8])
def test_purity_and_error_host_forms(gold, dim):
    from fbx import randomized_benchmarking as rb
    e, se = gold[f"pur{dim}_e"], gold[f"pur{dim}_se"]
    ex = np.concatenate([e, np.ones((len(e), 1))], axis=1)
    va = np.concatenate([se, np.zeros((len(e), 1))], axis=1) ** 2
    for renorm, kp, ke in ((True, "p", "err"), (False, "p_raw", "err_raw")):
        _close(rb.estimate_purity(dim, ex, renorm=renorm), gold[f"pur{dim}_{kp}"])
        _close(rb.estimate_purity_err(dim, ex, va, renorm=renorm), gold[f"pur{dim}_{ke}"])
        _close([rb.estimate_purity(dim, r, renorm=renorm) for r in ex], gold[f"pur{dim}_{kp}"])
        _close([rb.estimate_purity_err(dim, r, v, renorm=renorm) for r, v in zip(ex, va)], gold[f"pur{dim}_{ke}"])


def test_number_of_shots_is_validated():
    from fbx import randomized_benchmarking as rb
    for shots in (0, -5):
        with pytest.raises(ValueError, match="must be positive"):
            rb.z_obs_stats_to_survival_statistics([0.9, 0.8, 0.7], [0.01] * 3, shots)
        with pytest.raises(ValueError, match="must be positive"):
            rb.fit_rb_results([2, 4], [[0.9, 0.8, 0.7]] * 2, [[0.01] * 3] * 2, shots)


def test_moment_transforms(gold):
    from fbx import utils
    m, v = gold["moments_in"]
    _close(np.stack(utils.transform_pauli_moments_to_bit(m, v)), gold["moments_to_bit"])
    _close(np.stack(utils.transform_bit_moments_to_pauli(m, v)), gold["moments_to_pauli"])
    mean, var = utils.transform_pauli_moments_to_bit(0.5, 0)
    assert mean == 0.75 and var == 0


def test_stats_helpers_group_results():
    from fbx import randomized_benchmarking as rb, qubit_spectroscopy as qs
    from fbx.observable_estimation import ExperimentResult, ExperimentSetting, PauliTerm, zeros_state

    def res(term, e):
        return ExperimentResult(setting=ExperimentSetting(zeros_state(term.get_qubits()), term), expectation=e, std_err=0.1 * e,
                                total_counts=100)
    z0, z1 = PauliTerm({0: "Z"}), PauliTerm({1: "Z"})
    rounds = [[res(z0, 0.9), res(z1, 0.8)], [res(z0, 0.7), res(z1, 0.6)]]
    by_qubit = qs.get_stats_by_qubit(rounds)
    assert by_qubit[0]["expectation"] == [0.9, 0.7] and by_qubit[1]["std_err"] == pytest.approx([0.08, 0.06])
    by_group = rb.get_stats_by_qubit_group([(0,), (1,)], rounds)
    assert by_group[(0,)]["expectation"] == [[0.9], [0.7]] and by_group[(1,)]["expectation"] == [[0.8], [0.6]]
