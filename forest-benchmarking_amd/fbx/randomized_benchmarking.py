"""Randomized-benchmarking analysis (forest/benchmarking/randomized_benchmarking.py) on the device.

The analysis half of the reference's module under its own names: survival statistics from I/Z expectations, shifted purities for
unitarity, the decay fits, and the interleaved-RB bounds.  ``fit_rb_results_batch`` / ``fit_unitarity_results_batch`` take
``[B, S, .]`` arrays (B decays of S sequences each) and run statistics -> weights and guess -> fit as one chain of device calls
(fbx_rb_survival_dev / fbx_rb_purity_dev -> fbx_fit_prepare_dev -> fbx_curve_fit_dev); the single-experiment functions are that
chain with B = 1.  The scalar conversion and bound formulas are plain numpy and accept arrays.  Sequence generation and data
acquisition (``generate_*``, ``acquire_*``, ``do_rb``) need pyquil, quilc and a QuantumComputer and are not part of this package.
"""
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .analysis import fitting
from .observable_estimation import get_results_by_qubit_groups


def _seq_sum(a):
    """Sum over the last axis in index order, starting from 0: Python's ``sum`` as the reference applies it, for stacked rows."""
    a = np.asarray(a, dtype=np.float64)
    acc = np.zeros(a.shape[:-1])
    for k in range(a.shape[-1]):
        acc = acc + a[..., k]
    return acc


def _shots_for_covariance(dim, num_shots, obs_are_independent):
    """0 when no covariance term is to be added (dim 2, or independent observables), else the validated number of shots."""
    if dim <= 2 or obs_are_independent:
        return 0
    if num_shots is None:
        raise ValueError("The number of shots is necessary information for computing the sample covariance.")
    if int(num_shots) <= 0:
        raise ValueError("The number of shots must be positive to compute the sample covariance.")
    return int(num_shots)


def _is_pos_pow_two(x) -> bool:
    x = int(x)
    return x > 0 and (x & (x - 1)) == 0


def get_stats_by_qubit_group(qubit_groups: Sequence[Sequence[int]], expt_results: Iterable[Iterable]) \
        -> Dict[Tuple[int, ...], Dict[str, List[List[float]]]]:
    """Expectations and standard errors of a simultaneous RB experiment, one list per sequence, for every qubit group
    (randomized_benchmarking.py:23-49)."""
    qubits = [tuple(group) for group in qubit_groups]
    stats = {group: {'expectation': [], 'std_err': []} for group in qubit_groups}
    for results in expt_results:
        by_group = get_results_by_qubit_groups(results, qubits)
        for group in qubit_groups:
            group_results = by_group[tuple(group)]
            stats[group]['expectation'].append([r.expectation for r in group_results])
            stats[group]['std_err'].append([r.std_err for r in group_results])
    return stats


def _rows(expectations, std_errs, width_of, what):
    e = np.ascontiguousarray(expectations, dtype=np.float64)
    s = np.ascontiguousarray(std_errs, dtype=np.float64)
    if e.shape != s.shape:
        raise ValueError(f"{what}: expectations and std_errs must have one shape")
    return e, s, width_of(e.shape[-1])


def survival_statistics_batch(expectations, std_errs, num_shots: Optional[int] = None, obs_are_independent: bool = False):
    """Survival probability and variance of every row of ``expectations[..., dim - 1]`` (fbx_rb_survival)."""
    e, s, dim = _rows(expectations, std_errs, lambda n: n + 1, "survival statistics")
    assert _is_pos_pow_two(dim)
    shots = _shots_for_covariance(dim, num_shots, obs_are_independent)
    lead = e.shape[:-1]
    S = int(np.prod(lead))
    surv, var = np.empty(S), np.empty(S)
    _lib.check(_lib.lib().fbx_rb_survival(dim, S, _lib.dptr(e), _lib.dptr(s), shots, _lib.dptr(surv), _lib.dptr(var)))
    return surv.reshape(lead), var.reshape(lead)


def covariances_of_all_iz_obs(expectations: Sequence[float], num_shots: int):
    """Summed covariance of every distinct pair of the dim - 1 I/Z observables estimated from one set of shots: the product of two
    of them is a third, so the sum is 2 sum_i e_i - sum_{i != j} e_i e_j, over the shots (randomized_benchmarking.py:308-345)."""
    e = [float(v) for v in expectations]
    assert _is_pos_pow_two(len(e) + 1)
    covariance = 2 * sum(e)                                    # E[O_i O_j] = E[O_k], every k twice
    covariance -= sum(a * b for i, a in enumerate(e) for j, b in enumerate(e) if i != j)
    return covariance / num_shots


def z_obs_stats_to_survival_statistics(expectations: Sequence[float], std_errs: Sequence[float],
                                       num_shots: Optional[int] = None, obs_are_independent: bool = False) -> Tuple[float, float]:
    """Survival (all-zeros) probability and its variance from the dim - 1 I/Z expectations of one sequence
    (randomized_benchmarking.py:348-383)."""
    surv, var = survival_statistics_batch(np.asarray(expectations, dtype=np.float64)[None, :],
                                          np.asarray(std_errs, dtype=np.float64)[None, :], num_shots, obs_are_independent)
    return float(surv[0]), float(var[0])


def _resident_decay_fit(kind, depths, d_values, d_errors, errors_are_variances, B, K, param_guesses, fit_kw):
    DB = _lib.DeviceBuffer
    d_w, d_g, d_has = DB(8 * B * K), DB(8 * B * 3), DB(4 * B)
    try:
        _lib.check(_lib.lib().fbx_fit_prepare_dev(kind, B, K, d_values.ptr, d_errors.ptr, int(errors_are_variances),
                                                  d_w.ptr, d_g.ptr, d_has.ptr))
        if param_guesses is not None:
            g = fitting._guess_array(_lib.FIT_BASE_DECAY, param_guesses, B)
            _lib.check(_lib.lib().fbx_memcpy_h2d(d_g.ptr, g.ctypes.data, g.nbytes))
        batch = fitting.curve_fit_resident(_lib.FIT_BASE_DECAY, depths, d_values, d_w, d_g, B, K, **fit_kw)
        batch.has_weights = d_has.to_array(np.int32, (B,)).astype(bool)
    finally:
        for b in (d_w, d_g, d_has):
            b.free()
    return batch


def fit_rb_results_batch(depths: Sequence[int], z_expectations, z_std_errs, num_shots: Optional[int] = None,
                         param_guesses=None, **fit_kw) -> "fitting.FitBatch":
    """B standard or interleaved RB decays at once: ``z_expectations`` / ``z_std_errs`` [B, S, dim - 1] for the S sequences at
    ``depths`` [S].  Returns the FitBatch of ``base_param_decay``; ``batch.value('decay')`` are the RB decays, ``batch.y`` the
    survival probabilities, ``batch.has_weights`` False where every variance was zero."""
    e, s, dim = _rows(z_expectations, z_std_errs, lambda n: n + 1, "fit_rb_results")
    if e.ndim != 3:
        raise ValueError("z_expectations must be [B, S, dim - 1]")
    B, K = e.shape[:2]
    assert len(depths) == K, 'There should be one expectation per sequence and depths should give the depth of each sequence.'
    assert _is_pos_pow_two(dim)
    shots = _shots_for_covariance(dim, num_shots, False)
    DB = _lib.DeviceBuffer
    d_e, d_s, d_surv, d_var = DB.from_array(e), DB.from_array(s), DB(8 * B * K), DB(8 * B * K)
    try:
        _lib.check(_lib.lib().fbx_rb_survival_dev(dim, B * K, d_e.ptr, d_s.ptr, shots, d_surv.ptr, d_var.ptr))
        return _resident_decay_fit(_lib.FIT_PREPARE_RB, depths, d_surv, d_var, True, B, K, param_guesses, fit_kw)
    finally:
        for b in (d_e, d_s, d_surv, d_var):
            b.free()


def fit_rb_results(depths: Sequence[int], z_expectations: Sequence[Sequence[float]], z_std_errs: Sequence[Sequence[float]],
                   num_shots: Optional[int] = None, param_guesses: Optional[tuple] = None, **fit_kw) -> "fitting.FitResult":
    """Fit one RB or IRB experiment (randomized_benchmarking.py:386-438): expectations -> survival probabilities -> weighted decay
    fit from the guess (survival[0] - survival[-1], 0.95, survival[-1]).  The decay is ``fit.params['decay'].value``."""
    return fit_rb_results_batch(depths, np.asarray(z_expectations, dtype=np.float64)[None], np.asarray(z_std_errs, dtype=np.float64)[None],
                                num_shots, param_guesses, **fit_kw)[0]


def purity_statistics_batch(expectations, std_errs, renorm: bool = True):
    """Shifted purity and its error for every row of ``expectations[..., dim^2 - 1]`` (fbx_rb_purity; the identity term is
    appended on the device)."""
    e, s, dim = _rows(expectations, std_errs, lambda n: int(round(np.sqrt(n + 1))), "purity statistics")
    if dim * dim - 1 != e.shape[-1]:
        raise ValueError("purity needs dim^2 - 1 expectations per sequence")
    lead = e.shape[:-1]
    S = int(np.prod(lead))
    pur, err = np.empty(S), np.empty(S)
    _lib.check(_lib.lib().fbx_rb_purity(dim, S, _lib.dptr(e), _lib.dptr(s), int(bool(renorm)), _lib.dptr(pur), _lib.dptr(err)))
    return pur.reshape(lead), err.reshape(lead)


def estimate_purity(dim: int, op_expect: np.ndarray, renorm: bool = True):
    """Purity from the expectations of all dim^2 Paulis, the identity (expectation 1) included; ``renorm`` shifts it onto [0, 1]
    (randomized_benchmarking.py:490-504).  Host arithmetic, as in the reference; the batched device form is
    ``purity_statistics_batch``."""
    op_expect = np.asarray(op_expect, dtype=np.float64)
    purity = (1 / dim) * _seq_sum(op_expect ** 2)
    if renorm:
        purity = (dim / (dim - 1.0)) * (purity - 1.0 / dim)
    return purity


def estimate_purity_err(dim: int, op_expect: np.ndarray, op_expect_var: np.ndarray, renorm=True):
    """Error of ``estimate_purity`` from independent variances of the expectations (randomized_benchmarking.py:507-533): first
    order in the variance, second order where the first-order term is within 1e-6 of zero."""
    op_expect = np.asarray(op_expect, dtype=np.float64)
    op_expect_var = np.asarray(op_expect_var, dtype=np.float64)
    v = (2 * np.abs(op_expect)) ** 2 * op_expect_var
    v = np.where(np.isclose(0.0, v, atol=1e-6), op_expect_var ** 2, v)
    purity_var = (1 / dim) ** 2 * np.sum(v, axis=-1)
    if renorm:
        purity_var = (dim / (dim - 1.0)) ** 2 * purity_var
    return np.sqrt(purity_var)


def fit_unitarity_results_batch(depths: Sequence[int], expectations, std_errs, param_guesses=None, **fit_kw) -> "fitting.FitBatch":
    """B unitarity decays at once: ``expectations`` / ``std_errs`` [B, S, dim^2 - 1]; the unitarities are
    ``batch.value('decay')``, ``batch.y`` the shifted purities."""
    e, s, dim = _rows(expectations, std_errs, lambda n: int(round(np.sqrt(n + 1))), "fit_unitarity_results")
    if e.ndim != 3 or dim * dim - 1 != e.shape[-1]:
        raise ValueError("expectations must be [B, S, dim^2 - 1]")
    B, K = e.shape[:2]
    assert len(depths) == K, 'There should be one group of 4**(num_qubits) - 1 expectations per sequence and depths should ' \
                             'give the depth of each sequence.'
    DB = _lib.DeviceBuffer
    d_e, d_s, d_pur, d_err = DB.from_array(e), DB.from_array(s), DB(8 * B * K), DB(8 * B * K)
    try:
        _lib.check(_lib.lib().fbx_rb_purity_dev(dim, B * K, d_e.ptr, d_s.ptr, 1, d_pur.ptr, d_err.ptr))
        return _resident_decay_fit(_lib.FIT_PREPARE_UNITARITY, depths, d_pur, d_err, False, B, K, param_guesses, fit_kw)
    finally:
        for b in (d_e, d_s, d_pur, d_err):
            b.free()


def fit_unitarity_results(depths: Sequence[int], expectations: Sequence[Sequence[float]], std_errs: Sequence[Sequence[float]],
                          param_guesses: Optional[tuple] = None, **fit_kw) -> "fitting.FitResult":
    """Fit one unitarity experiment (randomized_benchmarking.py:536-592): shifted purities -> weighted decay fit from the guess
    (purity[0], 0.95, 0).  The unitarity is ``fit.params['decay'].value``; 'amplitude' absorbs a factor 1 / unitarity."""
    return fit_unitarity_results_batch(depths, np.asarray(expectations, dtype=np.float64)[None],
                                       np.asarray(std_errs, dtype=np.float64)[None], param_guesses, **fit_kw)[0]


def unitarity_to_rb_decay(unitarity, dimension):
    """The RB decay a unitarity allows when the noise has no unitary part (randomized_benchmarking.py:595-619)."""
    r = (np.sqrt(unitarity) - 1) * (1 - dimension) / dimension
    return average_gate_error_to_rb_decay(r, dimension)


def coherence_angle(rb_decay, unitarity):
    """arccos(rb_decay / sqrt(unitarity)) (randomized_benchmarking.py:678-686)."""
    return np.arccos(rb_decay / np.sqrt(unitarity))


def gamma(irb_decay, unitarity):
    """irb_decay / sqrt(unitarity) (randomized_benchmarking.py:689-698)."""
    return irb_decay / np.sqrt(unitarity)


def interleaved_gate_fidelity_bounds(irb_decay, rb_decay, dim: int, unitarity=None):
    """[lower, upper] bound on the fidelity of the interleaved gate (randomized_benchmarking.py:701-749); with a unitarity, the
    tighter bounds through the coherence angle.  Arrays give arrays."""
    if unitarity is not None:
        theta = coherence_angle(rb_decay, unitarity)
        g = gamma(irb_decay, unitarity)
        decay_bounds = [sign * (sign * g * np.cos(theta) + np.sin(theta) * np.sqrt(1 - g ** 2)) for sign in (-1, 1)]
        return [1 - rb_decay_to_gate_error(decay, dim) for decay in decay_bounds]
    E1 = (np.abs(rb_decay - irb_decay / rb_decay) + (1 - rb_decay)) * (dim - 1) / dim
    E2 = 2 * (dim ** 2 - 1) * (1 - rb_decay) / (rb_decay * dim ** 2) + 4 * np.sqrt(1 - rb_decay) * np.sqrt(dim ** 2 - 1) / rb_decay
    E = np.minimum(E1, E2)
    error = irb_decay_to_gate_error(irb_decay, rb_decay, dim)
    return [1 - error - E, 1 - error + E]


def gate_error_to_irb_decay(irb_error, rb_decay, dim: int):
    """(1 - irb_error dim / (dim - 1)) rb_decay (randomized_benchmarking.py:752-763)."""
    return (1 - irb_error * (dim / (dim - 1))) * rb_decay


def irb_decay_to_gate_error(irb_decay, rb_decay, dim: int):
    """((dim - 1) / dim) (1 - irb_decay / rb_decay) (randomized_benchmarking.py:766-777)."""
    return ((dim - 1) / dim) * (1 - irb_decay / rb_decay)


def average_gate_error_to_rb_decay(gate_error, dimension: int):
    """(gate_error - 1 + 1 / d) / (1 / d - 1) (randomized_benchmarking.py:780-788)."""
    return (gate_error - 1 + 1 / dimension) / (1 / dimension - 1)


def rb_decay_to_gate_error(rb_decay, dimension: int):
    """1 - rb_decay - (1 - rb_decay) / d (randomized_benchmarking.py:791-800)."""
    return 1 - rb_decay - (1 - rb_decay) / dimension
