"""T1, T2, Rabi and CZ-phase-Ramsey analysis (forest/benchmarking/qubit_spectroscopy.py) on the device.

``get_stats_by_qubit`` and the four ``fit_*_results`` functions under the reference's names, signatures and default guesses,
each with a ``*_batch`` form over ``[B, K]`` expectations (one row per qubit, pair or resample) that fits the B curves in one
launch of fbx_curve_fit.  Experiment generation and acquisition need pyquil and a QuantumComputer and are not part of this package.
"""
from typing import Dict, List, Sequence

import numpy as np

from . import _lib
from .analysis import fitting
from .utils import transform_pauli_moments_to_bit

MICROSECOND = 1e-6
MHZ = 1e6


def get_stats_by_qubit(expt_results: List[List]) -> Dict[int, Dict[str, List[float]]]:
    """Expectation and standard error of a single-qubit-observable experiment, per qubit, in the order of the outer list
    (qubit_spectroscopy.py:49-78)."""
    stats_by_qubit = {}
    for results in expt_results:
        for res in results:
            qubits = res.setting.observable.get_qubits()
            if len(qubits) > 1:
                raise ValueError("This method is intended for single qubit observables.")
            entry = stats_by_qubit.setdefault(qubits[0], {'expectation': [], 'std_err': []})
            entry['expectation'].append(res.expectation)
            entry['std_err'].append(res.std_err)
    return stats_by_qubit


def _bit_data(expectations, std_errs):
    """Probability of measuring 1 and the fit weights, as every front end of the reference builds them: the Pauli expectation is
    negated and mapped onto a bit; weights are 1 / error with each zero error replaced by the row's smallest non-zero one, and
    None when there are no errors or none is above zero; in a batch, a row without any error above zero gets unit weights."""
    e = np.atleast_2d(np.asarray(expectations, dtype=np.float64))
    if std_errs is None:
        p1, _ = transform_pauli_moments_to_bit(-1 * e, 0)
        return p1, None
    s = np.atleast_2d(np.asarray(std_errs, dtype=np.float64))
    if s.shape != e.shape:
        raise ValueError("expectations and std_errs must have one shape")
    p1, var = transform_pauli_moments_to_bit(-1 * e, s ** 2)
    err = np.sqrt(var)
    pos = err > 0
    has = pos.any(axis=1, keepdims=True)
    if not has.any():
        return p1, None
    smallest = np.where(has, np.where(pos, err, np.inf).min(axis=1, keepdims=True), 1.0)
    weights = np.where(has, 1 / np.where(pos, err, smallest), 1.0)          # a row without any error: unit weights
    return p1, weights


def _fit(model, xs, expectations, std_errs, param_guesses, single, fit_kw):
    p1, weights = _bit_data(expectations, std_errs)
    batch = fitting.curve_fit_batch(model, np.asarray(xs, dtype=np.float64), p1, weights, param_guesses, **fit_kw)
    return batch[0] if single else batch


def fit_t1_results(times: Sequence[float], z_expectations: Sequence[float], z_std_errs: Sequence[float] = None,
                   param_guesses: tuple = (1.0, 15, 0.0), **fit_kw):
    """T1 of one qubit (qubit_spectroscopy.py:115-154): ``decay_time_param_decay`` fitted to the probability of 1;
    ``fit.params['decay_time']`` is T1 in the units of ``times`` (the default guess of 15 assumes microseconds)."""
    return _fit(_lib.FIT_TIME_DECAY, times, z_expectations, z_std_errs, param_guesses, True, fit_kw)


def fit_t1_results_batch(times, z_expectations, z_std_errs=None, param_guesses=(1.0, 15, 0.0), **fit_kw):
    return _fit(_lib.FIT_TIME_DECAY, times, z_expectations, z_std_errs, param_guesses, False, fit_kw)


def fit_t2_results(times: Sequence[float], y_expectations: Sequence[float], y_std_errs: Sequence[float] = None,
                   detuning: float = 1e6, param_guesses: tuple = None, **fit_kw):
    """T2 of one qubit (qubit_spectroscopy.py:279-322): ``decaying_cosine`` from the guess (0.5, 10, 0, 0.5, detuning / MHZ) --
    times in microseconds, detuning in Hz, frequency reported in MHz.  ``fit.params['decay_time']`` is T2."""
    if param_guesses is None:
        param_guesses = (.5, 10, 0.0, 0.5, detuning / MHZ)
    return _fit(_lib.FIT_DECAYING_COSINE, times, y_expectations, y_std_errs, param_guesses, True, fit_kw)


def fit_t2_results_batch(times, y_expectations, y_std_errs=None, detuning: float = 1e6, param_guesses=None, **fit_kw):
    if param_guesses is None:
        param_guesses = (.5, 10, 0.0, 0.5, detuning / MHZ)
    return _fit(_lib.FIT_DECAYING_COSINE, times, y_expectations, y_std_errs, param_guesses, False, fit_kw)


def fit_rabi_results(angles: Sequence[float], z_expectations: Sequence[float], z_std_errs: Sequence[float] = None,
                     param_guesses: tuple = (-.5, 0, .5, 1.), **fit_kw):
    """Rabi oscillation of one qubit (qubit_spectroscopy.py:359-418): ``shifted_cosine`` in (amplitude, offset, baseline,
    frequency); 'frequency' is the ratio of the rotated angle to the control angle."""
    return _fit(_lib.FIT_SHIFTED_COSINE, angles, z_expectations, z_std_errs, param_guesses, True, fit_kw)


def fit_rabi_results_batch(angles, z_expectations, z_std_errs=None, param_guesses=(-.5, 0, .5, 1.), **fit_kw):
    return _fit(_lib.FIT_SHIFTED_COSINE, angles, z_expectations, z_std_errs, param_guesses, False, fit_kw)


def fit_cz_phase_ramsey_results(angles: Sequence[float], y_expectations: Sequence[float], y_std_errs: Sequence[float] = None,
                                param_guesses: tuple = (.5, 0, .5, 1.), **fit_kw):
    """CZ phase Ramsey of one qubit (qubit_spectroscopy.py:450-512): ``shifted_cosine``; 'offset' estimates the phase the CZ
    imparts on the measured qubit."""
    return _fit(_lib.FIT_SHIFTED_COSINE, angles, y_expectations, y_std_errs, param_guesses, True, fit_kw)


def fit_cz_phase_ramsey_results_batch(angles, y_expectations, y_std_errs=None, param_guesses=(.5, 0, .5, 1.), **fit_kw):
    return _fit(_lib.FIT_SHIFTED_COSINE, angles, y_expectations, y_std_errs, param_guesses, False, fit_kw)
