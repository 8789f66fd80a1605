"""T1, T2, Rabi and CZ-phase-Ramsey experiments (forest/benchmarking/qubit_spectroscopy.py) on the device: analysis and acquisition.

Analysis: ``get_stats_by_qubit`` and the four ``fit_*_results`` functions under the reference's names, signatures and default
guesses, each with a ``*_batch`` form over ``[B, K]`` expectations (one row per qubit, pair or resample) that fits the B curves in
one launch of fbx_curve_fit.

Acquisition: ``simulate_*_batch`` stand in for ``do_t1_or_t2`` / ``acquire_rabi_data`` / ``acquire_cz_phase_ramsey_data`` -- B
qubits with their own relaxation times, thermal populations, contrasts and readout errors, K points each, ``shots`` shots per
point, in one launch of fbx_spec_acquire (include/fbx.h; ``synthetic.spectroscopy_probabilities`` and
``synthetic.restate_spectroscopy_counts`` mirror it on the host); ``simulate_and_fit_*_batch`` go on to the fit without leaving
the device, and ``simulate_spectroscopy_results`` gives one chip as the reference's ``List[List[ExperimentResult]]``.  The
programs themselves (``generate_*_experiments``) need pyquil and are not part of this package.
"""
from typing import Dict, List, Optional, Sequence

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


# ---------------------------------------------------------------- acquisition on the device: physical curves to shots (fbx_spec_acquire)
def _t2_curve(t2, detuning, frequency_offset, gauss_time, contrast):
    frequency = (np.asarray(detuning, dtype=np.float64) + np.asarray(frequency_offset, dtype=np.float64)) / MHZ
    return np.asarray(contrast, dtype=np.float64) / 2, t2, gauss_time, 2 * np.pi * frequency, 0.0, 0.5


# kind -> (fit model, the physical arguments with their defaults, physical arguments -> the curve (amplitude, decay_time,
# gauss_time, omega, offset, baseline) of fbx_spec_acquire, the prepared state and the measured Pauli of the reference's generator)
_KINDS = {
    "t1": (_lib.FIT_TIME_DECAY, dict(t1=None, thermal_population=0.0),
           lambda t1, thermal_population: (1 - np.asarray(thermal_population, dtype=np.float64), t1, np.inf, 0.0, 0.0,
                                           thermal_population),
           "minusZ", "Z"),
    "t2_star": (_lib.FIT_DECAYING_COSINE, dict(t2=None, detuning=1e6, frequency_offset=0.0, gauss_time=np.inf, contrast=1.0),
                _t2_curve, "minusY", "Y"),
    "t2_echo": (_lib.FIT_DECAYING_COSINE, dict(t2_echo=None, detuning=1e6, gauss_time=np.inf, contrast=1.0),
                lambda t2_echo, detuning, gauss_time, contrast: _t2_curve(t2_echo, detuning, 0.0, gauss_time, contrast),
                "minusY", "Y"),
    "rabi": (_lib.FIT_SHIFTED_COSINE, dict(scale=1.0, offset=0.0, contrast=1.0),
             lambda scale, offset, contrast: (-np.asarray(contrast, dtype=np.float64) / 2, np.inf, np.inf, scale, offset, 0.5),
             "plusZ", "Z"),
    "cz_phase_ramsey": (_lib.FIT_SHIFTED_COSINE, dict(cz_phase=None, scale=1.0, contrast=1.0),
                        lambda cz_phase, scale, contrast: (np.asarray(contrast, dtype=np.float64) / 2, np.inf, np.inf, scale,
                                                           cz_phase, 0.5),
                        "minusY", "Y"),
}


def _curve(kind, physical):
    """The six curve columns of ``kind`` from its physical arguments by name (defaults filled in, unknown names refused)."""
    if kind not in _KINDS:
        raise ValueError(f"kind must be one of {sorted(_KINDS)}")
    args = dict(_KINDS[kind][1])
    unknown = sorted(set(physical) - set(args))
    if unknown:
        raise ValueError(f"{kind} takes {sorted(args)}, not {unknown}")
    args.update(physical)
    missing = sorted(k for k, v in args.items() if v is None)
    if missing:
        raise ValueError(f"{kind} needs {missing}")
    return _KINDS[kind][2](**args)


def _flip_array(flips):
    f = np.asarray(flips, dtype=np.float64)
    if f.ndim not in (1, 2) or f.shape[-1] != 2:
        raise ValueError("flips must be [2] or [B, 2]: P(read 1 | 0), P(read 0 | 1)")
    return f


class _Acquisition:
    """Validated arguments of one fbx_spec_acquire call: ``x`` [K] (shared) or [B, K], the six curve columns (each a scalar or
    [B]), ``flips`` None, [2] or [B, 2]."""

    def __init__(self, x, curve, flips, shots, seed, first_item):
        x = np.asarray(x, dtype=np.float64)
        if x.ndim not in (1, 2):
            raise ValueError("the points must be [K] (one set for the batch) or [B, K]")
        cols = [np.asarray(c, dtype=np.float64) for c in curve]
        if any(c.ndim > 1 for c in cols):
            raise ValueError("every per-qubit argument is a scalar or [B]")
        f = None if flips is None else _flip_array(flips)
        rows = [c.shape for c in cols] + ([x.shape[:1]] if x.ndim == 2 else []) + ([f.shape[:1]] if f is not None and f.ndim == 2 else [])
        try:
            B = self.B = np.broadcast_shapes((1,), *rows)[0]
        except ValueError:
            raise ValueError(f"the per-qubit arguments, the rows of the points and of flips must agree on B (got {rows})") from None
        self.K = x.shape[-1]
        if not 1 <= self.K <= _lib.SPEC_MAX_POINTS:
            raise ValueError(f"an experiment has 1..{_lib.SPEC_MAX_POINTS} points (got {self.K})")
        self.x = np.ascontiguousarray(x if x.ndim == 1 else np.broadcast_to(x, (B, self.K)))
        self.params = np.ascontiguousarray(np.stack([np.broadcast_to(c, (B,)) for c in cols], axis=1))
        self.flips = None if f is None else np.ascontiguousarray(np.broadcast_to(f, (B, 2)))
        self.shots = 0 if shots is None else int(shots)
        if not 0 <= self.shots < 2 ** 32:
            raise ValueError("shots must be in 0 .. 2^32 - 1 (None or 0: exact expectations)")
        self.first_item = int(first_item)
        if self.first_item < 0:
            raise ValueError("first_item must not be negative")
        self.seed = (int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0]) if seed is None
                     else int(seed) & 0xFFFFFFFFFFFFFFFF)

    def launch(self, dev, *outputs):
        """Enqueue the acquisition on buffers owned by ``dev``; ``outputs`` names the [B, K] outputs wanted ('prob', 'exact',
        'expect', 'std_err', 'counts', 'bit', 'bit_err').  Returns the device buffers by name, 'status' among them."""
        names = ("prob", "exact", "expect", "std_err", "counts", "bit", "bit_err")
        d = {name: dev.alloc(8 * self.B * self.K) if name in outputs else None for name in names}
        d["status"] = dev.alloc(4 * self.B)
        d_x, d_p, d_f = dev.upload(self.x), dev.upload(self.params), dev.upload(self.flips)
        _lib.check(_lib.lib().fbx_spec_acquire_dev(
            self.B, self.K, d_x.ptr, self.K if self.x.ndim == 2 else 0, d_p.ptr, _lib.devptr(d_f), self.shots, self.seed,
            self.first_item, *[_lib.devptr(d[name]) for name in names], d["status"].ptr))
        return d

    def status(self, d_status, return_status):
        status = d_status.to_array(np.int32, (self.B,))
        if not return_status and status.any():
            raise ValueError(f"qubit {int(np.flatnonzero(status)[0])} is poisoned: a non-finite curve parameter or point, a decay "
                             "or Gaussian time that is not above zero, or a flip probability outside [0, 1]")
        return status


def _simulate(kind, x, physical, shots, flips, seed, first_item, return_probabilities, return_exact, return_status):
    a = _Acquisition(x, _curve(kind, physical), flips, shots, seed, first_item)
    if a.B == 0:
        raise ValueError("an empty batch")
    wanted = ["expect", "std_err"] + ["prob"] * bool(return_probabilities) + ["exact"] * bool(return_exact)
    with _lib.DeviceScope() as dev:
        d = a.launch(dev, *wanted)
        out = tuple(d[name].to_array(np.float64, (a.B, a.K)) for name in wanted)
        status = a.status(d["status"], return_status)
    return out + ((status,) if return_status else ())


def simulate_t1_batch(times, t1, thermal_population=0.0, shots: Optional[int] = None, flips=None, seed: Optional[int] = None,
                      first_item: int = 0, return_probabilities: bool = False, return_exact: bool = False,
                      return_status: bool = False):
    """T1 experiments of B qubits in one device call (fbx_spec_acquire): prepared in |1>, left alone for ``times`` ([K] shared
    or [B, K]), measured in Z; the probability of reading 1 is ``p_eq + (1 - p_eq) exp(-t / T1)`` with ``t1`` in the units of
    ``times`` and ``thermal_population`` = p_eq the excited population at equilibrium.  Every per-qubit argument is a scalar or
    [B].  ``flips`` [2] or [B, 2] are the readout errors (P(read 1 | 0), P(read 0 | 1)), ``shots`` the shots per point (None or
    0: the exact expectations, standard errors 0).  Qubit b is the global item ``first_item + b``: its shots depend on (seed,
    first_item + b, point) only.  Returns ``(z_expectations, z_std_errs)``, both [B, K], as ``fit_t1_results_batch`` takes them
    (the expectation of Z, -1 for a qubit read as 1); ``return_probabilities`` / ``return_exact`` append the probabilities of
    reading 1 (flips included) and the exact expectations; ``return_status`` appends the status [B] instead of raising for a
    poisoned qubit (a NaN or non-positive time, a non-finite parameter or point, a flip outside [0, 1]: NaN outputs)."""
    return _simulate("t1", times, dict(t1=t1, thermal_population=thermal_population), shots, flips, seed, first_item,
                     return_probabilities, return_exact, return_status)


def simulate_t2_star_batch(times, t2, detuning=1e6, frequency_offset=0.0, gauss_time=np.inf, contrast=1.0,
                           shots: Optional[int] = None, flips=None, seed: Optional[int] = None, first_item: int = 0,
                           return_probabilities: bool = False, return_exact: bool = False, return_status: bool = False):
    """T2* (Ramsey) experiments of B qubits: prepared in -Y, a delay with the frame detuned, measured in Y.  The probability of
    reading 1 is ``1/2 + (contrast / 2) env(t) cos(2 pi (detuning + frequency_offset) / MHZ t)`` with ``env = exp(-t / t2 -
    (t / gauss_time)^2)``: ``times`` in the units the fit is given (microseconds), ``detuning`` (the one the experiment applies)
    and ``frequency_offset`` (the qubit's own, unknown to the experimenter) in Hz, as ``fit_t2_results`` assumes; a finite
    ``gauss_time`` adds the Gaussian envelope of quasi-static dephasing, which the fit model does not have.  Returns
    ``(y_expectations, y_std_errs)`` for ``fit_t2_results_batch``; the other arguments are those of ``simulate_t1_batch``."""
    return _simulate("t2_star", times, dict(t2=t2, detuning=detuning, frequency_offset=frequency_offset, gauss_time=gauss_time,
                                            contrast=contrast), shots, flips, seed, first_item, return_probabilities, return_exact,
                     return_status)


def simulate_t2_echo_batch(times, t2_echo, detuning=1e6, gauss_time=np.inf, contrast=1.0, shots: Optional[int] = None, flips=None,
                           seed: Optional[int] = None, first_item: int = 0, return_probabilities: bool = False,
                           return_exact: bool = False, return_status: bool = False):
    """T2-echo experiments of B qubits: ``simulate_t2_star_batch`` without ``frequency_offset`` -- the echo pulse is IDEAL, so a
    static frequency offset is refocused completely and only the applied ``detuning`` is left in the fringe."""
    return _simulate("t2_echo", times, dict(t2_echo=t2_echo, detuning=detuning, gauss_time=gauss_time, contrast=contrast), shots,
                     flips, seed, first_item, return_probabilities, return_exact, return_status)


def simulate_rabi_batch(angles, scale=1.0, offset=0.0, contrast=1.0, shots: Optional[int] = None, flips=None,
                        seed: Optional[int] = None, first_item: int = 0, return_probabilities: bool = False,
                        return_exact: bool = False, return_status: bool = False):
    """Rabi experiments of B qubits: prepared in |0>, rotated about X by the control angle, measured in Z; the probability of
    reading 1 is ``1/2 - (contrast / 2) cos(scale theta + offset)``, ``scale`` the ratio of the rotated to the control angle.
    Returns ``(z_expectations, z_std_errs)`` for ``fit_rabi_results_batch``; the other arguments are those of
    ``simulate_t1_batch``."""
    return _simulate("rabi", angles, dict(scale=scale, offset=offset, contrast=contrast), shots, flips, seed, first_item,
                     return_probabilities, return_exact, return_status)


def simulate_cz_phase_ramsey_batch(angles, cz_phase, scale=1.0, contrast=1.0, shots: Optional[int] = None, flips=None,
                                   seed: Optional[int] = None, first_item: int = 0, return_probabilities: bool = False,
                                   return_exact: bool = False, return_status: bool = False):
    """CZ-phase Ramsey experiments of B measured qubits: the probability of reading 1 is ``1/2 + (contrast / 2) cos(scale theta
    + cz_phase)``.  Returns ``(y_expectations, y_std_errs)`` for ``fit_cz_phase_ramsey_results_batch``; the other arguments are
    those of ``simulate_t1_batch``."""
    return _simulate("cz_phase_ramsey", angles, dict(cz_phase=cz_phase, scale=scale, contrast=contrast), shots, flips, seed,
                     first_item, return_probabilities, return_exact, return_status)


def predicted_fit_parameters(kind: str, flips=None, **physical) -> np.ndarray:
    """The parameters ``[B, P]``, in the fit model's order, of the curve ``simulate_<kind>_batch`` measures, readout errors folded
    in: p_read = f0 + (1 - f0 - f1) p_true scales every amplitude by s = 1 - f0 - f1 and maps the baseline b to f0 + s b.
    ``kind``: 't1' (amplitude s (1 - p_eq), decay_time, offset 0 -- the model has no baseline, so the prediction is exact only
    where f0 + s p_eq = 0), 't2_star' / 't2_echo' (amplitude, decay_time, offset 0, baseline, frequency in MHz; exact for an
    infinite ``gauss_time``), 'rabi' and 'cz_phase_ramsey' (amplitude, offset, baseline, frequency).  ``physical``: the
    arguments of the simulator by name."""
    amplitude, decay_time, _, omega, offset, baseline = _curve(kind, physical)
    f = np.zeros(2) if flips is None else _flip_array(flips)
    s = 1 - f[..., 0] - f[..., 1]
    amplitude, baseline = s * amplitude, f[..., 0] + s * baseline
    model = _KINDS[kind][0]
    if model == _lib.FIT_TIME_DECAY:
        cols = (amplitude, decay_time, 0.0)
    elif model == _lib.FIT_DECAYING_COSINE:
        cols = (amplitude, decay_time, offset, baseline, np.asarray(omega) / (2 * np.pi))
    else:
        cols = (amplitude, offset, baseline, omega)
    return np.stack(np.broadcast_arrays(*[np.atleast_1d(np.asarray(c, dtype=np.float64)) for c in cols]), axis=1)


def _simulate_and_fit(kind, x, physical, shots, flips, seed, first_item, param_guesses, fit_kw):
    a = _Acquisition(x, _curve(kind, physical), flips, shots, seed, first_item)
    if a.x.ndim != 1:
        raise ValueError("the resident fit takes one set of points [K] for the batch")
    if not 2 <= a.K <= _lib.FIT_MAX_POINTS:
        raise ValueError(f"a fit takes 2..{_lib.FIT_MAX_POINTS} points (got {a.K})")
    model = _KINDS[kind][0]
    guess = fitting._guess_array(model, param_guesses, a.B)
    with _lib.DeviceScope() as dev:
        d = a.launch(dev, "bit", "bit_err")
        a.status(d["status"], False)
        d_w, d_has = dev.alloc(8 * a.B * a.K), dev.alloc(4 * a.B)
        _lib.check(_lib.lib().fbx_fit_prepare_dev(_lib.FIT_PREPARE_RB, a.B, a.K, d["bit"].ptr, d["bit_err"].ptr, 0, d_w.ptr, None,
                                                  d_has.ptr))
        batch = fitting.curve_fit_resident(model, a.x, d["bit"], d_w, dev.upload(guess), a.B, a.K, **fit_kw)
        batch.has_weights = d_has.to_array(np.int32, (a.B,)).astype(bool)
    return batch


def simulate_and_fit_t1_batch(times, t1, thermal_population=0.0, shots: Optional[int] = None, flips=None,
                              seed: Optional[int] = None, first_item: int = 0, param_guesses=(1.0, 15, 0.0),
                              **fit_kw) -> "fitting.FitBatch":
    """``simulate_t1_batch`` followed by ``fit_t1_results_batch`` without leaving the device: fbx_spec_acquire_dev (its bit
    outputs) -> fbx_fit_prepare_dev (the weights) -> fbx_curve_fit_dev, bit for bit what the two public calls return.  ``times``
    is one [K] for the batch, K = 2..256.  Returns the FitBatch of B decays with ``has_weights`` [B] (False where no standard
    error is above zero: unit weights); a poisoned qubit raises ``ValueError``."""
    return _simulate_and_fit("t1", times, dict(t1=t1, thermal_population=thermal_population), shots, flips, seed, first_item,
                             param_guesses, fit_kw)


def simulate_and_fit_t2_batch(times, t2, kind: str = "star", detuning=1e6, frequency_offset=0.0, gauss_time=np.inf, contrast=1.0,
                              shots: Optional[int] = None, flips=None, seed: Optional[int] = None, first_item: int = 0,
                              param_guesses=None, **fit_kw) -> "fitting.FitBatch":
    """``simulate_t2_star_batch`` (``kind="star"``) or ``simulate_t2_echo_batch`` (``kind="echo"``, which takes no
    ``frequency_offset``) followed by ``fit_t2_results_batch(..., detuning)`` on the device, as ``simulate_and_fit_t1_batch``."""
    if kind not in ("star", "echo"):
        raise ValueError("kind must be 'star' or 'echo'")
    if kind == "echo":
        if np.any(np.asarray(frequency_offset) != 0.0):
            raise ValueError("an ideal echo cancels a static frequency offset: kind='echo' takes no frequency_offset")
        physical = dict(t2_echo=t2, detuning=detuning, gauss_time=gauss_time, contrast=contrast)
    else:
        physical = dict(t2=t2, detuning=detuning, frequency_offset=frequency_offset, gauss_time=gauss_time, contrast=contrast)
    if param_guesses is None:
        d = np.atleast_1d(np.asarray(detuning, dtype=np.float64)) / MHZ
        param_guesses = np.stack([np.full_like(d, .5), np.full_like(d, 10.0), np.zeros_like(d), np.full_like(d, .5), d], axis=1)
        if len(d) == 1:
            param_guesses = param_guesses[0]
    return _simulate_and_fit("t2_" + kind, times, physical, shots, flips, seed, first_item, param_guesses, fit_kw)


def simulate_and_fit_rabi_batch(angles, scale=1.0, offset=0.0, contrast=1.0, shots: Optional[int] = None, flips=None,
                                seed: Optional[int] = None, first_item: int = 0, param_guesses=(-.5, 0, .5, 1.),
                                **fit_kw) -> "fitting.FitBatch":
    """``simulate_rabi_batch`` followed by ``fit_rabi_results_batch`` on the device, as ``simulate_and_fit_t1_batch``."""
    return _simulate_and_fit("rabi", angles, dict(scale=scale, offset=offset, contrast=contrast), shots, flips, seed, first_item,
                             param_guesses, fit_kw)


def simulate_and_fit_cz_phase_ramsey_batch(angles, cz_phase, scale=1.0, contrast=1.0, shots: Optional[int] = None, flips=None,
                                           seed: Optional[int] = None, first_item: int = 0, param_guesses=(.5, 0, .5, 1.),
                                           **fit_kw) -> "fitting.FitBatch":
    """``simulate_cz_phase_ramsey_batch`` followed by ``fit_cz_phase_ramsey_results_batch`` on the device, as
    ``simulate_and_fit_t1_batch``."""
    return _simulate_and_fit("cz_phase_ramsey", angles, dict(cz_phase=cz_phase, scale=scale, contrast=contrast), shots, flips, seed,
                             first_item, param_guesses, fit_kw)


def simulate_spectroscopy_results(kind: str, qubits: Sequence[int], xs, shots: Optional[int] = None, flips=None,
                                  seed: Optional[int] = None, first_item: int = 0, **physical) -> List[List]:
    """One chip's experiment as the reference's acquisition returns it: a list over the points ``xs`` [K] of lists with one
    ``ExperimentResult`` per qubit, carrying the setting of the reference's generator -- 't1': minusZ / Z; 't2_star', 't2_echo'
    and 'cz_phase_ramsey': minusY / Y; 'rabi': plusZ / Z -- so that ``get_stats_by_qubit`` and the reference-signature
    ``fit_*_results`` run on it unchanged.  ``physical``: the arguments of ``simulate_<kind>_batch`` by name, each a scalar or one
    value per qubit; qubit ``qubits[b]`` is item b of that call."""
    from . import observable_estimation as oe
    qubits = [int(q) for q in qubits]
    xs = np.asarray(xs, dtype=np.float64)
    if xs.ndim != 1 or not qubits:
        raise ValueError("xs must be [K] (a chip shares its points) and qubits must not be empty")
    # a row of points per qubit: the batch has len(qubits) items even where every physical argument is a scalar
    e, s = _simulate(kind, np.broadcast_to(xs, (len(qubits), len(xs))), physical, shots, flips, seed, first_item, False, False, False)
    prepare, pauli = getattr(oe, _KINDS[kind][3]), _KINDS[kind][4]
    settings = [oe.ExperimentSetting(prepare(q), oe.PauliTerm({q: pauli}, 1.0)) for q in qubits]
    counts = 0 if shots is None else int(shots)
    return [[oe.ExperimentResult(setting=settings[b], expectation=float(e[b, k]), total_counts=counts, std_err=float(s[b, k]))
             for b in range(len(qubits))] for k in range(len(xs))]
