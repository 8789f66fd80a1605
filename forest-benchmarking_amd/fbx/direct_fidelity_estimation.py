"""Direct fidelity estimation (forest/benchmarking/direct_fidelity_estimation.py).  ``estimate_dfe`` (:224-307) consumes the
same ``ExperimentResult`` records as the tomography estimators.  The four experiment generators (:15-182) work on a Clifford
circuit given as a gate list (``fbx.clifford_circuit``) of up to 64 qubits: the conjugation the reference asks quilc for runs on
the device, and so does the acquisition for a circuit with per-gate depolarizing noise and symmetric readout flips, whose
expectations are exact in the Heisenberg picture (include/fbx.h).  ``acquire_dfe_data`` / ``do_dfe`` themselves need a
``QuantumComputer`` and are out of scope.
"""
import ctypes as _C
import functools
from typing import List, Optional, Tuple

import numpy as np

from . import _lib
from . import clifford_circuit as _cc
from .observable_estimation import (ExperimentResult, ExperimentSetting, PauliTerm, TensorProductState, _OneQState,
                                    calibrate_expectations_batch)

MAX_SHOTS = 2 ** 32 - 1


def estimate_dfe_batch(expectations, std_errs, n_qubits: int, kind: str):
    """B experiments of m settings each: ``(fidelity[B], standard_error[B])``."""
    k = kind.lower()
    if k not in ("state", "process"):
        raise ValueError('Kind can only be \'state\' or \'process\'.')
    e = np.ascontiguousarray(expectations, dtype=np.float64)
    e = e.reshape(-1, e.shape[-1])
    se = np.ascontiguousarray(std_errs, dtype=np.float64).reshape(e.shape)
    B, m = e.shape
    mean, err = np.empty(B), np.empty(B)
    _lib.check(_lib.lib().fbx_dfe_estimate(int(n_qubits), _lib.KIND_PROCESS if k == "process" else _lib.KIND_STATE,
                                           B, m, _lib.dptr(e), _lib.dptr(se), _lib.dptr(mean), _lib.dptr(err)))
    return mean, err


def estimate_dfe(results: List, kind: str) -> Tuple[float, float]:
    """direct_fidelity_estimation.py:224-307: mean fidelity and its standard error; the qubit count
    is read off the union of the observables' supports, like the reference."""
    qubits = functools.reduce(lambda x, y: set(x) | set(y),
                              [res.setting.observable.get_qubits() for res in results])
    e = np.array([np.real(res.expectation) for res in results], dtype=np.float64)
    se = np.array([res.std_err for res in results], dtype=np.float64)
    mean, err = estimate_dfe_batch(e[None], se[None], len(qubits), kind)
    return float(mean[0]), float(err[0])


# ==================================================================================================
# experiment generators (:15-182) and the simulated acquisition
# ==================================================================================================
_U64, _U32, _U8, _I8 = _C.c_uint64, _C.c_uint32, _C.c_uint8, _C.c_int8


class DfeExperiment:
    """The settings of one DFE experiment as arrays (the formats of include/fbx.h): ``in_x, in_z, in_minus, obs_x, obs_z``
    (``uint64`` [m]) and ``obs_sign`` (``uint8`` [m]) for the circuit ``gates`` (``uint32`` words) on ``n_qubits`` qubits with the
    labels ``qubits``; ``kind`` is "state" or "process".  ``settings()`` gives the reference's ``List[ExperimentSetting]``."""

    def __init__(self, kind, qubits, gates, arrays, n_terms=0, seed=0):
        self.kind, self.qubits, self.n_qubits = kind, [int(q) for q in qubits], len(qubits)
        self.gates = _cc.encode_gates(gates, self.n_qubits)
        self.n_terms, self.seed = int(n_terms), int(seed)
        for name in ("in_x", "in_z", "in_minus", "obs_x", "obs_z"):
            setattr(self, name, np.ascontiguousarray(arrays[name], dtype=np.uint64))
        self.obs_sign = np.ascontiguousarray(arrays["obs_sign"], dtype=np.uint8)
        self._propagated = {}

    @property
    def m(self) -> int:
        return int(self.in_x.size)

    def __len__(self):
        return self.m

    def settings(self) -> List[ExperimentSetting]:
        n, qs = self.n_qubits, self.qubits
        ins = _cc.labels_from_paulis(n, self.in_x, self.in_z)
        obs = _cc.labels_from_paulis(n, self.obs_x, self.obs_z)
        out = []
        for lab, minus, o, sign in zip(ins, self.in_minus.tolist(), obs, self.obs_sign.tolist()):
            state = TensorProductState(_OneQState(c, (minus >> q) & 1, qs[q]) for q, c in enumerate(lab))
            out.append(ExperimentSetting(state, PauliTerm({qs[q]: c for q, c in enumerate(o)}, 1.0 - 2.0 * sign)))
        return out

    def propagate(self, noise_class=None, n_classes=1):
        """``(sigma int8 [m], touches uint32 [m, K])`` of ``fbx_dfe_propagate`` for the gates' noise classes (one ``uint8`` per
        gate, below ``n_classes`` or 255 for a noiseless gate; None = every gate is class 0); kept per argument."""
        K, cls = _noise_classes(self.gates.size, noise_class, n_classes)
        key = (K, None if cls is None else cls.tobytes())
        if key not in self._propagated:
            sigma, touches = np.empty(self.m, dtype=np.int8), np.empty((self.m, K), dtype=np.uint32)
            _lib.check(_lib.lib().fbx_dfe_propagate(
                self.n_qubits, self.gates.size, _lib.ptr(self.gates, _U32), _lib.ptr(cls, _U8), K, self.m,
                _lib.ptr(self.in_x, _U64), _lib.ptr(self.in_z, _U64), _lib.ptr(self.in_minus, _U64), _lib.ptr(self.obs_x, _U64),
                _lib.ptr(self.obs_z, _U64), _lib.ptr(self.obs_sign, _U8), _lib.ptr(sigma, _I8), _lib.ptr(touches, _U32)))
            self._propagated[key] = (sigma, touches)
        return self._propagated[key]


def _noise_classes(n_gates, noise_class, n_classes):
    K = int(n_classes)
    if not 1 <= K <= _lib.DFE_MAX_CLASSES:
        raise ValueError(f"the number of noise classes must be 1..{_lib.DFE_MAX_CLASSES}")
    if noise_class is None:
        return K, None
    cls = np.asarray(noise_class)
    if cls.shape != (n_gates,) or np.any(cls < 0) or np.any((cls >= K) & (cls != _lib.DFE_NOISELESS)):
        raise ValueError(f"noise_class needs one entry per gate ({n_gates}), each below {K} or {_lib.DFE_NOISELESS}")
    return K, np.ascontiguousarray(cls, dtype=np.uint8)


def _generate(kind, program, qubits, n_terms, seed) -> DfeExperiment:
    qubits = list(qubits)
    n = _cc.check_width(len(qubits))
    gates = _cc.encode_gates(program, n)
    n_terms = int(n_terms)
    if n_terms < 0:
        raise ValueError("n_terms must not be negative")
    m = n_terms if n_terms else _cc.exhaustive_size(n, kind)
    from .operator_tools.random_operators import _stream_seed
    seed = _stream_seed(seed) if n_terms else 0
    arrays = {name: np.empty(m, dtype=np.uint64) for name in ("in_x", "in_z", "in_minus", "obs_x", "obs_z")}
    arrays["obs_sign"] = np.empty(m, dtype=np.uint8)
    _lib.check(_lib.lib().fbx_dfe_settings(n, _lib.KIND_PROCESS if kind == "process" else _lib.KIND_STATE, n_terms, seed,
                                           gates.size, _lib.ptr(gates, _U32), m, *(_lib.ptr(arrays[k], _U64) for k in
                                                                                  ("in_x", "in_z", "in_minus", "obs_x", "obs_z")),
                                           _lib.ptr(arrays["obs_sign"], _U8)))
    return DfeExperiment(kind, qubits, gates, arrays, n_terms, seed)


def generate_exhaustive_process_dfe_experiment(benchmarker, program, qubits, seed=None) -> DfeExperiment:
    """direct_fidelity_estimation.py:15-66 for a Clifford circuit: all ``(4^n - 1) 2^n`` settings, in the reference's order.
    ``program`` is a list of ``(name, qubits)`` gates (``clifford_circuit.GATE_NAMES``; what ``clifford.to_gates`` emits) or an
    array of gate words, its qubit indices counting positions in ``qubits``; ``benchmarker`` is accepted and ignored, as
    ``generate_rb_sequence`` does; ``seed`` is not used by the exhaustive generators."""
    return _generate("process", program, qubits, 0, seed)


def generate_exhaustive_state_dfe_experiment(benchmarker, program, qubits, seed=None) -> DfeExperiment:
    """:69-94: the ``2^n - 1`` conjugated Z-strings measured on ``program |0..0>``."""
    return _generate("state", program, qubits, 0, seed)


def _monte_carlo_terms(n_terms):
    if int(n_terms) < 1:
        raise ValueError("n_terms must be at least 1")
    return int(n_terms)


def generate_monte_carlo_state_dfe_experiment(benchmarker, program, qubits, n_terms=200, seed=None) -> DfeExperiment:
    """:97-129 with the documented Philox stream of ``fbx_dfe_settings`` in place of ``np.random`` (``seed=None`` takes a fresh key
    from numpy's global stream): ``n_terms`` uniformly drawn non-identity Z-strings, conjugated."""
    return _generate("state", program, qubits, _monte_carlo_terms(n_terms), seed)


def generate_monte_carlo_process_dfe_experiment(benchmarker, program, qubits, n_terms=200, seed=None) -> DfeExperiment:
    """:132-182: ``n_terms`` uniformly drawn non-identity Paulis with uniformly drawn eigenstates."""
    return _generate("process", program, qubits, _monte_carlo_terms(n_terms), seed)


def _noise_arrays(experiment, class_error, readout_flip, noise_class, shots, seed, first_item, min_shots):
    """Checked before the library is touched: ``(B, K, class_error [B, K], flips [B, n] or None, classes, shots, seed, first_item)``."""
    n = experiment.n_qubits
    shots, first_item = int(shots), int(first_item)
    if not min_shots <= shots <= MAX_SHOTS or first_item < 0:
        raise ValueError(f"need {min_shots} <= shots < 2^32 and first_item >= 0")
    p = np.asarray(class_error, dtype=np.float64)
    if p.ndim == 1:
        p = p[:, None]
    if p.ndim != 2 or not 1 <= p.shape[1] <= _lib.DFE_MAX_CLASSES:
        raise ValueError(f"class_error must be [B] or [B, K] with K in 1..{_lib.DFE_MAX_CLASSES}")
    B, K = p.shape
    K, cls = _noise_classes(experiment.gates.size, noise_class, K)
    flips = None
    if readout_flip is not None:
        flips = np.asarray(readout_flip, dtype=np.float64)
        if flips.shape not in ((n,), (B, n)):
            raise ValueError(f"readout_flip must be [n] = {(n,)} or [B, n] = {(B, n)}, not {flips.shape}")
        flips = np.ascontiguousarray(np.broadcast_to(flips, (B, n)))
    from .operator_tools.random_operators import _stream_seed
    return B, K, np.ascontiguousarray(p), flips, cls, shots, _stream_seed(seed), first_item


def _settings_args(experiment, sigma, touches):
    e = experiment
    return (_lib.ptr(sigma, _I8), _lib.ptr(touches, _U32), _lib.ptr(e.obs_x, _U64), _lib.ptr(e.obs_z, _U64),
            _lib.ptr(e.obs_sign, _U8))


def _raise_poisoned(who, status, first_item):
    bad = np.flatnonzero(status)
    if bad.size:
        b = int(bad[0])
        raise ValueError(f"{who}: item {b} (global id {first_item + b}) cannot be simulated: a class error or a readout_flip "
                         f"value outside [0, 1] ({bad.size} such item(s) in the batch)")


def simulate_dfe_batch(experiment: DfeExperiment, class_error, shots, noise_class=None, readout_flip=None, calibrate=False,
                       seed=None, first_item=0, return_std_errs=False, return_exact=False, return_status=False):
    """B noisy copies of the experiment's circuit measured with its settings, ``shots`` shots per setting, on the device
    (``fbx_dfe_simulate``): ``(expectations [B, m], total_counts [B, m][, std_errs][, exact][, status])``.

    ``class_error`` [B, K] (or [B] for one class): the depolarizing probability of every gate of noise class c in item b;
    ``noise_class`` names each gate's class (``uint8`` per gate, 255 = noiseless, None = all class 0).  ``readout_flip`` ([n] or
    [B, n]): a symmetric flip probability per qubit.  ``calibrate=True`` runs the CALIBRATION of the same settings instead --
    every observable with coefficient 1 on its own +1 eigenstate, so that only the readout flips attenuate it -- under a key
    tag of its own; dividing by it is ``calibrate_expectations_batch``.  ``shots=0`` is the exact-only mode and returns
    ``exact`` (``[, status]``) alone.  ``seed`` / ``first_item`` / the poisoned-item rule are those of
    ``tomography.simulate_process_tomography_batch``; the stream is restated by ``synthetic.restate_dfe_counts``."""
    B, K, p, flips, cls, shots, seed, first_item = _noise_arrays(experiment, class_error, readout_flip, noise_class, shots, seed,
                                                                 first_item, 0)
    m = experiment.m
    sigma, touches = experiment.propagate(cls, K)
    sampled = shots > 0
    e, c = (np.empty((B, m)), np.empty((B, m))) if sampled else (None, None)
    se = np.empty((B, m)) if sampled and return_std_errs else None
    ex = np.empty((B, m)) if return_exact or not sampled else None
    status = np.zeros(B, dtype=np.int32)
    _lib.check(_lib.lib().fbx_dfe_simulate(experiment.n_qubits, m, K, *_settings_args(experiment, sigma, touches), B, _lib.dptr(p),
                                           _lib.dptr(flips), int(bool(calibrate)), shots, seed, first_item, _lib.dptr(e),
                                           _lib.dptr(c), _lib.dptr(se), _lib.dptr(ex), _lib.iptr(status)))
    if not return_status:
        _raise_poisoned("simulate_dfe_batch", status, first_item)
    tail = (status,) if return_status else ()
    if not sampled:
        return (ex,) + tail if tail else ex
    return (e, c) + ((se,) if return_std_errs else ()) + ((ex,) if return_exact else ()) + tail


def simulate_dfe_results(experiment: DfeExperiment, class_error, shots, noise_class=None, readout_flip=None, calibrate=False,
                         seed=None) -> List[ExperimentResult]:
    """One simulated experiment as the ``List[ExperimentResult]`` that ``estimate_dfe`` reads: the stand-in for
    ``acquire_dfe_data``.  ``class_error`` is one item ([K] or a number).  ``calibrate=True`` also simulates the calibration runs
    and rescales by them (``calibrate_observable_estimates``), filling the raw / calibration fields like the reference."""
    p = np.atleast_1d(np.asarray(class_error, dtype=np.float64))
    if p.ndim != 1:
        raise ValueError("simulate_dfe_results covers one experiment: class_error is a number or [K]")
    from .operator_tools.random_operators import _stream_seed
    seed = _stream_seed(seed)
    kw = dict(noise_class=noise_class, readout_flip=readout_flip, seed=seed, return_std_errs=True)
    e, c, se = simulate_dfe_batch(experiment, p[None], shots, **kw)
    settings = experiment.settings()
    if not calibrate:
        return [ExperimentResult(setting=s, expectation=float(x), total_counts=int(n), std_err=float(v))
                for s, x, n, v in zip(settings, e[0], c[0], se[0])]
    ce, cc, cse = simulate_dfe_batch(experiment, p[None], shots, calibrate=True, **kw)
    mean, err = calibrate_expectations_batch(e, se, ce[0], cse[0] ** 2)
    return [ExperimentResult(setting=s, expectation=float(x), total_counts=int(n), std_err=float(v), raw_expectation=float(r),
                             raw_std_err=float(rs), calibration_expectation=float(a), calibration_std_err=float(b),
                             calibration_counts=int(k))
            for s, x, n, v, r, rs, a, b, k in zip(settings, mean[0], c[0], err[0], e[0], se[0], ce[0], cse[0], cc[0])]


def simulate_and_estimate_dfe_batch(experiment: DfeExperiment, class_error, shots, noise_class=None, readout_flip=None,
                                    calibrate=False, seed=None, first_item=0):
    """The resident chain noise -> shots [-> calibration] -> fidelity (``fbx_dfe_simulate_fidelity``): ``(fidelity [B],
    standard_error [B])``, nothing of size [B, m] leaves the device, and ``d = 2^n`` is a double, so any width up to 64 qubits is
    covered.  With ``calibrate=True`` every result is divided by its own simulated calibration run.  Bit for bit what
    ``simulate_dfe_batch``, ``calibrate_expectations_batch`` and ``estimate_dfe_batch`` give when composed through the host."""
    B, K, p, flips, cls, shots, seed, first_item = _noise_arrays(experiment, class_error, readout_flip, noise_class, shots, seed,
                                                                 first_item, 1)
    if B == 0 or experiment.m == 0:
        raise ValueError("need a non-empty batch and experiment")
    sigma, touches = experiment.propagate(cls, K)
    fid, err, status = np.empty(B), np.empty(B), np.zeros(B, dtype=np.int32)
    _lib.check(_lib.lib().fbx_dfe_simulate_fidelity(
        experiment.n_qubits, experiment.m, K, *_settings_args(experiment, sigma, touches), B, _lib.dptr(p), _lib.dptr(flips), shots,
        seed, first_item, _lib.KIND_PROCESS if experiment.kind == "process" else _lib.KIND_STATE, int(bool(calibrate)),
        _lib.dptr(fid), _lib.dptr(err), _lib.iptr(status)))
    _raise_poisoned("simulate_and_estimate_dfe_batch", status, first_item)
    return fid, err
