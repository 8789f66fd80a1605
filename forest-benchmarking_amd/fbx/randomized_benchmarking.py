"""Randomized-benchmarking analysis (forest/benchmarking/randomized_benchmarking.py) on the device.

The analysis half of the reference's module under its own names: survival statistics from I/Z expectations, shifted purities for
unitarity, the decay fits, and the interleaved-RB bounds.  ``fit_rb_results_batch`` / ``fit_unitarity_results_batch`` take
``[B, S, .]`` arrays (B decays of S sequences each) and run statistics -> weights and guess -> fit as one chain of device calls
(fbx_rb_survival_dev / fbx_rb_purity_dev -> fbx_fit_prepare_dev -> fbx_curve_fit_dev); the single-experiment functions are that
chain with B = 1.  The scalar conversion and bound formulas are plain numpy and accept arrays.

Sequence generation (``generate_rb_sequence``, ``generate_rb_experiment_sequences``) keeps the reference's names and rules but
needs no quilc: a Clifford is an element word of ``fbx.clifford`` (include/fbx.h, "Clifford elements"), a sequence an array of
words drawn, composed and inverted on the device (fbx_rb_sequences); ``clifford.to_gates`` turns a word into native gates.
``simulate_rb_sequences_batch`` runs sequences under Pauli-transfer-matrix noise (fbx_rb_simulate), ``simulate_rb_experiment_batch``
turns that into the arrays ``fit_rb_results_batch`` takes.  ``simulate_rb_acquisition_batch`` /
``simulate_unitarity_acquisition_batch`` are the acquisition itself in one device call per batch of experiments (fbx_rb_acquire:
sequences drawn on the fly, per-experiment noise and readout error, shots counted on the device, IZ / ZI / ZZ from the same
shots), ``simulate_and_fit_rb_batch`` / ``simulate_and_fit_unitarity_batch`` the chains from channels to fitted decays that stay
on the device.  Data acquisition on a QuantumComputer (``acquire_*``, ``do_rb``) needs pyquil and is not part of this package.
"""
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, clifford
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


def _fit_decays_resident(statistics, kind, depths, e, s, errors_are_variances, param_guesses, fit_kw):
    """upload -> statistics kernel -> ``fbx_fit_prepare_dev`` -> resident decay fit, for expectations / std_errs [B, K, ...]:
    ``statistics(d_e, d_s, d_values, d_errors)`` issues the kernel that turns them into the [B, K] values to fit and their errors."""
    B, K = e.shape[:2]
    with _lib.DeviceScope() as dev:
        d_e, d_s, d_values, d_errors = dev.upload(e), dev.upload(s), dev.alloc(8 * B * K), dev.alloc(8 * B * K)
        _lib.check(statistics(d_e.ptr, d_s.ptr, d_values.ptr, d_errors.ptr))
        d_w, d_g, d_has = dev.alloc(8 * B * K), dev.alloc(8 * B * 3), dev.alloc(4 * B)
        _lib.check(_lib.lib().fbx_fit_prepare_dev(kind, B, K, d_values.ptr, d_errors.ptr, int(errors_are_variances),
                                                  d_w.ptr, d_g.ptr, d_has.ptr))
        if param_guesses is not None:
            g = fitting._guess_array(_lib.FIT_BASE_DECAY, param_guesses, B)
            _lib.check(_lib.lib().fbx_memcpy_h2d(d_g.ptr, g.ctypes.data, g.nbytes))
        batch = fitting.curve_fit_resident(_lib.FIT_BASE_DECAY, depths, d_values, d_w, d_g, B, K, **fit_kw)
        batch.has_weights = d_has.to_array(np.int32, (B,)).astype(bool)
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
    lib = _lib.lib()
    return _fit_decays_resident(lambda d_e, d_s, d_surv, d_var: lib.fbx_rb_survival_dev(dim, B * K, d_e, d_s, shots, d_surv, d_var),
                                _lib.FIT_PREPARE_RB, depths, e, s, True, param_guesses, fit_kw)


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
    lib = _lib.lib()
    return _fit_decays_resident(lambda d_e, d_s, d_pur, d_err: lib.fbx_rb_purity_dev(dim, B * K, d_e, d_s, 1, d_pur, d_err),
                                _lib.FIT_PREPARE_UNITARITY, depths, e, s, False, param_guesses, fit_kw)


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


# ---------------------------------------------------------------- sequences and their simulation (fbx_rb_sequences / fbx_rb_simulate)
def _n_qubits(n):
    n = int(n)
    if n > 2:
        raise ValueError("No RB gateset for more than two qubits.")
    if n < 1:
        raise ValueError("RB sequences need at least one qubit.")
    return n


def _interleaved_word(n, interleaved_gate):
    if interleaved_gate is None:
        return _lib.CLIFFORD_NONE
    if not clifford.is_valid(int(interleaved_gate), n):
        raise ValueError(f"interleaved_gate is not a valid {n}-qubit Clifford element word")
    return int(interleaved_gate)


def _seed64(random_seed):
    if random_seed is None:
        return int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0])
    return int(random_seed) & 0xFFFFFFFFFFFFFFFF


def z_product_indices(n_qubits: int) -> np.ndarray:
    """Pauli indices of the 2^n - 1 non-identity I/Z products, observable z = 1 .. 2^n - 1 read as a bit mask whose lowest bit is
    the LAST qubit (the order of ``synthetic.rb_data``): [3] for one qubit, [3, 12, 15] = IZ, ZI, ZZ for two."""
    n = _n_qubits(n_qubits)
    return np.array([sum(3 << (2 * t) for t in range(n) if (z >> t) & 1) for z in range(1, 1 << n)], dtype=np.int64)


def _rb_sequences(n, lengths, seed, interleaved, self_inverting):
    lengths = np.asarray(lengths, dtype=np.int64).ravel()
    if lengths.size and lengths.min() < 0:
        raise ValueError("sequence lengths must not be negative")
    offsets = np.zeros(lengths.size + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    total = int(offsets[-1])
    elems = np.empty(total, dtype=np.uint32)
    noise_ids = np.empty(total, dtype=np.uint8)
    _lib.check(_lib.lib().fbx_rb_sequences(n, lengths.size, offsets.ctypes.data_as(_lib._i64p), seed, interleaved, int(bool(self_inverting)),
                                           elems.ctypes.data_as(_lib._u32p), noise_ids.ctypes.data_as(_lib._u8p)))
    return offsets, elems, noise_ids


def _length_of_depth(depth, interleaved, self_inverting):
    """Elements of a sequence of ``depth`` Cliffords (the inverse included when self-inverting): an interleaved gate follows every
    random element."""
    randoms = depth - 1 if self_inverting else depth
    return (2 * randoms if interleaved != _lib.CLIFFORD_NONE else randoms) + (1 if self_inverting else 0)


def generate_rb_sequence(benchmarker, qubits: Sequence[int], depth: int, interleaved_gate: Optional[int] = None,
                         random_seed: Optional[int] = None) -> np.ndarray:
    """A complete self-inverting RB sequence (randomized_benchmarking.py:105-126) as a uint32 array of Clifford element words:
    ``depth`` Cliffords, the last one the inverse of the rest; with ``interleaved_gate`` (an element word) that gate follows each
    of the depth - 1 random Cliffords.  ``benchmarker`` is accepted for the reference's signature and ignored (None is fine); only
    ``len(qubits)`` matters, the words count their qubits 0, 1."""
    if depth < 2:
        raise ValueError("Sequence depth must be at least 2 for rb sequences, or at least 1 for "
                         "unitarity sequences.")
    n = _n_qubits(len(qubits))
    inter = _interleaved_word(n, interleaved_gate)
    return _rb_sequences(n, [_length_of_depth(int(depth), inter, True)], _seed64(random_seed), inter, True)[1]


def generate_rb_experiment_sequences(benchmarker, qubits: Sequence[int], depths: Sequence[int], interleaved_gate: Optional[int] = None,
                                     random_seed: Optional[int] = None, use_self_inv_seqs: bool = True) -> List[np.ndarray]:
    """One sequence per entry of ``depths`` (randomized_benchmarking.py:129-174).  As in the reference, ``random_seed`` advances
    by one per depth, and ``use_self_inv_seqs=False`` generates depth + 1 Cliffords without an interleaved gate and strips the
    inverse."""
    sequences = []
    for depth in depths:
        if random_seed is not None:
            random_seed += 1
        if use_self_inv_seqs:
            sequence = generate_rb_sequence(benchmarker, qubits, depth, interleaved_gate, random_seed)
        else:
            sequence = generate_rb_sequence(benchmarker, qubits, depth + 1, random_seed=random_seed)[:-1]
        sequences.append(sequence)
    return sequences


def generate_rb_sequences_batch(n_qubits: int, depths: Sequence[int], num_sequences: int, interleaved_gate: Optional[int] = None,
                                seed: Optional[int] = None, self_inverting: bool = True):
    """``num_sequences`` sequences for every entry of ``depths`` in one device call: ``(offsets, elems, noise_ids)`` with
    sequence ``i * num_sequences + s`` (depth i, repetition s) in ``elems[offsets[b]:offsets[b + 1]]`` and ``noise_ids`` 1 on
    the interleaved elements.  A depth counts Cliffords as ``generate_rb_sequence`` does (inverse included when self-inverting).
    Sequence b depends on ``(seed, b)`` only."""
    n = _n_qubits(n_qubits)
    inter = _interleaved_word(n, interleaved_gate)
    depths = [int(d) for d in depths]
    if any(d < (2 if self_inverting else 1) for d in depths):
        raise ValueError("Sequence depth must be at least 2 for rb sequences, or at least 1 for "
                         "unitarity sequences.")
    lengths = np.repeat([_length_of_depth(d, inter, self_inverting) for d in depths], int(num_sequences))
    return _rb_sequences(n, lengths, _seed64(seed), inter, self_inverting)


def simulate_rb_sequences_batch(n_qubits: int, offsets, elems, noise_ptms, noise_ids=None, prep=None) -> np.ndarray:
    """Final Pauli vectors ``[B, 4^n]`` of the sequences ``elems[offsets[b]:offsets[b + 1]]``: from ``prep`` (default |0..0>), every
    element's signed permutation followed by the Pauli transfer matrix ``noise_ptms[noise_ids[.]]`` (``[G, 4^n, 4^n]`` or one
    matrix; ``noise_ids`` default all 0)."""
    n = _n_qubits(n_qubits)
    D = 4 ** n
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    elems = np.ascontiguousarray(elems, dtype=np.uint32)
    ptms = np.ascontiguousarray(noise_ptms, dtype=np.float64)
    if ptms.ndim == 2:
        ptms = ptms[None]
    if ptms.ndim != 3 or ptms.shape[1:] != (D, D):
        raise ValueError(f"noise_ptms must be [G, {D}, {D}]")
    if offsets.ndim != 1 or offsets.size < 1:
        raise ValueError("offsets must be [B + 1]")
    B = offsets.size - 1
    if B and (offsets[0] != 0 or offsets[-1] != elems.size):
        raise ValueError("offsets must start at 0 and end at len(elems)")
    ids = None
    if noise_ids is not None:
        ids = np.ascontiguousarray(noise_ids, dtype=np.uint8)
        if ids.shape != elems.shape:
            raise ValueError("noise_ids must have the shape of elems")
    p = None
    if prep is not None:
        p = np.ascontiguousarray(prep, dtype=np.float64)
        if p.shape != (D,):
            raise ValueError(f"prep must be a Pauli vector of {D} components")
    out = np.empty((B, D))
    _lib.check(_lib.lib().fbx_rb_simulate(n, B, offsets.ctypes.data_as(_lib._i64p), elems.ctypes.data_as(_lib._u32p),
                                          None if ids is None else ids.ctypes.data_as(_lib._u8p), ptms.shape[0], _lib.dptr(ptms),
                                          _lib.dptr(p), _lib.dptr(out)))
    return out


def simulate_rb_experiment_batch(n_qubits: int, depths: Sequence[int], num_sequences: int, noise_ptms, interleaved_gate: Optional[int] = None,
                                 seed: Optional[int] = None, shots: Optional[int] = None, prep=None):
    """RB (or, with ``interleaved_gate``, IRB) experiments from noise channels: ``noise_ptms`` is ``[G, 4^n, 4^n]`` for one
    experiment or ``[E, G, 4^n, 4^n]`` for E of them (PTM 0 follows every random Clifford and the inverse, PTM 1 the interleaved
    gate); every experiment draws ``num_sequences`` self-inverting sequences per depth (seed + experiment index) and simulates
    them.  Returns ``(z_expectations, z_std_errs)``, both ``[E, len(depths), 2^n - 1]`` as ``fit_rb_results_batch`` takes them: the
    I/Z-product expectations (``z_product_indices``) averaged over the sequences of a depth, and the standard error of that mean
    (0 for a single sequence without shots).  ``shots`` samples every sequence's expectations first
    (``synthetic.sample_expectations``, independent observables; its streams are keyed by a hash of the experiment's seed, so
    another seed gives other sequences AND other shot noise).  For two qubits ``fit_rb_results_batch`` asks for ``num_shots``
    (the covariance of IZ, ZI, ZZ estimated from one set of shots): pass ``shots``, or a large number such as 10^12 for the exact
    expectations of ``shots=None``, whose covariance term vanishes."""
    n = _n_qubits(n_qubits)
    D = 4 ** n
    ptms = np.asarray(noise_ptms, dtype=np.float64)
    if ptms.ndim == 2:
        ptms = ptms[None]
    if ptms.ndim == 3:
        ptms = ptms[None]
    if ptms.ndim != 4 or ptms.shape[2:] != (D, D):
        raise ValueError(f"noise_ptms must be [G, {D}, {D}] or [E, G, {D}, {D}]")
    if interleaved_gate is not None and ptms.shape[1] < 2:
        raise ValueError("an interleaved experiment needs two noise PTMs: [0] after the random Cliffords, [1] after the gate")
    S, K = len(depths), int(num_sequences)
    if K < 1:
        raise ValueError("num_sequences must be positive")
    cols = z_product_indices(n)
    base = _seed64(seed)
    e_out, s_out = np.empty((ptms.shape[0], S, cols.size)), np.empty((ptms.shape[0], S, cols.size))
    for x in range(ptms.shape[0]):
        offsets, elems, ids = generate_rb_sequences_batch(n, depths, K, interleaved_gate, (base + x) & 0xFFFFFFFFFFFFFFFF, True)
        z = simulate_rb_sequences_batch(n, offsets, elems, ptms[x], ids, prep)[:, cols]             # [S K, 2^n - 1]
        shot_var = 0.0
        if shots is not None:
            from . import synthetic
            # the binomial streams follow the seed too: RandomState(seed_base + sequence index), seed_base a hash of (seed + x)
            z, _ = synthetic.sample_expectations(z, int(shots), seed_base=(((base + x) * 0x9E3779B1) >> 7) % (2 ** 31))
            shot_var = np.clip(1.0 - z * z, 0.0, None).reshape(S, K, -1).mean(axis=1) / float(shots)
        z = z.reshape(S, K, -1)
        e_out[x] = z.mean(axis=1)
        s_out[x] = np.sqrt(z.var(axis=1, ddof=1) / K) if K > 1 else np.sqrt(shot_var + np.zeros_like(e_out[x]))
    return e_out, s_out


# ---------------------------------------------------------------- acquisition on the device: channels to expectations (fbx_rb_acquire)
_DEPTH_MESSAGE = "Sequence depth must be at least 2 for rb sequences, or at least 1 for unitarity sequences."


def generate_unitarity_experiment_sequences(benchmarker, qubits: Sequence[int], depths: Sequence[int], num_sequences: int,
                                            random_seed: Optional[int] = None) -> List[np.ndarray]:
    """The sequences of a unitarity experiment (generate_unitarity_experiments, randomized_benchmarking.py:441-487, before the
    grouping into programs): ``num_sequences`` sequences of ``depth`` random Cliffords for every entry of ``depths``, NOT
    self-inverting, as a list of uint32 arrays of element words in the order depth 0 repetition 0, 1, ..., depth 1 repetition 0,
    ....  One device call (fbx_rb_sequences with self_inverting = 0); sequence b depends on ``(random_seed, b)`` only, and these are
    the sequences ``simulate_unitarity_acquisition_batch`` measures for the experiment whose seed + index is ``random_seed``.
    ``benchmarker`` is accepted for the reference's signature and ignored."""
    n = _n_qubits(len(qubits))
    if int(num_sequences) < 1:
        raise ValueError("num_sequences must be positive")
    offsets, elems, _ = generate_rb_sequences_batch(n, depths, int(num_sequences), None, random_seed, self_inverting=False)
    return [elems[offsets[b]:offsets[b + 1]].copy() for b in range(offsets.size - 1)]


def predicted_rb_decay(ptm):
    """The RB decay (tr L - 1) / (d^2 - 1) of gate-independent noise with Pauli transfer matrix ``ptm [..., d^2, d^2]``."""
    ptm = np.asarray(ptm, dtype=np.float64)
    return (np.trace(ptm, axis1=-2, axis2=-1) - 1.0) / (ptm.shape[-1] - 1)


def predicted_unitarity(ptm):
    """The unitarity of a channel: the squared Frobenius norm of the unital block of ``ptm [..., d^2, d^2]`` (rows and columns
    1..d^2 - 1) divided by d^2 - 1 (Wallman et al., New J. Phys. 17, 113020 (2015))."""
    ptm = np.asarray(ptm, dtype=np.float64)
    return np.sum(ptm[..., 1:, 1:] ** 2, axis=(-2, -1)) / (ptm.shape[-1] - 1)


def unitarity_basis_of_pauli(n_qubits: int, pauli: int) -> int:
    """The one measured basis of a unitarity acquisition that Pauli index ``pauli`` (1 .. 4^n - 1) is read from: its non-identity
    factors, and Z on every qubit where it has the identity.  Basis index in base 3, digits X, Y, Z = 0, 1, 2, qubit 0 most
    significant (include/fbx.h, fbx_rb_acquire step 5)."""
    n = _n_qubits(n_qubits)
    if not 1 <= int(pauli) < 4 ** n:
        raise ValueError("pauli must be a non-identity Pauli index")
    basis = 0
    for t in reversed(range(n)):
        digit = (int(pauli) >> (2 * t)) & 3
        basis = 3 * basis + (digit - 1 if digit else 2)
    return basis


class _Acquisition:
    """Validated arguments of one fbx_rb_acquire call."""

    def __init__(self, n_qubits, depths, num_sequences, noise_ptms, interleaved_gate, shots, flips, prep, seed, first_item, unitarity):
        n = self.n = _n_qubits(n_qubits)
        D = self.D = 4 ** n
        self.depths = np.array([int(d) for d in depths], dtype=np.int32)
        self.S, self.K = self.depths.size, int(num_sequences)
        if self.S < 1:
            raise ValueError("depths must not be empty")
        if self.depths.min() < (1 if unitarity else 2):
            raise ValueError(_DEPTH_MESSAGE)
        if self.S > _lib.RB_ACQUIRE_MAX_DEPTHS:
            raise ValueError(f"at most {_lib.RB_ACQUIRE_MAX_DEPTHS} depths per call")
        if self.K < 1:
            raise ValueError("num_sequences must be positive")
        if unitarity and interleaved_gate is not None:
            raise ValueError("a unitarity experiment takes no interleaved gate")
        self.inter = _interleaved_word(n, interleaved_gate)
        self.G = 2 if interleaved_gate is not None else 1
        ptms = np.asarray(noise_ptms, dtype=np.float64)
        if ptms.ndim == 2:
            ptms = ptms[None]
        if ptms.ndim == 3:
            ptms = ptms[None]
        if ptms.ndim != 4 or ptms.shape[2:] != (D, D):
            raise ValueError(f"noise_ptms must be [G, {D}, {D}] or [E, G, {D}, {D}]")
        if ptms.shape[1] < self.G:
            raise ValueError("an interleaved experiment needs two noise PTMs: [0] after the random Cliffords, [1] after the gate")
        self.ptms = np.ascontiguousarray(ptms[:, :self.G])
        self.E = self.ptms.shape[0]
        self.flips = None
        if flips is not None:
            f = np.asarray(flips, dtype=np.float64)
            if f.shape not in ((n, 2), (self.E, n, 2)):
                raise ValueError(f"flips must be [{n}, 2] or [E, {n}, 2]")
            self.flips = np.ascontiguousarray(np.broadcast_to(f, (self.E, n, 2)))
        self.prep = None
        if prep is not None:
            self.prep = np.ascontiguousarray(prep, dtype=np.float64)
            if self.prep.shape != (D,):
                raise ValueError(f"prep must be a Pauli vector of {D} components")
        self.shots = 0 if shots is None else int(shots)
        if not 0 <= self.shots < 2 ** 31:
            raise ValueError("shots must be in 0 .. 2^31 - 1 (None or 0: exact expectations)")
        self.first_item = int(first_item)
        if self.first_item < 0:
            raise ValueError("first_item must not be negative")
        self.seed = _seed64(seed)
        self.mode = _lib.RB_UNITARITY if unitarity else _lib.RB_STANDARD
        self.M = 2 ** n
        self.NB = 3 ** n if unitarity else 1
        self.C = D - 1 if unitarity else self.M - 1
        if self.S * self.K * self.NB >= 2 ** 32:
            raise ValueError("len(depths) * num_sequences * bases must be below 2^32")

    def launch(self, dev, vectors=False, probabilities=False, histograms=False):
        """Enqueue the acquisition on buffers owned by ``dev``; returns the device buffers (None where not asked for) as
        ``(expect, std_err, status, vec, prob, hist)``."""
        if histograms and self.shots == 0:
            raise ValueError("histograms need shots >= 1")
        seqs = self.E * self.S * self.K
        d_ptms, d_prep, d_flips = dev.upload(self.ptms), dev.upload(self.prep), dev.upload(self.flips)
        d_e, d_s, d_st = dev.alloc(8 * seqs * self.C), dev.alloc(8 * seqs * self.C), dev.alloc(4 * self.E)
        d_vec = dev.alloc(8 * seqs * self.D) if vectors else None
        d_prob = dev.alloc(8 * seqs * self.NB * self.M) if probabilities else None
        d_hist = dev.alloc(4 * seqs * self.NB * self.M) if histograms else None
        _lib.check(_lib.lib().fbx_rb_acquire_dev(
            self.n, self.E, self.S, self.depths.ctypes.data_as(_lib._ip), self.K, self.mode, self.inter, self.G, d_ptms.ptr,
            _lib.devptr(d_prep), _lib.devptr(d_flips), self.shots, self.seed, self.first_item, _lib.devptr(d_vec), _lib.devptr(d_prob),
            _lib.devptr(d_hist), d_e.ptr, d_s.ptr, d_st.ptr))
        return d_e, d_s, d_st, d_vec, d_prob, d_hist

    def status(self, d_status, return_status):
        status = d_status.to_array(np.int32, (self.E,))
        if not return_status and status.any():
            raise ValueError(f"experiment {int(np.flatnonzero(status)[0])} is poisoned: a non-finite noise PTM or prep entry, a flip "
                             "probability outside [0, 1], or an outcome distribution without a positive finite sum")
        return status


def _acquisition_batch(a, per_sequence, return_vectors, return_probabilities, return_histograms, return_status):
    seqs = a.S * a.K
    with _lib.DeviceScope() as dev:
        d_e, d_s, d_st, d_vec, d_prob, d_hist = a.launch(dev, return_vectors, return_probabilities, return_histograms)
        if per_sequence:
            e, s = d_e.to_array(np.float64, (a.E, seqs, a.C)), d_s.to_array(np.float64, (a.E, seqs, a.C))
        else:
            d_m, d_err = dev.alloc(8 * a.E * a.S * a.C), dev.alloc(8 * a.E * a.S * a.C)
            _lib.check(_lib.lib().fbx_rb_depth_means_dev(a.E, a.S, a.K, a.C, d_e.ptr, d_s.ptr, d_m.ptr, d_err.ptr))
            e, s = d_m.to_array(np.float64, (a.E, a.S, a.C)), d_err.to_array(np.float64, (a.E, a.S, a.C))
        status = a.status(d_st, return_status)
        out = (e, s)
        if return_vectors:
            out += (d_vec.to_array(np.float64, (a.E, seqs, a.D)),)
        if return_probabilities:
            out += (d_prob.to_array(np.float64, (a.E, seqs, a.NB, a.M)),)
        if return_histograms:
            out += (d_hist.to_array(np.uint32, (a.E, seqs, a.NB, a.M)),)
    return out + ((status,) if return_status else ())


def simulate_rb_acquisition_batch(n_qubits: int, depths: Sequence[int], num_sequences: int, noise_ptms,
                                  interleaved_gate: Optional[int] = None, shots: Optional[int] = None, flips=None, prep=None,
                                  seed: Optional[int] = None, first_item: int = 0, per_sequence: bool = False,
                                  return_vectors: bool = False, return_probabilities: bool = False,
                                  return_histograms: bool = False, return_status: bool = False):
    """E RB (or, with ``interleaved_gate``, IRB) experiments from noise channels to measured expectations in one device call
    (fbx_rb_acquire): ``noise_ptms [E, G, 4^n, 4^n]`` (lower ranks broadcast as in ``simulate_rb_experiment_batch``; matrix 0
    follows every random Clifford and the inverse, matrix 1 the interleaved gate), ``flips [E, n, 2]`` or ``[n, 2]`` the readout
    errors (P(read 1 | 0), P(read 0 | 1)) per qubit, ``shots`` per sequence (None or 0: exact expectations).  Experiment x is the
    global item ``first_item + x``; it runs the sequences ``generate_rb_sequences_batch(..., seed + first_item + x)`` -- those of
    ``simulate_rb_experiment_batch`` -- and IZ, ZI, ZZ are read off the SAME shots, as ``fit_rb_results_batch(..., num_shots)``
    assumes.  Returns ``(z_expectations, z_std_errs)``, both ``[E, S, 2^n - 1]`` in the order of ``z_product_indices``: the mean
    over the ``num_sequences`` sequences of a depth and the standard error of that mean (fbx_rb_depth_means; for one sequence
    per depth the sequence's own standard error).  ``per_sequence`` gives ``[E, S K, 2^n - 1]`` instead, sequence ``i K + s`` at
    depth ``np.repeat(depths, K)[i K + s]``: what the reference's ``fit_rb_results`` is fed.  ``return_vectors`` /
    ``return_probabilities`` / ``return_histograms`` append the final Pauli vectors ``[E, S K, 4^n]``, the outcome distributions
    and the counts ``[E, S K, 1, 2^n]``; ``return_status`` appends the status ``[E]`` instead of raising for a poisoned experiment
    (NaN outputs, zero counts)."""
    a = _Acquisition(n_qubits, depths, num_sequences, noise_ptms, interleaved_gate, shots, flips, prep, seed, first_item, False)
    return _acquisition_batch(a, per_sequence, return_vectors, return_probabilities, return_histograms, return_status)


def simulate_unitarity_acquisition_batch(n_qubits: int, depths: Sequence[int], num_sequences: int, noise_ptms,
                                         shots: Optional[int] = None, flips=None, prep=None, seed: Optional[int] = None,
                                         first_item: int = 0, return_vectors: bool = False, return_probabilities: bool = False,
                                         return_histograms: bool = False, return_status: bool = False):
    """E unitarity experiments in one device call: sequences of ``depth`` random Cliffords without the inverse
    (``generate_unitarity_experiment_sequences`` under the seed ``seed + first_item + x``), measured in all 3^n products of X, Y,
    Z with ``shots`` shots per sequence and basis; every Pauli is estimated from the one basis
    ``unitarity_basis_of_pauli`` names.  Returns ``(expectations, std_errs)`` of shape ``[E, S K, 4^n - 1]`` (Pauli indices
    1 .. 4^n - 1), as ``fit_unitarity_results_batch(np.repeat(depths, K), ...)`` and ``purity_statistics_batch`` take them; the
    other arguments and the appended outputs are those of ``simulate_rb_acquisition_batch`` (distributions and counts
    ``[E, S K, 3^n, 2^n]``)."""
    a = _Acquisition(n_qubits, depths, num_sequences, noise_ptms, None, shots, flips, prep, seed, first_item, True)
    return _acquisition_batch(a, True, return_vectors, return_probabilities, return_histograms, return_status)


def depth_means_batch(values, seq_std_errs=None):
    """Mean over the K sequences of a depth and the standard error of that mean for ``values [E, S, K, C]`` (fbx_rb_depth_means):
    ``sqrt(var(ddof=1) / K)``, or for K = 1 the sequence's own ``seq_std_errs [E, S, 1, C]`` (None: 0).  Returns two ``[E, S, C]``."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    if v.ndim != 4:
        raise ValueError("values must be [E, S, K, C]")
    E, S, K, C = v.shape
    se = None
    if seq_std_errs is not None:
        se = np.ascontiguousarray(seq_std_errs, dtype=np.float64)
        if se.shape != v.shape:
            raise ValueError("seq_std_errs must have the shape of values")
    mean, err = np.empty((E, S, C)), np.empty((E, S, C))
    _lib.check(_lib.lib().fbx_rb_depth_means(E, S, K, C, _lib.dptr(v), _lib.dptr(se) if K == 1 else None, _lib.dptr(mean), _lib.dptr(err)))
    return mean, err


def _fit_points(a, points):
    if points not in ("depth", "sequence"):
        raise ValueError("points must be 'depth' or 'sequence'")
    P = a.S if points == "depth" else a.S * a.K
    if not 2 <= P <= _lib.FIT_MAX_POINTS:
        raise ValueError(f"a fit takes 2..{_lib.FIT_MAX_POINTS} points (got {P}); use points='depth' or fewer sequences")
    return P, (a.depths.astype(np.float64) if points == "depth" else np.repeat(a.depths, a.K).astype(np.float64))


def _fit_resident(dev, kind, x, d_values, d_errors, errors_are_variances, B, P, param_guesses, fit_kw):
    d_w, d_g, d_has = dev.alloc(8 * B * P), dev.alloc(8 * B * 3), dev.alloc(4 * B)
    _lib.check(_lib.lib().fbx_fit_prepare_dev(kind, B, P, d_values.ptr, d_errors.ptr, int(errors_are_variances), d_w.ptr, d_g.ptr,
                                              d_has.ptr))
    if param_guesses is not None:
        g = fitting._guess_array(_lib.FIT_BASE_DECAY, param_guesses, B)
        _lib.check(_lib.lib().fbx_memcpy_h2d(d_g.ptr, g.ctypes.data, g.nbytes))
    batch = fitting.curve_fit_resident(_lib.FIT_BASE_DECAY, x, d_values, d_w, d_g, B, P, **fit_kw)
    batch.has_weights = d_has.to_array(np.int32, (B,)).astype(bool)
    return batch


def simulate_and_fit_rb_batch(n_qubits: int, depths: Sequence[int], num_sequences: int, noise_ptms,
                              interleaved_gate: Optional[int] = None, shots: Optional[int] = None, flips=None, prep=None,
                              seed: Optional[int] = None, first_item: int = 0, points: str = "depth", param_guesses=None,
                              **fit_kw) -> "fitting.FitBatch":
    """``simulate_rb_acquisition_batch`` followed by ``fit_rb_results_batch(..., num_shots=shots)`` without leaving the device:
    fbx_rb_acquire_dev -> (``points="depth"``: fbx_rb_depth_means_dev over the sequences of a depth) -> fbx_rb_survival_dev ->
    fbx_fit_prepare_dev -> fbx_curve_fit_dev, bit for bit what the two public calls return.  ``points="sequence"`` fits every
    sequence as a point of its own (``per_sequence=True``; S K <= 256).  Without shots the covariance term of IZ, ZI, ZZ is left
    out (it vanishes).  Returns the FitBatch of E decays; a poisoned experiment raises ``ValueError``."""
    a = _Acquisition(n_qubits, depths, num_sequences, noise_ptms, interleaved_gate, shots, flips, prep, seed, first_item, False)
    P, x = _fit_points(a, points)
    num_shots = a.shots if a.M > 2 else 0                      # exact expectations (shots None or 0) have no covariance term
    with _lib.DeviceScope() as dev:
        d_e, d_s, d_st = a.launch(dev)[:3]
        if points == "depth":
            d_m, d_err = dev.alloc(8 * a.E * a.S * a.C), dev.alloc(8 * a.E * a.S * a.C)
            _lib.check(_lib.lib().fbx_rb_depth_means_dev(a.E, a.S, a.K, a.C, d_e.ptr, d_s.ptr, d_m.ptr, d_err.ptr))
            d_e, d_s = d_m, d_err
        d_surv, d_var = dev.alloc(8 * a.E * P), dev.alloc(8 * a.E * P)
        _lib.check(_lib.lib().fbx_rb_survival_dev(a.M, a.E * P, d_e.ptr, d_s.ptr, num_shots, d_surv.ptr, d_var.ptr))
        a.status(d_st, False)
        return _fit_resident(dev, _lib.FIT_PREPARE_RB, x, d_surv, d_var, True, a.E, P, param_guesses, fit_kw)


def simulate_and_fit_unitarity_batch(n_qubits: int, depths: Sequence[int], num_sequences: int, noise_ptms,
                                     shots: Optional[int] = None, flips=None, prep=None, seed: Optional[int] = None,
                                     first_item: int = 0, points: str = "depth", param_guesses=None, **fit_kw) -> "fitting.FitBatch":
    """``simulate_unitarity_acquisition_batch`` followed by the unitarity fit without leaving the device: fbx_rb_acquire_dev ->
    fbx_rb_purity_dev -> (``points="depth"``: fbx_rb_depth_means_dev of the purities, C = 1) -> fbx_fit_prepare_dev ->
    fbx_curve_fit_dev.  ``points="sequence"`` is ``fit_unitarity_results_batch(np.repeat(depths, K), ...)`` bit for bit (S K <=
    256); ``points="depth"`` is ``purity_statistics_batch`` -> ``depth_means_batch`` -> the same preparation and fit.  The
    unitarities are ``batch.value('decay')``."""
    a = _Acquisition(n_qubits, depths, num_sequences, noise_ptms, None, shots, flips, prep, seed, first_item, True)
    P, x = _fit_points(a, points)
    seqs = a.E * a.S * a.K
    with _lib.DeviceScope() as dev:
        d_e, d_s, d_st = a.launch(dev)[:3]
        d_pur, d_err = dev.alloc(8 * seqs), dev.alloc(8 * seqs)
        _lib.check(_lib.lib().fbx_rb_purity_dev(a.M, seqs, d_e.ptr, d_s.ptr, 1, d_pur.ptr, d_err.ptr))
        if points == "depth":
            d_m, d_me = dev.alloc(8 * a.E * a.S), dev.alloc(8 * a.E * a.S)
            _lib.check(_lib.lib().fbx_rb_depth_means_dev(a.E, a.S, a.K, 1, d_pur.ptr, d_err.ptr, d_m.ptr, d_me.ptr))
            d_pur, d_err = d_m, d_me
        a.status(d_st, False)
        return _fit_resident(dev, _lib.FIT_PREPARE_UNITARITY, x, d_pur, d_err, False, a.E, P, param_guesses, fit_kw)
