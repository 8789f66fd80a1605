"""Tomography estimators with the reference's names and signatures, running on MI355X.

Mirror of forest/benchmarking/tomography.py:130-633.  Every estimator takes the same
``(results: List[ExperimentResult], qubits: List[int], **kwargs)`` and returns the same dense
complex128 ``np.ndarray``; ``*_batch`` variants take SoA arrays ``expectations[B, m]``,
``total_counts[B, m]`` plus a :class:`fbx.design.Design` and are where the throughput lives.
"""
import ctypes as C
import warnings
from typing import Callable, List, Sequence, Tuple

import numpy as np

from . import _lib
from . import distance_measures as dm
from .design import Design, Grouping, flatten_results, group_design, process_design, state_design  # noqa: F401
from .observable_estimation import (ExperimentResult, ExperimentSetting, PauliTerm,
                                    TensorProductState, zeros_state, SIC0, SIC1, SIC2, SIC3,  # noqa: F401
                                    plusX, minusX, plusY, minusY, plusZ, minusZ)  # noqa: F401
from .observable_estimation import _OneQState
from .design import PAULI_LABELS, STATE_LABELS

import functools


# ==================================================================================================
# Experiment settings (tomography.py:31-123) -- read off the design tables (fbx.design), which hold
# the canonical order: input states outer, traceless Pauli observables inner.  No pyquil Program.
# ==================================================================================================
def _settings_of(design: Design, qubits: Sequence[int]) -> List[ExperimentSetting]:
    qubits = list(qubits)
    out = []
    for prep_codes, pauli_codes in zip(design.in_labels, design.paulis):
        prepared = TensorProductState(_OneQState(*STATE_LABELS[int(c)], q) for c, q in zip(prep_codes, qubits))
        measured = PauliTerm({q: PAULI_LABELS[int(c)] for c, q in zip(pauli_codes, qubits)})
        out.append(ExperimentSetting(in_state=prepared, observable=measured))
    return out


def generate_state_tomography_settings(qubits: List[int]) -> List[ExperimentSetting]:
    """The settings of generate_state_tomography_experiment (tomography.py:46-60): |0..0> in, every
    traceless Pauli out."""
    return _settings_of(state_design(len(qubits)), qubits)


def generate_process_tomography_settings(qubits: List[int], in_basis='pauli') -> List[ExperimentSetting]:
    """The settings of generate_process_tomography_experiment (tomography.py:100-123); an unknown
    ``in_basis`` raises the reference's ``ValueError``."""
    return _settings_of(process_design(len(qubits), in_basis), qubits)


def _batch_arrays(design, expectations, total_counts=None):
    e = np.ascontiguousarray(expectations, dtype=np.float64)
    if e.ndim == 1:
        e = e[None, :]
    if e.ndim != 2 or e.shape[1] != design.m:
        raise ValueError(f"expectations must have shape [B, {design.m}]")
    if total_counts is None:
        return e, None
    c = np.ascontiguousarray(total_counts, dtype=np.float64)
    if c.ndim == 1:
        c = np.ascontiguousarray(np.broadcast_to(c[None, :], e.shape))
    if c.shape != e.shape:
        raise ValueError("total_counts must have the shape of expectations")
    return e, c


# ==================================================================================================
# STATE tomography
# ==================================================================================================
def linear_inv_state_estimate_batch(design: Design, expectations) -> np.ndarray:
    e, _ = _batch_arrays(design, expectations)
    d = design.dim
    out = np.empty((e.shape[0], d, d), dtype=np.complex128)
    _lib.check(_lib.lib().fbx_linv_state(design.handle, e.shape[0], _lib.dptr(e),
                                         _lib.dptr(out.view(np.float64))))
    return out


def linear_inv_state_estimate(results: List[ExperimentResult], qubits: List[int]) -> np.ndarray:
    """tomography.py:130-165."""
    design, e, _ = flatten_results(results, qubits, "state")
    return linear_inv_state_estimate_batch(design, e)[0]


def iterative_mle_state_estimate_batch(design: Design, expectations, total_counts, epsilon=.1,
                                       entropy_penalty=0.0, beta=0.0, tol=1e-9, maxiter=10_000,
                                       return_stats=False):
    if (entropy_penalty != 0.0) and (beta != 0.0):
        raise ValueError("One can't sensibly do entropy penalty and hedging. Do one or the other"
                         " but not both.")
    e, c = _batch_arrays(design, expectations, total_counts)
    B, d = e.shape[0], design.dim
    rho = np.empty((B, d, d), dtype=np.complex128)
    iters = np.zeros(B, dtype=np.int32)
    hit = np.zeros(B, dtype=np.int32)
    _lib.check(_lib.lib().fbx_mle_state(design.handle, B, _lib.dptr(e), _lib.dptr(c),
                                        float(epsilon), float(entropy_penalty), float(beta),
                                        float(tol), int(maxiter), _lib.dptr(rho.view(np.float64)),
                                        _lib.iptr(iters), _lib.iptr(hit)))
    if hit.any():
        warnings.warn('Maximum number of iterations reached before convergence.')
    if return_stats:
        return rho, {"iterations": iters, "hit_max": hit.astype(bool)}
    return rho


def iterative_mle_state_estimate(results: List[ExperimentResult], qubits: List[int], epsilon=.1,
                                 entropy_penalty=0.0, beta=0.0, tol=1e-9, maxiter=10_000) \
        -> np.ndarray:
    """tomography.py:168-270 (diluted iterative MLE; max-entropy or hedged variants)."""
    if (entropy_penalty != 0.0) and (beta != 0.0):
        raise ValueError("One can't sensibly do entropy penalty and hedging. Do one or the other"
                         " but not both.")
    design, e, c = flatten_results(results, qubits, "state")
    return iterative_mle_state_estimate_batch(design, e, c, epsilon, entropy_penalty, beta, tol,
                                              maxiter)[0]


def _R_batch(states, design: Design, expectations) -> np.ndarray:
    e, _ = _batch_arrays(design, expectations)
    d = design.dim
    rho = _lib.c128(states).reshape(-1, d, d)
    out = np.empty_like(rho)
    _lib.check(_lib.lib().fbx_r_operator(design.handle, rho.shape[0], _lib.dptr(rho.view(np.float64)),
                                         _lib.dptr(e), _lib.dptr(out.view(np.float64))))
    return out


def _R(state, results, qubits):
    """tomography.py:273-338.  NOTE: like the reference's private helper, ``qubits`` here is
    the *reversed* list the public estimators pass down (tomography.py:233,248)."""
    design, e, _ = flatten_results(results, list(qubits)[::-1], "state")
    return _R_batch(np.asarray(state)[None], design, e)[0]


def state_log_likelihood_batch(states, design: Design, expectations, total_counts) -> np.ndarray:
    e, c = _batch_arrays(design, expectations, total_counts)
    d = design.dim
    rho = _lib.c128(states).reshape(-1, d, d)
    out = np.empty(rho.shape[0])
    _lib.check(_lib.lib().fbx_state_log_likelihood(design.handle, rho.shape[0],
                                                   _lib.dptr(rho.view(np.float64)), _lib.dptr(e),
                                                   _lib.dptr(c), _lib.dptr(out)))
    return out


def state_log_likelihood(state: np.ndarray, results, qubits: Sequence[int]) -> float:
    """tomography.py:341-375 (log10 likelihood)."""
    design, e, c = flatten_results(list(results), qubits, "state")
    return float(state_log_likelihood_batch(np.asarray(state)[None], design, e, c)[0])


def _resample_expectations_with_beta(results, prior_counts=1):
    """tomography.py:378-409: one Beta-posterior redraw of every expectation, from numpy's global
    stream in result order (one vectorised ``np.random.beta`` call draws in exactly that order)."""
    e = np.array([np.real(r.expectation) for r in results], dtype=float)
    c = np.array([r.total_counts for r in results], dtype=float)
    redrawn = resample_expectations_with_beta_batch(e, c, 1, prior_counts)[0]
    return [ExperimentResult(setting=r.setting, expectation=float(x), std_err=r.std_err, total_counts=r.total_counts)
            for r, x in zip(results, redrawn)]


def resample_expectations_with_beta_batch(expectations, total_counts, n_resamples, prior_counts=1, seed=None):
    """Beta-resampled expectations, ``[n_resamples, *expectations.shape]``.

    ``seed=None``: drawn on the host from the global np.random stream in the order the reference
    draws them (resample by resample, result by result; tomography.py:391-402) -- expectations must
    then be one experiment ``[m]``.  ``seed=int``: drawn on the device by the counter-based generator
    of ``fbx_beta_resample`` (reproducible, any batch shape; same distribution, different stream)."""
    e = np.asarray(expectations, dtype=float)
    c = np.asarray(total_counts, dtype=float)
    if seed is not None:
        e = np.ascontiguousarray(e)
        c = np.ascontiguousarray(np.broadcast_to(c, e.shape))
        out = np.empty((int(n_resamples),) + e.shape)
        _lib.check(_lib.lib().fbx_beta_resample(e.size, int(n_resamples), _lib.dptr(e), _lib.dptr(c),
                                               float(prior_counts), int(seed) & (2 ** 64 - 1), _lib.dptr(out)))
        return out
    num_plus = ((e + 1) / 2) * c
    num_minus = c - num_plus
    a = np.broadcast_to(num_plus + prior_counts, (n_resamples, e.size))
    b = np.broadcast_to(num_minus + prior_counts, (n_resamples, e.size))
    return 2 * np.random.beta(a, b) - 1


_BATCHED_ESTIMATORS = {}     # filled below: reference-signature estimator -> batched implementation


def _batched_form(tomo_estimator):
    """(batched function, kwargs) when `tomo_estimator` is one of this module's state estimators
    (possibly wrapped in functools.partial), else None."""
    kwargs = {}
    f = tomo_estimator
    while isinstance(f, functools.partial):
        if f.args:
            return None
        kwargs = {**f.keywords, **kwargs}
        f = f.func
    impl = _BATCHED_ESTIMATORS.get(f)
    return (impl, kwargs) if impl is not None else None


def estimate_variance(results: List[ExperimentResult], qubits: List[int], tomo_estimator: Callable,
                      functional: Callable, target_state=None, n_resamples: int = 40,
                      project_to_physical: bool = False, seed=None) -> Tuple[float, float]:
    """tomography.py:412-453 (bootstrap error bar of a functional of the state).

    When `tomo_estimator` is one of this module's state estimators and `functional` one of
    ``dm.purity / fidelity / infidelity / trace_distance / hilbert_schmidt_ip`` the whole bootstrap
    is three batched device calls (estimate, project, measure) over the `n_resamples` resampled
    experiments -- the resamples are the batch axis; any other callables take the reference's
    one-at-a-time loop.  ``seed`` (extension): None = the reference's np.random stream, an int = the
    device generator (batched path only)."""
    from .operator_tools.project_state_matrix import (project_state_matrix_to_physical,
                                                       project_state_matrix_to_physical_batch)
    if functional != dm.purity:
        if target_state is None:
            raise ValueError("You're not using the `purity` functional. "
                             "Please specify a target state.")
    batched = _batched_form(tomo_estimator)
    measures = {dm.purity: "purity", dm.fidelity: "fidelity", dm.infidelity: "fidelity",
                dm.trace_distance: "trace_distance", dm.hilbert_schmidt_ip: "hs_ip"}
    if batched is not None and functional in measures:
        impl, kwargs = batched
        design, e, c = flatten_results(results, qubits, "state")
        e_rs = resample_expectations_with_beta_batch(e, c, n_resamples, seed=seed)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            rhos = impl(design, e_rs, np.broadcast_to(c, e_rs.shape), **kwargs)
        for w in {str(w.message) for w in caught}:
            warnings.warn(w)
        if project_to_physical:
            rhos = project_state_matrix_to_physical_batch(rhos)
        key = measures[functional]
        if functional == dm.purity:
            vals = dm.state_measures_batch(rhos, None, (key,))[key]
        else:
            tgt = np.broadcast_to(np.asarray(target_state, dtype=np.complex128), rhos.shape)
            vals = dm.state_measures_batch(np.ascontiguousarray(tgt), rhos, (key,))[key]
            if functional == dm.infidelity:
                vals = 1 - vals
        return np.mean(vals), np.var(vals)
    # opaque callables: one reconstruction per resample, through whatever the caller passed in
    def one_sample():
        rho = tomo_estimator(_resample_expectations_with_beta(results), qubits)
        if project_to_physical:
            rho = project_state_matrix_to_physical(rho)
        value = dm.purity(rho, dim_renorm=False) if functional == dm.purity else functional(target_state, rho)
        return np.real(value)

    values = np.array([one_sample() for _ in range(n_resamples)])
    return np.mean(values), np.var(values)


_BATCHED_ESTIMATORS[linear_inv_state_estimate] = lambda design, e, c: linear_inv_state_estimate_batch(design, e)
_BATCHED_ESTIMATORS[iterative_mle_state_estimate] = iterative_mle_state_estimate_batch


# ==================================================================================================
# PROCESS tomography
# ==================================================================================================
def linear_inv_process_estimate_batch(design: Design, expectations) -> np.ndarray:
    e, _ = _batch_arrays(design, expectations)
    D = design.dim ** 2
    out = np.empty((e.shape[0], D, D), dtype=np.complex128)
    _lib.check(_lib.lib().fbx_linv_process(design.handle, e.shape[0], _lib.dptr(e),
                                           _lib.dptr(out.view(np.float64))))
    return out


def linear_inv_process_estimate(results: List[ExperimentResult], qubits: List[int]) -> np.ndarray:
    """tomography.py:459-491."""
    design, e, _ = flatten_results(results, qubits, "process")
    return linear_inv_process_estimate_batch(design, e)[0]


def pgdb_process_estimate_batch(design: Design, expectations, total_counts, trace_preserving=True,
                                mode="converge", max_iters=0, return_stats=False, eig_rel_tol=None,
                                trace_iters=0, out=None, devices=None, line_search="exact"):
    """Batched pgdb_process_estimate.  ``mode='converge'`` is the reference loop (optionally
    capped by ``max_iters``); ``mode='fixed'`` runs exactly ``max_iters`` outer iterations.
    ``eig_rel_tol``: the eigensolver tolerance factor for THIS call (None = the process default,
    0 = the reference's trajectory iteration by iteration; include/fbx.h fbx_pgdb_process_ex).
    ``trace_iters`` > 0 adds ``stats['trace']`` [B, trace_iters, 2]: Dykstra iterations and halvings of
    every outer iteration.  ``out``: a C-contiguous complex128 [B, D, D] array for the result; when it and both inputs
    are page-locked (``fbx._lib.pinned_empty`` / ``pinned_copy``) the library overlaps transfers and kernels.
    ``devices``: ``'all'`` or a list of GPU ordinals -- the batch is split into contiguous blocks over those GPUs inside
    this one call (``fbx._lib.set_devices``; results are bit-identical to the single-GPU call); None keeps the process's
    current device list.
    ``line_search``: ``'exact'`` (default) tests the exact cost difference of a small step; ``'reference'`` evaluates the
    full cost at every halving and uses the reference's rounded comparison (``FBX_MODE_LS_REFERENCE``, include/fbx.h) --
    identical up to the reference's own stopping point, another rounding-driven walk past it."""
    if devices is not None:
        _lib.set_devices(devices)
    if mode not in ("converge", "fixed"):
        raise ValueError("mode must be 'converge' or 'fixed'")
    if line_search not in ("exact", "reference"):
        raise ValueError("line_search must be 'exact' or 'reference'")
    e, c = _batch_arrays(design, expectations, total_counts)
    B, D = e.shape[0], design.dim ** 2
    if out is None:
        choi = np.empty((B, D, D), dtype=np.complex128)
    else:
        if out.shape != (B, D, D) or out.dtype != np.complex128 or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous complex128 array of shape {(B, D, D)}")
        choi = out
    iters = np.zeros(B, dtype=np.int32)
    dyk = np.zeros(B, dtype=np.int32)
    bt = np.zeros(B, dtype=np.int32)
    cost = np.zeros(B)
    work = np.zeros((B, 4), dtype=np.int32)
    trace = np.zeros((B, int(trace_iters), 2), dtype=np.int32) if trace_iters > 0 else None
    _lib.check(_lib.lib().fbx_pgdb_process_ex(
        design.handle, B, _lib.dptr(e), _lib.dptr(c), int(bool(trace_preserving)),
        (_lib.MODE_FIXED if mode == "fixed" else _lib.MODE_CONVERGE) | (_lib.MODE_LS_REFERENCE if line_search == "reference" else 0),
        int(max_iters), -1.0 if eig_rel_tol is None else float(eig_rel_tol),
        _lib.dptr(choi.view(np.float64)), _lib.iptr(iters), _lib.iptr(dyk), _lib.iptr(bt),
        _lib.dptr(cost), _lib.iptr(work), _lib.iptr(trace), int(trace_iters) if trace is not None else 0))
    if return_stats:
        st = {"iterations": iters, "dykstra": dyk, "backtracks": bt, "cost": cost,
              "jacobi_sweeps": work[:, 0], "eig_terms": work[:, 1], "cost_evals": work[:, 2],
              "power_sum_passes": work[:, 3]}
        if trace is not None:
            st["trace"] = trace
        return choi, st
    return choi


def pgdb_process_estimate(results: List[ExperimentResult], qubits: List[int],
                          trace_preserving=True) -> np.ndarray:
    """tomography.py:542-594 (projected gradient descent with backtracking)."""
    design, e, c = flatten_results(results, qubits, "process")
    return pgdb_process_estimate_batch(design, e, c, trace_preserving)[0]


# --------------------------------------------------------------------------------------------------
# _extract_from_results / _cost / _grad_cost (tomography.py:494-539, :597-633) as callable functions.
# The reference's A in C^{2m x D^2} is never materialised here: the design tables stand for it.
# --------------------------------------------------------------------------------------------------
class DesignMatrix:
    """What ``_extract_from_results`` returns in the place of the reference's dense ``A``: the design tables the kernels apply
    it through (``p = A vec(E)`` is ``T = R C`` plus ``2 m`` look-ups).  ``shape`` is that of the dense matrix."""

    def __init__(self, design: Design):
        self.design = design
        self.shape = (2 * design.m, design.dim ** 4)

    def __repr__(self):
        return f"DesignMatrix({self.design.n_qubits} qubits, {self.design.m} settings; dense shape {self.shape})"


def normalised_counts(expectations, total_counts) -> np.ndarray:
    """The reference's ``n`` (tomography.py:528-538) for a batch: [B, 2 m], row 2 k / 2 k + 1 = the +1 / -1 counts of result k
    over the grand total of the experiment -- the same three floating-point operations per entry as the reference's."""
    e = np.atleast_2d(np.asarray(expectations, dtype=np.float64))
    c = np.broadcast_to(np.atleast_2d(np.asarray(total_counts, dtype=np.float64)), e.shape)
    plus = (1 + e) / 2
    n = np.empty(e.shape[:1] + (2 * e.shape[1],))
    n[:, 0::2] = c * plus
    n[:, 1::2] = c * (1 - plus)
    return n / c.sum(axis=1, keepdims=True)


def _extract_from_results(results: List[ExperimentResult], qubits: List[int]) -> Tuple[DesignMatrix, np.ndarray]:
    """tomography.py:494-539: ``(A, n)`` with ``n`` the [2 m, 1] column of normalised counts exactly as the reference builds it and
    ``A`` a :class:`DesignMatrix` (the tables that apply the reference's dense matrix)."""
    design, e, c = flatten_results(results, qubits, "process")
    return DesignMatrix(design), normalised_counts(e, c)[0][:, None]


def cost_and_gradient_batch(design: Design, n, estimates, eps=1e-6, gradient=True):
    """``(_cost, _grad_cost)`` for a batch: ``n`` [B, 2 m] (:func:`normalised_counts`), ``estimates`` [B, D, D] Hermitian Choi
    matrices; one launch of ``fbx_pgdb_cost_grad`` (the reconstruction kernels' own table products).  Returns ``cost[B]`` and
    ``grad[B, D, D]`` (None when ``gradient`` is False)."""
    design = design.design if isinstance(design, DesignMatrix) else design
    D = design.dim ** 2
    est = _lib.c128(estimates).reshape(-1, D, D)
    nv = np.ascontiguousarray(np.asarray(n, dtype=np.float64).reshape(est.shape[0], -1))
    if nv.shape[1] != 2 * design.m:
        raise ValueError(f"n must hold 2 m = {2 * design.m} normalised counts per estimate")
    cost = np.empty(est.shape[0])
    grad = np.empty_like(est) if gradient else None
    _lib.check(_lib.lib().fbx_pgdb_cost_grad(design.handle, est.shape[0], _lib.dptr(nv), _lib.dptr(est.view(np.float64)), float(eps),
                                             _lib.dptr(cost), _lib.dptr(grad.view(np.float64)) if gradient else None))
    return cost, grad


def _cost(A, n, estimate, eps=1e-6):
    """tomography.py:597-614 -- returns the reference's [1, 1] array (``-n.T @ log(p)``)."""
    return cost_and_gradient_batch(A, np.asarray(n).reshape(1, -1), np.asarray(estimate)[None], eps, gradient=False)[0].reshape(1, 1)


def _grad_cost(A, n, estimate, eps=1e-6):
    """tomography.py:617-633."""
    return cost_and_gradient_batch(A, np.asarray(n).reshape(1, -1), np.asarray(estimate)[None], eps)[1][0]


def _resampled(dev, e, c, R, seed, prior_counts):
    """Front of every bootstrap chain: upload (expectations, counts) [B, m] and draw ``R`` Beta resamples of each on the device.
    Returns the buffers of the resampled expectations and counts, [R, B, m] each, owned by the scope ``dev``."""
    d_e, d_c = dev.upload(e), dev.upload(c)
    d_er, d_cr = dev.alloc(R * e.size * 8), dev.alloc(R * e.size * 8)
    _lib.check(_lib.lib().fbx_beta_resample_dev(e.size, R, d_e.ptr, d_c.ptr, float(prior_counts), int(seed) & (2 ** 64 - 1),
                                                d_er.ptr, d_cr.ptr))
    return d_er, d_cr


def _resampled_pgdb(dev, design, e, c, R, seed, prior_counts, trace_preserving, mode, max_iters):
    """resample -> PGDB: the buffer of the [R, B, D, D] Choi matrices of the resampled process tomographies."""
    d_er, d_cr = _resampled(dev, e, c, R, seed, prior_counts)
    RB, D = R * e.shape[0], design.dim ** 2
    d_choi = dev.alloc(RB * D * D * 16)
    _lib.check(_lib.lib().fbx_pgdb_process_dev(design.handle, RB, d_er.ptr, d_cr.ptr, int(bool(trace_preserving)),
                                               _lib.MODE_FIXED if mode == "fixed" else _lib.MODE_CONVERGE, int(max_iters),
                                               d_choi.ptr, None, None, None, None, None))
    return d_choi


def _resampled_states(dev, design, e, c, R, seed, estimator, project_to_physical):
    """resample -> state estimate ("mle": the reference's defaults; "linv") -> optional physical projection: the buffer of the
    [R, B, d, d] estimates of the resampled state tomographies."""
    lib = _lib.lib()
    d_er, d_cr = _resampled(dev, e, c, R, seed, 1.0)
    RB, d = R * e.shape[0], design.dim
    d_est = dev.alloc(RB * d * d * 16)
    if estimator == "mle":
        _lib.check(lib.fbx_mle_state_dev(design.handle, RB, d_er.ptr, d_cr.ptr, .1, 0.0, 0.0, 1e-9, 10_000, d_est.ptr, None, None))
    else:
        _lib.check(lib.fbx_linv_state_dev(design.handle, RB, d_er.ptr, d_est.ptr))
    if not project_to_physical:
        return d_est
    d_phys = dev.alloc(RB * d * d * 16)
    _lib.check(lib.fbx_proj_state_physical_dev(design.n_qubits, RB, d_est.ptr, d_phys.ptr))
    return d_phys


def _bootstrap_stats(samples, return_samples):
    """(mean[B], var[B]) over the resamples of ``samples`` [R, B], and the samples themselves on request."""
    stats = samples.mean(axis=0), samples.var(axis=0)
    return stats + (samples,) if return_samples else stats


def process_fidelity_variance_batch(design: Design, expectations, total_counts, target_ptm,
                                    n_resamples: int = 40, seed: int = 0, prior_counts=1,
                                    trace_preserving=True, mode="converge", max_iters=0,
                                    return_samples=False):
    """Bootstrap error bars of the process fidelity of B process tomographies (the
    process analogue of ``estimate_variance``, tomography.py:412-453): every experiment is resampled
    ``n_resamples`` times (Beta posterior of each expectation, tomography.py:378-409), all
    ``n_resamples * B`` resampled experiments are reconstructed by PGDB in ONE launch, converted to
    Pauli transfer matrices and compared with ``target_ptm`` ([D, D] or [B, D, D]).  Everything between
    the upload of (expectations, counts) and the download of the fidelities stays in HBM.
    Returns (mean[B], var[B]) (and the [n_resamples, B] fidelities with ``return_samples``)."""
    if mode not in ("converge", "fixed"):
        raise ValueError("mode must be 'converge' or 'fixed'")
    e, c = _batch_arrays(design, expectations, total_counts)
    B, n, D = e.shape[0], design.n_qubits, design.dim ** 2
    R = int(n_resamples)
    tgt = np.asarray(target_ptm, dtype=np.complex128)
    if tgt.shape == (D, D):
        tgt = np.broadcast_to(tgt, (B, D, D))
    if tgt.shape != (B, D, D):
        raise ValueError("target_ptm must be [D, D] or [B, D, D]")
    if R < 1 or B == 0:
        raise ValueError("need n_resamples >= 1 and a non-empty batch")
    lib = _lib.lib()
    with _lib.DeviceScope() as dev:
        d_choi = _resampled_pgdb(dev, design, e, c, R, seed, prior_counts, trace_preserving, mode, max_iters)
        d_ptm = dev.alloc(R * B * D * D * 16)
        _lib.check(lib.fbx_convert_dev(_lib.REP_CHOI, _lib.REP_PAULI_LIOUVILLE, n, R * B, d_choi.ptr, 0, d_ptm.ptr))
        d_tgt = dev.upload(np.ascontiguousarray(np.broadcast_to(tgt, (R, B, D, D))))
        d_f = dev.alloc(R * B * 8)
        _lib.check(lib.fbx_process_fidelity_dev(n, R * B, d_tgt.ptr, d_ptm.ptr, None, d_f.ptr))
        _lib.synchronize()
        fid = d_f.to_array(np.float64, (R, B))
    return _bootstrap_stats(fid, return_samples)


def process_diamond_distance_variance_batch(design: Design, expectations, total_counts, target_choi,
                                            n_resamples: int = 40, seed: int = 0, prior_counts=1,
                                            trace_preserving=True, mode="converge", max_iters=0,
                                            tol=1e-7, diamond_max_iters=200, return_samples=False):
    """Bootstrap error bars of the diamond-norm distance of B process tomographies to ``target_choi`` ([D, D] or [B, D, D]):
    the diamond analogue of ``process_fidelity_variance_batch``.  Every experiment is resampled ``n_resamples`` times (Beta
    posterior, fbx_beta_resample), all ``n_resamples * B`` resampled experiments are reconstructed by PGDB in one launch and
    their diamond distances to the target solved on the device (fbx_diamond_norm, ``tol`` / ``diamond_max_iters`` as in
    ``distance_measures.diamond_norm_distance_batch``); nothing leaves HBM in between.
    Returns (mean[B], var[B]) (and the [n_resamples, B] distances with ``return_samples``)."""
    if mode not in ("converge", "fixed"):
        raise ValueError("mode must be 'converge' or 'fixed'")
    e, c = _batch_arrays(design, expectations, total_counts)
    B, n, D = e.shape[0], design.n_qubits, design.dim ** 2
    R = int(n_resamples)
    tgt = np.asarray(target_choi, dtype=np.complex128)
    if tgt.shape not in ((D, D), (B, D, D)):
        raise ValueError("target_choi must be [D, D] or [B, D, D]")
    if R < 1 or B == 0:
        raise ValueError("need n_resamples >= 1 and a non-empty batch")
    with _lib.DeviceScope() as dev:
        d_choi = _resampled_pgdb(dev, design, e, c, R, seed, prior_counts, trace_preserving, mode, max_iters)
        shared = tgt.ndim == 2
        d_tgt = dev.upload(np.ascontiguousarray(tgt if shared else np.broadcast_to(tgt, (R, B, D, D))))
        d_dist = dev.alloc(R * B * 8)
        _lib.check(_lib.lib().fbx_diamond_norm_dev(n, R * B, d_choi.ptr, d_tgt.ptr, int(shared), float(tol), int(diamond_max_iters),
                                                   d_dist.ptr, None, None, None))
        _lib.synchronize()
        dist = d_dist.to_array(np.float64, (R, B))
    return _bootstrap_stats(dist, return_samples)


def state_chernoff_variance_batch(design: Design, expectations, total_counts, target_state, n_resamples: int = 40,
                                  seed: int = 0, estimator="mle", project_to_physical=True, tol=1e-10,
                                  return_samples=False):
    """Bootstrap error bars of the quantum Chernoff bound of B state tomographies against ``target_state`` ([d, d] or
    [B, d, d]): the state analogue of ``process_diamond_distance_variance_batch``.  Every experiment is resampled
    ``n_resamples`` times (Beta posterior, fbx_beta_resample), all ``n_resamples * B`` resampled experiments are estimated in one
    launch (``estimator`` "mle": iterative MLE with the reference's defaults, "linv": linear inversion), optionally projected to
    physical states, and their Chernoff bounds to the target found on the device (fbx_chernoff_bound with the
    estimates as rho and the target as sigma, ``tol`` as in ``distance_measures.quantum_chernoff_bound_batch``); nothing leaves
    HBM in between.  Returns (mean[B], var[B]) (and the [n_resamples, B] values with ``return_samples``)."""
    if estimator not in ("mle", "linv"):
        raise ValueError("estimator must be 'mle' or 'linv'")
    e, c = _batch_arrays(design, expectations, total_counts)
    B, n, d = e.shape[0], design.n_qubits, design.dim
    R = int(n_resamples)
    tgt = np.asarray(target_state, dtype=np.complex128)
    if tgt.shape not in ((d, d), (B, d, d)):
        raise ValueError("target_state must be [d, d] or [B, d, d]")
    if R < 1 or B == 0:
        raise ValueError("need n_resamples >= 1 and a non-empty batch")
    with _lib.DeviceScope() as dev:
        d_rho = _resampled_states(dev, design, e, c, R, seed, estimator, project_to_physical)
        shared = tgt.ndim == 2
        d_tgt = dev.upload(np.ascontiguousarray(tgt if shared else np.broadcast_to(tgt, (R, B, d, d))))
        d_q = dev.alloc(R * B * 8)
        _lib.check(_lib.lib().fbx_chernoff_bound_dev(n, R * B, d_rho.ptr, d_tgt.ptr, int(shared), float(tol), 100, 1e-12, d_q.ptr,
                                                     None, None, None))
        _lib.synchronize()
        q = d_q.to_array(np.float64, (R, B))
    return _bootstrap_stats(q, return_samples)


_STATE_MEASURES = ("purity", "fidelity", "infidelity", "trace_distance", "hs_ip")


def state_measure_variance_batch(design: Design, expectations, total_counts, target_state=None, measure="fidelity",
                                 n_resamples: int = 40, seed: int = 0, estimator="mle", project_to_physical=True,
                                 return_samples=False):
    """Bootstrap error bars of a state measure of B state tomographies of 1..5 qubits: ``estimate_variance`` with the
    resamples and the experiments as one batch that never leaves HBM.  Every experiment is resampled ``n_resamples`` times (Beta
    posterior, fbx_beta_resample), all ``n_resamples * B`` resampled experiments are estimated in one launch (``estimator``
    "mle": iterative MLE with the reference's defaults, "linv": linear inversion), optionally projected to physical states
    (fbx_proj_state_physical) and measured (fbx_state_measures).  ``measure`` is "purity" (no target), "fidelity",
    "infidelity", "trace_distance" or "hs_ip" against ``target_state`` ([d, d] or [B, d, d]), the target as rho and the
    estimates as sigma like ``estimate_variance`` passes them.  Returns (mean[B], var[B]) (and the [n_resamples, B] values with
    ``return_samples``)."""
    if measure not in _STATE_MEASURES:
        raise ValueError(f"measure must be one of {_STATE_MEASURES}")
    if estimator not in ("mle", "linv"):
        raise ValueError("estimator must be 'mle' or 'linv'")
    d = design.dim
    R = int(n_resamples)
    if R < 1:
        raise ValueError("need n_resamples >= 1")
    tgt = None
    if measure != "purity":
        if target_state is None:
            raise ValueError(f"measure '{measure}' needs a target state")
        tgt = np.asarray(target_state, dtype=np.complex128)
        if tgt.ndim not in (2, 3) or tgt.shape[-2:] != (d, d):
            raise ValueError("target_state must be [d, d] or [B, d, d]")
    e, c = _batch_arrays(design, expectations, total_counts)
    B, n = e.shape[0], design.n_qubits
    if B == 0:
        raise ValueError("need a non-empty batch")
    if tgt is not None and tgt.ndim == 3 and tgt.shape[0] != B:
        raise ValueError("target_state must be [d, d] or [B, d, d]")
    with _lib.DeviceScope() as dev:
        d_est = _resampled_states(dev, design, e, c, R, seed, estimator, project_to_physical)
        d_v = dev.alloc(R * B * 8)
        key = "fidelity" if measure == "infidelity" else measure
        d_rho = d_est if tgt is None else dev.upload(np.ascontiguousarray(np.broadcast_to(tgt, (R, B, d, d))))
        outs = [d_v.ptr if k == key else None for k in ("purity", "fidelity", "trace_distance", "hs_ip")]
        _lib.check(_lib.lib().fbx_state_measures_dev(n, R * B, d_rho.ptr, d_est.ptr, *outs))
        _lib.synchronize()
        v = d_v.to_array(np.float64, (R, B))
    return _bootstrap_stats(1 - v if measure == "infidelity" else v, return_samples)


def estimate_by_qubit_groups(results, qubit_groups, kind="process", estimator="pgdb", **kwargs):
    """Tomography of several qubit groups measured in one (merged) experiment: split the results
    with ``get_results_by_qubit_groups`` (observable_estimation.py:1145-1173, the process notebook's
    per-pair loop), keep for every group the settings that belong to its tomography (observable and,
    for processes, the prepared state both inside the group), and run every set of groups that share
    a design as ONE batched call.  Returns ``{sorted group tuple: estimate}``.

    ``estimator``: 'pgdb' | 'linear_inv' for processes, 'mle' | 'linear_inv' for states; keyword
    arguments go to the batched estimator."""
    from .observable_estimation import get_results_by_qubit_groups
    if kind not in ("process", "state"):
        raise ValueError("kind must be 'process' or 'state'")
    by_group = get_results_by_qubit_groups(results, qubit_groups)
    batches = {}                                   # design key -> (design, [group], [e], [c])
    for group, res in by_group.items():
        res = [r for r in res if len(r.setting.observable.get_qubits()) > 0]
        if not res:
            raise ValueError(f"no results for qubit group {group}")
        design, e, c = flatten_results(res, list(group), kind)
        entry = batches.setdefault(design.key(), (design, [], [], []))
        entry[1].append(group); entry[2].append(e); entry[3].append(c)
    out = {}
    for design, groups, es, cs in batches.values():
        e, c = np.stack(es), np.stack(cs)
        if kind == "process":
            if estimator == "pgdb":
                est = pgdb_process_estimate_batch(design, e, c, **kwargs)
            elif estimator == "linear_inv":
                est = linear_inv_process_estimate_batch(design, e)
            else:
                raise ValueError("process estimators: 'pgdb', 'linear_inv'")
        else:
            if estimator == "mle":
                est = iterative_mle_state_estimate_batch(design, e, c, **kwargs)
            elif estimator == "linear_inv":
                est = linear_inv_state_estimate_batch(design, e)
            else:
                raise ValueError("state estimators: 'mle', 'linear_inv'")
        for g, x in zip(groups, est):
            out[g] = x
    return out


# ==================================================================================================
# SIMULATED experiments (fbx_tomo_simulate): truth -> the noisy (expectations, total_counts) the estimators above read.  The
# acquisition half of do_tomography (observable_estimation.py:856-920, a QVM in the reference) as one device call.
# ==================================================================================================
_SIM_REPS = ("pauli_liouville", "unitary", "kraus", "choi")
_SIM_ESTIMATORS = ("pgdb", "linear_inv")
MAX_SHOTS = 2 ** 32 - 1


def _sim_process_truth(design: Design, channels, rep):
    """The real Pauli transfer matrices [B, D, D] of ``channels`` given in ``rep``; shape errors are raised before the library
    is touched, the conversion itself runs on the device (``convert_batch``)."""
    if rep not in _SIM_REPS:
        raise ValueError(f"rep must be one of {_SIM_REPS}, not {rep!r}")
    if design.kind != "process":
        raise ValueError("simulate_process_tomography_batch needs a process design")
    d, D = design.dim, design.dim ** 2
    x = np.asarray(channels)
    if rep == "pauli_liouville":
        if x.ndim == 2:
            x = x[None]
        if x.ndim != 3 or x.shape[1:] != (D, D):
            raise ValueError(f"pauli_liouville channels must be [B, {D}, {D}]")
        if np.iscomplexobj(x):
            if np.any(x.imag != 0.0):
                raise ValueError("pauli_liouville channels must be real")
            x = x.real
        return np.ascontiguousarray(x, dtype=np.float64)
    if rep == "unitary":
        if x.ndim == 2:
            x = x[None]
        if x.ndim != 3 or x.shape[1:] != (d, d):
            raise ValueError(f"unitary channels must be [B, {d}, {d}]")
        x, src = x[:, None], "kraus"
    elif rep == "kraus":
        if x.ndim == 3:
            x = x[None]
        if x.ndim != 4 or x.shape[1] < 1 or x.shape[2:] != (d, d):
            raise ValueError(f"kraus channels must be [B, K, {d}, {d}]")
        src = "kraus"
    else:
        if x.ndim == 2:
            x = x[None]
        if x.ndim != 3 or x.shape[1:] != (D, D):
            raise ValueError(f"choi channels must be [B, {D}, {D}]")
        src = "choi"
    from .operator_tools.superoperator_transformations import convert_batch
    return np.ascontiguousarray(convert_batch(src, "pauli_liouville", x).real)


def _sim_state_truth(design: Design, states):
    if design.kind != "state":
        raise ValueError("simulate_state_tomography_batch needs a state design")
    d = design.dim
    x = np.asarray(states)
    if x.ndim == 2:
        x = x[None]
    if x.ndim != 3 or x.shape[1:] != (d, d):
        raise ValueError(f"states must be [B, {d}, {d}]")
    return _lib.c128(x)


def _sim_noise(B, n, shots, readout_flip, seed, first_item):
    shots, first_item = int(shots), int(first_item)
    if not 1 <= shots <= MAX_SHOTS or first_item < 0:
        raise ValueError("need 1 <= shots < 2^32 and first_item >= 0")
    flips = None
    if readout_flip is not None:
        flips = np.asarray(readout_flip, dtype=np.float64)
        if flips.shape not in ((n, 2), (B, n, 2)):
            raise ValueError(f"readout_flip must be [n, 2] = {(n, 2)} or [B, n, 2] = {(B, n, 2)}, not {flips.shape}")
        flips = np.ascontiguousarray(np.broadcast_to(flips, (B, n, 2)))
    from .operator_tools.random_operators import _stream_seed
    return shots, flips, _stream_seed(seed), first_item


def _simulate_batch(who, design, truth, shots, readout_flip, seed, first_item, return_std_errs, return_exact, return_status):
    B, m = truth.shape[0], design.m
    shots, flips, seed, first_item = _sim_noise(B, design.n_qubits, shots, readout_flip, seed, first_item)
    e, c = np.empty((B, m)), np.empty((B, m))
    se = np.empty((B, m)) if return_std_errs else None
    ex = np.empty((B, m)) if return_exact else None
    status = np.zeros(B, dtype=np.int32)
    _lib.check(_lib.lib().fbx_tomo_simulate(design.handle, B, _lib.dptr(truth.view(np.float64)), shots, _lib.dptr(flips), seed,
                                            first_item, _lib.dptr(e), _lib.dptr(c), _lib.dptr(se), _lib.dptr(ex),
                                            _lib.iptr(status)))
    if not return_status:
        bad = np.flatnonzero(status)
        if bad.size:
            b = int(bad[0])
            raise ValueError(f"{who}: item {b} (global id {first_item + b}) cannot be simulated: a truth entry that is not finite "
                             f"or a readout_flip value outside [0, 1] ({bad.size} such item(s) in the batch)")
    out = (e, c) + ((se,) if return_std_errs else ()) + ((ex,) if return_exact else ())
    return out + ((status,) if return_status else ())


def simulate_process_tomography_batch(design: Design, channels, shots, rep="pauli_liouville", readout_flip=None, seed=None,
                                      first_item=0, return_std_errs=False, return_exact=False, return_status=False):
    """B true channels measured with the settings of a process design (1..3 qubits), ``shots`` shots per setting, on the device:
    ``(expectations [B, m], total_counts [B, m][, std_errs][, exact])`` -- what ``pgdb_process_estimate_batch`` and
    ``linear_inv_process_estimate_batch`` take.

    ``channels``: Pauli transfer matrices [B, D, D] (``rep="pauli_liouville"``, the reference's convention), or ``"unitary"``
    [B, d, d], ``"kraus"`` [B, K, d, d], ``"choi"`` [B, D, D], converted by the package's conversion kernels.  ``readout_flip``
    ([n, 2] for the batch or [B, n, 2]): ``[j, 0]`` = P(read 1 | drawn 0), ``[j, 1]`` = P(read 0 | drawn 1) of qubit j,
    independent per bit; the means take them in exactly.  ``seed=None`` takes a fresh key from numpy's global stream; item b is
    global item ``first_item + b`` of the stream, which is part of the C contract (include/fbx.h) and restated on the host by
    ``synthetic.restate_tomography_counts``.  ``exact`` is the coefficient times the mean of the measured product (flips
    included), ``std_errs`` the reference's ``sqrt(var / N)``.  An item with a non-finite truth entry or a flip probability
    outside [0, 1] raises ``ValueError``; with ``return_status=True`` nothing is raised and ``status [B]`` is appended: 1 and NaN
    values for such an item, its neighbours untouched."""
    truth = _sim_process_truth(design, channels, rep)
    return _simulate_batch("simulate_process_tomography_batch", design, truth, shots, readout_flip, seed, first_item,
                           return_std_errs, return_exact, return_status)


def simulate_state_tomography_batch(design: Design, states, shots, readout_flip=None, seed=None, first_item=0,
                                    return_std_errs=False, return_exact=False, return_status=False):
    """B true density matrices [B, d, d] measured with the settings of a state design (1..5 qubits): the options and returns of
    ``simulate_process_tomography_batch``; the result is what the state estimators take."""
    truth = _sim_state_truth(design, states)
    return _simulate_batch("simulate_state_tomography_batch", design, truth, shots, readout_flip, seed, first_item,
                           return_std_errs, return_exact, return_status)


def _sim_grouping(design: Design, groups) -> Grouping:
    """``groups`` of the grouped simulators as a ``Grouping`` of ``design``: a ``Grouping``, a ``group_of [m]`` array, or a method
    name of ``design.group_design`` (grouped once, kept on the design)."""
    if isinstance(groups, Grouping):
        if groups.design is not design:
            raise ValueError("the grouping was made for another design")
        return groups
    if isinstance(groups, str):
        cache = design.__dict__.setdefault("_groupings", {})
        if groups not in cache:
            cache[groups] = group_design(design, groups)
        return cache[groups]
    return Grouping(design, groups)


def _simulate_grouped_batch(who, design, truth, shots, groups, readout_flip, seed, first_item, return_std_errs, return_exact,
                            return_probabilities, return_histograms, return_status):
    grouping = _sim_grouping(design, groups)
    B, m, cells = truth.shape[0], design.m, (grouping.n_groups, design.dim)
    shots, flips, seed, first_item = _sim_noise(B, design.n_qubits, shots, readout_flip, seed, first_item)
    e, c = np.empty((B, m)), np.empty((B, m))
    se = np.empty((B, m)) if return_std_errs else None
    ex = np.empty((B, m)) if return_exact else None
    pr = np.empty((B,) + cells) if return_probabilities else None
    hi = np.empty((B,) + cells, dtype=np.uint32) if return_histograms else None
    status = np.zeros(B, dtype=np.int32)
    _lib.check(_lib.lib().fbx_tomo_simulate_grouped(design.handle, grouping.handle, B, _lib.dptr(truth.view(np.float64)), shots,
                                                    _lib.dptr(flips), seed, first_item, _lib.dptr(e), _lib.dptr(c), _lib.dptr(se),
                                                    _lib.dptr(ex), _lib.dptr(pr), _lib.ptr(hi, C.c_uint32), _lib.iptr(status)))
    if not return_status:
        bad = np.flatnonzero(status)
        if bad.size:
            b = int(bad[0])
            raise ValueError(f"{who}: item {b} (global id {first_item + b}) cannot be simulated: a truth entry that is not finite, "
                             f"a readout_flip value outside [0, 1] or a group whose clamped outcome probabilities do not sum to a "
                             f"positive finite number ({bad.size} such item(s) in the batch)")
    out = (e, c) + tuple(x for x, on in ((se, return_std_errs), (ex, return_exact), (pr, return_probabilities),
                                         (hi, return_histograms), (status, return_status)) if on)
    return out


def simulate_grouped_process_tomography_batch(design: Design, channels, shots, groups="greedy", rep="pauli_liouville",
                                              readout_flip=None, seed=None, first_item=0, return_std_errs=False,
                                              return_exact=False, return_probabilities=False, return_histograms=False,
                                              return_status=False):
    """``simulate_process_tomography_batch`` with GROUPED settings (``fbx_tomo_simulate_grouped``): the settings of a group --
    one input state, one tensor-product basis -- are read off the same ``shots`` shots, as ``do_tomography(...,
    group_tpb_settings=True)`` acquires them, so that the results of a group are correlated the way real data are.  ``groups``: a
    ``design.Grouping``, a ``group_of [m]`` array, or a method of ``design.group_design`` ("greedy", "clique-removal"; grouped once
    and kept on the design).  Returns ``(expectations [B, m], total_counts [B, m][, std_errs][, exact][, probabilities [B, G,
    2^n]][, histograms [B, G, 2^n] uint32][, status])``: ``exact`` is bit for bit that of the ungrouped call, ``probabilities`` the
    outcome distribution of every group (bit t of an outcome = qubit n - 1 - t, 1 = eigenvalue -1; flips included),
    ``histograms`` the outcomes drawn.  The stream is part of the C contract and restated by
    ``synthetic.restate_grouped_tomography_counts``; it is not the stream of the ungrouped call under the same seed."""
    truth = _sim_process_truth(design, channels, rep)
    return _simulate_grouped_batch("simulate_grouped_process_tomography_batch", design, truth, shots, groups, readout_flip, seed,
                                   first_item, return_std_errs, return_exact, return_probabilities, return_histograms, return_status)


def simulate_grouped_state_tomography_batch(design: Design, states, shots, groups="greedy", readout_flip=None, seed=None,
                                            first_item=0, return_std_errs=False, return_exact=False, return_probabilities=False,
                                            return_histograms=False, return_status=False):
    """B true density matrices [B, d, d] measured with the grouped settings of a state design (1..5 qubits): the options and
    returns of ``simulate_grouped_process_tomography_batch``."""
    truth = _sim_state_truth(design, states)
    return _simulate_grouped_batch("simulate_grouped_state_tomography_batch", design, truth, shots, groups, readout_flip, seed,
                                   first_item, return_std_errs, return_exact, return_probabilities, return_histograms, return_status)


# --------------------------------------------------------------------------------------------------
# symmetrized readout and calibration under a joint confusion matrix (fbx_tomo_simulate_symmetrized / _calibration):
# the reference's defaults symm_type = -1 and calibrate_observables = True of do_tomography
# --------------------------------------------------------------------------------------------------
def _sim_symm_type(symm_type):
    if symm_type not in (-1, 0):
        raise ValueError("symm_type must be -1 (exhaustive symmetrization) or 0 (none); the orthogonal arrays 1, 2, 3 are not "
                         "implemented")
    return int(symm_type)


def _sim_confusion(B, n, confusion):
    """``confusion`` as [B, 2^n, 2^n] float64; a row whose (finite) sum is not 1 is refused -- ``np.allclose(row sums, 1.0)``, the
    rule of ``synthetic.readout_shots``.  A row with a non-finite sum goes on to the library, which poisons the item."""
    d = 1 << n
    c = np.asarray(confusion, dtype=np.float64)
    if c.shape not in ((d, d), (B, d, d)):
        raise ValueError(f"confusion must be [2^n, 2^n] = {(d, d)} or [B, 2^n, 2^n] = {(B, d, d)}, not {c.shape}")
    c = np.ascontiguousarray(np.broadcast_to(c, (B, d, d)))
    sums = c.sum(axis=2)
    finite = np.isfinite(sums)
    if not np.allclose(sums[finite], 1.0):
        raise ValueError("every row of the confusion matrix ([drawn][read]) must sum to 1")
    return c


def calibration_list(design: Design):
    """The readout calibrations of ``design`` (``fbx_tomo_calibration_list``): ``(cal_paulis [n_cal, n] uint8, cal_index [m]
    int32)`` -- its distinct non-identity observables in order of first appearance, and the calibration of every setting (-1 for
    an all-identity observable)."""
    n_cal = C.c_int32(0)
    idx = np.empty(design.m, dtype=np.int32)
    pidx = np.empty(design.m, dtype=np.int32)
    _lib.check(_lib.lib().fbx_tomo_calibration_list(design.handle, C.byref(n_cal), _lib.iptr(pidx),
                                                    _lib.iptr(idx)))
    n = design.n_qubits
    pidx = pidx[:n_cal.value]
    codes = np.array([[(int(p) >> (2 * (n - 1 - q))) & 3 for q in range(n)] for p in pidx], dtype=np.uint8).reshape(-1, n)
    return codes, idx


def _simulate_symmetrized_batch(who, design, truth, shots, confusion, symm_type, groups, seed, first_item, return_std_errs,
                                return_exact, return_probabilities, return_histograms, return_status):
    grouping = _sim_grouping(design, groups)
    B, m, d = truth.shape[0], design.m, design.dim
    symm_type = _sim_symm_type(symm_type)
    shots, _, seed, first_item = _sim_noise(B, design.n_qubits, shots, None, seed, first_item)
    conf = _sim_confusion(B, design.n_qubits, confusion)
    e, c = np.empty((B, m)), np.empty((B, m))
    se = np.empty((B, m)) if return_std_errs else None
    ex = np.empty((B, m)) if return_exact else None
    pr = np.empty((B, grouping.n_groups, d, d)) if return_probabilities else None
    hi = np.empty((B, grouping.n_groups, d), dtype=np.uint32) if return_histograms else None
    status = np.zeros(B, dtype=np.int32)
    _lib.check(_lib.lib().fbx_tomo_simulate_symmetrized(design.handle, grouping.handle, B, _lib.dptr(truth.view(np.float64)),
                                                        _lib.dptr(conf), symm_type, shots, seed, first_item, _lib.dptr(e),
                                                        _lib.dptr(c), _lib.dptr(se), _lib.dptr(ex), _lib.dptr(pr),
                                                        _lib.ptr(hi, C.c_uint32), _lib.iptr(status)))
    if not return_status:
        bad = np.flatnonzero(status)
        if bad.size:
            b = int(bad[0])
            raise ValueError(f"{who}: item {b} (global id {first_item + b}) cannot be simulated: a truth entry that is not finite, "
                             f"a confusion entry that is not finite or outside [0, 1], or a flip pattern whose clamped outcome "
                             f"probabilities do not sum to a positive finite number ({bad.size} such item(s) in the batch)")
    return (e, c) + tuple(x for x, on in ((se, return_std_errs), (ex, return_exact), (pr, return_probabilities),
                                          (hi, return_histograms), (status, return_status)) if on)


def simulate_symmetrized_process_tomography_batch(design: Design, channels, shots, confusion, symm_type=-1, groups="greedy",
                                                  rep="pauli_liouville", seed=None, first_item=0, return_std_errs=False,
                                                  return_exact=False, return_probabilities=False, return_histograms=False,
                                                  return_status=False):
    """``simulate_grouped_process_tomography_batch`` under a JOINT readout confusion matrix and the reference's readout
    symmetrization (``fbx_tomo_simulate_symmetrized``).  ``confusion`` ([2^n, 2^n] for the batch or [B, 2^n, 2^n]): ``[drawn,
    read]`` = the probability of reading bitstring ``read`` when ``drawn`` was drawn, index = the bitstring as a binary number
    with qubit 0 first (the layout of ``readout.joint_confusion_matrices_batch`` and ``synthetic.readout_shots``;
    ``readout.confusion_from_flips`` builds it from a ``readout_flip`` array); rows sum to 1.  ``symm_type=-1`` (the default of
    ``do_tomography``): every group is measured under every combination of pre-measurement flips of the qubits its members act
    on, the flips undone in the record, ``floor(shots / patterns)`` shots each; ``symm_type=0``: no symmetrization, the plain
    correlated readout error.  ``total_counts`` of a setting = the shots its group really drew, ``floor(shots / patterns) x
    patterns``, which can differ between the groups of one call.  ``exact`` is the mean of what is measured (matrix included),
    ``probabilities [B, G, 2^n, 2^n]`` the distribution of the un-flipped record per flip mask (a zero row for a mask that is no
    pattern of the group), ``histograms [B, G, 2^n]`` the merged record.  The stream is restated by
    ``synthetic.restate_symmetrized_tomography_counts``."""
    truth = _sim_process_truth(design, channels, rep)
    return _simulate_symmetrized_batch("simulate_symmetrized_process_tomography_batch", design, truth, shots, confusion, symm_type,
                                       groups, seed, first_item, return_std_errs, return_exact, return_probabilities,
                                       return_histograms, return_status)


def simulate_symmetrized_state_tomography_batch(design: Design, states, shots, confusion, symm_type=-1, groups="greedy", seed=None,
                                                first_item=0, return_std_errs=False, return_exact=False, return_probabilities=False,
                                                return_histograms=False, return_status=False):
    """B true density matrices [B, d, d] measured with the grouped settings of a state design (1..5 qubits) under a joint confusion
    matrix: the options and returns of ``simulate_symmetrized_process_tomography_batch``."""
    truth = _sim_state_truth(design, states)
    return _simulate_symmetrized_batch("simulate_symmetrized_state_tomography_batch", design, truth, shots, confusion, symm_type,
                                       groups, seed, first_item, return_std_errs, return_exact, return_probabilities,
                                       return_histograms, return_status)


def simulate_readout_calibration_batch(design: Design, confusion, shots, symm_type=-1, seed=None, first_item=0, batch=None,
                                       return_exact=False, return_status=False):
    """The calibration runs of ``calibrate_observable_estimates`` simulated on the device (``fbx_tomo_simulate_calibration``):
    every distinct non-identity observable of ``design`` is measured on its +1 eigenstate -- every bit drawn as 0 -- through
    ``confusion`` with the symmetrization of ``symm_type``, ``shots`` shots in all per observable.  ``confusion`` [B, 2^n, 2^n],
    or one matrix for ``batch`` items (default 1).  Returns ``(cal_means [B, n_cal], cal_vars [B, n_cal], cal_counts [B, n_cal],
    cal_index [m][, exact [B, n_cal]][, status [B]])``: what ``observable_estimation.calibrate_expectations_batch`` takes per
    item, ``cal_index`` as ``calibration_list`` gives it.  The stream is restated by
    ``synthetic.restate_readout_calibration_counts``."""
    n, d = design.n_qubits, design.dim
    c = np.asarray(confusion, dtype=np.float64)
    B = c.shape[0] if c.ndim == 3 else (1 if batch is None else int(batch))
    symm_type = _sim_symm_type(symm_type)
    shots, _, seed, first_item = _sim_noise(B, n, shots, None, seed, first_item)
    conf = _sim_confusion(B, n, c)
    cal_paulis, cal_index = calibration_list(design)
    n_cal = cal_paulis.shape[0]
    mean, var, cnt = np.empty((B, n_cal)), np.empty((B, n_cal)), np.empty((B, n_cal))
    ex = np.empty((B, n_cal)) if return_exact else None
    status = np.zeros(B, dtype=np.int32)
    _lib.check(_lib.lib().fbx_tomo_simulate_calibration(design.handle, B, _lib.dptr(conf), symm_type, shots, seed, first_item,
                                                        _lib.dptr(mean), _lib.dptr(var), _lib.dptr(ex), _lib.dptr(cnt),
                                                        _lib.iptr(status)))
    if not return_status:
        bad = np.flatnonzero(status)
        if bad.size:
            raise ValueError(f"simulate_readout_calibration_batch: item {int(bad[0])} (global id {first_item + int(bad[0])}) cannot "
                             f"be simulated: a confusion entry that is not finite or outside [0, 1], or a flip pattern whose "
                             f"probabilities do not sum to a positive finite number ({bad.size} such item(s) in the batch)")
    return (mean, var, cnt, cal_index) + ((ex,) if return_exact else ()) + ((status,) if return_status else ())


def _flat_cal_index(cal_index, B, n_cal):
    """[B m] int32: the calibration of (item, setting) among the B n_cal calibrations of a batch laid out [B][n_cal]"""
    if np.any(cal_index < 0):
        raise ValueError("a design with an all-identity observable cannot be calibrated here: it has no calibration run")
    return np.ascontiguousarray((np.arange(B, dtype=np.int64)[:, None] * n_cal + cal_index[None, :]).reshape(-1), dtype=np.int32)


def simulate_tomography_results(qubits, kind, truth, shots, in_basis="pauli", group_tpb_settings=False, confusion=None,
                                symm_type=0, calibrate_observables=False, calibration_shots=None,
                                **kw) -> List[ExperimentResult]:
    """One simulated experiment as the ``List[ExperimentResult]`` the reference-signature estimators and ``estimate_dfe`` read:
    the stand-in for the acquisition half of ``do_tomography``.  ``kind`` "process" (``truth`` a channel, ``rep`` and the other
    options of ``simulate_process_tomography_batch`` by keyword; settings of ``generate_process_tomography_settings(qubits,
    in_basis)``) or "state" (``truth`` a density matrix; ``generate_state_tomography_settings(qubits)``).
    ``group_tpb_settings=True`` (the default of ``do_tomography``; not here) takes the settings of a greedy group from the same
    shots (``simulate_grouped_*_tomography_batch``); the results come back in the order of the settings either way.
    ``confusion`` (a joint [2^n, 2^n] matrix) measures through ``simulate_symmetrized_*_tomography_batch`` with ``symm_type``
    (0 here; ``do_tomography`` has -1) instead of ``readout_flip``, every setting a group of its own unless
    ``group_tpb_settings``; ``calibrate_observables=True`` adds the calibration runs (``calibration_shots``, default ``shots``;
    ``simulate_readout_calibration_batch``) and fills ``raw_expectation``, ``raw_std_err`` and the ``calibration_*`` fields through
    ``calibrate_observable_estimates_from_moments``.  Without these options nothing changes."""
    qubits = list(qubits)
    if kind not in ("process", "state"):
        raise ValueError("kind must be 'process' or 'state'")
    for name in ("return_std_errs", "return_exact", "return_status", "first_item"):
        if name in kw:
            raise ValueError(f"simulate_tomography_results does not take {name}")
    if confusion is not None or calibrate_observables:
        if kw.get("readout_flip") is not None:
            raise ValueError("give the readout error as confusion (readout.confusion_from_flips), not as readout_flip")
        kw.pop("readout_flip", None)
        design = process_design(len(qubits), in_basis) if kind == "process" else state_design(len(qubits))
        conf = np.eye(design.dim) if confusion is None else np.asarray(confusion, dtype=np.float64)
        if conf.shape != (design.dim, design.dim):
            raise ValueError(f"confusion must be one [2^n, 2^n] = {(design.dim, design.dim)} matrix")
        from .operator_tools.random_operators import _stream_seed
        seed = _stream_seed(kw.pop("seed", None))              # one key for the measurement and the calibration runs
        groups = kw.pop("groups", "greedy" if group_tpb_settings else np.arange(design.m))
        simulate = simulate_symmetrized_process_tomography_batch if kind == "process" else simulate_symmetrized_state_tomography_batch
        e, c, se = simulate(design, truth, shots, conf, symm_type=symm_type, groups=groups, seed=seed, return_std_errs=True, **kw)
        if e.shape[0] != 1:
            raise ValueError("simulate_tomography_results covers one experiment: pass one channel or state")
        settings = _settings_of(design, qubits)
        results = [ExperimentResult(setting=s, expectation=float(x), total_counts=int(n), std_err=float(v))
                   for s, x, n, v in zip(settings, e[0], c[0], se[0])]
        if not calibrate_observables:
            return results
        from .observable_estimation import calibrate_observable_estimates_from_moments, operations_as_set
        means, variances, counts, index = simulate_readout_calibration_batch(
            design, conf, shots if calibration_shots is None else calibration_shots, symm_type=symm_type, seed=seed)
        if np.any(index < 0):
            raise ValueError("a design with an all-identity observable cannot be calibrated here: it has no calibration run")
        calibrations = {operations_as_set(s.observable): (float(means[0, i]), float(variances[0, i]), int(counts[0, i]))
                        for s, i in zip(settings, index)}
        return calibrate_observable_estimates_from_moments(results, calibrations)
    if kind == "process":
        design = process_design(len(qubits), in_basis)
        simulate = simulate_grouped_process_tomography_batch if group_tpb_settings else simulate_process_tomography_batch
    else:
        design = state_design(len(qubits))
        simulate = simulate_grouped_state_tomography_batch if group_tpb_settings else simulate_state_tomography_batch
    e, c, se = simulate(design, truth, shots, return_std_errs=True, **kw)
    if e.shape[0] != 1:
        raise ValueError("simulate_tomography_results covers one experiment: pass one channel or state")
    return [ExperimentResult(setting=s, expectation=float(x), total_counts=int(n), std_err=float(v))
            for s, x, n, v in zip(_settings_of(design, qubits), e[0], c[0], se[0])]


def simulate_and_estimate_process_batch(design: Design, channels, shots, rep="pauli_liouville", readout_flip=None, seed=None,
                                        first_item=0, estimator="pgdb", groups=None, confusion=None, symm_type=-1, calibrate=True,
                                        calibration_shots=None, **estimator_kw):
    """The resident loop truth -> shots -> estimate -> fidelity to truth: the truth's transfer matrices are uploaded once,
    ``fbx_tomo_simulate_dev`` writes (expectations, counts) into HBM, the estimator's ``_dev`` form (``estimator`` "pgdb":
    ``trace_preserving``, ``mode``, ``max_iters`` by keyword as in ``pgdb_process_estimate_batch``; "linear_inv": no options)
    reconstructs from them, and the Choi matrices go through Choi -> Pauli-Liouville into ``fbx_process_fidelity_dev`` against
    the truth.  Returns ``(chois [B, D, D], fidelity_to_truth [B])`` -- all that leaves the device; bit for bit what
    ``simulate_process_tomography_batch``, the batched estimator and ``distance_measures.process_fidelity_batch`` give when
    composed through the host.  ``groups`` (a ``Grouping``, a ``group_of`` array or a method name, as in
    ``simulate_grouped_process_tomography_batch``): ``fbx_tomo_simulate_grouped_dev`` draws the shots instead, one set per group.
    ``confusion`` (a joint matrix [2^n, 2^n] or [B, 2^n, 2^n], instead of ``readout_flip``; ``groups`` defaults to "greedy"): the
    chain becomes ``fbx_tomo_simulate_symmetrized_dev`` (``symm_type``) -> with ``calibrate``, ``fbx_tomo_simulate_calibration_dev``
    (``calibration_shots``, default ``shots``; the same seed) and ``fbx_calibrate_expectations_dev`` with the calibration of every
    (item, setting) -> the estimator -> the fidelity, resident as before and bit for bit what
    ``simulate_symmetrized_process_tomography_batch``, ``simulate_readout_calibration_batch``,
    ``observable_estimation.calibrate_expectations_batch`` and the estimator give when composed through the host."""
    if estimator not in _SIM_ESTIMATORS:
        raise ValueError(f"estimator must be one of {_SIM_ESTIMATORS}, not {estimator!r}")
    allowed = {"trace_preserving", "mode", "max_iters"} if estimator == "pgdb" else set()
    if set(estimator_kw) - allowed:
        raise ValueError(f"estimator {estimator!r} does not take {sorted(set(estimator_kw) - allowed)}")
    mode = estimator_kw.get("mode", "converge")
    if mode not in ("converge", "fixed"):
        raise ValueError("mode must be 'converge' or 'fixed'")
    truth = _sim_process_truth(design, channels, rep)
    if confusion is not None and groups is None:
        groups = "greedy"
    grouping = None if groups is None else _sim_grouping(design, groups)
    B, m, n, D = truth.shape[0], design.m, design.n_qubits, design.dim ** 2
    shots, flips, seed, first_item = _sim_noise(B, n, shots, readout_flip, seed, first_item)
    if B == 0:
        raise ValueError("need a non-empty batch")
    lib = _lib.lib()
    if confusion is not None:
        if flips is not None:
            raise ValueError("give the readout error as confusion (readout.confusion_from_flips) or as readout_flip, not both")
        symm_type = _sim_symm_type(symm_type)
        conf = _sim_confusion(B, n, confusion)
        cal_shots = _sim_noise(B, n, shots if calibration_shots is None else calibration_shots, None, seed, first_item)[0]
        if calibrate:
            cal_paulis, cal_index = calibration_list(design)
            n_cal = cal_paulis.shape[0]
            flat_index = _flat_cal_index(cal_index, B, n_cal)
    with _lib.DeviceScope() as dev:
        d_truth, d_truth_c = dev.upload(truth), dev.upload(truth.astype(np.complex128))
        d_flips = dev.upload(flips)
        d_e, d_c, d_status = dev.alloc(B * m * 8), dev.alloc(B * m * 8), dev.alloc(B * 4)
        d_choi, d_ptm, d_f = dev.alloc(B * D * D * 16), dev.alloc(B * D * D * 16), dev.alloc(B * 8)
        if confusion is not None:
            d_conf, d_se = dev.upload(conf), dev.alloc(B * m * 8)
            _lib.check(lib.fbx_tomo_simulate_symmetrized_dev(design.handle, grouping.handle, B, d_truth.ptr, d_conf.ptr, symm_type,
                                                             shots, seed, first_item, d_e.ptr, d_c.ptr, d_se.ptr, None, None, None,
                                                             d_status.ptr))
            if calibrate:
                d_cm, d_cv, d_ci = dev.alloc(B * n_cal * 8), dev.alloc(B * n_cal * 8), dev.upload(flat_index)
                d_e2, d_se2, d_cst = dev.alloc(B * m * 8), dev.alloc(B * m * 8), dev.alloc(B * 4)
                _lib.check(lib.fbx_tomo_simulate_calibration_dev(design.handle, B, d_conf.ptr, symm_type, cal_shots, seed, first_item,
                                                                 d_cm.ptr, d_cv.ptr, None, None, d_cst.ptr))
                # every (item, setting) has the calibration of its item: one "experiment" of B m settings and B n_cal calibrations
                _lib.check(lib.fbx_calibrate_expectations_dev(1, B * m, d_e.ptr, d_se.ptr, d_ci.ptr, B * n_cal, d_cm.ptr, d_cv.ptr,
                                                              d_e2.ptr, d_se2.ptr))
                d_e = d_e2
        elif grouping is None:
            _lib.check(lib.fbx_tomo_simulate_dev(design.handle, B, d_truth.ptr, shots, _lib.devptr(d_flips), seed,
                                                 first_item, d_e.ptr, d_c.ptr, None, None, d_status.ptr))
        else:
            _lib.check(lib.fbx_tomo_simulate_grouped_dev(design.handle, grouping.handle, B, d_truth.ptr, shots,
                                                         _lib.devptr(d_flips), seed, first_item, d_e.ptr, d_c.ptr,
                                                         None, None, None, None, d_status.ptr))
        if estimator == "pgdb":
            _lib.check(lib.fbx_pgdb_process_dev(design.handle, B, d_e.ptr, d_c.ptr,
                                                int(bool(estimator_kw.get("trace_preserving", True))),
                                                _lib.MODE_FIXED if mode == "fixed" else _lib.MODE_CONVERGE,
                                                int(estimator_kw.get("max_iters", 0)), d_choi.ptr, None, None, None, None, None))
        else:
            _lib.check(lib.fbx_linv_process_dev(design.handle, B, d_e.ptr, d_choi.ptr))
        _lib.check(lib.fbx_convert_dev(_lib.REP_CHOI, _lib.REP_PAULI_LIOUVILLE, n, B, d_choi.ptr, 0, d_ptm.ptr))
        _lib.check(lib.fbx_process_fidelity_dev(n, B, d_truth_c.ptr, d_ptm.ptr, None, d_f.ptr))
        _lib.synchronize()
        status = d_status.to_array(np.int32, (B,))
        if confusion is not None and calibrate:
            status |= d_cst.to_array(np.int32, (B,))
        choi = d_choi.to_array(np.complex128, (B, D, D))
        fid = d_f.to_array(np.float64, (B,))
    bad = np.flatnonzero(status)
    if bad.size:
        raise ValueError(f"simulate_and_estimate_process_batch: item {int(bad[0])} cannot be simulated: a truth entry that is not "
                         f"finite or a readout_flip value or confusion entry outside [0, 1]" + (" or outcome probabilities of a group that do not sum "
                         f"to a positive finite number" if grouping is not None else "") + f" ({bad.size} such item(s) in the batch)")
    return choi, fid
