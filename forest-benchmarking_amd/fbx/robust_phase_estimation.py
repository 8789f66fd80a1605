"""Robust phase estimation (forest/benchmarking/robust_phase_estimation.py) without the acquisition: from the moments, or the
measured bits, of an RPE experiment to phases and their error bars.

What runs where:
  * ``estimate_phase_from_moments`` / ``robust_phase_estimate`` (the reference's signatures) and ``estimate_phase_from_moments_batch``
    -- ``fbx_rpe_phase``: the reference's recursion (:377-404) for B estimates in one launch, one estimate per GPU lane;
  * ``robust_phase_estimate_from_shots_batch`` -- ``fbx_rpe_from_shots``: the same estimate straight from the ``[B, K, shots, qubits]``
    bit arrays of the X and the Y basis, one wavefront per estimate;
  * ``phase_variance_batch`` -- bootstrap error bars: ``fbx_beta_resample_dev`` -> ``fbx_rpe_phase_dev`` -> ``fbx_circular_stats_dev``
    without a copy in between; ``circular_stats`` is the last step on its own;
  * ``simulate_rpe_batch`` / ``simulate_rpe_results`` / ``simulate_and_estimate_rpe_batch`` -- ``fbx_rpe_simulate``: the
    acquisition, simulated.  The gate is a Pauli transfer matrix (noise included), depth 2^j is j squarings, the shots are Philox
    draws from the exact outcome distributions with the readout flips folded in; the last one feeds ``fbx_rpe_phase_dev`` without
    a copy in between;
  * ``num_trials``, ``get_additive_error_factor``, ``_p_max``, ``_xci``, ``get_variance_upper_bound``,
    ``bloch_rotation_to_eigenvectors``, ``get_change_of_basis_from_eigvecs``, ``all_eigenvector_prep_meas_settings``,
    ``pick_two_eigenvecs_prep_meas_settings`` (a change of basis is a unitary matrix here, not a ``Program``) -- host arithmetic.

There is no host fallback for the estimates or the simulation: without a GPU they raise ``FbxError(FBX_ERR_NO_DEVICE)``.
``generate_rpe_experiments``, ``acquire_rpe_data``, ``do_rpe``, ``change_of_basis_matrix_to_quil`` (pyquil ``Program`` /
``QuantumComputer``) and ``plot_rpe_iterations`` are not mirrored.
"""
import warnings
from typing import List, Optional, Sequence, Union

import numpy as np
from numpy import pi

__all__ = ["get_additive_error_factor", "num_trials", "get_variance_upper_bound", "bloch_rotation_to_eigenvectors",
           "get_change_of_basis_from_eigvecs", "estimate_phase_from_moments", "robust_phase_estimate",
           "estimate_phase_from_moments_batch", "robust_phase_estimate_from_shots_batch", "phase_variance_batch", "circular_stats",
           "all_eigenvector_prep_meas_settings", "pick_two_eigenvecs_prep_meas_settings", "rpe_shot_schedule",
           "simulate_rpe_batch", "simulate_rpe_results", "simulate_and_estimate_rpe_batch"]

MAX_DEPTHS = 62
_WARNING = ("Decoherence limited estimate of phase {0:.3f} to depth {1:d}. You may want to increase the additive_error and/or "
            "multiplicative_factor and try again.")


# ------------------------------------------------------------------------------------------------ experiment design (host)
def bloch_rotation_to_eigenvectors(theta: float, phi: float) -> Sequence[np.ndarray]:
    """robust_phase_estimation.py:23-40: the two eigenvectors (column vectors) of a one-qubit rotation about the Bloch vector with
    azimuthal angle ``theta`` and polar angle ``phi``, ordered so that the right-hand rule gives a positive phase."""
    def ket(t, p):
        return np.array([[np.cos(t / 2), np.exp(1j * p) * np.sin(t / 2)]]).T
    return ket(theta, phi), ket(pi - theta, pi + phi)


def get_change_of_basis_from_eigvecs(eigenvectors: Sequence[np.ndarray]) -> np.ndarray:
    """robust_phase_estimation.py:43-79: the unitary that sends computational basis state i to ``eigenvectors[i]`` (lists, 1-d arrays,
    row or column vectors are accepted)."""
    n = len(eigenvectors)
    assert n > 1 and n & (n - 1) == 0, "Specification of all dim-many eigenvectors is required."
    columns = []
    for vec in eigenvectors:
        vec = np.asarray(vec)
        columns.append(vec.reshape(max(vec.shape), 1))
    dim = columns[0].shape[0]
    basis = np.eye(dim)
    return sum(np.kron(col, basis[i][np.newaxis]) for i, col in enumerate(columns))


def get_additive_error_factor(M_j: float, max_additive_error: float) -> float:
    """robust_phase_estimation.py:217-231, Eq. V.17 of Kimmel et al. (arXiv:1502.02677): the factor on the number of trials of
    iteration j that keeps Heisenberg scaling under an additive error of at most ``max_additive_error`` (< 1 / sqrt(8))."""
    slack = 1 - np.sqrt(8) * max_additive_error
    return np.log(.5 * slack ** (1 / M_j)) / np.log(1 - .5 * slack ** 2)


def num_trials(depth, max_depth, multiplicative_factor: float = 1.0, additive_error: Optional[float] = None,
               alpha: float = 5 / 2, beta: float = 1 / 2) -> int:
    """robust_phase_estimation.py:234-257, Eqs. V.11 and V.17: the number of shots of the program of this depth."""
    iteration, last_iteration = np.log2(depth) + 1, np.log2(max_depth) + 1     # depth 2^(j - 1) belongs to iteration j of K
    shots = alpha * (last_iteration - iteration) + beta
    factor = multiplicative_factor
    if additive_error:
        factor = factor * get_additive_error_factor(shots, additive_error)
    return int(np.ceil(shots * factor))


def _p_max(M_j: int) -> float:
    """robust_phase_estimation.py:315-323, Eq. V.6: bound on the probability of an error at an iteration of M_j shots"""
    return (1 / np.sqrt(2 * pi * M_j)) * (2 ** -M_j)


def _xci(h: int) -> float:
    """robust_phase_estimation.py:326-334, Eq. V.7: the largest error of the estimate when the first error happens at iteration h"""
    return 2 * pi / (2 ** h)


def get_variance_upper_bound(num_depths: int, multiplicative_factor: float = 1.0, additive_error: Optional[float] = None) -> float:
    """robust_phase_estimation.py:337-358, Eq. V.9: an upper bound on the variance of the estimate of a ``num_depths`` experiment
    run with the shot schedule of ``num_trials``: no error in any iteration, or the first error at iteration i."""
    deepest = 2 ** (num_depths - 1)
    schedule = [num_trials(2 ** i, deepest, multiplicative_factor, additive_error) for i in range(num_depths)]
    no_error = (1 - _p_max(schedule[-1])) * _xci(num_depths + 1) ** 2
    first_error_at = sum(_xci(i + 1) ** 2 * _p_max(shots) for i, shots in enumerate(schedule))
    return no_error + first_error_at


# ------------------------------------------------------------------------------------------------ estimates (device)
def _moment_arrays(arrays, names):
    out = []
    shape = None
    for a, name in zip(arrays, names):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim != 2:
            raise ValueError(f"{name} must be [B, K]")
        if shape is None:
            shape = a.shape
        if a.shape != shape:
            raise ValueError(f"{name} must have the shape of x, {shape}, not {a.shape}")
        out.append(a)
    if shape[1] < 1:
        raise ValueError("need at least one depth")
    return out, shape


def _phase_outputs(B, K, phase, depth, bloch):
    return (np.empty(B) if phase else None, np.empty(B, dtype=np.int32) if depth else None,
            np.empty((B, K, 2)) if bloch else None)


def estimate_phase_from_moments_batch(x, y, x_err, y_err, xz=None, yz=None, xz_err=None, yz_err=None, post_select: int = 0,
                                      errors_are_variances: bool = False, return_stats: bool = False):
    """B phase estimates in one launch (``fbx_rpe_phase``): ``x, y, x_err, y_err`` are ``[B, K]``, the expectations of X and Y at depth
    2^j, j < K <= 62, and the standard errors of those means (their variances with ``errors_are_variances``).  With the partner
    arrays ``xz, yz, xz_err, yz_err`` (all four) the recursion runs on ``x + xz`` (``post_select=0``) or ``x - xz`` (``1``) with the
    errors added in quadrature, the post-selection of ``robust_phase_estimate``.  Returns the phases ``[B]`` in [0, 2 pi); with
    ``return_stats`` also a dict of ``depth_reached [B]`` (int32, K when never cut short) and ``bloch [B, K, 2]`` (the reference's
    ``bloch_data``: radius and angle per iteration, NaN beyond the cut)."""
    partners = (xz, yz, xz_err, yz_err)
    given = [p is not None for p in partners]
    if any(given) and not all(given):
        raise ValueError("xz, yz, xz_err and yz_err come together or not at all")
    if post_select not in (0, 1):
        raise ValueError("post_select must be 0 or 1")
    arrays, (B, K) = _moment_arrays((x, y, x_err, y_err) + (partners if all(given) else ()),
                                    ("x", "y", "x_err", "y_err", "xz", "yz", "xz_err", "yz_err"))
    from . import _lib
    phase, depth, bloch = _phase_outputs(B, K, True, return_stats, return_stats)
    ptrs = [_lib.dptr(a) for a in arrays] + [None] * (8 - len(arrays))
    _lib.check(_lib.lib().fbx_rpe_phase(B, K, ptrs[0], ptrs[1], ptrs[2], ptrs[3], int(bool(errors_are_variances)), ptrs[4], ptrs[5],
                                        ptrs[6], ptrs[7], int(post_select), _lib.dptr(phase), _lib.iptr(depth), _lib.dptr(bloch)))
    return (phase, {"depth_reached": depth, "bloch": bloch}) if return_stats else phase


def _warn_cut(phase, depth_reached):
    warnings.warn(_WARNING.format(phase, (2 ** int(depth_reached)) // 2))


def estimate_phase_from_moments(xs: List, ys: List, x_stds: List, y_stds: List, bloch_data: Optional[List] = None) -> float:
    """robust_phase_estimation.py:361-404 with the reference's signature, computed on the device: the phase in [0, 2 pi) from the
    X / Y expectations at depths 1, 2, 4, ... and their standard errors.  ``bloch_data``, when given, is extended by the (radius, angle)
    of every iteration used.  An estimate cut short by decoherence warns with the reference's text."""
    K = min(len(xs), len(ys), len(x_stds), len(y_stds))             # zip semantics
    if K == 0:
        return 0.0
    rows = [np.asarray(list(v)[:K], dtype=np.float64)[None] for v in (xs, ys, x_stds, y_stds)]
    phase, stats = estimate_phase_from_moments_batch(*rows, return_stats=True)
    used = int(stats["depth_reached"][0])
    if used < K and not np.isnan(phase[0]):
        _warn_cut(phase[0], used)
    if bloch_data is not None:
        bloch_data.extend((float(r), float(a)) for r, a in stats["bloch"][0, :used])
    return float(phase[0])


def _is_z_eigenstate(state, index, qubit) -> bool:
    return (getattr(state, "label", None), getattr(state, "index", None), getattr(state, "qubit", None)) == ("Z", index, qubit)


def _phase_inputs(results, qubits):
    """The selection of robust_phase_estimate (:426-521): one (x, y, x_err, y_err) tuple of sequences per relative phase, in the
    reference's order."""
    if len(qubits) == 1:
        q = qubits[0]
        flat = [res for depth in results for res in depth]
        xr = [res for res in flat if res.setting.observable[q] == 'X']
        yr = [res for res in flat if res.setting.observable[q] == 'Y']
        return [([r.expectation for r in xr], [r.expectation for r in yr], [r.std_err for r in xr], [r.std_err for r in yr])]
    inputs = []
    for xy_q in qubits:
        z_qubits = [q for q in qubits if q != xy_q]
        per_label = []                                     # 'X' then 'Y': (expectation sequences, std_err sequences)
        for label in ('X', 'Y'):
            with_z = {q: [] for q in z_qubits}            # results that carry a Z, by the (first) qubit that carries it
            alone = []                                     # results with only the X / Y on xy_q
            for depth in results:
                hits = [res for res in depth if res.setting.observable[xy_q] == label]
                if not hits:
                    break
                for res in hits:
                    z_q = next((q for q in z_qubits if res.setting.observable[q] == 'Z'), None)
                    (alone if z_q is None else with_z[z_q]).append(res)
            if not alone:
                break                                      # this qubit's rotation was not measured
            exps, errs = [], []
            if max(len(v) for v in with_z.values()) == 0:
                exps.append([res.expectation for res in alone])
                errs.append([res.std_err for res in alone])
            else:
                for q, partners in with_z.items():
                    in_state = alone[0].setting.in_state[q]
                    for post_select_state in (0, 1):
                        if _is_z_eigenstate(in_state, 1 - post_select_state, q):
                            continue                       # q was prepared in the orthogonal state: nothing to select
                        sign = 1 if post_select_state == 0 else -1
                        exps.append([i_res.expectation + res.expectation if sign > 0 else i_res.expectation - res.expectation
                                     for res, i_res in zip(partners, alone)])
                        errs.append([np.sqrt(res.std_err ** 2 + i_res.std_err ** 2) for res, i_res in zip(partners, alone)])
            per_label.append((exps, errs))
        if not per_label:
            continue
        (x_exps, x_errs), (y_exps, y_errs) = per_label    # (an X without its Y is an error, as in the reference)
        inputs.extend(zip(x_exps, y_exps, x_errs, y_errs))
    return inputs


def robust_phase_estimate(results, qubits: Sequence[int]) -> Union[float, Sequence[float]]:
    """robust_phase_estimation.py:407-521 with the reference's signature: ``results`` is the list over depths of lists of
    ``ExperimentResult``.  One qubit: the phase, a float.  Several: a list with one phase per choice of X / Y qubit, Z partner and
    post-selection state that the settings allow (an explicitly orthogonal in-state is skipped), in the reference's order.  The
    selection runs on the host; all phases of the call are estimated in one launch."""
    qubits = list(qubits)
    inputs = _phase_inputs(results, qubits)
    lengths = [min(len(s) for s in item) for item in inputs]
    K = max(lengths, default=0)
    phases = [0.0] * len(inputs)
    if K > 0:
        # shorter items are padded with moments that end them (r = 0 < r_std = 1): the padding is never used
        x, y = np.zeros((len(inputs), K)), np.zeros((len(inputs), K))
        xe, ye = np.ones((len(inputs), K)), np.ones((len(inputs), K))
        for b, (item, n) in enumerate(zip(inputs, lengths)):
            for dst, src in zip((x, y, xe, ye), item):
                dst[b, :n] = np.asarray(list(src)[:n], dtype=np.float64)
        got, stats = estimate_phase_from_moments_batch(x, y, xe, ye, return_stats=True)
        for b, n in enumerate(lengths):
            phases[b] = float(got[b])
            if stats["depth_reached"][b] < n and not np.isnan(got[b]):
                _warn_cut(got[b], stats["depth_reached"][b])
    return phases[0] if len(qubits) == 1 else phases


def robust_phase_estimate_from_shots_batch(x_bits, y_bits, col: int, zcol: Optional[int] = None, post_select: int = 0,
                                           return_stats: bool = False):
    """B phase estimates straight from measured bits (``fbx_rpe_from_shots``): ``x_bits`` and ``y_bits`` are ``[B, K, shots, qubits]``
    0 / 1 arrays as ``qc.run`` returns them, measured in the X and in the Y basis at depth 2^j; ``col`` is the column of the rotated
    qubit, ``zcol`` the column of a partner measured in Z (``None``: no post-selection), ``post_select`` the partner's selected
    state.  1..8 qubits; the number of shots is the same at every depth.  Returns the phases ``[B]``; with ``return_stats`` also a
    dict of ``depth_reached``, ``bloch`` (as ``estimate_phase_from_moments_batch``) and ``moments [B, K, 4]`` = (x, y, x_err, y_err)
    as the recursion consumed them."""
    xb, yb = np.asarray(x_bits), np.asarray(y_bits)
    if xb.ndim != 4 or xb.shape != yb.shape:
        raise ValueError("x_bits and y_bits must be [B, K, shots, qubits] arrays of one shape")
    B, K, shots, n = xb.shape
    if K < 1 or shots < 1:
        raise ValueError("need at least one depth and one shot")
    if not 1 <= n <= 8:
        raise ValueError("records of 1..8 qubits are supported")
    zc = -1 if zcol is None else int(zcol)
    if not 0 <= int(col) < n or not -1 <= zc < n or zc == int(col):
        raise ValueError("col must be a column of the record and zcol another one (or None)")
    if post_select not in (0, 1):
        raise ValueError("post_select must be 0 or 1")
    for bits in (xb, yb):
        if bits.size and (bits.min() < 0 or bits.max() > 1):
            raise ValueError("the bit arrays must hold 0 / 1")
    xb, yb = np.ascontiguousarray(xb, dtype=np.uint8), np.ascontiguousarray(yb, dtype=np.uint8)
    from . import _lib
    import ctypes as C
    u8 = C.POINTER(C.c_uint8)
    phase, depth, bloch = _phase_outputs(B, K, True, return_stats, return_stats)
    moments = np.empty((B, K, 4)) if return_stats else None
    _lib.check(_lib.lib().fbx_rpe_from_shots(n, B, K, shots, xb.ctypes.data_as(u8), yb.ctypes.data_as(u8), int(col), zc,
                                             int(post_select), _lib.dptr(phase), _lib.iptr(depth), _lib.dptr(bloch),
                                             _lib.dptr(moments)))
    return (phase, {"depth_reached": depth, "bloch": bloch, "moments": moments}) if return_stats else phase


def circular_stats(angles):
    """``fbx_circular_stats`` of ``angles [R, B]`` over R: (circular mean ``[B]`` in [0, 2 pi), circular standard deviation ``[B]`` =
    sqrt(-2 ln Rbar), number of NaN entries ``[B]``, which are skipped)."""
    a = np.ascontiguousarray(angles, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("angles must be [R, B]")
    R, B = a.shape
    from . import _lib
    mean, std, skipped = np.empty(B), np.empty(B), np.empty(B, dtype=np.int32)
    _lib.check(_lib.lib().fbx_circular_stats(R, B, _lib.dptr(a), _lib.dptr(mean), _lib.dptr(std), _lib.iptr(skipped)))
    return mean, std, skipped


def phase_variance_batch(x, y, x_err, y_err, num_shots, n_resamples: int = 200, seed: int = 0, prior_counts: float = 1.0,
                         return_samples: bool = False):
    """Bootstrap error bars of B phase estimates, resident on the device: every expectation is redrawn ``n_resamples`` times from
    its Beta posterior (``fbx_beta_resample_dev``, ``num_shots`` -- a number or ``[B, K]`` -- counts behind each expectation), the
    recursion runs on all ``B * n_resamples`` redrawn experiments in one launch with the errors held at ``x_err, y_err``
    (``fbx_rpe_phase_dev``), and the phases of an item are reduced to their circular mean and standard deviation
    (``fbx_circular_stats_dev``); nothing is copied in between.  Every item is redrawn from the same counter-based streams
    (keyed by seed, resample and depth), so an item's result depends on its own moments and the seed only, not on the batch or
    its place in it.  Returns (circular mean ``[B]``, circular variance estimate ``std**2 [B]``, number of NaN resamples ``[B]``),
    and the ``[B, n_resamples]`` phases with ``return_samples``."""
    (x, y, xe, ye), (B, K) = _moment_arrays((x, y, x_err, y_err), ("x", "y", "x_err", "y_err"))
    R = int(n_resamples)
    if R < 1 or B == 0:
        raise ValueError("need n_resamples >= 1 and a non-empty batch")
    counts = np.ascontiguousarray(np.broadcast_to(np.asarray(num_shots, dtype=np.float64), (B, K)))
    if not np.all(counts > 0):
        raise ValueError("num_shots must be positive")
    if not prior_counts > 0:
        raise ValueError("prior_counts must be positive")
    from . import _lib
    lib = _lib.lib()
    seed = int(seed) & (2 ** 64 - 1)
    seed_y = (seed ^ 0x9E3779B97F4A7C15) & (2 ** 64 - 1)              # X and Y are independent draws
    with _lib.DeviceScope() as dev:
        d_x, d_y, d_c = dev.upload(x), dev.upload(y), dev.upload(counts)
        # item-major [B][R][K]: item b is redrawn by a launch of its own, so its streams do not know b
        d_xe = dev.upload(np.ascontiguousarray(np.broadcast_to(xe[:, None, :], (B, R, K))))
        d_ye = dev.upload(np.ascontiguousarray(np.broadcast_to(ye[:, None, :], (B, R, K))))
        d_xr, d_yr = dev.alloc(B * R * K * 8), dev.alloc(B * R * K * 8)
        d_phase, d_mean, d_std, d_nan = dev.alloc(B * R * 8), dev.alloc(B * 8), dev.alloc(B * 8), dev.alloc(B * 4)
        for b in range(B):
            for src, dst, s in ((d_x, d_xr, seed), (d_y, d_yr, seed_y)):
                _lib.check(lib.fbx_beta_resample_dev(K, R, src.at(b * K * 8), d_c.at(b * K * 8), float(prior_counts), s,
                                                     dst.at(b * R * K * 8), None))
        _lib.check(lib.fbx_rpe_phase_dev(B * R, K, d_xr.ptr, d_yr.ptr, d_xe.ptr, d_ye.ptr, 0, None, None, None, None, 0,
                                         d_phase.ptr, None, None))
        for b in range(B):
            _lib.check(lib.fbx_circular_stats_dev(R, 1, d_phase.at(b * R * 8), d_mean.at(b * 8), d_std.at(b * 8), d_nan.at(b * 4)))
        _lib.synchronize()
        mean, std = d_mean.to_array(np.float64, (B,)), d_std.to_array(np.float64, (B,))
        skipped = d_nan.to_array(np.int32, (B,))
        samples = d_phase.to_array(np.float64, (B, R)) if return_samples else None
    return (mean, std ** 2, skipped, samples) if return_samples else (mean, std ** 2, skipped)


# ------------------------------------------------------------------------------------------------ experiment settings (host)
def _basis_unitary(change_of_basis, n_qubits):
    d = 1 << n_qubits
    if change_of_basis is None:
        return np.eye(d, dtype=complex)
    u = np.asarray(change_of_basis, dtype=complex)
    if u.shape != (d, d):
        raise ValueError(f"change_of_basis must be a {d} x {d} unitary for {n_qubits} qubit(s), not {u.shape}")
    return u


def all_eigenvector_prep_meas_settings(qubits: Sequence[int], change_of_basis):
    """robust_phase_estimation.py:111-126 with the change of basis as a unitary matrix (or None for the identity) instead of a
    ``Program``: every qubit starts in ``plusX``; for every choice of the X / Y qubit the settings X, X Z.., Y, Y Z.. with a Z on
    each other qubit in turn, in the reference's order.  Returns ``(prep, pre_meas, settings)``: the unitary, its inverse and the
    list of ``ExperimentSetting``.  ``qubits[i]`` is tensor factor i of the matrices, the first the most significant."""
    from .observable_estimation import ExperimentSetting, PauliTerm, TensorProductState, plusX
    qubits = list(qubits)
    prep = _basis_unitary(change_of_basis, len(qubits))
    init_state = TensorProductState()
    for q in qubits:
        init_state = init_state * plusX(q)
    settings = []
    for xy_q in qubits:
        z_qubits = [q for q in qubits if q != xy_q]
        for label in ('X', 'Y'):
            settings.append(ExperimentSetting(init_state, PauliTerm({xy_q: label})))
            settings += [ExperimentSetting(init_state, PauliTerm({xy_q: label, q: 'Z'})) for q in z_qubits]
    return prep, prep.conj().T, settings


def pick_two_eigenvecs_prep_meas_settings(fix_qubit, rotate_qubit: int, change_of_basis=None):
    """robust_phase_estimation.py:129-149: ``fix_qubit = (qubit, 0 | 1)`` stays in that computational state (``plusZ`` /
    ``minusZ``), ``rotate_qubit`` starts in ``plusX``; the settings are X, Y, Z X, Z Y (the Z on the fixed qubit), in the
    reference's order.  ``change_of_basis``: a 4 x 4 unitary on (the smaller qubit label first) or None.  Returns ``(prep,
    pre_meas, settings)`` as ``all_eigenvector_prep_meas_settings``."""
    from .observable_estimation import ExperimentSetting, PauliTerm, minusZ, plusX, plusZ
    fixed, value = int(fix_qubit[0]), int(fix_qubit[1])
    prep = _basis_unitary(change_of_basis, 2)
    init_state = (minusZ(fixed) if value == 1 else plusZ(fixed)) * plusX(rotate_qubit)
    settings = [ExperimentSetting(init_state, PauliTerm({**fixed_op, rotate_qubit: label}))
                for fixed_op in ({}, {fixed: 'Z'}) for label in ('X', 'Y')]
    return prep, prep.conj().T, settings


def rpe_shot_schedule(num_depths: int, multiplicative_factor: float = 1.0, additive_error: Optional[float] = None,
                      min_shots: int = 500) -> np.ndarray:
    """The shots ``acquire_rpe_data`` (robust_phase_estimation.py:288-294) takes at depth 2^j, j < num_depths:
    ``max(min_shots, num_trials(2^j, 2^(num_depths - 1), ...))``, int32 ``[num_depths]``."""
    K = int(num_depths)
    deepest = 2 ** (K - 1) if K > 0 else 1
    return np.array([max(int(min_shots), num_trials(2 ** j, deepest, multiplicative_factor, additive_error)) for j in range(K)],
                    dtype=np.int32)


# ------------------------------------------------------------------------------------------------ simulated acquisition (device)
_BLOCH = {("X", 0): (1, 1, 0, 0), ("X", 1): (1, -1, 0, 0), ("Y", 0): (1, 0, 1, 0), ("Y", 1): (1, 0, -1, 0),
          ("Z", 0): (1, 0, 0, 1), ("Z", 1): (1, 0, 0, -1)}


def _pauli_vector_of_product_state(in_state, qubits):
    """tr[P_k rho] of a ``TensorProductState`` of Pauli eigenstates on ``qubits`` (a qubit it does not name is in |0>)"""
    vec = np.ones(1)
    for q in qubits:
        hit = [s for s in in_state.states if s.qubit == q]
        key = (hit[0].label, hit[0].index) if hit else ("Z", 0)
        if key not in _BLOCH:
            raise ValueError(f"the simulated RPE settings start from Pauli eigenstates, not {hit[0]}")
        vec = np.kron(vec, np.array(_BLOCH[key], dtype=np.float64))
    return vec


def _rpe_ptms(x, what, n_qubits=None):
    """``x`` as real Pauli transfer matrices ``[B', D, D]`` and the number of qubits.  Unitaries ([.., d, d]) are converted by the
    package's conversion kernels.  Without ``n_qubits`` a 4 x 4 array is a two-qubit unitary when its dtype is complex and a
    one-qubit transfer matrix when it is real."""
    from . import _lib
    a = np.asarray(x)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[1] != a.shape[2]:
        raise ValueError(f"{what} must be a stack of square matrices, not {a.shape}")
    side = a.shape[1]
    if n_qubits is None:
        if side not in (2, 4, 8, 16, 64):
            raise ValueError(f"{what} must be unitaries or Pauli transfer matrices of qubits, not {side} x {side}")
        n_qubits = {2: 1, 4: 2 if np.iscomplexobj(a) else 1, 16: 2}.get(side, 3)
    if n_qubits not in (1, 2):
        raise _lib.FbxError(_lib.FBX_ERR_UNSUPPORTED, f"{what}: gates of 1 and 2 qubits are simulated (got {n_qubits} qubits)")
    d = 1 << n_qubits
    if side == d:
        from .operator_tools.superoperator_transformations import convert_batch
        return np.ascontiguousarray(convert_batch("kraus", "pauli_liouville", a[:, None]).real), n_qubits
    if side != d * d:
        raise ValueError(f"{what} must be {d} x {d} unitaries or {d * d} x {d * d} Pauli transfer matrices, not {side} x {side}")
    if np.iscomplexobj(a):
        if np.any(a.imag != 0.0):
            raise ValueError(f"{what}: Pauli transfer matrices must be real")
        a = a.real
    return np.ascontiguousarray(a, dtype=np.float64), n_qubits


class _RpeSimCall:
    """The validated arguments of one ``fbx_rpe_simulate`` call."""

    def __init__(self, rotations, prep, pre_meas, init, xy_qubit, z_qubit, num_depths, num_shots, multiplicative_factor,
                 additive_error, min_shots, flips, seed, first_item, n_qubits):
        self.gate, n = _rpe_ptms(rotations, "rotations", n_qubits)
        self.n, self.B, self.K = n, self.gate.shape[0], int(num_depths)
        B, D = self.B, 4 ** n
        bases = []
        for x, what in ((prep, "prep"), (pre_meas, "pre_meas")):
            if x is None:
                bases.append(None)
                continue
            m, _ = _rpe_ptms(x, what, n)
            if m.shape[0] not in (1, B):
                raise ValueError(f"{what} must be one matrix or one per item ({B}), not {m.shape[0]}")
            bases.append(m)
        self.per_item = int(any(m is not None and m.shape[0] == B and B > 1 for m in bases))
        if self.per_item:
            bases = [None if m is None else np.ascontiguousarray(np.broadcast_to(m, (B, D, D))) for m in bases]
        self.prep, self.meas = bases
        self.init = None
        if init is not None:
            self.init = np.ascontiguousarray(init, dtype=np.float64)
            if self.init.shape != (D,):
                raise ValueError(f"init must be the Pauli vector [{D}] of the input state, not {self.init.shape}")
        self.xy, self.zq = int(xy_qubit), -1 if z_qubit is None else int(z_qubit)
        self.M = 2 if self.zq < 0 else 4
        if num_shots is None:
            shots = rpe_shot_schedule(self.K, multiplicative_factor, additive_error, min_shots)
        else:
            shots = np.asarray(num_shots)
            if shots.ndim == 0:
                shots = np.full(self.K, shots)
            if shots.shape != (self.K,) or np.any(shots != np.floor(shots)) or np.any(np.abs(shots) >= 2 ** 31):
                raise ValueError(f"num_shots must be one integer or one per depth [{self.K}], below 2^31")
        self.shots = np.ascontiguousarray(shots, dtype=np.int32)
        self.flips = None
        if flips is not None:
            f = np.asarray(flips, dtype=np.float64)
            if f.shape not in ((n, 2), (B, n, 2)):
                raise ValueError(f"flips must be [n, 2] = {(n, 2)} or [B, n, 2] = {(B, n, 2)}, not {f.shape}")
            self.flips = np.ascontiguousarray(np.broadcast_to(f, (B, n, 2)))
        self.seed, self.first_item = int(seed) & (2 ** 64 - 1), int(first_item)
        self.uniform = self.K > 0 and bool(np.all(self.shots == self.shots[0]))


def simulate_rpe_batch(rotations, prep=None, pre_meas=None, init=None, xy_qubit: int = 0, z_qubit: Optional[int] = None,
                       num_depths: int = 6, num_shots=None, multiplicative_factor: float = 1.0,
                       additive_error: Optional[float] = None, min_shots: int = 500, flips=None, seed: int = 0, first_item: int = 0,
                       n_qubits: Optional[int] = None, return_probabilities: bool = False, return_histograms: bool = False,
                       return_records: bool = False, return_status: bool = False):
    """B simulated RPE experiments of ``num_depths`` depths in one call (``fbx_rpe_simulate``, include/fbx.h): the data
    ``generate_rpe_experiments`` + ``acquire_rpe_data`` acquire, from the gate instead of a QVM.

    ``rotations``: ``[B, d, d]`` unitaries or ``[B, D, D]`` real Pauli transfer matrices (the way to give a NOISY gate: compose
    the rotation with its decoherence), one or two qubits; a 4 x 4 array is read as two-qubit unitaries when its dtype is complex
    and as one-qubit transfer matrices when it is real unless ``n_qubits`` says which.  ``prep`` / ``pre_meas``: the change of basis
    and its inverse (each a unitary or a transfer matrix, shared or per item, None = identity).  ``init``: the Pauli vector
    ``[D]`` of the input state (None: ``plusX`` on every qubit).  ``xy_qubit`` is measured in X and in Y, ``z_qubit`` (or None) in
    Z on the same shots; qubit 0 is the most significant tensor factor.  ``flips`` (``[n, 2]`` or ``[B, n, 2]``): P(read 1 | 0)
    and P(read 0 | 1) per qubit.  ``num_shots``: one number, one per depth, or None for the schedule of ``acquire_rpe_data``
    (``rpe_shot_schedule``).  Item b is global item ``first_item + b`` of the stream keyed by ``seed``; the stream is part of the
    C contract and restated by ``synthetic.restate_rpe_counts``.

    Returns ``(moments [8, B, K], n_shots [K][, probabilities [B, K, 2, M]][, histograms [B, K, 2, M] uint32][, x_bits, y_bits
    [B, K, S, n] uint8][, status [B]])``.  The planes of ``moments`` are x, y, xz, yz and the variances of those means (NaN in
    the xz / yz planes without ``z_qubit``): ``estimate_phase_from_moments_batch(m[0], m[1], m[4], m[5], m[2], m[3], m[6], m[7],
    errors_are_variances=True)``.  M = 4 outcomes ``2 s + t`` with a partner, else 2.  Records need one shot count for all
    depths (``ValueError`` otherwise) and go to ``robust_phase_estimate_from_shots_batch(x_bits, y_bits, xy_qubit, z_qubit)``.  An
    item that cannot be simulated (a non-finite input, a flip outside [0, 1], an all-zero or overflowing matrix) raises
    ``ValueError``; with ``return_status`` nothing is raised and it has status 1, NaN moments and zero counts."""
    from . import _lib
    import ctypes as C
    a = _RpeSimCall(rotations, prep, pre_meas, init, xy_qubit, z_qubit, num_depths, num_shots, multiplicative_factor, additive_error,
                    min_shots, flips, seed, first_item, n_qubits)
    B, K, M, n = a.B, a.K, a.M, a.n
    if return_records and not a.uniform:
        raise ValueError("simulate_rpe_batch: bit records need the same number of shots at every depth")
    moments = np.empty((8, B, K))
    probs = np.empty((B, K, 2, M)) if return_probabilities else None
    hist = np.empty((B, K, 2, M), dtype=np.uint32) if return_histograms else None
    S = int(a.shots[0]) if return_records else 0
    xb = np.empty((B, K, S, n), dtype=np.uint8) if return_records else None
    yb = np.empty((B, K, S, n), dtype=np.uint8) if return_records else None
    status = np.zeros(B, dtype=np.int32)
    _lib.check(_lib.lib().fbx_rpe_simulate(n, B, K, _lib.dptr(a.gate), _lib.dptr(a.prep), _lib.dptr(a.meas), a.per_item,
                                           _lib.dptr(a.init), a.xy, a.zq, _lib.dptr(a.flips), _lib.iptr(a.shots), a.seed,
                                           a.first_item, _lib.dptr(probs), _lib.ptr(hist, C.c_uint32), _lib.dptr(moments),
                                           _lib.ptr(xb, C.c_uint8), _lib.ptr(yb, C.c_uint8), _lib.iptr(status)))
    if not return_status:
        bad = np.flatnonzero(status)
        if bad.size:
            b = int(bad[0])
            raise ValueError(f"simulate_rpe_batch: item {b} (global id {a.first_item + b}) cannot be simulated: a matrix or init "
                             f"entry that is not finite, a flip outside [0, 1] or outcome probabilities whose clamped sum is not a "
                             f"positive finite number ({bad.size} such item(s) in the batch)")
    out = (moments, a.shots)
    out += tuple(x for x, on in ((probs, return_probabilities), (hist, return_histograms)) if on)
    out += (xb, yb) if return_records else ()
    return out + ((status,) if return_status else ())


def simulate_and_estimate_rpe_batch(rotations, prep=None, pre_meas=None, init=None, xy_qubit: int = 0,
                                    z_qubit: Optional[int] = None, num_depths: int = 6, num_shots=None,
                                    multiplicative_factor: float = 1.0, additive_error: Optional[float] = None,
                                    min_shots: int = 500, flips=None, seed: int = 0, first_item: int = 0,
                                    n_qubits: Optional[int] = None, post_select: int = 0, true_phases=None):
    """``simulate_rpe_batch`` followed by ``estimate_phase_from_moments_batch`` without leaving the device:
    ``fbx_rpe_simulate_dev`` writes the eight moment planes and ``fbx_rpe_phase_dev`` reads them (variances, and with ``z_qubit``
    the post-selected combination ``post_select``), bit for bit what the two calls give.  Returns ``(phases [B], depth_reached
    [B])`` and, with ``true_phases [B]``, the circular distance ``|phase - true|`` in [0, pi] as a third array.  An item that
    cannot be simulated has a NaN phase."""
    from . import _lib
    if post_select not in (0, 1):
        raise ValueError("post_select must be 0 or 1")
    a = _RpeSimCall(rotations, prep, pre_meas, init, xy_qubit, z_qubit, num_depths, num_shots, multiplicative_factor, additive_error,
                    min_shots, flips, seed, first_item, n_qubits)
    B, K = a.B, a.K
    truth = None
    if true_phases is not None:
        truth = np.asarray(true_phases, dtype=np.float64)
        if truth.shape != (B,):
            raise ValueError(f"true_phases must be [B] = {(B,)}, not {truth.shape}")
    lib, ptr = _lib.lib(), _lib.devptr
    with _lib.DeviceScope() as dev:
        d_gate, d_prep, d_meas, d_init, d_flips = (dev.upload(x) for x in (a.gate, a.prep, a.meas, a.init, a.flips))
        d_mom, d_phase, d_depth = dev.alloc(8 * B * K * 8), dev.alloc(B * 8), dev.alloc(B * 4)
        _lib.check(lib.fbx_rpe_simulate_dev(a.n, B, K, ptr(d_gate), ptr(d_prep), ptr(d_meas), a.per_item, ptr(d_init), a.xy, a.zq,
                                            ptr(d_flips), _lib.iptr(a.shots), a.seed, a.first_item, None, None, d_mom.ptr, None, None,
                                            None))
        plane = [d_mom.at(i * B * K * 8) for i in range(8)]
        partner = [plane[i] if a.zq >= 0 else None for i in (2, 3, 6, 7)]
        _lib.check(lib.fbx_rpe_phase_dev(B, K, plane[0], plane[1], plane[4], plane[5], 1, partner[0], partner[1], partner[2],
                                         partner[3], int(post_select), d_phase.ptr, d_depth.ptr, None))
        _lib.synchronize()
        phases, depth = d_phase.to_array(np.float64, (B,)), d_depth.to_array(np.int32, (B,))
    if truth is None:
        return phases, depth
    delta = np.abs(phases - truth) % (2 * pi)
    return phases, depth, np.minimum(delta, 2 * pi - delta)


def simulate_rpe_results(rotation, change_of_basis, qubits: Sequence[int], num_depths: int = 6, settings=None,
                         multiplicative_factor: float = 1.0, additive_error: Optional[float] = None, min_shots: int = 500,
                         num_shots=None, flips=None, seed: int = 0, first_item: int = 0) -> List[list]:
    """One simulated experiment in the reference's structure: the list over depths of lists of ``ExperimentResult`` that
    ``acquire_rpe_data`` returns for ``generate_rpe_experiments(rotation, prep, pre_meas, settings, num_depths)``, which
    ``robust_phase_estimate(results, qubits)`` consumes.  ``rotation``: a unitary on ``qubits`` (one or two; ``qubits[0]`` the most
    significant factor) or its -- possibly noisy -- Pauli transfer matrix; ``change_of_basis``: the unitary that maps the
    computational basis to the rotation's eigenvectors, or None.  ``settings`` default to those of
    ``all_eigenvector_prep_meas_settings(qubits, change_of_basis)`` (pass the list of ``pick_two_eigenvecs_prep_meas_settings`` for
    that experiment).  The settings are grouped as the reference groups them (``group_settings``): a group is one measured basis
    -- X or Y on one qubit, Z on at most one partner -- and its members are read off the same simulated shots; every depth lists
    its results group by group.  One device call serves each distinct (input state, X / Y qubit, partner); call c draws the
    stream of global item ``first_item + c``.  The shot counts are those of ``acquire_rpe_data`` unless ``num_shots`` is given."""
    from .observable_estimation import ExperimentResult, ObservablesExperiment, group_settings
    qubits = list(qubits)
    n = len(qubits)
    if n not in (1, 2):
        from . import _lib
        raise _lib.FbxError(_lib.FBX_ERR_UNSUPPORTED, f"simulate_rpe_results: gates of 1 and 2 qubits are simulated (got {n} qubits)")
    prep, pre_meas, default_settings = all_eigenvector_prep_meas_settings(qubits, change_of_basis)
    settings = list(default_settings if settings is None else settings)
    groups = list(group_settings(ObservablesExperiment(settings)))
    calls, plan = {}, []                                    # (init, xy, z) -> call index; per group: (call, basis, members)
    for group in groups:
        xy = {(q, op) for s in group for q, op in s.observable if op in ('X', 'Y')}
        zs = {q for s in group for q, op in s.observable if op == 'Z'}
        states = {s.in_state for s in group}
        if len(xy) != 1 or len(zs) > 1 or len(states) != 1 or not all(s.observable[next(iter(xy))[0]] != 'I' for s in group):
            raise ValueError("simulate_rpe_results: every group of settings must measure X or Y on one qubit, Z on at most one "
                             "other qubit, from one input state")
        (xy_q, label), z_q = next(iter(xy)), (next(iter(zs)) if zs else None)
        if xy_q not in qubits or (z_q is not None and z_q not in qubits):
            raise ValueError("simulate_rpe_results: a setting measures a qubit outside `qubits`")
        key = (next(iter(states)), xy_q, z_q)
        plan.append((calls.setdefault(key, len(calls)), 0 if label == 'X' else 1, list(group)))
    moments = [None] * len(calls)
    shots = None
    for (state, xy_q, z_q), c in calls.items():
        moments[c], shots = simulate_rpe_batch(
            np.asarray(rotation)[None], prep=prep, pre_meas=pre_meas, init=_pauli_vector_of_product_state(state, qubits),
            xy_qubit=qubits.index(xy_q), z_qubit=None if z_q is None else qubits.index(z_q), num_depths=num_depths,
            num_shots=num_shots, multiplicative_factor=multiplicative_factor, additive_error=additive_error, min_shots=min_shots,
            flips=flips, seed=seed, first_item=first_item + c, n_qubits=n)
    results = []
    for j in range(int(num_depths)):
        layer = []
        for c, basis, members in plan:
            for setting in members:
                which = 1 if any(op == 'Z' for _, op in setting.observable) else 0
                mean, var = moments[c][2 * which + basis, 0, j], moments[c][4 + 2 * which + basis, 0, j]
                layer.append(ExperimentResult(setting=setting, expectation=float(mean), total_counts=int(shots[j]),
                                              std_err=float(np.sqrt(var))))
        results.append(layer)
    return results
