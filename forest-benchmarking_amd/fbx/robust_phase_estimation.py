"""Robust phase estimation (forest/benchmarking/robust_phase_estimation.py) without the acquisition: from the moments, or the
measured bits, of an RPE experiment to phases and their error bars.

What runs where:
  * ``estimate_phase_from_moments`` / ``robust_phase_estimate`` (the reference's signatures) and ``estimate_phase_from_moments_batch``
    -- ``fbx_rpe_phase``: the reference's recursion (:377-404) for B estimates in one launch, one estimate per GPU lane;
  * ``robust_phase_estimate_from_shots_batch`` -- ``fbx_rpe_from_shots``: the same estimate straight from the ``[B, K, shots, qubits]``
    bit arrays of the X and the Y basis, one wavefront per estimate;
  * ``phase_variance_batch`` -- bootstrap error bars: ``fbx_beta_resample_dev`` -> ``fbx_rpe_phase_dev`` -> ``fbx_circular_stats_dev``
    without a copy in between; ``circular_stats`` is the last step on its own;
  * ``num_trials``, ``get_additive_error_factor``, ``_p_max``, ``_xci``, ``get_variance_upper_bound``,
    ``bloch_rotation_to_eigenvectors``, ``get_change_of_basis_from_eigvecs`` -- host arithmetic.

There is no host fallback for the estimates: without a GPU they raise ``FbxError(FBX_ERR_NO_DEVICE)``.
``generate_rpe_experiments``, ``acquire_rpe_data``, ``do_rpe``, ``change_of_basis_matrix_to_quil``, the two ``*_prep_meas_settings``
functions (pyquil ``Program`` / ``QuantumComputer``) and ``plot_rpe_iterations`` are not mirrored.
"""
import warnings
from typing import List, Optional, Sequence, Union

import numpy as np
from numpy import pi

__all__ = ["get_additive_error_factor", "num_trials", "get_variance_upper_bound", "bloch_rotation_to_eigenvectors",
           "get_change_of_basis_from_eigvecs", "estimate_phase_from_moments", "robust_phase_estimate",
           "estimate_phase_from_moments_batch", "robust_phase_estimate_from_shots_batch", "phase_variance_batch", "circular_stats"]

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
    import ctypes as C
    lib, DB = _lib.lib(), _lib.DeviceBuffer
    seed = int(seed) & (2 ** 64 - 1)
    seed_y = (seed ^ 0x9E3779B97F4A7C15) & (2 ** 64 - 1)              # X and Y are independent draws
    bufs = [DB.from_array(a) for a in (x, y, counts)]
    d_x, d_y, d_c = bufs
    # item-major [B][R][K]: item b is redrawn by a launch of its own, so its streams do not know b
    d_xe = DB.from_array(np.ascontiguousarray(np.broadcast_to(xe[:, None, :], (B, R, K))))
    d_ye = DB.from_array(np.ascontiguousarray(np.broadcast_to(ye[:, None, :], (B, R, K))))
    d_xr, d_yr = DB(B * R * K * 8), DB(B * R * K * 8)
    d_phase, d_mean, d_std, d_nan = DB(B * R * 8), DB(B * 8), DB(B * 8), DB(B * 4)
    bufs += [d_xe, d_ye, d_xr, d_yr, d_phase, d_mean, d_std, d_nan]

    def at(buf, offset):
        return C.c_void_p(buf.ptr.value + offset)
    try:
        for b in range(B):
            for src, dst, s in ((d_x, d_xr, seed), (d_y, d_yr, seed_y)):
                _lib.check(lib.fbx_beta_resample_dev(K, R, at(src, b * K * 8), at(d_c, b * K * 8), float(prior_counts), s,
                                                     at(dst, b * R * K * 8), None))
        _lib.check(lib.fbx_rpe_phase_dev(B * R, K, d_xr.ptr, d_yr.ptr, d_xe.ptr, d_ye.ptr, 0, None, None, None, None, 0,
                                         d_phase.ptr, None, None))
        for b in range(B):
            _lib.check(lib.fbx_circular_stats_dev(R, 1, at(d_phase, b * R * 8), at(d_mean, b * 8), at(d_std, b * 8), at(d_nan, b * 4)))
        _lib.synchronize()
        mean, std = d_mean.to_array(np.float64, (B,)), d_std.to_array(np.float64, (B,))
        skipped = d_nan.to_array(np.int32, (B,))
        samples = d_phase.to_array(np.float64, (B, R)) if return_samples else None
    finally:
        for buf in bufs:
            buf.free()
    return (mean, std ** 2, skipped, samples) if return_samples else (mean, std ** 2, skipped)
