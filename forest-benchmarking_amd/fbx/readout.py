"""Readout characterisation (forest/benchmarking/readout.py) without the acquisition: the reference's ``estimate_*`` functions run
programs on a ``QuantumComputer`` and then count, shot by shot in Python, how often each bitstring came back.  The functions here
take the shots such a run returned and do the counting on the device (``fbx_bit_histogram``, joint kind: one launch for every
prepared bitstring of every group of one size), the division by the number of shots there too (``fbx_counts_to_frequencies``), and
the marginals with ``fbx_marginalize_confusion``.  ``get_flipped_program`` and everything that builds or runs a ``Program`` is not
mirrored.

Conventions (readout.py:116-120): a matrix has the prepared bitstring as its row and the observed one as its column, both in
increasing bitstring order with the most significant (leftmost) bit on the first qubit of the group; rows sum to 1."""
import ctypes as C
from typing import Dict, Sequence, Tuple

import numpy as np

from .utils import bitstring_histogram_batch, counts_to_frequencies

__all__ = ["estimate_confusion_matrix_from_shots", "joint_confusion_matrices_batch", "estimate_joint_confusion_in_set_from_shots",
           "estimate_joint_reset_confusion_from_shots", "marginalize_confusion_matrix", "marginalize_confusion_matrix_batch"]


def _column(shots):
    a = np.asarray(shots)
    if a.ndim == 2 and a.shape[1] == 1:
        a = a[:, 0]
    if a.ndim != 1 or a.size == 0:
        raise ValueError("shots of one qubit must be [n_shots] or [n_shots, 1], n_shots >= 1")
    return a.reshape(1, -1, 1)


def estimate_confusion_matrix_from_shots(should_be_0, should_be_1) -> np.ndarray:
    """readout.py:30-66 from the two register arrays its programs return (prepare 0 and measure; prepare 1 and measure):
    ``[[p00, 1 - p00], [1 - p11, p11]]`` with each row the relative frequencies of reading 0 and 1."""
    zero, one = _column(should_be_0), _column(should_be_1)
    if zero.shape == one.shape:
        return bitstring_histogram_batch(np.concatenate([zero, one]), frequencies=True)[1]
    return np.concatenate([bitstring_histogram_batch(zero, frequencies=True)[1], bitstring_histogram_batch(one, frequencies=True)[1]])


def _joint_counts(bitarrays):
    bits = np.asarray(bitarrays)
    if bits.ndim != 4 or bits.shape[1] != 1 << bits.shape[3]:
        raise ValueError("bitarrays must be [G, 2^g, n_shots, g]: for every group the shots of every prepared bitstring")
    G, rows, n_shots, g = bits.shape
    counts = bitstring_histogram_batch(bits.reshape(G * rows, n_shots, g), kind="joint")
    return counts.reshape(G, rows, rows), n_shots


def joint_confusion_matrices_batch(bitarrays, num_trials: int = None) -> np.ndarray:
    """``bitarrays [G, 2^g, n_shots, g]`` -- for each of G groups of g qubits and each prepared bitstring (in
    ``itertools.product([0, 1], repeat=g)`` order) the measured shots, column i = the group's i-th qubit -- -> ``[G, 2^g, 2^g]``
    confusion matrices, counts over ``n_shots`` (over ``num_trials`` when given: readout.py:327).  One launch for the batch."""
    counts, n_shots = _joint_counts(bitarrays)
    return counts_to_frequencies(counts, n_shots if num_trials is None else num_trials)


def _in_set(shots_by_group, num_trials=None) -> Dict[Tuple[int, ...], np.ndarray]:
    keys = sorted(tuple(int(q) for q in key) for key in shots_by_group)
    lookup = {tuple(int(q) for q in key): np.asarray(val) for key, val in shots_by_group.items()}
    out = {}
    by_shape: Dict[tuple, list] = {}
    for key in keys:
        arr = lookup[key]
        if arr.ndim != 3 or arr.shape[2] != len(key) or arr.shape[0] != 1 << len(key):
            raise ValueError(f"the shots of group {key} must be [2^g, n_shots, g] with g = {len(key)}")
        by_shape.setdefault(arr.shape, []).append(key)
    for members in by_shape.values():
        mats = joint_confusion_matrices_batch(np.stack([lookup[key] for key in members]), num_trials)
        for key, mat in zip(members, mats):
            out[key] = mat
    return {key: out[key] for key in keys}


def estimate_joint_confusion_in_set_from_shots(shots_by_group) -> Dict[Tuple[int, ...], np.ndarray]:
    """The reduction of ``estimate_joint_confusion_in_set`` (readout.py:69-180): a dict ``group -> [2^g, n_shots, g]`` of the shots
    measured after preparing each bitstring on the group (the ``qc.run`` results of :168, stacked over the rows) -> a dict
    ``group -> [2^g, 2^g]`` matrix, keys as sorted tuples in sorted order (the order ``itertools.combinations(sorted(qubits), g)``
    gives).  All groups of one size and shot count go to the device as one launch."""
    return _in_set(shots_by_group)


def estimate_joint_reset_confusion_from_shots(shots_by_group, num_trials: int = None) -> Dict[Tuple[int, ...], np.ndarray]:
    """The reduction of ``estimate_joint_reset_confusion`` (readout.py:236-335): ``group -> [2^g, n, g]``, the post-reset
    measurements of all trials of a row stacked along the shot axis, every count divided by ``num_trials`` (default: n, one shot
    per trial as the reference's programs return)."""
    return _in_set(shots_by_group, num_trials)


def marginalize_confusion_matrix_batch(confusion_matrices, all_qubits: Sequence[int], marginal_subset: Sequence[int]) -> np.ndarray:
    """``marginalize_confusion_matrix`` for stacked ``[B, 2^n, 2^n]`` matrices over the same ``all_qubits``, on the device."""
    from . import _lib
    all_qubits = list(all_qubits)
    n = len(all_qubits)
    mats = np.ascontiguousarray(confusion_matrices, dtype=np.float64)
    if mats.ndim != 3 or mats.shape[1:] != (1 << n, 1 << n):
        raise ValueError(f"confusion matrices must be [B, 2^n, 2^n] with n = len(all_qubits) = {n}")
    keep = np.flatnonzero(np.isin(all_qubits, list(marginal_subset))).astype(np.uint8)      # in the order of all_qubits (:207-209)
    if len(keep) != len(marginal_subset):
        raise ValueError("every element of marginal_subset must appear exactly once in all_qubits")     # the reference asserts (:211)
    if len(keep) == 0:
        raise ValueError("marginal_subset is empty")
    out = np.zeros((mats.shape[0], 1 << len(keep), 1 << len(keep)))
    _lib.check(_lib.lib().fbx_marginalize_confusion(n, mats.shape[0], len(keep), keep.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                    _lib.dptr(mats), _lib.dptr(out)))
    return out


def marginalize_confusion_matrix(confusion_matrix: np.ndarray, all_qubits: Sequence[int],
                                 marginal_subset: Tuple[int, ...]) -> np.ndarray:
    """readout.py:183-233: the joint confusion matrix on ``all_qubits`` (first qubit = most significant bit) -> the one on
    ``marginal_subset``, whose qubits may come in any order; the result is ordered as they appear in ``all_qubits``.  Raises
    ``ValueError`` where the reference asserts."""
    mat = np.asarray(confusion_matrix, dtype=np.float64)
    return marginalize_confusion_matrix_batch(mat[None], all_qubits, marginal_subset)[0]


def confusion_from_flips(readout_flip) -> np.ndarray:
    """The joint confusion matrix of independent per-bit flips: ``readout_flip [n, 2]`` (or ``[B, n, 2]``) with ``[j, 0]`` = P(read
    1 | drawn 0) and ``[j, 1]`` = P(read 0 | drawn 1) of qubit j, the convention of the simulators' ``readout_flip`` argument ->
    ``[2^n, 2^n]`` (``[B, 2^n, 2^n]``), the Kronecker product of the per-qubit [drawn][read] matrices with qubit 0 the most
    significant bit: what the ``confusion`` argument of ``tomography.simulate_symmetrized_*_tomography_batch`` takes."""
    f = np.asarray(readout_flip, dtype=np.float64)
    single = f.ndim == 2
    f = f[None] if single else f
    if f.ndim != 3 or f.shape[2] != 2 or f.shape[1] < 1:
        raise ValueError("readout_flip must be [n, 2] or [B, n, 2]")
    out = np.ones((f.shape[0], 1, 1))
    for j in range(f.shape[1]):
        one = np.empty((f.shape[0], 2, 2))
        one[:, 0, 0], one[:, 0, 1] = 1.0 - f[:, j, 0], f[:, j, 0]
        one[:, 1, 0], one[:, 1, 1] = f[:, j, 1], 1.0 - f[:, j, 1]
        out = np.einsum("bij,bkl->bikjl", out, one).reshape(f.shape[0], 2 * out.shape[1], 2 * out.shape[2])
    return out[0] if single else out
