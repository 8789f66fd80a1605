"""Measured bitstrings drawn on the device from outcome distributions (``fbx_sample_bitstrings``): the step between an ideal
distribution -- ``quantum_volume.collect_heavy_outputs_batch(..., return_probabilities=True)``, a row of a confusion matrix, the
diagonal of a state -- and the ``[shots, n]`` bit arrays that ``qc.run`` returns and every ``*_from_shots`` function of this
package consumes.  The reference gets such arrays from a QVM; nothing of it is mirrored here.

The stream is part of the C contract (include/fbx.h): a record depends on ``(seed, first_item + b, shot)`` and its item's inputs
only, so a batch may be drawn in pieces, on any number of calls, and checked shot by shot on the host.

``sample_clifford_circuit_batch`` needs no distribution: it draws the shots of a Clifford circuit with Pauli gate noise on up to 64
qubits from the gate list itself (``fbx_clifford_sample_shots``, one Pauli frame per shot)."""
import ctypes as C

import numpy as np

from .operator_tools.random_operators import _stream_seed

__all__ = ["sample_bitstrings_batch", "sample_bitstrings_wide_batch", "sample_clifford_circuit_batch"]

MIN_WIDTH, MAX_WIDTH = 1, 13
MIN_WIDE_WIDTH, MAX_WIDE_WIDTH = 14, 26                  # fbx_sample_bitstrings_wide


def _noise(B, n, shots, depolarizing, readout_flip, first_item=0):
    """The broadcasting of one call: (shots, lam [B] or None, flips [B, n, 2] or None, first_item)."""
    shots, first_item = int(shots), int(first_item)
    if shots < 0 or first_item < 0:
        raise ValueError("need shots >= 0 and first_item >= 0")
    lam = None
    if depolarizing is not None:
        lam = np.asarray(depolarizing, dtype=np.float64)
        if lam.shape not in ((), (B,)):
            raise ValueError(f"depolarizing must be a scalar or [B] = {(B,)}, not {lam.shape}")
        lam = np.ascontiguousarray(np.broadcast_to(lam, (B,)))
    flips = None
    if readout_flip is not None:
        flips = np.asarray(readout_flip, dtype=np.float64)
        if flips.shape not in ((n, 2), (B, n, 2)):
            raise ValueError(f"readout_flip must be [n, 2] = {(n, 2)} or [B, n, 2] = {(B, n, 2)}, not {flips.shape}")
        flips = np.ascontiguousarray(np.broadcast_to(flips, (B, n, 2)))
    return shots, lam, flips, first_item


def _raise_poisoned(status, first_item, who="sample_bitstrings_batch"):
    bad = np.flatnonzero(status)
    if bad.size:
        b = int(bad[0])
        raise ValueError(f"{who}: item {b} (global id {first_item + b}) cannot be sampled: a weight that is "
                         f"negative or not finite, weights without a positive finite sum, or a depolarizing / readout_flip "
                         f"value outside [0, 1] ({bad.size} such item(s) in the batch)")


def _sample_bitstrings(wide, probabilities, shots, depolarizing, readout_flip, seed, first_item, return_status):
    """The body of ``sample_bitstrings_batch`` (``fbx_sample_bitstrings``) and, with ``wide``, of ``sample_bitstrings_wide_batch`` past
    13 qubits (``fbx_sample_bitstrings_wide``)."""
    from . import _lib
    p = np.ascontiguousarray(probabilities, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] < 2 or p.shape[1] & (p.shape[1] - 1):
        raise ValueError("probabilities must be [B, 2^n] with n >= 1")
    B, N = p.shape
    n = N.bit_length() - 1
    shots, lam, flips, first_item = _noise(B, n, shots, depolarizing, readout_flip, first_item)
    ok = wide or MIN_WIDTH <= n <= MAX_WIDTH             # (outside, the library refuses before it touches a buffer)
    bits = np.zeros((B, shots, n) if ok else (0, 0, n), dtype=np.uint8)
    status = np.zeros(B, dtype=np.int32)
    entry = _lib.lib().fbx_sample_bitstrings_wide if wide else _lib.lib().fbx_sample_bitstrings
    _lib.check(entry(n, B, shots, _lib.dptr(p), _lib.dptr(lam), _lib.dptr(flips), _stream_seed(seed), first_item,
                     bits.ctypes.data_as(C.POINTER(C.c_uint8)), _lib.iptr(status)))
    if return_status:
        return bits, status
    _raise_poisoned(status, first_item, *(("sample_bitstrings_wide_batch",) if wide else ()))
    return bits


def sample_bitstrings_batch(probabilities, shots, depolarizing=None, readout_flip=None, seed=None, first_item=0,
                            return_status=False):
    """``probabilities [B, 2^n]`` (non-negative weights, not necessarily normalised; outcome index i has qubit 0 as its most
    significant bit), n = 1..13 -> ``[B, shots, n]`` uint8 bit arrays, first column = qubit 0.

    ``depolarizing`` (a scalar or ``[B]``): item b is drawn from ``(1 - lambda_b) p + lambda_b sum(p) / 2^n``.  ``readout_flip``
    (``[n, 2]`` for the whole batch or ``[B, n, 2]``): after the draw, column j flips with probability ``[j, 0]`` when the drawn bit
    is 0 (P(read 1 | 0)) and ``[j, 1]`` when it is 1 (P(read 0 | 1)), independently per bit.  ``seed=None`` takes a fresh key from
    numpy's global stream (the rule of ``random_operators``); item b is global item ``first_item + b`` of the stream.

    An item that cannot be sampled (a negative or non-finite weight, no positive finite sum, a probability outside [0, 1]) raises
    ``ValueError`` naming the first one; with ``return_status=True`` nothing is raised and ``(bits, status [B] int32)`` comes back,
    status 1 and a record of zeros for such an item, its neighbours untouched."""
    return _sample_bitstrings(False, probabilities, shots, depolarizing, readout_flip, seed, first_item, return_status)


def sample_bitstrings_wide_batch(probabilities, shots, depolarizing=None, readout_flip=None, seed=None, first_item=0,
                                 return_status=False):
    """``sample_bitstrings_batch`` for widths 1..26 through one call: up to 13 qubits it IS ``sample_bitstrings_batch``; from 14 on
    ``fbx_sample_bitstrings_wide`` draws from a table of prefix sums in device memory.  Arguments,
    broadcasting, the stream (column j of a shot reads word ``2 + j`` of its Philox blocks, now up to seven of them), the
    ``ValueError`` for an item that cannot be sampled and ``return_status`` are those of ``sample_bitstrings_batch``.  Wider than 26:
    ``FbxError(FBX_ERR_UNSUPPORTED)``; there is no host sampler behind it."""
    from . import _lib
    p = np.asarray(probabilities)
    if p.ndim != 2 or p.shape[1] < 2 or p.shape[1] & (p.shape[1] - 1):
        raise ValueError("probabilities must be [B, 2^n] with n >= 1")
    n = p.shape[1].bit_length() - 1
    if n <= MAX_WIDTH:
        return sample_bitstrings_batch(p, shots, depolarizing, readout_flip, seed, first_item, return_status)
    if n > MAX_WIDE_WIDTH:
        raise _lib.FbxError(_lib.FBX_ERR_UNSUPPORTED, f"sample_bitstrings_wide_batch: width must be {MIN_WIDTH}..{MAX_WIDE_WIDTH} "
                                                      f"(got {n}); there is no host fallback")
    return _sample_bitstrings(True, p, shots, depolarizing, readout_flip, seed, first_item, return_status)


def sample_clifford_circuit_batch(gates, n_qubits, shots, class_error=None, noise_class=None, readout_flip=None, seed=None,
                                  first_item=0, packed=False, return_status=False):
    """The shots of a Clifford circuit with Pauli gate noise, 1..64 qubits, without a state vector: ``gates`` (``(name, qubits)``
    tuples or gate words, ``clifford_circuit.encode_gates``) on |0..0>, every qubit measured in Z -> ``[B, shots, n]`` uint8 bit
    records, first column = qubit 0, or with ``packed=True`` ``[B, shots]`` uint64 words, bit q = qubit q.

    The B items share the circuit and differ in noise (``clifford_circuit.frame_noise``): ``class_error`` a scalar or ``[B, K]``,
    the depolarizing probability of every gate of class c -- with that probability a Pauli drawn uniformly from all 4 or 16 on the
    gate's qubits follows the gate, the model of ``direct_fidelity_estimation.simulate_dfe_batch``; ``noise_class`` one class per
    gate or 255 for a gate without noise (default: all class 0); ``readout_flip`` ``[n, 2]`` or ``[B, n, 2]`` as in
    ``sample_bitstrings_batch``.  ``seed=None`` takes a fresh key; item b is global item ``first_item + b`` of the stream, which
    ``clifford_circuit.restate_frame_shots`` restates on the host bit for bit.

    An item with a probability outside [0, 1] (or NaN) raises ``ValueError``; with ``return_status=True`` nothing is raised and
    ``(records, status [B] int32)`` comes back, status 1 and a record of zeros for such an item."""
    from . import _lib
    from . import clifford_circuit as cc
    n = cc.check_width(n_qubits)
    words = cc.encode_gates(gates, n)
    B, K, ce, cls, flips = cc.frame_noise(n, words.size, class_error, noise_class, readout_flip)
    shots, first_item = int(shots), int(first_item)
    if shots < 0 or first_item < 0:
        raise ValueError("need shots >= 0 and first_item >= 0")
    lib = _lib.lib()
    reference = np.zeros(1, dtype=np.uint64)
    _lib.check(lib.fbx_clifford_reference_sample(n, words.size, _lib.ptr(words, C.c_uint32), _lib.ptr(reference, C.c_uint64)))
    out = np.zeros((B, shots) if packed else (B, shots, n), dtype=np.uint64 if packed else np.uint8)
    status = np.zeros(B, dtype=np.int32)
    _lib.check(lib.fbx_clifford_sample_shots(n, words.size, _lib.ptr(words, C.c_uint32), _lib.ptr(cls, C.c_uint8), K,
                                             _lib.ptr(reference, C.c_uint64), B, shots, _lib.dptr(ce), _lib.dptr(flips),
                                             _stream_seed(seed), first_item, None if packed else _lib.ptr(out, C.c_uint8),
                                             _lib.ptr(out, C.c_uint64) if packed else None, _lib.iptr(status)))
    if return_status:
        return out, status
    bad = np.flatnonzero(status)
    if bad.size:
        raise ValueError(f"sample_clifford_circuit_batch: item {int(bad[0])} (global id {first_item + int(bad[0])}) cannot be "
                         f"sampled: a class_error or readout_flip value outside [0, 1] ({bad.size} such item(s) in the batch)")
    return out
