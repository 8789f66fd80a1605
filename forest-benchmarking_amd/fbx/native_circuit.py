"""Circuits of native gates (``I``, ``RX``, ``RZ``, ``CZ``, ``XY``: what ``fbx.compilation.basic_compile`` emits) as words, their
host mirror in pure numpy, and the wrappers of ``fbx_native_trajectories`` / ``fbx_native_unitary`` (csrc/fbx_native.hip,
DESIGN.md 4.26).  The mirror is written from the contract in include/fbx.h -- THE WORD, THE MODEL, THE STREAM -- as
``fbx.clifford_circuit`` and ``classical_logic.reversible`` are for their kernels; the GPU tests hold the device against it.

A native gate is ``(name, qubits)``, ``(name, qubits, angle)`` or ``(name, qubits, angle, input_bit)``; the fourth entry makes
the gate conditional: it, and its error site, exist iff that bit of the unit's input word is set.  A state vector is indexed with
qubit 0 as the MOST significant bit (``fbx_qv_heavy_outputs``' order); only ``native_unitary`` speaks pyquil's order.
"""
import ctypes as C

import numpy as np

from . import _lib
from .clifford_circuit import NOISELESS, _bad_probabilities, frame_noise
from .compilation import gate_matrix

__all__ = ["encode_native", "decode_native", "check_words", "native_noise_classes", "apply_native", "exact_native_distribution",
           "restate_native_trajectories", "native_trajectories", "native_trajectories_dev", "native_unitary", "native_unitary_dev",
           "marginal_distribution", "OPCODES", "NATIVE_KEY_TAG", "MAX_QUBITS", "WAVE_MAX_QUBITS", "SEGMENT"]

OPCODES = {"I": _lib.NAT_I, "RX": _lib.NAT_RX, "RZ": _lib.NAT_RZ, "CZ": _lib.NAT_CZ, "XY": _lib.NAT_XY}
_NAMES = {v: k for k, v in OPCODES.items()}
_TWO_QUBIT = (_lib.NAT_CZ, _lib.NAT_XY)
_WITH_ANGLE = (_lib.NAT_RX, _lib.NAT_RZ, _lib.NAT_XY)
NATIVE_KEY_TAG = 0x4E415456             # "NATV": the stream of fbx_native_trajectories
MAX_QUBITS = 13
MAX_DENSE_QUBITS = 6                    # exact_native_distribution holds a density matrix
WAVE_MAX_QUBITS = _lib.NAT_WAVE_MAX_QUBITS      # up to here one wavefront runs a trajectory, above a workgroup
SEGMENT = _lib.NAT_SEG                  # trajectories per partial sum of probs_mean_out
_PAULI = (np.eye(2), np.array([[0.0, 1.0], [1.0, 0.0]]), np.array([[0.0, -1.0], [1.0, 0.0]]), np.diag([1.0, -1.0]))   # Y as X Z


def _check_width(n) -> int:
    n = int(n)
    if not 1 <= n <= MAX_QUBITS:
        raise ValueError(f"n_qubits must be 1..{MAX_QUBITS}")
    return n


def _fields(w):
    """(opcode, q0, q1, conditional, input bit) of one word."""
    return w & 7, (w >> 3) & 15, (w >> 7) & 15, (w >> 11) & 1, (w >> 12) & 63


def _qubits(op, q0, q1):
    return (q0, q1) if op in _TWO_QUBIT else (q0,)


def check_words(words, n, angles=None):
    """Words validated by the rule of include/fbx.h and returned as contiguous ``uint32``; with ``angles`` also those, as
    ``float64 [G]``, all finite: ``(words, angles)``."""
    n = _check_width(n)
    words = np.ascontiguousarray(words, dtype=np.uint32).ravel()
    for g, w in enumerate(words.tolist()):
        op, q0, q1, cond, bit = _fields(w)
        ok = op <= _lib.NAT_XY and (w >> 18) == 0 and q0 < n and (cond or bit == 0)
        ok = ok and ((q1 < n and q1 != q0) if op in _TWO_QUBIT else q1 == 0)
        if not ok:
            raise ValueError(f"word {g} is not a valid native-gate word on {n} qubits: {w:#x}")
    if angles is None:
        return words
    angles = np.ascontiguousarray(angles, dtype=np.float64).ravel()
    if angles.size != words.size:
        raise ValueError("angles needs one entry per word")
    if not np.all(np.isfinite(angles)):
        raise ValueError(f"the angle of gate {int(np.flatnonzero(~np.isfinite(angles))[0])} is not finite")
    return words, angles


def encode_native(gates, n):
    """A list of native gates as ``(words uint32 [G], angles float64 [G])`` (THE WORD of include/fbx.h; the angle of ``I`` and
    ``CZ`` is 0).  Refused with the gate's index: a name outside the native set (compile with ``basic_compile`` first), a wrong
    number of qubits, a qubit outside ``range(n)`` or repeated, a missing or non-finite angle, an input bit outside 0..63."""
    n = _check_width(n)
    gates = list(gates)
    words, angles = np.zeros(len(gates), dtype=np.uint32), np.zeros(len(gates))
    for i, gate in enumerate(gates):
        if not isinstance(gate, (tuple, list)) or len(gate) not in (2, 3, 4):
            raise ValueError(f"gate {i}: a native gate is (name, qubits[, angle[, input bit]])")
        name = gate[0]
        if name not in OPCODES:
            raise ValueError(f"gate {i}: {name!r} is not a native gate; basic_compile produces them")
        op, qs = OPCODES[name], tuple(int(q) for q in gate[1])
        if len(qs) != (2 if op in _TWO_QUBIT else 1) or len(set(qs)) != len(qs) or not all(0 <= q < n for q in qs):
            raise ValueError(f"gate {i}: {name} on qubits {qs} of {n}")
        angle = gate[2] if len(gate) >= 3 else None
        if op in _WITH_ANGLE:
            if angle is None or not np.isfinite(float(angle)):
                raise ValueError(f"gate {i}: {name} needs a finite angle")
            angles[i] = float(angle)
        elif angle is not None:
            raise ValueError(f"gate {i}: {name} takes no angle")
        w = op | (qs[0] << 3) | ((qs[1] << 7) if len(qs) == 2 else 0)
        if len(gate) == 4 and gate[3] is not None:
            bit = int(gate[3])
            if not 0 <= bit < 64:
                raise ValueError(f"gate {i}: the input bit of a conditional gate is 0..63, not {bit}")
            w |= (1 << 11) | (bit << 12)
        words[i] = w
    return words, angles


def decode_native(words, angles):
    """The inverse of ``encode_native``: the gate list of ``(words, angles)``."""
    words = np.asarray(words, dtype=np.uint32).ravel()
    angles = np.asarray(angles, dtype=np.float64).ravel()
    gates = []
    for w, a in zip(words.tolist(), angles.tolist()):
        op, q0, q1, cond, bit = _fields(w)
        if op not in _NAMES:
            raise ValueError(f"unknown opcode in word {w:#x}")
        gate = (_NAMES[op], _qubits(op, q0, q1)) + ((a,) if op in _WITH_ANGLE else ())
        if cond:
            gate = gate + ((None,) if op not in _WITH_ANGLE else ()) + (bit,)
        gates.append(gate)
    return gates


def native_noise_classes(words) -> np.ndarray:
    """The default noise classes, ``uint8 [G]`` with K = 3: class 0 the pulses ``RX`` and ``I``, class 1 ``RZ`` -- the virtual
    gate, to which callers usually give error 0 -- and class 2 the two-qubit gates ``CZ`` and ``XY``."""
    op = np.asarray(words, dtype=np.uint32) & np.uint32(7)
    return np.where(op == _lib.NAT_RZ, 1, np.where(op >= _lib.NAT_CZ, 2, 0)).astype(np.uint8)


# --------------------------------------------------------------------------------------------------
# The mirror: state vectors and density matrices in numpy
# --------------------------------------------------------------------------------------------------
def _apply_matrix(v, matrix, qubits, n):
    """``matrix`` on ``qubits`` (first = most significant bit of the matrix index) from the left on ``v [2^n, ...]``, whose
    leading index has qubit 0 as its most significant bit."""
    k = len(qubits)
    t = v.reshape((2,) * n + (-1,))
    t = np.tensordot(matrix.reshape((2,) * (2 * k)), t, axes=(list(range(k, 2 * k)), list(qubits)))
    return np.moveaxis(t, list(range(k)), list(qubits)).reshape(v.shape)


def _pauli_matrix(index, k):
    """The Pauli with THE STREAM's index on k operands: operand i has digit ``(index >> 2 (k - 1 - i)) & 3``; Y is X Z."""
    m = np.ones((1, 1))
    for i in range(k):
        m = np.kron(m, _PAULI[(index >> (2 * (k - 1 - i))) & 3])
    return m


def _gate_matrix(op, angle):
    return gate_matrix(_NAMES[op], angle)


def apply_native(words, angles, n, state, input_word=0, paulis=None) -> np.ndarray:
    """The circuit on the state vector ``state [2^n]`` (qubit 0 the most significant index bit): the mirror of the kernel's
    gate loop.  A conditional gate exists iff its bit of ``input_word`` is set.  ``paulis [G]``: after gate l the Pauli with
    index ``paulis[l]`` on the gate's qubits (THE STREAM's index), nothing where it is negative; it is ignored for a gate that
    does not exist."""
    words, angles = check_words(words, n, angles)
    state = np.array(state, dtype=np.complex128).reshape(1 << n)
    for l, (w, a) in enumerate(zip(words.tolist(), angles.tolist())):
        op, q0, q1, cond, bit = _fields(w)
        if cond and not (int(input_word) >> bit) & 1:
            continue
        qs = _qubits(op, q0, q1)
        m = _gate_matrix(op, a)
        if paulis is not None and int(paulis[l]) >= 0:
            m = _pauli_matrix(int(paulis[l]), len(qs)) @ m
        state = _apply_matrix(state, m, qs, n)
    return state


def marginal_distribution(probs, n, out_qubits) -> np.ndarray:
    """``probs [.., 2^n]`` -> ``[.., 2^m]`` on ``out_qubits``: column c of ``out_qubits`` is bit m - 1 - c of the result's index."""
    out = [int(q) for q in np.asarray(out_qubits).ravel()]
    if not 1 <= len(out) <= n or len(set(out)) != len(out) or not all(0 <= q < n for q in out):
        raise ValueError(f"out_qubits must be 1..{n} different qubit indices below {n}")
    probs = np.asarray(probs, dtype=np.float64)
    lead = probs.shape[:-1]
    t = probs.reshape(lead + (2,) * n)
    rest = [q for q in range(n) if q not in out]
    t = np.transpose(t, list(range(len(lead))) + [len(lead) + q for q in out + rest])
    return t.reshape(lead + (1 << len(out), -1)).sum(axis=-1)


def exact_native_distribution(words, angles, n, input_word=0, class_error=None, noise_class=None, out_qubits=None) -> np.ndarray:
    """The outcome distribution of the noisy circuit on ``out_qubits`` (default all) for one input word and one item of noise
    ``class_error [K]``, exactly: the density matrix pushed through the circuit, every existing gate of class c followed by
    ``rho -> (1 - p) rho + p 4^-k sum_P P rho P`` over all Paulis of its k qubits (THE MODEL).  ``n <= 6``."""
    words, angles = check_words(words, n, angles)
    if n > MAX_DENSE_QUBITS:
        raise ValueError(f"exact_native_distribution is dense: n <= {MAX_DENSE_QUBITS}")
    ce = None if class_error is None else np.atleast_1d(np.asarray(class_error, dtype=np.float64))[None]
    _, K, ce, cls, _ = frame_noise(n, words.size, ce, noise_class, None)
    N = 1 << n
    rho = np.zeros((N, N), dtype=np.complex128)
    rho[0, 0] = 1.0

    def conjugate(r, m, qs):
        return _apply_matrix(_apply_matrix(r, m, qs, n).conj().T, m, qs, n).conj().T

    for l, (w, a) in enumerate(zip(words.tolist(), angles.tolist())):
        op, q0, q1, cond, bit = _fields(w)
        if cond and not (int(input_word) >> bit) & 1:
            continue
        qs = _qubits(op, q0, q1)
        rho = conjugate(rho, _gate_matrix(op, a), qs)
        c = 0 if cls is None else int(cls[l])
        p = 0.0 if (ce is None or c == NOISELESS) else float(ce[0, c])
        if p > 0.0:
            k = len(qs)
            mixed = sum(conjugate(rho, _pauli_matrix(i, k).astype(np.complex128), qs) for i in range(4 ** k)) / 4 ** k
            rho = (1.0 - p) * rho + p * mixed
    dist = np.real(np.diag(rho))
    return dist if out_qubits is None else marginal_distribution(dist, n, out_qubits)


def restate_native_trajectories(words, angles, n, inputs, out_qubits, trajectories, class_error=None, noise_class=None, seed=0,
                                first_item=0, first_input=0, probs=True):
    """What ``fbx_native_trajectories`` computes, restated from THE MODEL and THE STREAM of include/fbx.h on the Philox of
    ``fbx.synthetic`` and evaluated by ``apply_native``.  Returns a dict: ``paulis`` ``int8 [B, P, T, G]`` -- the Pauli index
    after every gate, -1 where the gate did not err (or does not exist); ``n_errors`` ``int32 [B, P, T]``; ``status`` ``int32
    [B]``; and with ``probs`` the mean marginal distribution ``probs_mean [B, P, 2^m]``.  A poisoned item has no Paulis, zero
    counts and NaN probabilities, as on the device.  The noise arguments are those of ``clifford_circuit.frame_noise``."""
    from .synthetic import _philox4x32_10
    words, angles = check_words(words, n, angles)
    out = [int(q) for q in np.asarray(out_qubits).ravel()]
    m, G, T = len(out), int(words.size), int(trajectories)
    inputs = np.ascontiguousarray(np.asarray(inputs, dtype=np.uint64).ravel())
    P = int(inputs.size)
    B, K, ce, cls, _ = frame_noise(n, G, class_error, noise_class, None)
    seed, first_item, first_input = int(seed) & (2 ** 64 - 1), int(first_item), int(first_input)
    if not 0 <= T < 2 ** 32 or first_item < 0 or first_input < 0 or first_item + B > 2 ** 32 or first_input + P > 2 ** 32:
        raise ValueError("need 0 <= trajectories < 2^32 and item and input indices in 0 .. 2^32 - 1")
    k0, k1 = (seed & 0xFFFFFFFF) ^ NATIVE_KEY_TAG, seed >> 32
    fields = [_fields(w) for w in words.tolist()]
    t_all = np.arange(T, dtype=np.uint64)
    paulis = np.full((B, P, T, G), -1, dtype=np.int8)
    status = np.zeros(B, dtype=np.int32)
    mean = np.full((B, P, 1 << m), np.nan) if probs else None
    zero = np.zeros(1 << n, dtype=np.complex128)
    zero[0] = 1.0
    for b in range(B):
        if _bad_probabilities(ce[b] if ce is not None else None):
            status[b] = 1
            paulis[b] = -1
            continue
        for r in range(P):
            word = int(inputs[r])
            for l, (op, q0, q1, cond, bit) in enumerate(fields):
                if cond and not (word >> bit) & 1:
                    continue
                c = 0 if cls is None else int(cls[l])
                p = 0.0 if (ce is None or c == NOISELESS) else float(ce[b, c])
                if p > 0.0:
                    x = _philox4x32_10(np.uint64(first_item + b), np.uint64(first_input + r), t_all, np.uint64(l >> 1), k0, k1)
                    first, second = (x[2], x[3]) if l & 1 else (x[0], x[1])
                    k = 2 if op in _TWO_QUBIT else 1
                    errs = first.astype(np.float64) * 2.0 ** -32 < p
                    paulis[b, r, :, l] = np.where(errs, (second >> np.uint64(32 - 2 * k)).astype(np.int64), -1)
            if probs:
                total = np.zeros(1 << n)
                for t in range(T):
                    v = apply_native(words, angles, n, zero, word, paulis[b, r, t])
                    total += v.real * v.real + v.imag * v.imag
                mean[b, r] = marginal_distribution(total, n, out) / T if T else np.nan
    res = {"paulis": paulis, "n_errors": (paulis >= 0).sum(axis=3).astype(np.int32), "status": status}
    if probs:
        res["probs_mean"] = mean
    return res


# --------------------------------------------------------------------------------------------------
# The device
# --------------------------------------------------------------------------------------------------
def _out_qubits(out_qubits, n) -> np.ndarray:
    out = np.ascontiguousarray(np.asarray(out_qubits, dtype=np.int64).ravel())
    if not 1 <= out.size <= n or np.any(out < 0) or np.any(out >= n) or np.unique(out).size != out.size:
        raise ValueError(f"out_qubits must be 1..{n} different qubit indices below {n}")
    return out.astype(np.uint8)


def native_trajectories(words, angles, n, inputs, out_qubits, trajectories, class_error=None, noise_class=None, seed=0, first_item=0,
                        first_input=0, probs_mean=True, n_errors=True):
    """``fbx_native_trajectories`` on the selected GPU, host form: the circuit ``(words, angles)`` on ``n`` qubits for the B items
    of ``class_error`` (a scalar or ``[B, K]``; ``noise_class [G]``, default every gate class 0 -- ``native_noise_classes`` gives
    the usual three) x the P input words ``inputs`` x ``trajectories`` Pauli-error trajectories.  Returns a dict with ``status``
    (``int32 [B]``) and what was asked for: ``probs_mean`` ``[B, P, 2^m]``, the mean outcome distribution of ``out_qubits`` (column
    0 the most significant index bit), and ``n_errors`` ``int32 [B, P, T]``."""
    words, angles = check_words(words, n, angles)
    out = _out_qubits(out_qubits, n)
    m, T = int(out.size), int(trajectories)
    inputs = np.ascontiguousarray(np.asarray(inputs, dtype=np.uint64).ravel())
    P = int(inputs.size)
    B, K, ce, cls, _ = frame_noise(n, words.size, class_error, noise_class, None)
    if T < 0:
        raise ValueError("trajectories must not be negative")
    res = {"status": np.zeros(B, dtype=np.int32)}
    if probs_mean:
        res["probs_mean"] = np.zeros((B, P, 1 << m))
    if n_errors:
        res["n_errors"] = np.zeros((B, P, T), dtype=np.int32)
    _lib.check(_lib.lib().fbx_native_trajectories(
        int(n), words.size, _lib.ptr(words, C.c_uint32), _lib.dptr(angles), _lib.ptr(cls, C.c_uint8), K, P,
        _lib.ptr(inputs, C.c_uint64), m, _lib.ptr(out, C.c_uint8), B, T, _lib.dptr(ce), int(seed) & (2 ** 64 - 1), int(first_item),
        int(first_input), _lib.dptr(res.get("probs_mean")), _lib.iptr(res.get("n_errors")), _lib.iptr(res["status"])))
    return res


def native_trajectories_dev(dev, n, G, d_words, d_angles, d_noise_class, K, P, d_inputs, m, d_out_qubits, B, trajectories,
                            d_class_error, seed=0, first_item=0, first_input=0, probs_mean=True, n_errors=False):
    """``fbx_native_trajectories_dev``: every input a ``DeviceBuffer`` (or None where the header allows NULL), the outputs
    allocated in the ``_lib.DeviceScope`` ``dev``, which owns them.  Returns a dict of device buffers: ``status`` ``int32 [B]``,
    ``probs_mean`` ``float64 [B, P, 2^m]`` and ``n_errors`` ``int32 [B, P, T]`` as asked for.  Nothing is validated or
    synchronised: the call is enqueued on the calling thread's stream."""
    B, P, T, m = int(B), int(P), int(trajectories), int(m)
    res = {"status": dev.alloc(4 * B)}
    if probs_mean:
        res["probs_mean"] = dev.alloc(8 * B * P * (1 << max(m, 0)))
    if n_errors:
        res["n_errors"] = dev.alloc(4 * B * P * T)
    _lib.check(_lib.lib().fbx_native_trajectories_dev(
        int(n), int(G), _lib.devptr(d_words), _lib.devptr(d_angles), _lib.devptr(d_noise_class), int(K), P, _lib.devptr(d_inputs), m,
        _lib.devptr(d_out_qubits), B, T, _lib.devptr(d_class_error), int(seed) & (2 ** 64 - 1), int(first_item), int(first_input),
        _lib.devptr(res.get("probs_mean")), _lib.devptr(res.get("n_errors")), res["status"].ptr))
    return res


def native_unitary(words, angles, n) -> np.ndarray:
    """``fbx_native_unitary``, host form: the ``2^n x 2^n`` unitary of the circuit in the index order of
    ``compilation.program_unitary`` (qubit 0 the least significant bit).  Conditional gates are refused."""
    words, angles = check_words(words, n, angles)
    N = 1 << int(n)
    u = np.zeros((N, N), dtype=np.complex128)
    _lib.check(_lib.lib().fbx_native_unitary(int(n), words.size, _lib.ptr(words, C.c_uint32), _lib.dptr(angles),
                                             _lib.dptr(u.view(np.float64))))
    return u


def native_unitary_dev(dev, n, G, d_words, d_angles):
    """``fbx_native_unitary_dev``: the unitary as a device buffer of ``16 * 4^n`` bytes owned by the scope ``dev``."""
    d_u = dev.alloc(16 << (2 * int(n)))
    _lib.check(_lib.lib().fbx_native_unitary_dev(int(n), int(G), _lib.devptr(d_words), _lib.devptr(d_angles), d_u.ptr))
    return d_u
