"""Reversible circuits on up to 64 qubits as lists of micro-op words: the host mirror of csrc/fbx_reversible.hip in pure numpy,
written from the contract in include/fbx.h, as ``fbx.clifford_circuit`` is for Clifford circuits.

The circuits meant are those of the ripple-carry adder: X, H, CNOT, CZ and CCNOT arranged so that the register only ever holds a
product of Z eigenstates (|0>, |1>) or X eigenstates (|+>, |->) and every gate acts classically on the bits they spell.  A
shot is then one integer -- bit q is the bit qubit q holds -- and which basis a qubit holds its bit in is a property of the
circuit, not of the shot: ``encode_reversible`` tracks it through the gate list and resolves every gate to a micro-op word (NOT,
XOR, AND-XOR or nothing) plus, per operand, whether a Pauli error flips it through its X part or its Z part.  Under Pauli noise
after each gate that description is exact (``tests/test_reversible_cpu.py`` holds it against a density-matrix simulation).

A gate is a ``(name, qubits)`` tuple in the style of ``fbx.clifford.to_gates``: ``"X"``, ``"H"``, ``"CNOT"``, ``"CZ"``,
``"CCNOT"`` and ``("XIN", (q, k))`` -- X on qubit q iff bit k of the unit's input word is set; the gate, and its error site,
exist only then (``bitstring_prep``'s ``RX(pi * bit)``), so one gate list serves every pair of summands.
"""
import ctypes as C

import numpy as np

from ..clifford_circuit import NOISELESS, _bad_probabilities, check_width, frame_noise, unpack_shots

OP_SITE, OP_NOT, OP_XOR, OP_ANDXOR, OP_XIN = range(5)
_ARITY = {OP_NOT: 1, OP_XOR: 2, OP_ANDXOR: 3, OP_XIN: 1}
REVERSIBLE_KEY_TAG = 0x52565253         # "RVRS": the stream of fbx_reversible_sample_shots
MAX_DENSE_QUBITS = 12
_U1 = np.uint64(1)
_BASIS = "ZX"


def _word(op, qubits, on_z, input_bit=0) -> int:
    w = op | (len(qubits) << 3) | (input_bit << 26)
    for i, (q, f) in enumerate(zip(qubits, on_z)):
        w |= (q << (5 + 6 * i)) | (int(f) << (23 + i))
    return w


def _fields(w):
    """(micro-op, operands, their flips-on-the-Z-part flags, input bit) of one word."""
    k = (w >> 3) & 3
    return w & 7, tuple((w >> (5 + 6 * i)) & 63 for i in range(k)), tuple((w >> (23 + i)) & 1 for i in range(k)), w >> 26


def check_words(words, n) -> np.ndarray:
    """An array of micro-op words validated by the rule of include/fbx.h and returned as contiguous ``uint32``."""
    n = check_width(n)
    words = np.ascontiguousarray(words, dtype=np.uint32).ravel()
    for g, w in enumerate(words.tolist()):
        op, k = w & 7, (w >> 3) & 3
        _, qs, fs, bit = _fields(w)
        ok = op <= OP_XIN and 1 <= k <= 3 and _ARITY.get(op, k) == k and (op == OP_XIN or bit == 0)
        ok = ok and all(q < n for q in qs) and len(set(qs)) == k and (op != OP_XIN or fs[0] == 0)
        ok = ok and all(((w >> (5 + 6 * i)) & 63) == 0 and ((w >> (23 + i)) & 1) == 0 for i in range(k, 3))
        if not ok:
            raise ValueError(f"word {g} is not a valid micro-op word on {n} qubits: {w:#x}")
    return words


def encode_reversible(gates, n) -> np.ndarray:
    """A reversible circuit as ``uint32`` micro-op words (THE WORD of include/fbx.h).  ``gates``: an iterable of ``(name,
    qubits)`` tuples, or an array of words, which is validated and returned.  The list is walked with the basis of every
    qubit's bit -- all start in Z, ``H`` toggles:

    ========= ====================== =====================================
    gate      bases                  micro-op
    ========= ====================== =====================================
    ``H``     any                    error site only
    ``X``     bit held in Z          NOT
    ``X``     bit held in X          error site only
    ``XIN``   bit held in Z          NOT iff the input bit is set
    ``CNOT``  both in Z              XOR into the target
    ``CNOT``  both in X              XOR into the control
    ``CZ``    one in Z, one in X     XOR of the Z-held bit into the X-held one
    ``CZ``    both in Z              error site only
    ``CCNOT`` all three in Z         AND-XOR into the target
    ========= ====================== =====================================

    Anything else would entangle or needs a gate this model does not have: ``ValueError`` with the gate's index and the bases."""
    n = check_width(n)
    if isinstance(gates, np.ndarray) and gates.dtype.kind in "ui":
        return check_words(gates, n)
    gates = list(gates)
    words = np.empty(len(gates), dtype=np.uint32)
    in_x = [False] * n
    arity = {"H": 1, "X": 1, "XIN": 2, "CNOT": 2, "CZ": 2, "CCNOT": 3}
    for i, (name, qubits) in enumerate(gates):
        if name not in arity:
            raise ValueError(f"gate {i}: unknown gate {name!r}")
        qs = tuple(int(q) for q in qubits)
        input_bit = 0
        if name == "XIN":
            if len(qs) != 2 or not 0 <= qs[1] < 64:
                raise ValueError(f"gate {i}: XIN takes (qubit, input bit below 64), not {qs}")
            qs, input_bit = qs[:1], qs[1]
        if len(qs) != (1 if name == "XIN" else arity[name]) or len(set(qs)) != len(qs) or not all(0 <= q < n for q in qs):
            raise ValueError(f"gate {i}: {name} on qubits {qs} of {n}")
        bases = tuple(in_x[q] for q in qs)

        def refuse():
            held = ", ".join(f"qubit {q} in {_BASIS[b]}" for q, b in zip(qs, bases))
            return ValueError(f"gate {i}: {name} with {held} does not act classically on the bits")
        if name == "H":
            in_x[qs[0]] = not in_x[qs[0]]
            words[i] = _word(OP_SITE, qs, (in_x[qs[0]],))
        elif name == "X":
            words[i] = _word(OP_SITE if bases[0] else OP_NOT, qs, bases)
        elif name == "XIN":
            if bases[0]:
                raise refuse()
            words[i] = _word(OP_XIN, qs, bases, input_bit)
        elif name == "CNOT":
            if bases[0] != bases[1]:
                raise refuse()
            words[i] = _word(OP_XOR, qs if bases[0] else qs[::-1], bases)
        elif name == "CZ":
            if bases[0] and bases[1]:
                raise refuse()
            if not bases[0] and not bases[1]:
                words[i] = _word(OP_SITE, qs, bases)
            else:
                words[i] = _word(OP_XOR, qs if bases[0] else qs[::-1], (True, False))
        else:
            if any(bases):
                raise refuse()
            words[i] = _word(OP_ANDXOR, (qs[2], qs[0], qs[1]), (False, False, False))
    return words


def gate_arity(words) -> np.ndarray:
    """The number of qubits of every gate, ``uint8 [G]``: what the default noise classes are made from (class = arity - 1)."""
    return ((np.asarray(words, dtype=np.uint32) >> np.uint32(3)) & np.uint32(3)).astype(np.uint8)


def _bit(v, q):
    return (v >> np.uint64(q)) & _U1


def _apply(op, qs, input_bit, state, inputs):
    """One micro-op on an array of state words; ``inputs`` is the array (or scalar) of input words XIN reads.  Returns the new
    states and, per state, whether the gate exists."""
    exists = np.ones(np.shape(state), dtype=bool)
    if op == OP_NOT:
        state = state ^ (_U1 << np.uint64(qs[0]))
    elif op == OP_XOR:
        state = state ^ (_bit(state, qs[1]) << np.uint64(qs[0]))
    elif op == OP_ANDXOR:
        state = state ^ ((_bit(state, qs[1]) & _bit(state, qs[2])) << np.uint64(qs[0]))
    elif op == OP_XIN:
        on = _bit(np.asarray(inputs, dtype=np.uint64), input_bit)
        state = state ^ (on << np.uint64(qs[0]))
        exists = np.broadcast_to(on != 0, np.shape(state))
    return state, exists


def evaluate(words, n, inputs) -> np.ndarray:
    """The noiseless final state word of every input word, ``uint64`` of ``inputs``' shape: bit q = the bit qubit q holds."""
    words = check_words(words, n)
    inputs = np.asarray(inputs, dtype=np.uint64)
    state = np.zeros(inputs.shape, dtype=np.uint64)
    for w in words.tolist():
        op, qs, _, bit = _fields(w)
        state, _ = _apply(op, qs, bit, state, inputs)
    return state


def check_out_qubits(out_qubits, n) -> np.ndarray:
    out = np.ascontiguousarray(np.asarray(out_qubits, dtype=np.int64).ravel())
    if not 1 <= out.size <= 64 or np.any(out < 0) or np.any(out >= n):
        raise ValueError(f"out_qubits must be 1..64 qubit indices below {n}")
    return out.astype(np.uint8)


def gather_record(state, out_qubits) -> np.ndarray:
    """State words -> packed records: bit j of a record = column j = the bit of qubit ``out_qubits[j]``."""
    state = np.asarray(state, dtype=np.uint64)
    rec = np.zeros(state.shape, dtype=np.uint64)
    for j, q in enumerate(np.asarray(out_qubits).tolist()):
        rec |= _bit(state, q) << np.uint64(j)
    return rec


def pack_records(bits) -> np.ndarray:
    """Bit records ``[.., m]`` 0 / 1 -> packed ``uint64 [..]``, bit j = column j (the form of ``expected`` and ``words_out``)."""
    bits = np.asarray(bits, dtype=np.uint64)
    if bits.shape[-1] > 64:
        raise ValueError("a record has at most 64 columns")
    return (bits << np.arange(bits.shape[-1], dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)


def exact_distribution(words, n, input_word, class_error=None, noise_class=None, readout_flip=None, out_qubits=None):
    """The exact outcome distribution of the noisy circuit on ``out_qubits`` for one input word and one item of noise, without
    sampling: the probability vector over the 2^n classical states is pushed through the circuit -- a gate permutes it, a
    depolarizing site of probability p on k qubits mixes it with its average over the 2^k flips of those bits (a uniformly
    random Pauli flips each operand with probability 1/2, whichever part does the flipping) -- then marginalised and passed
    through the readout confusion of each column.  ``class_error`` is ``[K]`` (or a scalar), ``readout_flip`` ``[m, 2]``.
    Returns ``float64 [2^m]``, column 0 being the most significant bit of the index.  ``n <= 12``."""
    words = check_words(words, n)
    if n > MAX_DENSE_QUBITS:
        raise ValueError(f"exact_distribution is dense: n <= {MAX_DENSE_QUBITS}")
    out = check_out_qubits(range(n) if out_qubits is None else out_qubits, n)
    m = out.size
    ce = None if class_error is None else np.atleast_1d(np.asarray(class_error, dtype=np.float64))[None]
    _, K, ce, cls, flips = frame_noise(m, words.size, ce, noise_class, None if readout_flip is None else np.asarray(readout_flip)[None])
    idx = np.arange(1 << n, dtype=np.uint64)
    p = np.zeros(1 << n)
    p[0] = 1.0
    for l, w in enumerate(words.tolist()):
        op, qs, _, bit = _fields(w)
        image, exists = _apply(op, qs, bit, idx, np.uint64(input_word))
        if not exists.all():
            continue
        moved = np.empty_like(p)
        moved[image.astype(np.int64)] = p
        p = moved
        c = 0 if cls is None else int(cls[l])
        e = 0.0 if (ce is None or c == NOISELESS) else float(ce[0, c])
        if e > 0.0:
            mixed = np.zeros_like(p)
            for pattern in range(1 << len(qs)):
                mask = sum(1 << q for i, q in enumerate(qs) if (pattern >> i) & 1)
                mixed += p[(idx ^ np.uint64(mask)).astype(np.int64)]
            p = (1.0 - e) * p + e * mixed / (1 << len(qs))
    rec = gather_record(idx, out)
    dist = np.zeros(1 << m)
    msb_first = np.zeros(idx.size, dtype=np.int64)
    for j in range(m):
        msb_first |= _bit(rec, j).astype(np.int64) << (m - 1 - j)
    np.add.at(dist, msb_first, p)
    if flips is not None:
        t = dist.reshape((2,) * m)
        for j in range(m):
            f0, f1 = flips[0, j]
            confusion = np.array([[1.0 - f0, f1], [f0, 1.0 - f1]])                  # [read, drawn]
            t = np.moveaxis(np.tensordot(confusion, t, axes=([1], [j])), 0, j)
        dist = t.reshape(-1)
    return dist


def _pauli_flips(d, on_z):
    """Whether the Pauli with index d (0 I, 1 X, 2 Y, 3 Z) flips a bit held in Z (its X part) or in X (its Z part)."""
    return ((d >> _U1) if on_z else (d ^ (d >> _U1))) & _U1


def restate_reversible_shots(words, n, inputs, out_qubits, shots, class_error=None, noise_class=None, readout_flip=None, seed=0,
                             first_item=0, first_input=0) -> np.ndarray:
    """The packed records ``fbx_reversible_sample_shots`` writes, ``uint64 [B, P, shots]`` with bit j = column j, restated shot
    by shot from THE MODEL and THE STREAM of include/fbx.h on the Philox of ``fbx.synthetic``, vectorised over the shots of a
    unit.  The noise arguments are those of ``clifford_circuit.frame_noise`` with ``readout_flip`` per record column
    (``[m, 2]`` or ``[B, m, 2]``); item b is global item ``first_item + b``, input r global input ``first_input + r``.  A
    poisoned item is zeros, as on the device."""
    from ..synthetic import _philox4x32_10
    words = check_words(words, n)
    out = check_out_qubits(out_qubits, n)
    m, G = out.size, int(words.size)
    inputs = np.ascontiguousarray(np.asarray(inputs, dtype=np.uint64).ravel())
    B, K, ce, cls, flips = frame_noise(m, G, class_error, noise_class, readout_flip)
    shots, seed, first_item, first_input = int(shots), int(seed) & (2 ** 64 - 1), int(first_item), int(first_input)
    if not 0 <= shots < 2 ** 32 or first_item < 0 or first_input < 0 or first_item + B > 2 ** 32 or first_input + inputs.size > 2 ** 32:
        raise ValueError("need 0 <= shots < 2^32 and item and input indices in 0 .. 2^32 - 1")
    k0, k1 = (seed & 0xFFFFFFFF) ^ REVERSIBLE_KEY_TAG, seed >> 32
    s = np.arange(shots, dtype=np.uint64)
    records = np.zeros((B, inputs.size, shots), dtype=np.uint64)
    scale = 2.0 ** -32
    fields = [_fields(w) for w in words.tolist()]
    for b in range(B):
        if _bad_probabilities(ce[b] if ce is not None else None) or _bad_probabilities(flips[b] if flips is not None else None):
            continue
        for r in range(inputs.size):
            def block(j):
                return _philox4x32_10(np.uint64(first_item + b), np.uint64(first_input + r), s, np.uint64(j), k0, k1)
            state = np.zeros(shots, dtype=np.uint64)
            have, x = -1, None
            for l, (op, qs, on_z, bit) in enumerate(fields):
                state, exists = _apply(op, qs, bit, state, inputs[r])
                c = 0 if cls is None else int(cls[l])
                p = 0.0 if (ce is None or c == NOISELESS or not exists.all()) else float(ce[b, c])
                if p > 0.0:
                    if have != l >> 1:
                        x, have = block(l >> 1), l >> 1
                    first, second = (x[2], x[3]) if l & 1 else (x[0], x[1])
                    errs = (first.astype(np.float64) * scale < p).astype(np.uint64)
                    k = len(qs)
                    index = second >> np.uint64(32 - 2 * k)
                    for i, q in enumerate(qs):
                        d = (index >> np.uint64(2 * (k - 1 - i))) & np.uint64(3)
                        state = state ^ ((_pauli_flips(d, on_z[i]) & errs) << np.uint64(q))
            rec = gather_record(state, out)
            if flips is not None:
                J = (G + 1) >> 1
                for j in range(m):
                    if j & 3 == 0:
                        x = block(J + (j >> 2))
                    f = np.where(_bit(rec, j) == 1, flips[b, j, 1], flips[b, j, 0])
                    rec = rec ^ ((x[j & 3].astype(np.float64) * scale < f).astype(np.uint64) << np.uint64(j))
            records[b, r] = rec
    return records


def unpack_records(records, m) -> np.ndarray:
    """Packed records ``[..]`` -> bit records ``[.., m]`` uint8, column j = bit j: the layout of ``bits_out``."""
    return unpack_shots(records, m)


def weight_counts(records, expected, m) -> np.ndarray:
    """``int64 [.., P, m + 1]``: per unit the number of packed ``records [.., P, shots]`` that differ from ``expected [P]`` in w
    columns, w = 0..m -- what the device's fused histogram must equal."""
    diff = np.asarray(records, dtype=np.uint64) ^ np.asarray(expected, dtype=np.uint64)[:, None]
    weight = np.zeros(diff.shape, dtype=np.int64)
    for j in range(m):
        weight += _bit(diff, j).astype(np.int64)
    return (weight[..., None] == np.arange(m + 1)).sum(axis=-2).astype(np.int64)


def sample_reversible_shots(words, n, inputs, out_qubits, shots, class_error=None, noise_class=None, readout_flip=None, seed=0,
                            first_item=0, first_input=0, expected=None, bits=True, packed=False, counts=False):
    """``fbx_reversible_sample_shots`` on the selected GPU.  Returns a dict with ``status`` (``int32 [B]``) and what was asked
    for: ``bits`` ``uint8 [B, P, shots, m]``, ``packed`` ``uint64 [B, P, shots]``, ``counts`` ``int64 [B, P, m + 1]`` (needs
    ``expected [P]`` packed records).  With ``counts`` alone no record leaves the device."""
    from .. import _lib
    words = check_words(words, n)
    out = check_out_qubits(out_qubits, n)
    m = int(out.size)
    inputs = np.ascontiguousarray(np.asarray(inputs, dtype=np.uint64).ravel())
    P, shots = int(inputs.size), int(shots)
    B, K, ce, cls, flips = frame_noise(m, words.size, class_error, noise_class, readout_flip)
    exp = None
    if expected is not None:
        exp = np.ascontiguousarray(np.asarray(expected, dtype=np.uint64).ravel())
        if exp.size != P:
            raise ValueError("expected needs one packed record per input")
    if shots < 0:
        raise ValueError("shots must not be negative")
    res = {"status": np.zeros(B, dtype=np.int32)}
    if bits:
        res["bits"] = np.zeros((B, P, shots, m), dtype=np.uint8)
    if packed:
        res["packed"] = np.zeros((B, P, shots), dtype=np.uint64)
    if counts:
        res["counts"] = np.zeros((B, P, m + 1), dtype=np.int64)
    _lib.check(_lib.lib().fbx_reversible_sample_shots(
        int(n), words.size, _lib.ptr(words, C.c_uint32), _lib.ptr(cls, C.c_uint8), K, P, _lib.ptr(inputs, C.c_uint64), m,
        _lib.ptr(out, C.c_uint8), _lib.ptr(exp, C.c_uint64), B, shots, _lib.dptr(ce), _lib.dptr(flips), int(seed) & (2 ** 64 - 1),
        int(first_item), int(first_input), _lib.ptr(res.get("bits"), C.c_uint8), _lib.ptr(res.get("packed"), C.c_uint64),
        _lib.ptr(res.get("counts"), C.c_int64), _lib.iptr(res["status"])))
    return res
