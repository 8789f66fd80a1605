"""The reference's rudimentary compiler (forest/benchmarking/compilation.py) on gate lists: every gate is substituted, one for
one and in a fixed order, by gates of the native set ``I``, ``RX(k pi/2)``, ``RZ(theta)``, ``CZ``, ``XY`` -- no rewiring, no
optimisation, so the output is predictable gate by gate and an error model can be attached to every native gate
(``fbx.native_circuit``).

A gate is ``(name, qubits)`` or ``(name, qubits, angle)`` in the style of ``fbx.clifford.to_gates`` and
``classical_logic.reversible.encode_reversible``.  Accepted: ``I``, ``X``, ``H``, ``T``, ``TDG`` (the reference's ``DAGGER T``),
``RX``, ``RY``, ``RZ``, ``CZ``, ``XY``, ``CNOT``, ``CCNOT``, ``SWAP`` and ``("XIN", (q, k))`` -- ``ripple_carry_adder.adder``'s
run-time input gate, X on qubit q iff bit k of the unit's input word is set.  ``XIN`` compiles to ONE conditional ``RX(pi)``,
written ``("RX", (q,), pi, k)`` (``bitstring_prep``'s ``RX(pi * bit)`` is a magic angle): one error site, and only where the bit
is set.

The helpers ``_RY`` .. ``_CCNOT`` return the reference's expansions as gate lists.  Like the reference's they are right up to a
global phase: ``_X``, ``_H`` and everything built on them must not be controlled.
"""
from math import pi

import numpy as np

__all__ = ["match_global_phase", "is_magic_angle", "basic_compile", "program_unitary", "NATIVE_GATES"]

NATIVE_GATES = ("I", "RX", "RZ", "CZ", "XY")
_ARITY = {"I": 1, "X": 1, "H": 1, "T": 1, "TDG": 1, "RX": 1, "RY": 1, "RZ": 1, "CZ": 2, "XY": 2, "CNOT": 2, "CCNOT": 3, "SWAP": 2,
          "XIN": 1}
_WITH_ANGLE = ("RX", "RY", "RZ", "XY")


def match_global_phase(a, b):
    """compilation.py:12-47 (after cirq): ``(a', b')`` with ``a' == b'`` iff ``a == b exp(i t)`` for some t.  Both matrices are
    rotated so that the entry at the position of ``b``'s largest entry is real and positive in each; an entry on an axis is
    rotated by an exact unit (no rounding is introduced).  Different shapes are returned as they are."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return a, b
    k = np.unravel_index(int(np.argmax(np.abs(b))), b.shape) if b.size else ()

    def unit(v):
        re, im = float(np.real(v)), float(np.imag(v))
        if im == 0:
            return -1 if re < 0 else 1
        if re == 0:
            return 1j if im < 0 else -1j
        return np.exp(-1j * np.arctan2(im, re))

    if not b.size:
        return a, b
    return a * unit(a[k]), b * unit(b[k])


def _RY(angle, q):
    """RY from RX(+-pi/2) and RZ (compilation.py:50-58)."""
    return [("RX", (q,), pi / 2), ("RZ", (q,), angle), ("RX", (q,), -pi / 2)]


def _RX(angle, q):
    """RX of any angle from RX(+-pi/2) and RZ (compilation.py:61-71)."""
    return [("RZ", (q,), pi / 2), ("RX", (q,), pi / 2), ("RZ", (q,), angle), ("RX", (q,), -pi / 2), ("RZ", (q,), -pi / 2)]


def _X(q):
    """X as two RX(pi/2) (compilation.py:74-87); a global phase."""
    return [("RX", (q,), pi / 2), ("RX", (q,), pi / 2)]


def _H(q):
    """H as RY(-pi/2) and RZ(pi) (compilation.py:90-100); a global phase."""
    return _RY(-pi / 2, q) + [("RZ", (q,), pi)]


def _CNOT(q1, q2):
    """CNOT(control q1, target q2) as H CZ H on the target (compilation.py:103-116)."""
    return _H(q2) + [("CZ", (q1, q2))] + _H(q2)


def _T(q, dagger=False):
    """T or its inverse as RZ(+-pi/4) (compilation.py:119-126)."""
    return [("RZ", (q,), -pi / 4 if dagger else pi / 4)]


def _SWAP(q1, q2):
    """SWAP as three CNOTs (compilation.py:129-142)."""
    return _CNOT(q1, q2) + _CNOT(q2, q1) + _CNOT(q1, q2)


def _CCNOT(q1, q2, q3):
    """CCNOT(controls q1, q2; target q3) for a line q1 - q2 - q3 (compilation.py:145-172): the sequence of that listing,
    piece by piece."""
    return (_H(q3) + _CNOT(q2, q3) + _T(q3, dagger=True) + _SWAP(q2, q3) + _CNOT(q1, q2) + _T(q2) + _CNOT(q3, q2)
            + _T(q2, dagger=True) + _CNOT(q1, q2) + _SWAP(q2, q3) + _T(q2) + _T(q3) + _CNOT(q1, q2) + _H(q3) + _T(q1)
            + _T(q2, dagger=True) + _CNOT(q1, q2))


def is_magic_angle(angle) -> bool:
    """compilation.py:175-178: an RX angle the hardware has a pulse for -- 0, +-pi/2 or +-pi, to numpy.isclose."""
    return bool(np.isclose(np.abs(angle), pi / 2) or np.isclose(np.abs(angle), pi) or np.isclose(angle, 0.0))


def _parse(index, gate):
    """``(name, qubits, angle or None, input bit or None)`` of one gate of a list, checked."""
    if not isinstance(gate, (tuple, list)) or len(gate) not in (2, 3, 4):
        raise ValueError(f"gate {index}: a gate is (name, qubits), (name, qubits, angle) or (name, qubits, angle, input bit)")
    name, qubits = gate[0], tuple(int(q) for q in gate[1])
    if name not in _ARITY:
        raise ValueError(f"gate {index}: unknown gate {name!r}")
    extra, bit = None, None
    if name == "XIN":
        if len(qubits) != 2 or len(gate) != 2:
            raise ValueError(f"gate {index}: XIN takes (qubit, input bit), not {qubits}")
        qubits, bit = qubits[:1], qubits[1]
    elif len(gate) == 4 and gate[3] is not None:
        if name not in NATIVE_GATES:
            raise ValueError(f"gate {index}: only a native gate can be conditional, not {name}")
        bit = int(gate[3])
    if bit is not None and not 0 <= bit < 64:
        raise ValueError(f"gate {index}: the input bit of a conditional gate is 0..63, not {bit}")
    if len(qubits) != _ARITY[name]:
        raise ValueError(f"gate {index}: {name} takes {_ARITY[name]} qubit(s), not {len(qubits)}")
    if len(set(qubits)) != len(qubits) or any(q < 0 for q in qubits):
        raise ValueError(f"gate {index}: {name} on qubits {qubits}: a qubit repeats or is negative")
    if name in _WITH_ANGLE:
        if len(gate) < 3 or gate[2] is None:
            raise ValueError(f"gate {index}: {name} needs an angle")
        extra = float(gate[2])
    elif len(gate) >= 3 and gate[2] is not None:
        raise ValueError(f"gate {index}: {name} takes no angle")
    return name, qubits, extra, bit


def _expand(name, qubits, extra, bit):
    if name == "XIN":
        return [("RX", qubits, pi, bit)]                   # bitstring_prep's RX(pi * bit): one gate, there iff the bit is set
    if bit is not None:
        return [(name, qubits, extra, bit)]                # a conditional native gate stays as it is
    if name == "CZ":
        return [("CZ", qubits)]
    if name == "XY":
        return [("XY", qubits, extra)]
    if name == "I":
        return [("I", qubits)]
    if name == "RZ":
        return [("RZ", qubits, extra)]
    if name == "RX":
        return [("RX", qubits, extra)] if is_magic_angle(extra) else _RX(extra, qubits[0])
    if name == "RY":
        return _RY(extra, qubits[0])
    if name == "CNOT":
        return _CNOT(*qubits)
    if name == "CCNOT":
        return _CCNOT(*qubits)
    if name == "SWAP":
        return _SWAP(*qubits)
    if name in ("T", "TDG"):
        return _T(qubits[0], dagger=name == "TDG")
    if name == "H":
        return _H(qubits[0])
    return _X(qubits[0])


def basic_compile(gates, return_origin=False):
    """compilation.py:181-262 on a gate list: every gate replaced by the reference's expansion, in order; the result holds only
    ``I``, ``RX`` (magic angles), ``RZ``, ``CZ``, ``XY``.  ``XIN`` becomes the conditional ``("RX", (q,), pi, k)``: a fourth entry
    of a native gate is the bit of the unit's input word that decides whether the gate, and its error site, exist.
    ``return_origin=True`` also returns ``origin``, ``int64 [G']``: the index of the source gate of every native gate, from
    which a caller builds noise classes per source gate.  An unknown name, a wrong arity or a repeated qubit is a ValueError
    that carries the gate's index."""
    out, origin = [], []
    for i, gate in enumerate(gates):
        piece = _expand(*_parse(i, gate))
        out += piece
        origin += [i] * len(piece)
    return (out, np.asarray(origin, dtype=np.int64)) if return_origin else out


# --------------------------------------------------------------------------------------------------
# The unitary of a gate list
# --------------------------------------------------------------------------------------------------
def _rx(a):
    c, s = np.cos(a / 2), np.sin(a / 2)
    return np.array([[c, -1j * s], [-1j * s, c]])


def _ry(a):
    c, s = np.cos(a / 2), np.sin(a / 2)
    return np.array([[c, -s], [s, c]], dtype=np.complex128)


def _rz(a):
    return np.diag([np.exp(-0.5j * a), np.exp(0.5j * a)])


def _xy(a):
    c, s = np.cos(a / 2), 1j * np.sin(a / 2)
    return np.array([[1, 0, 0, 0], [0, c, s, 0], [0, s, c, 0], [0, 0, 0, 1]], dtype=np.complex128)


def _permutation(k, image):
    m = np.zeros((1 << k, 1 << k), dtype=np.complex128)
    for j in range(1 << k):
        m[image(j), j] = 1.0
    return m


# matrices on the gate's own qubits, the FIRST listed qubit being the most significant bit of the matrix index (pyquil's gate
# definitions: CNOT(control, target) = [[1,0,0,0],[0,1,0,0],[0,0,0,1],[0,0,1,0]])
_FIXED = {
    "I": np.eye(2, dtype=np.complex128),
    "X": np.array([[0, 1], [1, 0]], dtype=np.complex128),
    "H": np.array([[1, 1], [1, -1]], dtype=np.complex128) / np.sqrt(2.0),
    "T": np.diag([1.0, np.exp(0.25j * pi)]),
    "TDG": np.diag([1.0, np.exp(-0.25j * pi)]),
    "CZ": np.diag([1.0, 1.0, 1.0, -1.0]).astype(np.complex128),
    "CNOT": _permutation(2, lambda j: j ^ 1 if j & 2 else j),
    "SWAP": _permutation(2, lambda j: ((j & 1) << 1) | (j >> 1)),
    "CCNOT": _permutation(3, lambda j: j ^ 1 if (j & 6) == 6 else j),
}
_ROTATION = {"RX": _rx, "RY": _ry, "RZ": _rz, "XY": _xy}


def gate_matrix(name, angle=None) -> np.ndarray:
    """The matrix of a gate on its own qubits, the first listed qubit as the most significant bit."""
    return _ROTATION[name](angle) if name in _ROTATION else _FIXED[name]


def apply_gate_dense(u, matrix, qubits, n):
    """``matrix`` (on ``qubits``, first = most significant) applied from the left to ``u [2^n, ...]`` whose row index has qubit
    0 as its LEAST significant bit."""
    k = len(qubits)
    t = u.reshape((2,) * n + (-1,))                          # axis a = qubit n - 1 - a
    axes = [n - 1 - q for q in qubits]
    t = np.tensordot(matrix.reshape((2,) * (2 * k)), t, axes=(list(range(k, 2 * k)), axes))
    return np.moveaxis(t, list(range(k)), axes).reshape(u.shape)


def program_unitary(gates, n_qubits, device=None) -> np.ndarray:
    """The ``2^n x 2^n`` unitary of a gate list of the names ``basic_compile`` accepts (``XIN`` and conditional gates excepted:
    they have no unitary without an input word).  The bit order is pyquil's ``program_unitary`` as the reference's tests use it: qubit 0 is the LEAST
    significant bit of the row and column index, so ``CNOT(0, 1)`` -- control 0 -- exchanges indices 1 and 3 and ``CNOT(1, 0)``
    indices 2 and 3.  (The state-vector kernels index the other way round, qubit 0 most significant; ``fbx_native_unitary``
    converts.)  ``device=None``: dense numpy, gate by gate.  ``device=k``: the list is compiled by ``basic_compile`` and run by
    ``fbx_native_unitary`` on GPU k, so the result agrees with the numpy one up to a global phase."""
    n = int(n_qubits)
    if n < 1:
        raise ValueError("n_qubits must be at least 1")
    parsed = [_parse(i, g) for i, g in enumerate(gates)]
    for i, (name, qubits, _, bit) in enumerate(parsed):
        if bit is not None:
            raise ValueError(f"gate {i}: a conditional gate has no unitary without an input word")
        if any(q >= n for q in qubits):
            raise ValueError(f"gate {i}: {name} on qubits {qubits} of {n}")
    if device is not None:
        from . import _lib, native_circuit
        if int(device) != _lib.device_id()[0]:
            _lib.set_device(int(device))
        words, angles = native_circuit.encode_native(basic_compile(gates), n)
        return native_circuit.native_unitary(words, angles, n)
    u = np.eye(1 << n, dtype=np.complex128)
    for name, qubits, angle, _ in parsed:
        u = apply_gate_dense(u, gate_matrix(name, angle), qubits, n)
    return u
