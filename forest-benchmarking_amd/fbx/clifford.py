"""The 1- and 2-qubit Clifford groups modulo global phase, on the host (pure numpy, no device, no quilc).

This is the host mirror of csrc/fbx_clifford.hip and the stand-in for the reference's ``BenchmarkConnection`` (quilc): sample,
compose, invert, conjugate a Pauli, and compile to native gates.

Element word (include/fbx.h, "Clifford elements"): a group element C is the signed Pauli images C g C^+ of the generators
g = X_0, Z_0 (n = 1) or X_0, Z_0, X_1, Z_1 (n = 2), five bits each, image j in bits [5 j, 5 j + 5): the low four bits are the Pauli
index of the image, bit 4 is set for a minus sign.  Pauli indices are the project's: base-4 digits I X Y Z = 0 1 2 3, qubit 0 the
most significant digit (``itertools.product('IXYZ', repeat=n)``).  A word is valid when every other bit is zero, the images of X_q
and Z_q anticommute, and images that belong to different qubits commute; there are 24 / 11 520 valid words.

``from_index`` enumerates the group by choosing the images one after the other (a symplectic basis built greedily, the idea of
Koenig and Smolin's enumeration without their transvections, times the 4^n sign choices): ``idx = signs + 4^n r``; for n = 2,
``r = c0 + 15 (c1 + 8 (c2 + 3 c3))`` and
  X_0 -> the c0-th non-identity Pauli,                                   15 choices
  Z_0 -> the c1-th Pauli that anticommutes with the image of X_0,         8
  X_1 -> the c2-th non-identity Pauli that commutes with both,            3
  Z_1 -> the c3-th Pauli that commutes with both and anticommutes with the image of X_1,   2
each counted in ascending Pauli index; for n = 1, ``r = c0 + 3 c1`` with 3 and 2 choices.  Bit j of ``signs`` is the sign of image j.
Every valid word is produced by exactly one index.
"""
from collections import deque
from functools import lru_cache

import numpy as np

ORDER = {1: 24, 2: 11520}
NONE = 0xFFFFFFFF               # "no interleaved element" in fbx_rb_sequences
# 2-bit phase exponents of single-qubit Pauli products a b = i^ph P_{a xor b}, entry 4 a + b: XY = iZ, YZ = iX, ZX = iY
_PHASE_LUT = 0x344CD000
_GEN_INDEX = {1: (1, 3), 2: (4, 12, 1, 3)}      # Pauli indices of X_0, Z_0[, X_1, Z_1]


def _check_n(n):
    if n not in (1, 2):
        raise ValueError("Clifford group engine: n_qubits must be 1 or 2")
    return int(n)


def _mul_phase(a, b):
    """Phase exponent (mod 4, unreduced) of the product of the Paulis with indices a, b < 16; the product's index is a ^ b."""
    return ((_PHASE_LUT >> (2 * ((a & 12) | (b >> 2)))) & 3) + ((_PHASE_LUT >> (2 * (((a & 3) << 2) | (b & 3)))) & 3)


def _anticommute(a, b):
    return _mul_phase(a, b) & 1


def _images(n, elem):
    return [((elem >> (5 * j)) & 15, (elem >> (5 * j + 4)) & 1) for j in range(2 * n)]


def _pack(images):
    w = 0
    for j, (p, s) in enumerate(images):
        w |= (p | (s << 4)) << (5 * j)
    return w


def identity(n):
    return _pack([(g, 0) for g in _GEN_INDEX[_check_n(n)]])


def is_valid(elem, n=None) -> bool:
    """Whether the word is an element of the n-qubit group; ``n`` defaults, as everywhere, to the width the word's size implies."""
    elem = int(elem)
    n = _infer_n(elem) if n is None else _check_n(n)
    if elem < 0 or elem >> (10 * n):
        return False
    im = [p for p, _ in _images(n, elem)]
    if n == 1 and any(p >> 2 for p in im):
        return False
    for i in range(2 * n):
        for j in range(i + 1, 2 * n):
            partners = (i >> 1) == (j >> 1)
            if _anticommute(im[i], im[j]) != int(partners):
                return False
    return True


def _require_valid(n, elem):
    if not is_valid(elem, n):
        raise ValueError(f"not a valid {n}-qubit Clifford element word: {int(elem):#x}")
    return int(elem)


def from_index(n, idx):
    """The idx-th element of the n-qubit Clifford group, idx in range(24) / range(11520); arrays give uint32 arrays."""
    n = _check_n(n)
    if np.ndim(idx):
        return np.array([from_index(n, int(i)) for i in np.asarray(idx).ravel()], dtype=np.uint32).reshape(np.shape(idx))
    idx = int(idx)
    if not 0 <= idx < ORDER[n]:
        raise ValueError(f"Clifford index must be in range({ORDER[n]})")
    signs, r = idx & (4 ** n - 1), idx >> (2 * n)
    radix = (3, 2) if n == 1 else (15, 8, 3, 2)
    chosen = []
    for j, base in enumerate(radix):
        c, r = r % base, r // base
        for cand in range(1, 4 ** n):
            ok = all(not _anticommute(cand, p) for p in chosen[:2 * (j >> 1)])
            if j & 1:
                ok = ok and _anticommute(cand, chosen[j - 1])
            if ok:
                if c == 0:
                    chosen.append(cand)
                    break
                c -= 1
    return _pack([(p, (signs >> j) & 1) for j, p in enumerate(chosen)])


def _apply(n, elem, k):
    """(index, sign bit) of C P_k C^+ for a word known to be valid."""
    im = _images(n, elem)
    acc, ph = 0, 0
    for q in range(n):
        g = (k >> (2 * (n - 1 - q))) & 3
        (px, sx), (pz, sz) = im[2 * q], im[2 * q + 1]
        if g == 1 or g == 2:
            ph += _mul_phase(acc, px) + 2 * sx
            acc ^= px
        if g == 2 or g == 3:
            ph += _mul_phase(acc, pz) + 2 * sz
            acc ^= pz
        if g == 2:
            ph += 1                     # Y = i X Z
    assert ph & 1 == 0
    return acc, (ph >> 1) & 1


def apply_to_pauli(elem, pauli_index, n=None):
    """Conjugate the Pauli with index ``pauli_index`` by the element: ``(index, sign)`` with sign +1 / -1.  ``n`` defaults to the
    width the word's size implies (a 2-qubit word has bits above bit 9)."""
    n = _infer_n(elem) if n is None else _check_n(n)
    elem = _require_valid(n, elem)
    if not 0 <= int(pauli_index) < 4 ** n:
        raise ValueError(f"Pauli index must be in range({4 ** n})")
    p, s = _apply(n, elem, int(pauli_index))
    return p, 1 - 2 * s


def _infer_n(elem):
    return 2 if int(elem) >> 10 else 1


def _table(n, elem):
    return [_apply(n, elem, k) for k in range(4 ** n)]


def compose(a, b, n=None):
    """a after b: ``to_ptm(compose(a, b)) == to_ptm(a) @ to_ptm(b)``."""
    n = _infer_n(a) if n is None else _check_n(n)
    return _compose(n, _require_valid(n, a), _require_valid(n, b))


def _compose(n, a, b):
    out = []
    for p, s in _images(n, b):
        q, t = _apply(n, a, p)
        out.append((q, s ^ t))
    return _pack(out)


def inverse(elem, n=None):
    n = _infer_n(elem) if n is None else _check_n(n)
    elem = _require_valid(n, elem)
    tab = _table(n, elem)
    out = []
    for g in _GEN_INDEX[n]:
        k = next(k for k, (p, _) in enumerate(tab) if p == g)
        out.append((k, tab[k][1]))
    return _pack(out)


def to_ptm(elem, n=None):
    """The Pauli transfer matrix of the element: a signed permutation matrix, entry [apply(k), k] = sign."""
    n = _infer_n(elem) if n is None else _check_n(n)
    elem = _require_valid(n, elem)
    D = 4 ** n
    m = np.zeros((D, D))
    for k, (p, s) in enumerate(_table(n, elem)):
        m[p, k] = 1.0 - 2.0 * s
    return m


# ---- native gates.  Conjugation by RX(+-pi/2), RZ(pi/2), CZ on the generators (U g U^+):
#   RX(pi/2): X -> X, Z -> -Y      RX(-pi/2): X -> X, Z -> Y      RZ(pi/2): X -> Y, Z -> Z      CZ: X_0 -> X_0 Z_1, X_1 -> Z_0 X_1
def _native_gates(n):
    one = {"RX(pi/2)": ((1, 0), (2, 1)), "RX(-pi/2)": ((1, 0), (2, 0)), "RZ(pi/2)": ((2, 0), (3, 0))}
    gates = []
    for q in range(n):
        shift = 2 * (n - 1 - q)
        for name, (ix, iz) in one.items():
            im = [(g, 0) for g in _GEN_INDEX[n]]
            im[2 * q] = (ix[0] << shift, ix[1])
            im[2 * q + 1] = (iz[0] << shift, iz[1])
            gates.append(((name, (q,)), _pack(im)))
    if n == 2:
        gates.append((("CZ", (0, 1)), _pack([(4 | 3, 0), (12, 0), (12 | 1, 0), (3, 0)])))
    return gates


def gate_word(name, qubits, n=None):
    """The element word of one native gate: ``name`` in 'RX(pi/2)', 'RX(-pi/2)', 'RZ(pi/2)' with ``qubits = (q,)``, or 'CZ' with
    ``(0, 1)``; ``n`` defaults to 2 for CZ and to q + 1 otherwise."""
    qubits = tuple(int(q) for q in qubits)
    n = (2 if name == "CZ" else max(qubits, default=0) + 1) if n is None else n
    for label, word in _native_gates(_check_n(n)):
        if label == (name, qubits):
            return word
    raise ValueError(f"no native gate {name!r} on qubits {qubits} of {n}")


@lru_cache(maxsize=None)
def _gate_table(n):
    """Breadth-first search over the whole group from the identity: element -> (previous element, gate applied after it)."""
    gates = _native_gates(n)
    start = identity(n)
    back = {start: None}
    queue = deque([start])
    while queue:
        e = queue.popleft()
        for label, g in gates:
            nxt = _compose(n, g, e)
            if nxt not in back:
                back[nxt] = (e, label)
                queue.append(nxt)
    assert len(back) == ORDER[n]
    return back


def to_gates(elem, n=None):
    """A shortest word for the element over RX(pi/2), RX(-pi/2), RZ(pi/2) on each qubit and CZ, in the order the gates are
    applied: a list of ``(name, qubits)`` tuples, qubits counted within the element (0, 1).  Equal up to a global phase."""
    n = _infer_n(elem) if n is None else _check_n(n)
    elem = _require_valid(n, elem)
    back = _gate_table(n)
    word = []
    while back[elem] is not None:
        elem, label = back[elem]
        word.append(label)
    return word[::-1]


def group(n):
    """All elements, ``from_index(n, range(order))``, cached."""
    return _group(_check_n(n)).copy()


@lru_cache(maxsize=None)
def _group(n):
    return from_index(n, np.arange(ORDER[n]))
