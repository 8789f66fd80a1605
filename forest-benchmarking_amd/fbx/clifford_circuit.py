"""Clifford circuits on up to 64 qubits as lists of gate words, and signed Paulis as (x, z, sign) bit masks: the host mirror of
csrc/fbx_dfe.hip and csrc/fbx_frames.hip in pure numpy (``uint64`` arrays, no device), written from the contract in include/fbx.h.

A Pauli on n <= 64 qubits is two ``uint64`` masks and a sign bit -- bit q belongs to qubit q, per qubit (x, z) = 00 I, 10 X, 11 Y
(the Hermitian Y), 01 Z, and the operator is (-1)^sign times the tensor product.  A gate is one ``uint32`` word: opcode in bits
0..7, q0 in bits 8..15, q1 in bits 16..23.  Conjugating by a gate is a few bit operations on the masks, so what the reference asks
quilc for (``BenchmarkConnection.apply_clifford_to_pauli``) is a loop over the gate list here; ``conjugate_paulis(..., device=0)``
runs the same loop on the GPU, a lane per Pauli.
"""
import numpy as np

from .observable_estimation import PauliTerm

GATE_NAMES = ("H", "S", "SDG", "X", "Y", "Z", "RX(pi/2)", "RX(-pi/2)", "RY(pi/2)", "RY(-pi/2)", "RZ(pi/2)", "RZ(-pi/2)",
              "CNOT", "CZ", "SWAP")
OPCODES = {name: code for code, name in enumerate(GATE_NAMES)}
_FIRST_TWO_QUBIT = OPCODES["CNOT"]
_INVERSE = {OPCODES[a]: OPCODES[b] for a, b in (("S", "SDG"), ("SDG", "S"), ("RX(pi/2)", "RX(-pi/2)"), ("RX(-pi/2)", "RX(pi/2)"),
                                                 ("RY(pi/2)", "RY(-pi/2)"), ("RY(-pi/2)", "RY(pi/2)"), ("RZ(pi/2)", "RZ(-pi/2)"),
                                                 ("RZ(-pi/2)", "RZ(pi/2)"))}
SETTINGS_KEY_TAG = 0x44464553       # "DFES": the stream of the Monte Carlo settings (include/fbx.h)
MAX_ATTEMPTS = 256
NOISELESS = 255
_U1 = np.uint64(1)


def check_width(n) -> int:
    n = int(n)
    if not 1 <= n <= 64:
        raise ValueError("n_qubits must be 1..64")
    return n


def valid_mask(n) -> np.uint64:
    """The mask of the n low bits, without shifting by 64."""
    return np.uint64((2 ** 64 - 1) >> (64 - check_width(n)))


def encode_gates(gates, n) -> np.ndarray:
    """A circuit as ``uint32`` gate words.  ``gates``: an iterable of ``(name, qubits)`` tuples -- the names of ``GATE_NAMES``, which
    include everything ``clifford.to_gates`` emits -- or an array of words, which is validated and returned.  Refused: an unknown
    name or opcode, a qubit index outside ``range(n)``, the wrong number of qubits, ``q0 == q1``, a word with other bits set."""
    n = check_width(n)
    if isinstance(gates, np.ndarray) and gates.dtype.kind in "ui":
        words = np.ascontiguousarray(gates, dtype=np.uint32).ravel()
    else:
        words = np.empty(len(gates), dtype=np.uint32)
        for i, (name, qubits) in enumerate(gates):
            if name not in OPCODES:
                raise ValueError(f"gate {i}: unknown gate {name!r}")
            op = OPCODES[name]
            qs = tuple(int(q) for q in qubits)
            if len(qs) != (2 if op >= _FIRST_TWO_QUBIT else 1) or not all(0 <= q < 256 for q in qs):
                raise ValueError(f"gate {i}: {name} on qubits {qs}")
            words[i] = op | (qs[0] << 8) | ((qs[1] << 16) if len(qs) == 2 else 0)
    op, q0, q1 = words & 0xFF, (words >> 8) & 0xFF, (words >> 16) & 0xFF
    two = op >= _FIRST_TWO_QUBIT
    ok = (op < len(GATE_NAMES)) & (words >> 24 == 0) & (q0 < n) & np.where(two, (q1 < n) & (q1 != q0), q1 == 0)
    if not ok.all():
        raise ValueError(f"gate {int(np.flatnonzero(~ok)[0])} is not a valid gate word on {n} qubits")
    return words


def decode_gates(words):
    """Inverse of ``encode_gates``: the list of ``(name, qubits)`` tuples."""
    out = []
    for w in np.asarray(words, dtype=np.uint32).ravel().tolist():
        op = w & 0xFF
        if op >= len(GATE_NAMES) or w >> 24:
            raise ValueError(f"not a gate word: {w:#x}")
        qs = ((w >> 8) & 0xFF, (w >> 16) & 0xFF) if op >= _FIRST_TWO_QUBIT else ((w >> 8) & 0xFF,)
        out.append((GATE_NAMES[op], qs))
    return out


def _bit(v, q):
    return (v >> np.uint64(q)) & _U1


def _apply_gate(op, q0, q1, x, z, s):
    """U P U^+ for one gate on arrays of Paulis (the table of include/fbx.h): new ``(x, z, sign)``."""
    a, b = np.uint64(q0), np.uint64(q1)
    xa, za = _bit(x, q0), _bit(z, q0)
    name = GATE_NAMES[op]
    if name in ("H", "RY(pi/2)", "RY(-pi/2)"):
        f = {"H": xa & za, "RY(pi/2)": xa & (za ^ _U1), "RY(-pi/2)": za & (xa ^ _U1)}[name]
        d = (xa ^ za) << a
        x, z = x ^ d, z ^ d
    elif name in ("S", "RZ(pi/2)", "SDG", "RZ(-pi/2)"):
        f = xa & za if name in ("S", "RZ(pi/2)") else xa & (za ^ _U1)
        z = z ^ (xa << a)
    elif name == "X":
        f = za
    elif name == "Y":
        f = xa ^ za
    elif name == "Z":
        f = xa
    elif name in ("RX(pi/2)", "RX(-pi/2)"):
        f = za & (xa ^ _U1) if name == "RX(pi/2)" else za & xa
        x = x ^ (za << a)
    else:
        xb, zb = _bit(x, q1), _bit(z, q1)
        if name == "CNOT":
            f = xa & zb & (xb ^ za ^ _U1)
            x, z = x ^ (xa << b), z ^ (zb << a)
        elif name == "CZ":
            f = xa & xb & (za ^ zb)
            z = z ^ (xb << a) ^ (xa << b)
        else:
            f = np.zeros_like(xa)
            x = x ^ ((xa ^ xb) << a) ^ ((xa ^ xb) << b)
            z = z ^ ((za ^ zb) << a) ^ ((za ^ zb) << b)
    return x, z, s ^ f.astype(np.uint8)


def _as_paulis(n, x, z, sign):
    v = valid_mask(n)
    x = np.atleast_1d(np.asarray(x, dtype=np.uint64)) & v
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64)) & v
    s = np.zeros(x.shape, dtype=np.uint8) if sign is None else np.atleast_1d(np.asarray(sign, dtype=np.uint8)) & np.uint8(1)
    if not x.shape == z.shape == s.shape or x.ndim != 1:
        raise ValueError("x, z and sign must be one-dimensional and of one length")
    return np.ascontiguousarray(x), np.ascontiguousarray(z), np.ascontiguousarray(s)


def conjugate_paulis(gates, n, x, z, sign=None, inverse=False, device=None):
    """M Paulis through the circuit: ``U P U^+``, or ``U^+ P U`` with ``inverse=True`` (the list walked backwards, every gate
    inverted).  Returns ``(x, z, sign)``, ``uint64`` / ``uint64`` / ``uint8`` arrays [M].  ``device=None`` computes here in numpy;
    any other value runs ``fbx_clifford_conjugate`` on the selected GPU -- the same bits."""
    words = encode_gates(gates, n)
    x, z, s = _as_paulis(n, x, z, sign)
    if device is not None:
        from . import _lib
        import ctypes as C
        xo, zo, so = np.empty_like(x), np.empty_like(z), np.empty_like(s)
        _lib.check(_lib.lib().fbx_clifford_conjugate(int(n), words.size, _lib.ptr(words, C.c_uint32), int(bool(inverse)), x.size,
                                                     _lib.ptr(x, C.c_uint64), _lib.ptr(z, C.c_uint64), _lib.ptr(s, C.c_uint8),
                                                     _lib.ptr(xo, C.c_uint64), _lib.ptr(zo, C.c_uint64), _lib.ptr(so, C.c_uint8)))
        return xo, zo, so
    seq = words[::-1] if inverse else words
    for w in seq.tolist():
        op = w & 0xFF
        x, z, s = _apply_gate(_INVERSE.get(op, op) if inverse else op, (w >> 8) & 0xFF, (w >> 16) & 0xFF, x, z, s)
    return x, z, s


def paulis_from_labels(labels):
    """Label strings over ``IXYZ`` (index q of a string is qubit q, as ``str_to_pauli_term``) -> ``(x, z)`` ``uint64`` arrays."""
    labels = [labels] if isinstance(labels, str) else list(labels)
    x, z = np.zeros(len(labels), dtype=np.uint64), np.zeros(len(labels), dtype=np.uint64)
    for i, lab in enumerate(labels):
        if len(lab) > 64 or set(lab) - set("IXYZ"):
            raise ValueError(f"not a Pauli label of at most 64 qubits: {lab!r}")
        x[i] = sum(1 << q for q, c in enumerate(lab) if c in "XY")
        z[i] = sum(1 << q for q, c in enumerate(lab) if c in "YZ")
    return x, z


def labels_from_paulis(n, x, z):
    """Inverse of ``paulis_from_labels``: a list of n-character strings."""
    n = check_width(n)
    out = []
    for xi, zi in zip(np.atleast_1d(np.asarray(x, dtype=np.uint64)).tolist(), np.atleast_1d(np.asarray(z, dtype=np.uint64)).tolist()):
        out.append("".join("IXZY"[((xi >> q) & 1) | (((zi >> q) & 1) << 1)] for q in range(n)))
    return out


def apply_clifford_to_pauli(gates, pauli_term, n=None) -> PauliTerm:
    """``BenchmarkConnection.apply_clifford_to_pauli`` for a gate list: the ``PauliTerm`` ``U P U^+``, the input's coefficient times
    the sign of the conjugation.  ``n`` defaults to the smallest width that holds the term's and the circuit's qubits."""
    qubits = [int(q) for q in pauli_term.get_qubits()]
    if n is None:
        used = qubits + ([q for _, qs in gates for q in qs] if not isinstance(gates, np.ndarray)
                         else [q for _, qs in decode_gates(gates) for q in qs])
        n = max(used, default=0) + 1
    if any(not 0 <= q < n for q in qubits):
        raise ValueError(f"the term acts outside range({n})")
    lab = "".join(pauli_term[q] for q in range(n))
    x, z = paulis_from_labels(lab)
    x, z, s = conjugate_paulis(gates, n, x, z)
    out = labels_from_paulis(n, x, z)[0]
    return PauliTerm({q: c for q, c in enumerate(out)}, pauli_term.coefficient * (1 - 2 * int(s[0])))


def _popcount(v):
    v = np.asarray(v, dtype=np.uint64)
    out = np.zeros(v.shape, dtype=np.uint64)
    for q in range(64):
        out += _bit(v, q)
    return out


def propagate_settings(gates, n, in_x, in_z, in_minus, obs_x, obs_z, noise_class=None, n_classes=1):
    """The mirror of ``fbx_dfe_propagate``: every setting's unsigned observable walked backwards through the circuit.  Returns
    ``(sigma int8 [m], touches uint32 [m, K])``: ``touches[k, c]`` counts the gates of class c on whose qubits the walking Pauli is
    not the identity, ``sigma[k]`` is the ideal expectation of the unsigned observable in the setting's in-state (0 when the Pauli
    that arrives at the start is not a stabilizer of the in-state up to sign)."""
    words = encode_gates(gates, n)
    K = int(n_classes)
    if not 1 <= K <= 16:
        raise ValueError("n_classes must be 1..16")
    cls = np.zeros(words.size, dtype=np.uint8) if noise_class is None else np.asarray(noise_class, dtype=np.uint8).ravel()
    if cls.size != words.size or np.any((cls >= K) & (cls != NOISELESS)):
        raise ValueError("noise_class needs one entry per gate, each below n_classes or 255")
    v = valid_mask(n)
    x, z, s = _as_paulis(n, obs_x, obs_z, None)
    in_x, in_z, in_minus = (np.atleast_1d(np.asarray(a, dtype=np.uint64)) & v for a in (in_x, in_z, in_minus))
    if np.any((in_x | in_z) != v):
        raise ValueError("an in-state label is I: every qubit is prepared in an X, Y or Z eigenstate")
    touches = np.zeros((x.size, K), dtype=np.uint32)
    for g in range(words.size - 1, -1, -1):
        w = int(words[g])
        op, q0, q1 = w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF
        if cls[g] != NOISELESS:
            on = _bit(x | z, q0)
            if op >= _FIRST_TWO_QUBIT:
                on = on | _bit(x | z, q1)
            touches[:, cls[g]] += on.astype(np.uint32)
        x, z, s = _apply_gate(_INVERSE.get(op, op), q0, q1, x, z, s)
    support = x | z
    wrong = ((x ^ in_x) | (z ^ in_z)) & support
    parity = (s.astype(np.uint64) + _popcount(in_minus & support)) & _U1
    sigma = np.where(wrong != 0, 0, 1 - 2 * parity.astype(np.int64)).astype(np.int8)
    return sigma, touches


def _reverse_bits(v, n):
    out = np.zeros(v.shape, dtype=np.uint64)
    for q in range(n):
        out |= _bit(v, n - 1 - q) << np.uint64(q)
    return out


def exhaustive_size(n, kind):
    """m of an exhaustive experiment: ``2^n - 1`` (state) or ``(4^n - 1) 2^n`` (process); refused from 2^31 on."""
    n = check_width(n)
    m = (4 ** n - 1) * 2 ** n if kind == "process" else 2 ** n - 1
    if m >= 2 ** 31:
        raise ValueError(f"an exhaustive {kind} experiment on {n} qubits has {m} >= 2^31 settings; use n_terms > 0")
    return m


def restate_dfe_settings(n, kind, n_terms, seed, gates):
    """The settings ``fbx_dfe_settings`` writes, restated from the contract in include/fbx.h -- the exhaustive orders from their
    definition, the Monte Carlo stream on the Philox of ``fbx.synthetic`` -- and conjugated with ``conjugate_paulis``.  Returns
    the dict ``in_x, in_z, in_minus, obs_x, obs_z`` (``uint64`` [m]) and ``obs_sign`` (``uint8`` [m])."""
    from .synthetic import _philox4x32_10
    n = check_width(n)
    if kind not in ("state", "process"):
        raise ValueError('Kind can only be \'state\' or \'process\'.')
    n_terms, seed = int(n_terms), int(seed) & (2 ** 64 - 1)
    if n_terms < 0:
        raise ValueError("n_terms must not be negative")
    process = kind == "process"
    v = valid_mask(n)
    if n_terms == 0:
        k = np.arange(exhaustive_size(n, kind), dtype=np.uint64)
        px = np.zeros(k.size, dtype=np.uint64)
        if not process:
            pz, minus = _reverse_bits(k + _U1, n), np.zeros(k.size, dtype=np.uint64)
        else:
            j, e = (k >> np.uint64(n)) + _U1, k & v
            pz = np.zeros(k.size, dtype=np.uint64)
            for q in range(n):
                digit = (j >> np.uint64(2 * (n - 1 - q))) & np.uint64(3)
                px |= ((digit == 1) | (digit == 2)).astype(np.uint64) << np.uint64(q)
                pz |= ((digit == 2) | (digit == 3)).astype(np.uint64) << np.uint64(q)
            minus = _reverse_bits(e, n)
    else:
        k = np.arange(n_terms, dtype=np.uint64)
        lo, hi = k & np.uint64(0xFFFFFFFF), k >> np.uint64(32)
        k0, k1 = (seed & 0xFFFFFFFF) ^ SETTINGS_KEY_TAG, seed >> 32
        px, pz = np.zeros(k.size, dtype=np.uint64), np.zeros(k.size, dtype=np.uint64)
        attempt = np.zeros(k.size, dtype=np.uint64)
        open_ = np.ones(k.size, dtype=bool)
        for a in range(MAX_ATTEMPTS):
            if not open_.any():
                break
            idx = np.flatnonzero(open_)
            w = _philox4x32_10(lo[idx], hi[idx], np.uint64(a), np.uint64(0), k0, k1)
            first, second = (w[0] | (w[1] << np.uint64(32))) & v, (w[2] | (w[3] << np.uint64(32))) & v
            cx, cz = (first, second) if process else (np.zeros_like(first), first)
            keep = (cx | cz) != 0
            px[idx[keep]], pz[idx[keep]], attempt[idx[keep]] = cx[keep], cz[keep], np.uint64(a)
            open_[idx[keep]] = False
        pz[open_], attempt[open_] = v, np.uint64(MAX_ATTEMPTS)
        if process:
            px[open_] = v
            w = _philox4x32_10(lo, hi, attempt, np.uint64(1), k0, k1)
            minus = (w[0] | (w[1] << np.uint64(32))) & v
        else:
            minus = np.zeros(k.size, dtype=np.uint64)
    support = px | pz
    ox, oz, s = conjugate_paulis(gates, n, px, pz)
    sign = (s.astype(np.uint64) + _popcount(minus & support)) & _U1
    return {"in_x": px, "in_z": pz | (~support & v), "in_minus": minus, "obs_x": ox, "obs_z": oz,
            "obs_sign": sign.astype(np.uint8)}


# --------------------------------------------------------------------------------------------------
# Shots of a noisy Clifford circuit (fbx_clifford_reference_sample, fbx_clifford_sample_shots), restated in numpy from the
# contract in include/fbx.h: a reference outcome of the noiseless circuit and one Pauli frame per shot.
# --------------------------------------------------------------------------------------------------
FRAMES_KEY_TAG = 0x43465253         # "CFRS": the stream of fbx_clifford_sample_shots


def _weight(v) -> int:
    return bin(v).count("1")


def _multiply(a, b):
    """The product of two signed Hermitian Paulis ``(x, z, sign)`` as Python ints.  With P = i^(x.z) X^x Z^z the product is i^e
    times the Pauli ``(x1 ^ x2, z1 ^ z2)``, e = x1.z1 + x2.z2 - x3.z3 + 2 z1.x2 mod 4; for commuting factors e is 0 or 2 and
    its bit 1 is the sign (for anticommuting ones the result is not Hermitian and the sign returned is meaningless)."""
    (x1, z1, r1), (x2, z2, r2) = a, b
    x3, z3 = x1 ^ x2, z1 ^ z2
    e = (_weight(x1 & z1) + _weight(x2 & z2) - _weight(x3 & z3) + 2 * _weight(z1 & x2)) % 4
    return x3, z3, r1 ^ r2 ^ (e >> 1)


def reference_sample(gates, n, device=None) -> int:
    """One outcome of the noiseless circuit ``gates`` on |0..0> measured in Z on every qubit, as an int whose bit q is qubit q:
    the outcome of non-zero probability with the smallest outcome index (qubit 0 is the most significant bit of the index) --
    measure qubits 0, 1, .., n - 1 in this order and take every random result as 0.  ``device=None`` computes here (the stabilizer
    tableau of Aaronson and Gottesman, rows as Python ints); any other value runs ``fbx_clifford_reference_sample`` on the
    selected GPU."""
    n = check_width(n)
    words = encode_gates(gates, n)
    if device is not None:
        from . import _lib
        import ctypes as C
        out = np.zeros(1, dtype=np.uint64)
        _lib.check(_lib.lib().fbx_clifford_reference_sample(n, words.size, _lib.ptr(words, C.c_uint32), _lib.ptr(out, C.c_uint64)))
        return int(out[0])
    one = _U1 << np.arange(n, dtype=np.uint64)
    zero = np.zeros(n, dtype=np.uint64)
    dx, dz, _ = conjugate_paulis(words, n, one, zero)                     # destabilizers U X_i U^+ (their signs are never read)
    sx, sz, sr = conjugate_paulis(words, n, zero, one)                    # stabilizers U Z_i U^+
    destab = [(int(x), int(z)) for x, z in zip(dx, dz)]
    stab = [(int(x), int(z), int(r)) for x, z, r in zip(sx, sz, sr)]
    x0 = 0
    for a in range(n):
        anti = [i for i in range(n) if (stab[i][0] >> a) & 1]
        if anti:                                                          # random: taken as 0
            p = anti[0]
            pivot = stab[p]
            for i in range(n):
                if i == p:
                    continue
                if (stab[i][0] >> a) & 1:
                    stab[i] = _multiply(stab[i], pivot)
                if (destab[i][0] >> a) & 1:
                    destab[i] = (destab[i][0] ^ pivot[0], destab[i][1] ^ pivot[1])
            destab[p] = pivot[:2]
            stab[p] = (0, 1 << a, 0)
        else:                                                             # determined: the sign of a product of stabilizers
            acc = (0, 0, 0)
            for i in range(n):
                if (destab[i][0] >> a) & 1:
                    acc = _multiply(acc, stab[i])
            x0 |= acc[2] << a
    return x0


def frame_noise(n, n_gates, class_error=None, noise_class=None, readout_flip=None):
    """The noise arguments of one frame-sampling call, checked and broadcast: ``(B, K, class_error [B, K] or None, noise_class
    [G] uint8 or None, readout_flip [B, n, 2] or None)``.  ``class_error``: a scalar (B = 1, K = 1) or ``[B, K]``;
    ``noise_class``: one entry per gate, a class below K or 255 (K is ``class_error``'s, or one more than the largest class
    without it); ``readout_flip``: ``[n, 2]`` for the whole batch or ``[B, n, 2]``.  B is 1 when nothing says otherwise."""
    n = check_width(n)
    ce = None
    if class_error is not None:
        ce = np.asarray(class_error, dtype=np.float64)
        if ce.ndim == 0:
            ce = ce.reshape(1, 1)
        if ce.ndim != 2 or not 1 <= ce.shape[1] <= 16:
            raise ValueError("class_error must be a scalar or [B, K] with K in 1..16")
        ce = np.ascontiguousarray(ce)
    cls = None
    if noise_class is not None:
        cls = np.ascontiguousarray(np.asarray(noise_class, dtype=np.uint8).ravel())
        if cls.size != n_gates:
            raise ValueError("noise_class needs one entry per gate")
    if ce is not None:
        K = ce.shape[1]
    else:
        used = cls[cls != NOISELESS] if cls is not None else np.zeros(0, dtype=np.uint8)
        K = int(used.max()) + 1 if used.size else 1
    if cls is not None and np.any((cls >= K) & (cls != NOISELESS)):
        raise ValueError("a noise class is neither below K nor 255")
    if K > 16:
        raise ValueError("at most 16 noise classes")
    flips = None
    if readout_flip is not None:
        flips = np.asarray(readout_flip, dtype=np.float64)
        if flips.shape[-2:] != (n, 2) or flips.ndim not in (2, 3):
            raise ValueError(f"readout_flip must be [n, 2] = {(n, 2)} or [B, n, 2], not {flips.shape}")
    B = ce.shape[0] if ce is not None else (flips.shape[0] if flips is not None and flips.ndim == 3 else 1)
    if flips is not None:
        if flips.ndim == 3 and flips.shape[0] != B:
            raise ValueError(f"readout_flip has {flips.shape[0]} items, class_error {B}")
        flips = np.ascontiguousarray(np.broadcast_to(flips, (B, n, 2)))
    return B, K, ce, cls, flips


def _bad_probabilities(a):
    return a is not None and not bool(np.all((a >= 0.0) & (a <= 1.0)))          # NaN included


def _pauli_bits(k):
    """Pauli index 0 I, 1 X, 2 Y, 3 Z -> (x bit, z bit) as uint64 arrays."""
    return ((k == 1) | (k == 2)).astype(np.uint64), (k >> np.uint64(1)) & _U1


def restate_frame_shots(gates, n, shots, class_error=None, noise_class=None, readout_flip=None, seed=0, first_item=0):
    """The packed outcomes ``fbx_clifford_sample_shots`` writes, ``uint64 [B, shots]`` with bit q = qubit q, restated from THE
    MODEL and THE STREAM of include/fbx.h on the Philox of ``fbx.synthetic``, vectorised over the shots of an item.  The noise
    arguments are those of ``frame_noise``; item b is global item ``first_item + b``.  A poisoned item (a probability outside
    [0, 1] or NaN) is a row of zeros, as on the device."""
    from .synthetic import _philox4x32_10
    n = check_width(n)
    words = encode_gates(gates, n)
    G = int(words.size)
    B, K, ce, cls, flips = frame_noise(n, G, class_error, noise_class, readout_flip)
    shots, seed, first_item = int(shots), int(seed) & (2 ** 64 - 1), int(first_item)
    if not 0 <= shots < 2 ** 32 or first_item < 0:
        raise ValueError("need 0 <= shots < 2^32 and first_item >= 0")
    x0 = np.uint64(reference_sample(words, n))
    v = valid_mask(n)
    k0, k1 = (seed & 0xFFFFFFFF) ^ FRAMES_KEY_TAG, seed >> 32
    s = np.arange(shots, dtype=np.uint64)
    out = np.zeros((B, shots), dtype=np.uint64)
    scale = 2.0 ** -32
    for b in range(B):
        if _bad_probabilities(ce[b] if ce is not None else None) or _bad_probabilities(flips[b] if flips is not None else None):
            continue
        g = first_item + b
        g_lo, g_hi = np.uint64(g & 0xFFFFFFFF), np.uint64(g >> 32)

        def block(j):
            return _philox4x32_10(g_lo, g_hi, s, np.uint64(j), k0, k1)
        w = block(0)
        fx, fz = np.zeros(shots, dtype=np.uint64), (w[0] | (w[1] << np.uint64(32))) & v
        sign = np.zeros(shots, dtype=np.uint8)
        have, w = -1, None
        for l in range(G):
            word = int(words[l])
            op, q0, q1 = word & 0xFF, (word >> 8) & 0xFF, (word >> 16) & 0xFF
            fx, fz, _ = _apply_gate(op, q0, q1, fx, fz, sign)
            c = 0 if cls is None else int(cls[l])
            p = 0.0 if (ce is None or c == NOISELESS) else float(ce[b, c])
            if p > 0.0:
                if have != l >> 1:
                    w, have = block(1 + (l >> 1)), l >> 1
                first, second = (w[2], w[3]) if l & 1 else (w[0], w[1])
                errs = (first.astype(np.float64) * scale < p).astype(np.uint64)
                if op >= _FIRST_TWO_QUBIT:
                    k = second >> np.uint64(28)
                    ax, az = _pauli_bits(k >> np.uint64(2))
                    cx, cz = _pauli_bits(k & np.uint64(3))
                    fx = fx ^ (((ax << np.uint64(q0)) ^ (cx << np.uint64(q1))) * errs)
                    fz = fz ^ (((az << np.uint64(q0)) ^ (cz << np.uint64(q1))) * errs)
                else:
                    px, pz = _pauli_bits(second >> np.uint64(30))
                    fx = fx ^ ((px << np.uint64(q0)) * errs)
                    fz = fz ^ ((pz << np.uint64(q0)) * errs)
        outcome = (x0 ^ fx) & v
        if flips is not None:
            J = 1 + ((G + 1) >> 1)
            for j in range(n):
                if j & 3 == 0:
                    w = block(J + (j >> 2))
                d = _bit(outcome, j)
                f = np.where(d == 1, flips[b, j, 1], flips[b, j, 0])
                outcome = outcome ^ ((w[j & 3].astype(np.float64) * scale < f).astype(np.uint64) << np.uint64(j))
        out[b] = outcome
    return out


def unpack_shots(words, n):
    """Packed outcomes ``[..]`` uint64 (bit q = qubit q) -> bit records ``[.., n]`` uint8, first column = qubit 0."""
    words = np.asarray(words, dtype=np.uint64)
    return ((words[..., None] >> np.arange(check_width(n), dtype=np.uint64)) & _U1).astype(np.uint8)
