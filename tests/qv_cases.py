"""Quantum-volume cases for tests/test_quantum_volume_cpu.py and tests/test_quantum_volume_gpu.py: a numpy restatement of the
state-vector simulation behind ``collect_heavy_outputs`` (the comparison partner above the widths of the goldens; itself pinned to
tests/golden/qv_cases.npz in the CPU test), the derived tolerance, and circuits whose answers are known exactly.

Conventions (quantum_volume.py:113-115 with pyquil's NumpyWavefunctionSimulator): the state is an array of shape (2,) * n with
axis q = qubit q, so the flat index has qubit 0 as its most significant bit; a gate on (q0, q1) contracts the 4 x 4 matrix, its
row / column index split most-significant-first over (q0, q1), with those two axes.
"""
from statistics import median as _median

import numpy as np

U_ROUND = 2.0 ** -53


def simulate(n, pairs, gates):
    """probabilities [2^n] of the circuit of flat gate list pairs [L][2], gates [L][4][4], from |0...0>"""
    wf = np.zeros((2,) * n, dtype=np.complex128)
    wf[(0,) * n] = 1.0
    for (q0, q1), u in zip(pairs, gates):
        q0, q1 = int(q0), int(q1)
        t = np.tensordot(np.asarray(u, dtype=np.complex128).reshape(2, 2, 2, 2), wf, axes=((2, 3), (q0, q1)))
        wf = np.moveaxis(t, (0, 1), (q0, q1))
    return np.abs(wf.reshape(-1)) ** 2


def pairs_of(permutations, pairing="reference"):
    """[depth][width] permutations -> flat [depth * (width // 2)][2] pairs: the index arithmetic of the two pairings, restated"""
    out = []
    for perm in permutations:
        w = len(perm)
        for g in range(w // 2):
            out.append((perm[g], perm[g + 1]) if pairing == "reference" else (perm[2 * g], perm[2 * g + 1]))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def heavy_of(probs):
    """(median, boolean heavy table) by the reference's rule: statistics.median, strictly greater"""
    med = _median([float(p) for p in probs])
    return med, np.asarray(probs) > med


def middle_gap(probs):
    """relative gap between the two middle order statistics, (p_(N/2) - p_(N/2-1)) / median"""
    s = np.sort(probs)
    N = len(s)
    return (s[N // 2] - s[N // 2 - 1]) / (0.5 * (s[N // 2] + s[N // 2 - 1]))


def delta(L):
    """bound on the 2-norm distance of two float64 simulations of L gates: one gate = four length-4 complex dot products, rounding
    error at most about 17 u in the 2-norm of the state (|U| of a 4 x 4 unitary has 2-norm <= 2), for both sides: 64 L u"""
    return 64.0 * L * U_ROUND


def prob_bound(p_ref, L):
    """element-wise bound on |p_dev - p_ref|: 2 sqrt(p_ref) delta_L + delta_L^2"""
    d = delta(L)
    return 2.0 * np.sqrt(p_ref) * d + d * d


def random_circuits(n, count, seed, min_gap=1e-7):
    """`count` model circuits of width n from a seeded Generator (permutations, Haar gates by QR), each with a relative middle gap of
    at least min_gap under BOTH pairings (re-drawn otherwise): permutations [count, n, n], gates [count, n, n // 2, 4, 4]"""
    rng = np.random.default_rng(seed)
    perms, gates = [], []
    while len(perms) < count:
        p = np.stack([rng.permutation(n) for _ in range(n)])
        z = rng.standard_normal((n, n // 2, 4, 4)) + 1j * rng.standard_normal((n, n // 2, 4, 4))
        q, r = np.linalg.qr(z)
        d = np.diagonal(r, axis1=-2, axis2=-1)
        g = q * (d / np.abs(d))[..., None, :]
        flat = g.reshape(-1, 4, 4)
        if all(middle_gap(simulate(n, pairs_of(p, pairing), flat)) >= min_gap for pairing in ("reference", "disjoint")):
            perms.append(p); gates.append(g)
    return np.stack(perms), np.stack(gates)


# ------------------------------------------------------------------------------------------------ exact circuits
I2 = np.eye(2)
X = np.array([[0.0, 1.0], [1.0, 0.0]])
H2 = np.array([[1.0, 1.0], [1.0, -1.0]])                  # sqrt(2) H
XI = np.kron(X, I2)                                        # X on q0 (the more significant bit of the matrix index)
IX = np.kron(I2, X)                                        # X on q1
CNOT = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]], dtype=float)       # control q0, target q1
SWAP = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=float)
HH = np.kron(H2, H2) / 2.0                                 # H (x) H: every entry +-1/2, every product exact


def bit(n, q):
    """value of qubit q in the output index: qubit 0 is the most significant bit"""
    return 1 << (n - 1 - q)


def basis_state_cases(n):
    """[(name, pairs, gates, index)]: permutation-matrix circuits from |0...0>; the whole probability sits at `index`, computed
    here by hand from 'qubit 0 is the most significant bit' and 'q0 is the more significant bit of the matrix index'"""
    a, b = 0, n - 1
    cases = [
        ("XI_first_last", [(a, b)], [XI], bit(n, a)),
        ("IX_first_last", [(a, b)], [IX], bit(n, b)),
        ("XI_last_first", [(b, a)], [XI], bit(n, b)),                                       # q0 > q1
        ("IX_last_first", [(b, a)], [IX], bit(n, a)),
        ("X_then_CNOT", [(a, b), (a, b)], [XI, CNOT], bit(n, a) | bit(n, b)),                  # control set: target flips
        ("X_then_CNOT_reversed_pair", [(b, a), (b, a)], [XI, CNOT], bit(n, a) | bit(n, b)),    # q0 = last qubit is the control
        ("CNOT_control_clear", [(a, b), (b, a)], [XI, CNOT], bit(n, a)),                       # control = last qubit, clear
        ("X_then_SWAP", [(a, b), (a, b)], [XI, SWAP], bit(n, b)),
        ("X_then_SWAP_reversed", [(a, b), (b, a)], [XI, SWAP], bit(n, b)),
    ]
    if n >= 3:
        m = n // 2
        cases += [
            ("XI_middle", [(m, a)], [XI], bit(n, m)),
            ("chain", [(a, m), (a, m), (m, b)], [XI, CNOT, CNOT], bit(n, a) | bit(n, m) | bit(n, b)),
            # X on q1 = m; SWAP (m, b) moves the 1 to b; SWAP (a, m) exchanges two zeros
            ("swap_chain", [(b, m), (m, b), (a, m)], [IX, SWAP, SWAP], bit(n, b)),
        ]
    return [(name, np.asarray(p, dtype=np.int64), np.asarray(g, dtype=np.complex128), idx) for name, p, g, idx in cases]


def hadamard_case(n, kind):
    """H (x) H on the disjoint pairs (0, 1), (2, 3), ...: (pairs, gates, probabilities, median, heavy table), all exact.
    kind 'all': every pair (even n: uniform 2^-n, empty heavy set; odd n, last qubit idle: the N/2 outputs with the last bit 0 hold
    2^-(n-1), median 2^-n, heavy = those); 'all_but_last' (even n >= 4): N/4 outputs hold 2^-(n-2), median 0, heavy = those."""
    N = 1 << n
    npairs = n // 2 - (1 if kind == "all_but_last" else 0)
    pairs = np.asarray([(2 * k, 2 * k + 1) for k in range(npairs)], dtype=np.int64).reshape(-1, 2)
    gates = np.asarray([HH] * npairs, dtype=np.complex128).reshape(-1, 4, 4)
    idle = n - 2 * npairs                                        # the least significant bits of the index stay 0
    idx = np.arange(N)
    support = (idx & ((1 << idle) - 1)) == 0
    probs = np.where(support, 2.0 ** -(2 * npairs), 0.0)
    if idle == 0:
        med, heavy = 2.0 ** -n, np.zeros(N, dtype=bool)
    elif idle == 1:
        med, heavy = 2.0 ** -n, support
    else:
        med, heavy = 0.0, support
    return pairs, gates, probs, med, heavy


def relabel(pairs, pi):
    """the circuit with qubit q renamed pi[q]"""
    return np.asarray(pi)[np.asarray(pairs)]


def relabel_index_map(n, pi):
    """new[i]: the output index of the relabelled circuit that corresponds to output i of the original"""
    idx = np.arange(1 << n)
    new = np.zeros_like(idx)
    for q in range(n):
        new |= ((idx >> (n - 1 - q)) & 1) << (n - 1 - int(pi[q]))
    return new


def bit_array_to_int_rows(bits):
    """utils.py:32-42 for every row: first column most significant"""
    bits = np.asarray(bits).astype(np.int64)
    n = bits.shape[-1]
    return (bits << np.arange(n - 1, -1, -1)).sum(axis=-1)


def count_heavy_direct(bitarrays, heavy_tables):
    """the reference's loop (:333-341) evaluated directly: per circuit, the number of shots whose integer is in the heavy list"""
    return np.asarray([int(np.count_nonzero(np.asarray(h, dtype=bool)[bit_array_to_int_rows(b)])) if len(b) else 0
                       for b, h in zip(bitarrays, heavy_tables)], dtype=np.int64)
