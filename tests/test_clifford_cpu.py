"""fbx.clifford, the host mirror of the Clifford group engine (no device): group theory, and dense numpy unitaries built here.

The truth is the group's own structure (orders 24 and 11 520, inverses, associativity, the homomorphism onto signed permutation
matrices) and, for the conventions -- qubit order, Pauli order, signs, native gates -- the Pauli transfer matrices
``2^-n tr(P_i U P_j U^+)`` of the 2 x 2 / 4 x 4 unitaries of a word's gates, computed in this file."""
import itertools

import numpy as np
import pytest

from fbx import clifford as cl

PAULI_1Q = np.array([[[1, 0], [0, 1]], [[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]]], dtype=complex)


def paulis(n):
    """itertools.product('IXYZ', repeat=n), qubit 0 the left-most tensor factor: the project's order"""
    out = []
    for digits in itertools.product(range(4), repeat=n):
        m = np.ones((1, 1), dtype=complex)
        for g in digits:
            m = np.kron(m, PAULI_1Q[g])
        out.append(m)
    return np.array(out)


def unitary_ptm(u, n):
    p = paulis(n)
    return np.real(np.einsum('iab,bc,jcd,da->ij', p, u, p, u.conj().T)) / 2 ** n


def rx(theta):
    return np.cos(theta / 2) * PAULI_1Q[0] - 1j * np.sin(theta / 2) * PAULI_1Q[1]


def rz(theta):
    return np.cos(theta / 2) * PAULI_1Q[0] - 1j * np.sin(theta / 2) * PAULI_1Q[3]


GATE_1Q = {"RX(pi/2)": rx(np.pi / 2), "RX(-pi/2)": rx(-np.pi / 2), "RZ(pi/2)": rz(np.pi / 2)}
CZ = np.diag([1, 1, 1, -1]).astype(complex)


def gate_unitary(name, qubits, n):
    if name == "CZ":
        assert n == 2 and tuple(qubits) == (0, 1)
        return CZ
    factors = [np.eye(2, dtype=complex)] * n
    factors[qubits[0]] = GATE_1Q[name]
    u = np.ones((1, 1), dtype=complex)
    for f in factors:
        u = np.kron(u, f)                       # qubit 0 is the left-most factor
    return u


@pytest.fixture(scope="module", params=[1, 2])
def grp(request):
    n = request.param
    return n, [int(e) for e in cl.group(n)]


def test_from_index_is_a_bijection_onto_the_group(grp):
    n, g = grp
    assert len(g) == cl.ORDER[n] == (24 if n == 1 else 11520)
    assert len(set(g)) == len(g)
    assert all(cl.is_valid(e, n) for e in g)
    assert cl.identity(n) in g
    assert (cl.to_ptm(cl.identity(n), n) == np.eye(4 ** n)).all()
    assert cl.from_index(n, np.arange(5)).dtype == np.uint32


def test_every_element_times_its_inverse_is_the_identity(grp):
    n, g = grp
    one = cl.identity(n)
    for e in g:
        inv = cl.inverse(e, n)
        assert cl.compose(e, inv, n) == one and cl.compose(inv, e, n) == one


def test_composition_is_associative_and_a_homomorphism_onto_ptms(grp):
    n, g = grp
    rs = np.random.RandomState(11)
    for _ in range(200):
        a, b, c = (g[i] for i in rs.randint(0, len(g), 3))
        assert cl.compose(cl.compose(a, b, n), c, n) == cl.compose(a, cl.compose(b, c, n), n)
        assert (cl.to_ptm(cl.compose(a, b, n), n) == cl.to_ptm(a, n) @ cl.to_ptm(b, n)).all()


def test_gate_words_reproduce_the_ptm_of_every_element(grp):
    """pins qubit order, Pauli order, signs and the native gates to dense unitaries"""
    n, g = grp
    gate_ptm = {}
    longest = 0
    for e in g:
        word = cl.to_gates(e, n)
        longest = max(longest, len(word))
        m = np.eye(4 ** n)
        for name, qubits in word:                # applied in order: later gates multiply from the left
            key = (name, tuple(qubits))
            if key not in gate_ptm:
                gate_ptm[key] = np.round(unitary_ptm(gate_unitary(name, qubits, n), n), 12)
                assert set(np.unique(np.abs(gate_ptm[key]))) <= {0.0, 1.0}
            m = gate_ptm[key] @ m
        assert (m == cl.to_ptm(e, n)).all(), (hex(e), word)
    assert len(gate_ptm) == (3 if n == 1 else 7)
    assert longest == (4 if n == 1 else 11)              # the diameter of the group under this gate set
    assert cl.to_gates(cl.identity(n), n) == []


def test_gate_words_as_whole_unitaries_on_a_sample():
    """the product of the gates' UNITARIES (not of their rounded PTMs) gives the element's PTM after rounding at 1e-12"""
    rs = np.random.RandomState(5)
    for n in (1, 2):
        g = cl.group(n)
        for e in [int(x) for x in rs.choice(g, 24 if n == 1 else 60, replace=n == 2)]:
            u = np.eye(2 ** n, dtype=complex)
            for name, qubits in cl.to_gates(e, n):
                u = gate_unitary(name, qubits, n) @ u
            got = unitary_ptm(u, n)
            assert np.abs(got - np.round(got)).max() < 1e-12
            assert (np.round(got) == cl.to_ptm(e, n)).all()


def test_shortest_words_are_shortest_for_one_qubit():
    """brute force over all words of up to 3 gates: nothing shorter than to_gates reaches the same element"""
    gates = [e for _, e in cl._native_gates(1)]
    reach = {cl.identity(1): 0}
    frontier = [cl.identity(1)]
    for length in (1, 2, 3, 4):
        nxt = []
        for e in frontier:
            for g in gates:
                c = cl.compose(g, e, 1)
                if c not in reach:
                    reach[c] = length
                    nxt.append(c)
        frontier = nxt
    for e, length in reach.items():
        assert len(cl.to_gates(e, 1)) == length


def test_apply_to_pauli_is_the_ptm_column(grp):
    n, g = grp
    rs = np.random.RandomState(3)
    sample = g if n == 1 else [g[i] for i in rs.randint(0, len(g), 300)]
    for e in sample:
        m = cl.to_ptm(e, n)
        for k in range(4 ** n):
            p, s = cl.apply_to_pauli(e, k, n)
            col = np.zeros(4 ** n)
            col[p] = s
            assert s in (1, -1) and (m[:, k] == col).all()
        assert cl.apply_to_pauli(e, 0, n) == (0, 1)


def test_known_elements():
    # Hadamard: X <-> Z;  phase gate S = RZ(pi/2) up to phase: X -> Y, Z -> Z
    h = 3 | (1 << 5)
    assert cl.is_valid(h, 1) and cl.apply_to_pauli(h, 2) == (2, -1)            # H Y H = -Y
    s = 2 | (3 << 5)
    assert cl.to_gates(s) == [("RZ(pi/2)", (0,))]
    assert cl.apply_to_pauli(cl.compose(s, s), 1) == (1, -1)                   # Z X Z = -X
    cz = cl.gate_word("CZ", (0, 1))
    assert cl.gate_word("RZ(pi/2)", (0,)) == s and cl.is_valid(cz) and cl.is_valid(s)
    with pytest.raises(ValueError, match="no native gate"):
        cl.gate_word("CZ", (1, 0))
    assert cl.apply_to_pauli(cz, 4) == (7, 1) and cl.apply_to_pauli(cz, 1) == (13, 1)     # X_0 -> X_0 Z_1, X_1 -> Z_0 X_1
    assert cl.apply_to_pauli(cz, 5) == (10, 1)                                   # X_0 X_1 -> Y_0 Y_1
    assert cl.compose(cz, cz) == cl.identity(2)


def test_argument_errors():
    for n in (0, 3):
        with pytest.raises(ValueError, match="n_qubits must be 1 or 2"):
            cl.from_index(n, 0)
        with pytest.raises(ValueError, match="n_qubits must be 1 or 2"):
            cl.is_valid(0x61, n)
    for n, bad in ((1, 24), (1, -1), (2, 11520)):
        with pytest.raises(ValueError, match="Clifford index must be in range"):
            cl.from_index(n, bad)
    invalid_1q = [0, 1 | (1 << 5), 0x61 | (1 << 10), 5 | (3 << 5)]              # identity image; X, X; a stray high bit; index 5
    for w in invalid_1q:
        assert not cl.is_valid(w, 1)
        for fn in (cl.inverse, cl.to_ptm, cl.to_gates, lambda e, n: cl.compose(e, 0x61, n), lambda e, n: cl.compose(0x61, e, n),
                   lambda e, n: cl.apply_to_pauli(e, 1, n)):
            with pytest.raises(ValueError, match="not a valid 1-qubit Clifford element word"):
                fn(w, 1)
    two = cl.identity(2)
    assert not cl.is_valid(two ^ (1 << 10) ^ (4 << 10), 2)       # X_1 -> X_0: no longer commutes with the image of Z_0
    assert not cl.is_valid(two | (1 << 20), 2)
    assert not cl.is_valid(-1, 2) and not cl.is_valid(cl.NONE, 2) and not cl.is_valid(cl.NONE)
    with pytest.raises(ValueError, match="Pauli index must be in range"):
        cl.apply_to_pauli(0x61, 4)
    n_valid = sum(cl.is_valid(w, 1) for w in range(1 << 11))
    assert n_valid == 24
