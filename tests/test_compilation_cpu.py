"""fbx.compilation against the reference's compilation.py and its tests (no GPU): the expansions gate for gate -- the expected
sequences below are read off compilation.py:50-172 --, ``match_global_phase``, and the numpy ``program_unitary`` of every
helper and of the reference's random programs against the gates they replace, up to a global phase with the reference's own
tolerance atol = 1e-12 (its test_compilation.py:49-93, :167-174)."""
import itertools
from math import pi

import numpy as np
import pytest

import native_cases as cases
from fbx import compilation as comp

Q, R = 3, 5          # qubits of the literal expansions: neither 0 nor adjacent, so that a mixed-up operand shows


def rx(a, q):
    return ("RX", (q,), a)


def rz(a, q):
    return ("RZ", (q,), a)


H_Q = [rx(pi / 2, Q), rz(-pi / 2, Q), rx(-pi / 2, Q), rz(pi, Q)]
H_R = [rx(pi / 2, R), rz(-pi / 2, R), rx(-pi / 2, R), rz(pi, R)]


def test_literal_expansions():
    assert comp._RY(0.3, Q) == [rx(pi / 2, Q), rz(0.3, Q), rx(-pi / 2, Q)]
    assert comp._RX(0.3, Q) == [rz(pi / 2, Q), rx(pi / 2, Q), rz(0.3, Q), rx(-pi / 2, Q), rz(-pi / 2, Q)]
    assert comp._X(Q) == [rx(pi / 2, Q), rx(pi / 2, Q)]
    assert comp._H(Q) == H_Q
    assert comp._CNOT(Q, R) == H_R + [("CZ", (Q, R))] + H_R          # H on the target around CZ(control, target)
    assert comp._CNOT(R, Q) == H_Q + [("CZ", (R, Q))] + H_Q
    assert comp._T(Q) == [rz(pi / 4, Q)] and comp._T(Q, dagger=True) == [rz(-pi / 4, Q)]
    assert comp._SWAP(Q, R) == comp._CNOT(Q, R) + comp._CNOT(R, Q) + comp._CNOT(Q, R)


def test_gate_counts():
    assert len(comp._H(0)) == 4 and len(comp._CNOT(0, 1)) == 9 and len(comp._SWAP(0, 1)) == 27
    ccnot = comp._CCNOT(0, 1, 2)
    assert len(ccnot) == 123
    names = [g[0] for g in ccnot]
    # 2 H, 6 CNOT and 2 SWAP = 12 CNOT in all, 7 T: 2 * 4 + 12 * 9 + 7 gates; 2 + 2 * 12 = 26 H of two RX and two RZ each
    assert 2 * 4 + 12 * 9 + 7 == 123
    assert names.count("CZ") == 12 and names.count("RX") == 2 * 26 and names.count("RZ") == 2 * 26 + 7 and set(names) == {"RX", "RZ", "CZ"}
    quarter = [g[2] for g in ccnot if g[0] == "RZ" and np.isclose(abs(g[2]), pi / 4)]
    assert len(quarter) == 7 and sorted(np.sign(quarter)) == [-1.0] * 3 + [1.0] * 4


def test_ccnot_sequence_piece_by_piece():
    a, b, c = 4, 1, 6
    want = (comp._H(c) + comp._CNOT(b, c) + comp._T(c, True) + comp._SWAP(b, c) + comp._CNOT(a, b) + comp._T(b) + comp._CNOT(c, b)
            + comp._T(b, True) + comp._CNOT(a, b) + comp._SWAP(b, c) + comp._T(b) + comp._T(c) + comp._CNOT(a, b) + comp._H(c)
            + comp._T(a) + comp._T(b, True) + comp._CNOT(a, b))
    assert comp._CCNOT(a, b, c) == want == comp.basic_compile([("CCNOT", (a, b, c))])


def test_is_magic_angle():
    for k in (-1.0, -0.5, 0.0, 0.5, 1.0):
        assert comp.is_magic_angle(k * pi) and comp.is_magic_angle(k * pi + 1e-12)
    for a in (0.3, pi / 4, 3 * pi / 2, 2 * pi, -0.1):
        assert not comp.is_magic_angle(a)


def test_basic_compile_gate_by_gate():
    prog = [("I", (2,)), ("X", (1,)), ("H", (Q,)), ("T", (0,)), ("TDG", (0,)), ("RX", (1,), -pi / 2), ("RX", (1,), 0.3), ("RY", (2,), 1.1),
            ("RZ", (0,), -2.0), ("CZ", (2, 0)), ("XY", (0, 1), 0.7), ("CNOT", (Q, R)), ("SWAP", (0, 2)), ("CCNOT", (2, 0, 1)),
            ("XIN", (4, 9))]
    pieces = [[("I", (2,))], comp._X(1), H_Q, comp._T(0), comp._T(0, True), [rx(-pi / 2, 1)], comp._RX(0.3, 1), comp._RY(1.1, 2),
              [rz(-2.0, 0)], [("CZ", (2, 0))], [("XY", (0, 1), 0.7)], comp._CNOT(Q, R), comp._SWAP(0, 2), comp._CCNOT(2, 0, 1),
              [("RX", (4,), pi, 9)]]
    native, origin = comp.basic_compile(prog, return_origin=True)
    assert native == [g for piece in pieces for g in piece] == comp.basic_compile(prog)
    assert origin.dtype == np.int64 and origin.tolist() == [i for i, piece in enumerate(pieces) for _ in piece]
    assert {g[0] for g in native} <= set(comp.NATIVE_GATES)
    assert all(comp.is_magic_angle(g[2]) for g in native if g[0] == "RX")
    assert comp.basic_compile(native) == native                      # native gates, the conditional one included, pass through
    assert comp.basic_compile([]) == []


def test_the_input_gate_is_one_conditional_pulse():
    from fbx.classical_logic import ripple_carry_adder as rca
    gates, _ = rca.adder(*rca.default_adder_registers(3))
    native, origin = comp.basic_compile(gates, return_origin=True)
    conditional = [g for g in native if len(g) == 4]
    assert len(conditional) == 6 and all(g[0] == "RX" and g[2] == pi for g in conditional)
    assert sorted(g[3] for g in conditional) == list(range(6))
    assert np.bincount(origin)[[i for i, g in enumerate(gates) if g[0] == "XIN"]].tolist() == [1] * 6
    assert np.bincount(origin)[[i for i, g in enumerate(gates) if g[0] == "CCNOT"]].tolist() == [123] * 6


@pytest.mark.parametrize("gates,index", [
    ([("H", (0,)), ("FOO", (0,))], 1), ([("CNOT", (0,))], 0), ([("H", (0, 1))], 0), ([("H", (0,)), ("H", (1,)), ("CNOT", (1, 1))], 2),
    ([("CCNOT", (0, 1, 0))], 0), ([("RZ", (0,))], 0), ([("H", (0,), 0.5)], 0), ([("XIN", (0,))], 0), ([("XIN", (0, 64))], 0),
    ([("H", (-1,))], 0), ([("CNOT", (0, 1), None, 3)], 0), ([("I", (0,)), "H"], 1)])
def test_refusals_carry_the_gate_index(gates, index):
    with pytest.raises(ValueError, match=f"gate {index}:"):
        comp.basic_compile(gates)


def test_match_global_phase():
    rng = np.random.default_rng(5)
    a = rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4))
    for phase in (0.3, -2.0, pi):
        x, y = comp.match_global_phase(a, a * np.exp(1j * phase))
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-14)
        k = np.unravel_index(np.argmax(np.abs(a)), a.shape)
        assert abs(x[k].imag) < 1e-15 and x[k].real > 0             # the largest entry of b is made real and positive
    x, y = comp.match_global_phase(a, 2 * a)
    assert not np.allclose(x, y)
    # axis-aligned entries are rotated by exact units: no rounding at all
    m = np.array([[0, 1], [1, 0]], dtype=np.complex128)
    for unit in (1, -1, 1j, -1j):
        x, y = comp.match_global_phase(m, unit * m)
        assert np.array_equal(x, m) and np.array_equal(y, m)
    # the entry is chosen by b; different shapes come back as they are
    b = np.array([[0.1, 0], [0, -3j]])
    x, y = comp.match_global_phase(np.array([[0.1j, 0], [0, 3.0]]), b)
    assert np.array_equal(x, np.array([[0.1j, 0], [0, 3.0]])) and np.array_equal(y, 1j * b)
    c, d = np.eye(2), np.eye(4)
    x, y = comp.match_global_phase(c, d)
    assert x is c and y is d


def test_program_unitary_bit_order():
    """pyquil's order: qubit 0 is the least significant bit of the index."""
    cnot01 = np.array([[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [0, 1, 0, 0]])       # control 0: |01> <-> |11>, indices 1 and 3
    cnot10 = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]])       # control 1: indices 2 and 3
    assert np.array_equal(comp.program_unitary([("CNOT", (0, 1))], 2), cnot01)
    assert np.array_equal(comp.program_unitary([("CNOT", (1, 0))], 2), cnot10)
    x0 = comp.program_unitary([("X", (0,))], 2)
    assert np.array_equal(x0, np.kron(np.eye(2), [[0, 1], [1, 0]]))                 # qubit 0 is the RIGHT factor
    # later gates multiply from the left
    u = comp.program_unitary([("H", (0,)), ("T", (0,))], 1)
    np.testing.assert_allclose(u, np.diag([1, np.exp(0.25j * pi)]) @ (np.array([[1, 1], [1, -1]]) / np.sqrt(2)), atol=1e-15)
    with pytest.raises(ValueError, match="gate 0:"):
        comp.program_unitary([("XIN", (0, 0))], 1)
    with pytest.raises(ValueError, match="gate 1:"):
        comp.program_unitary([("H", (0,)), ("H", (2,))], 2)


def unitary(gates, n):
    return comp.program_unitary(gates, n)


def test_helpers_against_the_gates_they_replace():
    for theta in np.linspace(-2 * pi, 2 * pi, 50):
        cases.assert_close_up_to_global_phase(unitary([("RY", (0,), theta)], 1), unitary(comp._RY(theta, 0), 1))
        cases.assert_close_up_to_global_phase(unitary([("RX", (0,), theta)], 1), unitary(comp._RX(theta, 0), 1))
    for name, helper in (("X", comp._X), ("H", comp._H), ("T", comp._T)):
        cases.assert_close_up_to_global_phase(unitary([(name, (0,))], 1), unitary(helper(0), 1))
    cases.assert_close_up_to_global_phase(unitary([("TDG", (0,))], 1), unitary(comp._T(0, dagger=True), 1))
    for name, helper in (("CNOT", comp._CNOT), ("SWAP", comp._SWAP)):
        for pair in ((0, 1), (1, 0)):
            cases.assert_close_up_to_global_phase(unitary([(name, pair)], 2), unitary(helper(*pair), 2))
    for perm in itertools.permutations([0, 1, 2]):
        cases.assert_close_up_to_global_phase(unitary([("CCNOT", perm)], 3), unitary(comp._CCNOT(*perm), 3))


def test_random_programs():
    programs = cases.random_programs()
    assert len(programs) == 60 and {(n, len(p)) for n, p in programs} == {(n, l) for n in (3, 4) for l in (2, 50, 67)}
    assert {g[0] for _, p in programs for g in p} == set(cases.RANDOM_GATES)
    for n, prog in programs:
        native = comp.basic_compile(prog)
        assert {g[0] for g in native} <= set(comp.NATIVE_GATES)
        cases.assert_close_up_to_global_phase(unitary(prog, n), unitary(native, n))


def test_compiled_adder_is_the_permutation_of_the_reversible_model():
    from fbx.classical_logic import reversible, ripple_carry_adder as rca
    gates, _ = rca.adder(*rca.default_adder_registers(1))
    n = 4
    body = [g for g in gates if g[0] != "XIN"]
    u = comp.program_unitary(comp.basic_compile(body), n)
    np.testing.assert_allclose(u.conj().T @ u, np.eye(16), atol=1e-12)
    # column j = basis state j (bit q of j = qubit q): one entry of modulus 1, at the word reversible.evaluate gives -- there the
    # basis state is prepared by X gates in front of the same body
    for j in range(16):
        prep = [("X", (q,)) for q in range(n) if (j >> q) & 1]
        image = int(reversible.evaluate(reversible.encode_reversible(prep + body, n), n, np.uint64(0)))
        column = np.abs(u[:, j])
        assert abs(column[image] - 1.0) <= 1e-12 and np.abs(np.delete(column, image)).max() <= 1e-12
