"""The host side of the simulated ripple-carry adder (fbx/classical_logic/reversible.py, primitives.py, ripple_carry_adder.py), no
GPU: the circuits against the reference's gate counts and against arithmetic, the encoder's refusals, the register assignment, the
model against a density-matrix simulation written here, and the restated stream against the exact distribution."""
import itertools

import networkx as nx
import numpy as np
import pytest

from fbx.classical_logic import primitives as prim, reversible as rev, ripple_carry_adder as rca

CLASS_ERROR = (0.02, 0.05, 0.11)            # one-, two- and three-qubit gates
PERMUTED = {1: ([3], [0], 2, 1), 2: ([5, 0], [3, 1], 4, 2), 3: ([7, 2, 5], [0, 6, 3], 4, 1)}
# The seed of test_restated_shots_follow_the_exact_distribution, picked on the CPU so that the restatement meets the bound there.
RESTATE_SEED = 20261021


def msb_first(records, m):
    """Packed records (bit j = column j) -> the integer whose most significant bit is column 0."""
    records = np.asarray(records, dtype=np.uint64)
    out = np.zeros(records.shape, dtype=np.int64)
    for j in range(m):
        out |= ((records >> np.uint64(j)) & np.uint64(1)).astype(np.int64) << (m - 1 - j)
    return out


def adder_words(n, in_x_basis, registers=None):
    registers = rca.default_adder_registers(n) if registers is None else registers
    gates, out_qubits = rca.adder(*registers, in_x_basis=in_x_basis)
    return gates, rev.encode_reversible(gates, 2 * n + 2), out_qubits


# ------------------------------------------------------------------ 1. the circuits
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_gate_counts_are_the_references(n):
    assert len(rca.adder(*rca.default_adder_registers(n))[0]) == 8 * n + 1
    assert len(rca.adder(*rca.default_adder_registers(n), in_x_basis=True)[0]) == 31 * n + 6


def test_default_registers_and_record_order():
    a, b, carry, z = rca.default_adder_registers(3)
    assert (a, b, carry, z) == ([2, 4, 6], [1, 3, 5], 0, 7)
    gates, out_qubits = rca.adder(a, b, carry, z)
    assert out_qubits == [7, 5, 3, 1]
    assert gates[:6] == [("XIN", (2, 3)), ("XIN", (4, 4)), ("XIN", (6, 5)), ("XIN", (1, 0)), ("XIN", (3, 1)), ("XIN", (5, 2))]


@pytest.mark.parametrize("in_x_basis", [False, True])
@pytest.mark.parametrize("layout", ["default", "permuted"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_evaluate_adds_every_pair(n, layout, in_x_basis):
    registers = rca.default_adder_registers(n) if layout == "default" else PERMUTED[n]
    _, words, out_qubits = adder_words(n, in_x_basis, registers)
    inputs = np.arange(4 ** n, dtype=np.uint64)
    state = rev.evaluate(words, 2 * n + 2, inputs)
    got = msb_first(rev.gather_record(state, out_qubits), n + 1)
    a, b = inputs.astype(np.int64) >> n, inputs.astype(np.int64) & (2 ** n - 1)
    assert np.array_equal(got, a + b)
    assert np.array_equal(got, msb_first(rev.pack_records(rca.adder_expected_bits(n)), n + 1))
    # the a register and the carry ancilla come back as they were
    assert np.array_equal(msb_first(rev.gather_record(state, registers[0][::-1]), n), a)
    assert not np.any((state >> np.uint64(registers[2])) & np.uint64(1))


def run_block(gates, in_x_basis):
    """A 3-qubit block (qubits a = 0, b = 1, c = 2) on all 8 inputs: input bit q on qubit q, -> the 8 final (a, b, c)."""
    h = [("H", (q,)) for q in range(3)] if in_x_basis else []
    prep = [g for q in range(3) for g in ([("XIN", (q, q))] + ([("H", (q,))] if in_x_basis else []))]
    state = rev.evaluate(rev.encode_reversible(prep + gates + h, 3), 3, np.arange(8, dtype=np.uint64))
    return [tuple((int(s) >> q) & 1 for q in range(3)) for s in state]


@pytest.mark.parametrize("in_x_basis", [False, True])
def test_majority_and_unmajority_truth_tables(in_x_basis):
    maj = run_block(prim.majority_gate(0, 1, 2, in_x_basis), in_x_basis)
    both = run_block(prim.majority_gate(0, 1, 2, in_x_basis) + prim.unmajority_add_gate(0, 1, 2, in_x_basis), in_x_basis)
    for r, (got, undone) in enumerate(zip(maj, both)):
        a, b, c = r & 1, (r >> 1) & 1, (r >> 2) & 1
        assert got == (int(a + b + c >= 2), b ^ a, c ^ a), r
        assert undone == (a, a ^ b ^ c, c), r


@pytest.mark.parametrize("in_x_basis", [False, True])
def test_parallel_unmajority_is_unmajority(in_x_basis):
    assert run_block(prim.unmajority_add_parallel_gate(0, 1, 2, in_x_basis), in_x_basis) \
        == run_block(prim.unmajority_add_gate(0, 1, 2, in_x_basis), in_x_basis)
    assert len(prim.unmajority_add_parallel_gate(0, 1, 2)) == 6 and len(prim.unmajority_add_gate(0, 1, 2)) == 3


def test_x_basis_primitives_are_the_references_sequences():
    assert prim.CNOT_X_basis(3, 5) == [("H", (3,)), ("CZ", (3, 5)), ("H", (3,))]
    assert prim.CCNOT_X_basis(1, 2, 0) == [("H", (1,)), ("H", (2,)), ("H", (0,)), ("CCNOT", (1, 2, 0)),
                                           ("H", (1,)), ("H", (2,)), ("H", (0,))]


# ------------------------------------------------------------------ 2. the encoder
def test_micro_ops_follow_the_table():
    words = rev.encode_reversible([("X", (0,)), ("H", (0,)), ("X", (0,)), ("CZ", (0, 1)), ("CZ", (1, 0)), ("CZ", (1, 2)), ("H", (1,)),
                                   ("CNOT", (0, 1)), ("H", (0,)), ("H", (1,)), ("CNOT", (0, 1)), ("CCNOT", (0, 1, 2)),
                                   ("XIN", (2, 63))], 3)
    want = [(rev.OP_NOT, (0,), (0,), 0), (rev.OP_SITE, (0,), (1,), 0), (rev.OP_SITE, (0,), (1,), 0),
            (rev.OP_XOR, (0, 1), (1, 0), 0), (rev.OP_XOR, (0, 1), (1, 0), 0), (rev.OP_SITE, (1, 2), (0, 0), 0),
            (rev.OP_SITE, (1,), (1,), 0), (rev.OP_XOR, (0, 1), (1, 1), 0), (rev.OP_SITE, (0,), (0,), 0),
            (rev.OP_SITE, (1,), (0,), 0), (rev.OP_XOR, (1, 0), (0, 0), 0), (rev.OP_ANDXOR, (2, 0, 1), (0, 0, 0), 0),
            (rev.OP_XIN, (2,), (0,), 63)]
    assert [rev._fields(int(w)) for w in words] == want
    assert np.array_equal(rev.encode_reversible(words, 3), words)           # words pass through, validated
    assert list(rev.gate_arity(words)) == [1, 1, 1, 2, 2, 2, 1, 2, 1, 1, 2, 3, 1]


@pytest.mark.parametrize("gates, index", [
    ([("H", (0,)), ("CNOT", (0, 1))], 1),                                    # mixed-basis CNOT
    ([("H", (0,)), ("H", (1,)), ("CZ", (0, 1))], 2),                         # CZ on two X-held bits
    ([("H", (2,)), ("CCNOT", (0, 1, 2))], 1),                                # CCNOT after one H
    ([("H", (0,)), ("XIN", (0, 0))], 1),
])
def test_encoder_refuses_what_would_entangle(gates, index):
    with pytest.raises(ValueError, match=f"gate {index}: .*in X"):
        rev.encode_reversible(gates, 3)


@pytest.mark.parametrize("gates", [[("T", (0,))], [("X", (3,))], [("CNOT", (1, 1))], [("CNOT", (1,))], [("XIN", (0, 64))],
                                   [("XIN", (0,))]])
def test_encoder_refuses_malformed_gates(gates):
    with pytest.raises(ValueError):
        rev.encode_reversible(gates, 3)


@pytest.mark.parametrize("word", [5, 1 | (2 << 3), 2 | (2 << 3) | (1 << 5) | (1 << 11), 1 | (1 << 3) | (3 << 5),
                                  1 | (1 << 3) | (1 << 26), 1 | (1 << 3) | (1 << 24), 0])
def test_words_are_validated(word):
    with pytest.raises(ValueError):
        rev.check_words(np.array([word], dtype=np.uint32), 3)


# ------------------------------------------------------------------ 3. the register assignment
def test_register_assignment_on_a_line_and_a_cycle():
    assert rca.assign_registers_to_line_or_cycle(0, nx.path_graph(6), 2) == ([2, 4], [1, 3], 0, 5)
    assert rca.assign_registers_to_line_or_cycle(0, nx.cycle_graph(6), 2) == ([2, 4], [1, 3], 0, 5)
    assert rca.get_qubit_registers_for_adder(nx.path_graph(6), 2) in (([2, 4], [1, 3], 0, 5), ([3, 1], [4, 2], 5, 0))
    for graph in (nx.cycle_graph(6), nx.cycle_graph(9), nx.grid_2d_graph(2, 3)):
        a, b, carry, z = rca.get_qubit_registers_for_adder(graph, 2)
        order = [carry, b[0], a[0], b[1], a[1], z]
        assert len(set(order)) == 6
        assert all(graph.has_edge(u, v) for u, v in zip(order, order[1:]))
    # only the listed qubits are used
    a, b, carry, z = rca.get_qubit_registers_for_adder(nx.path_graph(10), 2, qubits=range(3, 10))
    assert min(a + b + [carry, z]) >= 3


def test_register_assignment_refuses_a_small_graph():
    with pytest.raises(ValueError):
        rca.assign_registers_to_line_or_cycle(0, nx.path_graph(5), 2)
    with pytest.raises(ValueError):
        rca.get_qubit_registers_for_adder(nx.path_graph(5), 2)
    with pytest.raises(ValueError):
        rca.get_qubit_registers_for_adder(nx.path_graph(8), 2, qubits=range(5))
    with pytest.raises(ValueError):
        rca.get_qubit_registers_for_adder(nx.star_graph(7), 2)              # eight qubits, no path of six


# ------------------------------------------------------------------ 4. the physics, pinned by a density-matrix simulation
_H = np.array([[1.0, 1.0], [1.0, -1.0]]) / np.sqrt(2.0)
_X = np.array([[0.0, 1.0], [1.0, 0.0]])
_PAULIS = [np.eye(2), _X, np.array([[0.0, -1.0], [1.0, 0.0]]), np.diag([1.0, -1.0])]     # Y up to the phase i: Y rho Y is the same
_CNOT = np.eye(4)[[0, 1, 3, 2]]
_CZ = np.diag([1.0, 1.0, 1.0, -1.0])
_CCNOT = np.eye(8)[[0, 1, 2, 3, 4, 5, 7, 6]]
UNITARY = {"H": _H, "X": _X, "CNOT": _CNOT, "CZ": _CZ, "CCNOT": _CCNOT}


def conjugate(rho, u, qubits, n):
    """U rho U^T for a real U on ``qubits``; rho is a tensor with row axes 0 .. n - 1 and column axes n .. 2n - 1, axis q = qubit q
    (the first qubit of ``qubits`` is the most significant bit of U's index)."""
    k = len(qubits)
    t = u.reshape((2,) * (2 * k))
    for shift in (0, n):
        axes = [q + shift for q in qubits]
        rho = np.moveaxis(np.tensordot(t, rho, axes=(list(range(k, 2 * k)), axes)), list(range(k)), axes)
    return rho


def depolarize(rho, p, qubits, n):
    """(1 - p) rho + p times the average of P rho P over all 4^k Paulis on ``qubits``."""
    total = np.zeros_like(rho)
    for paulis in itertools.product(_PAULIS, repeat=len(qubits)):
        u = paulis[0]
        for q in paulis[1:]:
            u = np.kron(u, q)
        total += conjugate(rho, u, qubits, n)
    return (1.0 - p) * rho + p * total / 4 ** len(qubits)


def density_matrix_distribution(gates, n, input_word, class_error, out_qubits):
    rho = np.zeros((2,) * (2 * n))
    rho[(0,) * (2 * n)] = 1.0
    for name, qubits in gates:
        if name == "XIN":
            if not (input_word >> qubits[1]) & 1:
                continue
            name, qubits = "X", qubits[:1]
        rho = depolarize(conjugate(rho, UNITARY[name], qubits, n), class_error[len(qubits) - 1], qubits, n)
    diag = np.einsum(rho, list(range(n)) + list(range(n)), list(range(n)))
    rest = tuple(q for q in range(n) if q not in out_qubits)
    kept = [q for q in range(n) if q not in rest]
    marginal = diag.sum(axis=rest) if rest else diag
    return np.transpose(marginal, [kept.index(q) for q in out_qubits]).reshape(-1)


@pytest.mark.parametrize("n, in_x_basis", [(1, False), (1, True), (2, False)])
def test_exact_distribution_is_the_density_matrix_diagonal(n, in_x_basis):
    gates, words, out_qubits = adder_words(n, in_x_basis)
    cls = rev.gate_arity(words) - 1
    for r in range(4 ** n):
        want = density_matrix_distribution(gates, 2 * n + 2, r, CLASS_ERROR, out_qubits)
        got = rev.exact_distribution(words, 2 * n + 2, r, CLASS_ERROR, cls, None, out_qubits)
        assert abs(want.sum() - 1.0) < 1e-12
        assert np.abs(got - want).max() < 1e-12, (r, got, want)


def test_exact_distribution_without_noise_is_the_answer():
    _, words, out_qubits = adder_words(2, True)
    for r in range(16):
        dist = rev.exact_distribution(words, 6, r, None, None, None, out_qubits)
        assert dist[(r >> 2) + (r & 3)] == 1.0 and dist.sum() == 1.0


def test_readout_confusion_of_the_exact_distribution():
    _, words, out_qubits = adder_words(1, False)
    flips = np.array([[0.1, 0.3], [0.05, 0.2]])
    dist = rev.exact_distribution(words, 4, 3, None, None, flips, out_qubits)           # 1 + 1 = 10
    want = np.array([0.3 * 0.95, 0.3 * 0.05, 0.7 * 0.95, 0.7 * 0.05])                    # column 0 reads 1 -> 0 with 0.3, column 1 0 -> 1 with 0.05
    assert np.abs(dist - want).max() < 1e-15


# ------------------------------------------------------------------ 5. the restated stream
READOUT = np.array([[0.01, 0.04], [0.03, 0.02], [0.0, 0.06]])


@pytest.mark.parametrize("in_x_basis", [False, True])
def test_restated_shots_follow_the_exact_distribution(in_x_basis):
    """n = 2, 20 000 shots per pair: every outcome frequency within 6 sqrt(p (1 - p) / S) + 1 / S of its exact probability."""
    S = 20000
    _, words, out_qubits = adder_words(2, in_x_basis)
    cls = rev.gate_arity(words) - 1
    records = rev.restate_reversible_shots(words, 6, np.arange(16), out_qubits, S, np.array([CLASS_ERROR]), cls, READOUT,
                                           seed=RESTATE_SEED)
    assert records.shape == (1, 16, S)
    worst = 0.0
    for r in range(16):
        p = rev.exact_distribution(words, 6, r, CLASS_ERROR, cls, READOUT, out_qubits)
        freq = np.bincount(msb_first(records[0, r], 3), minlength=8) / S
        bound = 6.0 * np.sqrt(p * (1.0 - p) / S) + 1.0 / S
        worst = max(worst, float((np.abs(freq - p) / bound).max()))
        assert np.all(np.abs(freq - p) <= bound), (r, freq, p)
    print(f"largest deviation / bound: {worst:.3f}")


def test_restatement_stream_properties():
    _, words, out_qubits = adder_words(1, True)
    cls = rev.gate_arity(words) - 1
    ce = np.array([[0.1, 0.2, 0.3], [0.3, 0.2, 0.1], [0.0, 0.5, 0.0]])
    full = rev.restate_reversible_shots(words, 4, np.arange(4), out_qubits, 70, ce, cls, READOUT[:2], seed=5)
    assert np.array_equal(rev.restate_reversible_shots(words, 4, np.arange(4), out_qubits, 70, ce[1:2], cls, READOUT[:2], seed=5,
                                                       first_item=1), full[1:2])
    assert np.array_equal(rev.restate_reversible_shots(words, 4, [2, 3], out_qubits, 33, ce, cls, READOUT[:2], seed=5,
                                                       first_input=2), full[:, 2:, :33])
    assert not np.array_equal(full[0], full[1])
    poisoned = ce.copy()
    poisoned[1, 2] = np.nan
    got = rev.restate_reversible_shots(words, 4, np.arange(4), out_qubits, 70, poisoned, cls, READOUT[:2], seed=5)
    assert not got[1].any() and np.array_equal(got[[0, 2]], full[[0, 2]])
    expected = rev.pack_records(rca.adder_expected_bits(1))
    counts = rev.weight_counts(full, expected, 2)
    assert counts.shape == (3, 4, 3) and np.all(counts.sum(axis=-1) == 70)
    bits = rev.unpack_records(full, 2)
    assert np.array_equal(counts[..., 0], (bits == rca.adder_expected_bits(1)[:, None, :]).all(axis=-1).sum(axis=-1))


def test_predicted_statistics_are_distributions():
    ce = np.array([[0.0, 0.0, 0.0], [0.01, 0.02, 0.05]])
    success, hamming = rca.predicted_adder_statistics(2, ce, in_x_basis=True)
    assert success.shape == (2, 16) and hamming.shape == (2, 16, 4)
    assert np.all(success[0] == 1.0) and np.all(success[1] < 1.0) and np.all(success[1] > 0.5)
    assert np.abs(hamming.sum(axis=-1) - 1.0).max() < 1e-12
