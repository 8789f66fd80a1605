"""The host mirror of the Pauli-frame sampler (fbx.clifford_circuit.reference_sample / restate_frame_shots) pinned to physics --
state-vector and density-matrix simulations, DFE's exact means -- and the circuit builders of fbx.entangled_states against the
reference's instruction order.  Nothing here loads the device."""
import math

import numpy as np
import pytest

import dfe_cases as dc
import frames_cases as fc
from fbx import clifford_circuit as cc, entangled_states as es

SHOTS = 40_000


# ------------------------------------------------------------------ 1. the reference sample
def test_reference_sample_is_the_smallest_outcome_of_the_dense_simulation():
    for n, gates, probs in fc.case_circuits():
        want = fc.index_to_word(fc.support_indices(probs)[0], n)
        assert cc.reference_sample(gates, n) == want, (n, gates)


def test_reference_sample_hand_cases():
    for n in (1, 5, 64):
        assert cc.reference_sample([], n) == 0
        assert cc.reference_sample([("X", (q,)) for q in range(n)], n) == 2 ** n - 1
        assert cc.reference_sample(dc.ghz_circuit(n), n) == 0
    assert cc.reference_sample([("H", (0,)), ("S", (0,)), ("S", (0,)), ("H", (0,))], 1) == 1          # H Z H = X
    assert cc.reference_sample([("X", (1,)), ("CNOT", (1, 0)), ("H", (2,))], 3) == 0b011


# ------------------------------------------------------------------ 2. noiseless frames
def test_noiseless_shots_cover_exactly_the_support():
    """4096 shots per circuit: every shot has non-zero probability, and where the support has at most 16 elements every element
    occurs (a miss has probability below 16 (15/16)^4096 < 1e-113)."""
    covered = 0
    for i, (n, gates, probs) in enumerate(fc.case_circuits()):
        support = fc.support_indices(probs)
        seen = np.unique(fc.words_to_indices(cc.restate_frame_shots(gates, n, 4096, seed=100 + i)[0], n))
        assert np.isin(seen, support).all(), (n, gates)
        if support.size <= 16:
            assert np.array_equal(seen, support), (n, gates)
            covered += support.size > 1
    assert covered >= 50


# ------------------------------------------------------------------ 3. the noise model against a density matrix
def noisy_case(n):
    rng = np.random.default_rng(300 + n)
    gates = dc.random_circuit(rng, n, 10)
    classes = rng.integers(0, 2, size=len(gates)).astype(np.uint8)
    classes[:2] = (0, 1)
    classes[4] = 255
    return gates, classes


def assert_frequencies(words, n, exact, what):
    got = fc.frequencies(words, n)
    for i, (f, q) in enumerate(zip(got, exact)):
        q = min(max(q, 0.0), 1.0)
        bound = 5 * math.sqrt(q * (1 - q) / len(words)) + 1e-12           # 1e-12: the rounding of the dense simulation
        print(what, "outcome", i, "frequency", f, "exact", q, "bound", bound)
        assert abs(f - q) <= bound, (what, i, f, q, bound)


@pytest.mark.parametrize("p", [0.05, 0.3, 1.0])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_outcome_frequencies_match_the_density_matrix(n, p):
    gates, classes = noisy_case(n)
    errors = np.array([[p, 0.5 * p]])
    words = cc.restate_frame_shots(gates, n, SHOTS, errors, classes, seed=11 * n + int(100 * p))
    assert_frequencies(words[0], n, fc.noisy_probabilities(gates, n, classes, errors[0]), (n, p))


def test_full_depolarizing_after_the_last_gate_gives_the_flat_marginal():
    gates = [("X", (0,))]
    exact = fc.noisy_probabilities(gates, 1, None, [1.0])
    assert np.allclose(exact, [0.5, 0.5], atol=1e-15)
    assert_frequencies(cc.restate_frame_shots(gates, 1, SHOTS, 1.0, seed=5)[0], 1, exact, "flat")


def test_zero_error_probability_reproduces_the_noiseless_shots_bit_for_bit():
    for i, (n, gates, _) in enumerate(fc.case_circuits()[:40]):
        classes = (np.arange(len(gates)) % 3).astype(np.uint8)
        clean = cc.restate_frame_shots(gates, n, 512, seed=100 + i)
        assert np.array_equal(cc.restate_frame_shots(gates, n, 512, np.zeros((1, 3)), classes, seed=100 + i), clean)
        assert np.array_equal(cc.restate_frame_shots(gates, n, 512, np.full((1, 3), 0.7), np.full(len(gates), 255), seed=100 + i), clean)


# ------------------------------------------------------------------ 4. DFE's exact means
def test_sampled_parities_agree_with_the_means_of_dfe():
    """6-qubit GHZ with three noise classes: the Z-product observables of the exhaustive state experiment have mu = sigma prod_c
    (1 - p_c)^touches (include/fbx.h, THE MEAN); the mean parity of the frame shots must lie within 5 standard errors."""
    n, errors = 6, np.array([[0.02, 0.05, 0.1]])
    gates = dc.ghz_circuit(n)
    classes = np.array([0] + [1 + q % 2 for q in range(n - 1)], dtype=np.uint8)
    s = cc.restate_dfe_settings(n, "state", 0, 0, gates)
    z_only = np.flatnonzero(s["obs_x"] == 0)
    assert z_only.size == 2 ** (n - 1) - 1
    sigma, touches = cc.propagate_settings(gates, n, s["in_x"], s["in_z"], s["in_minus"], s["obs_x"], s["obs_z"], classes, 3)
    words = cc.restate_frame_shots(gates, n, SHOTS, errors, classes, seed=2024)[0]
    for k in z_only:
        mu = float(sigma[k]) * float(np.prod((1 - errors[0]) ** touches[k]))
        want = (1 - 2 * int(s["obs_sign"][k])) * mu
        parity = cc._popcount(words & s["obs_z"][k]) & np.uint64(1)
        got = float(np.mean(1 - 2 * parity.astype(np.int64)))
        bound = 5 * math.sqrt((1 - mu * mu) / SHOTS)
        print("setting", k, "sampled", got, "exact", want, "bound", bound)
        assert abs(got - want) <= bound, (k, got, want, bound)
        assert abs(mu) < 1.0


# ------------------------------------------------------------------ 5. readout flips
def test_asymmetric_readout_flips():
    n = 5
    gates = [("X", (0,)), ("X", (2,)), ("X", (4,))]                       # the outcome is 10101 for certain
    drawn = np.array([1, 0, 1, 0, 1])
    flips = np.array([[0.3, 0.1], [0.25, 0.4], [0.0, 0.0], [1.0, 0.2], [0.9, 1.0]])
    bits = cc.unpack_shots(cc.restate_frame_shots(gates, n, SHOTS, readout_flip=flips, seed=77)[0], n)
    for j in range(n):
        f = flips[j, drawn[j]]
        got = float(np.mean(bits[:, j] != drawn[j]))
        bound = 5 * math.sqrt(f * (1 - f) / SHOTS)
        print("column", j, "flipped", got, "probability", f, "bound", bound)
        assert abs(got - f) <= bound
    assert not (bits[:, 2] != 1).any() and (bits[:, 4] != 1).all()        # probabilities 0 and 1 are exact
    # the other half of each pair is never read: changing it changes nothing
    other = flips.copy()
    other[np.arange(n), 1 - drawn] = 0.5
    assert np.array_equal(cc.unpack_shots(cc.restate_frame_shots(gates, n, SHOTS, readout_flip=other, seed=77)[0], n), bits)


def test_poisoned_items_are_rows_of_zeros_and_leave_their_neighbours_alone():
    gates = dc.ghz_circuit(3) + [("X", (1,))]
    clean = cc.restate_frame_shots(gates, 3, 100, np.full((3, 1), 0.2), seed=9)
    for bad in (np.nan, -0.1, 1.5):
        errors = np.full((3, 1), 0.2)
        errors[1, 0] = bad
        got = cc.restate_frame_shots(gates, 3, 100, errors, seed=9)
        assert not got[1].any() and np.array_equal(got[[0, 2]], clean[[0, 2]])


# ------------------------------------------------------------------ 6. the builders
PATH = [(0, 1), (1, 2), (2, 3)]
STAR = [(0, 1), (0, 2), (0, 3)]
RING_NODES, RING_EDGES = [0, 1, 2, 3], [(0, 1), (1, 2), (2, 3), (3, 0)]


def test_ghz_programs_follow_the_reference_instruction_order():
    assert es.create_ghz_program(PATH) == [("H", (0,)), ("CNOT", (0, 1)), ("CNOT", (1, 2)), ("CNOT", (2, 3))]
    assert es.create_ghz_program(STAR) == [("H", (0,)), ("CNOT", (0, 1)), ("CNOT", (0, 2)), ("CNOT", (0, 3))]
    assert es.create_ghz_program(PATH, skip_measurements=True) == es.create_ghz_program(PATH)
    # the root is the node without predecessors, wherever the edge list names it; generations come one after the other
    assert es.create_ghz_program([(2, 3), (1, 2), (1, 0), (3, 4)]) == [("H", (1,)), ("CNOT", (1, 2)), ("CNOT", (1, 0)),
                                                                       ("CNOT", (2, 3)), ("CNOT", (3, 4))]
    assert es.create_ghz_program(0) == [("H", (0,))]
    for n, gates in ((4, es.create_ghz_program(PATH)), (4, es.create_ghz_program(STAR))):
        probs = fc.dense_probabilities(gates, n)
        assert np.allclose(probs[[0, -1]], 0.5) and np.allclose(probs[1:-1], 0)


def test_ghz_programs_agree_with_networkx():
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(3)
    for n in (2, 5, 9, 20):
        parents = [int(rng.integers(0, q)) for q in range(1, n)]
        edges = [(p, q) for q, p in enumerate(parents, start=1)]
        edges = [edges[i] for i in rng.permutation(len(edges))]
        tree = nx.DiGraph(edges)
        want = [("H", (list(nx.topological_sort(tree))[0],))]
        for node in nx.topological_sort(tree):
            want += [("CNOT", (node, child)) for child in tree.successors(node)]
        assert es.create_ghz_program(tree) == want == es.create_ghz_program(edges)
    ring = nx.Graph()
    ring.add_nodes_from(RING_NODES)
    ring.add_edges_from(RING_EDGES)
    assert es.create_graph_state(ring) == es.create_graph_state((RING_NODES, list(ring.edges)))
    assert es.measure_graph_state(ring, 0) == es.measure_graph_state((RING_NODES, RING_EDGES), 0)


def test_graph_state_programs_follow_the_reference_instruction_order():
    h = [("H", (q,)) for q in range(4)]
    assert es.create_graph_state(([0, 1, 2, 3], PATH)) == h + [("CZ", (0, 1)), ("CZ", (1, 2)), ("CZ", (2, 3))]
    assert es.create_graph_state(([0, 1, 2, 3], STAR)) == h + [("CZ", (0, 1)), ("CZ", (0, 2)), ("CZ", (0, 3))]
    assert es.create_graph_state((RING_NODES, RING_EDGES)) == h + [("CZ", (0, 1)), ("CZ", (1, 2)), ("CZ", (2, 3)), ("CZ", (3, 0))]
    assert es.measure_graph_state(([0, 1, 2, 3], PATH), 1) == ([("RY(-pi/2)", (1,))], [1, 0, 2])
    assert es.measure_graph_state(([0, 1, 2, 3], STAR), 0, theta=math.pi / 2) == ([("RY(pi/2)", (0,))], [0, 1, 2, 3])
    assert es.measure_graph_state(([0, 1, 2, 3], STAR), 3, theta=0.0) == ([], [3, 0])
    assert es.measure_graph_state((RING_NODES, RING_EDGES), 3, theta=math.pi) == ([("Y", (3,))], [3, 0, 2])
    assert es.measure_graph_state((RING_NODES, RING_EDGES), 0, theta=-math.pi) == ([("Y", (0,))], [0, 1, 3])


@pytest.mark.parametrize("edges", [PATH, STAR, RING_EDGES])
def test_the_documented_sign_measures_x_with_even_parity(edges):
    """Dense state vector: with theta = -pi/2 the parity of (focal bit, neighbour bits) is even with certainty, with +pi/2 odd."""
    graph = ([0, 1, 2, 3], edges)
    for focal in range(4):
        for theta, want in ((-math.pi / 2, 0), (math.pi / 2, 1)):
            rotation, measured = es.measure_graph_state(graph, focal, theta)
            probs = fc.dense_probabilities(es.create_graph_state(graph) + rotation, 4)
            parity = np.array([sum((i >> (3 - q)) & 1 for q in measured) & 1 for i in range(16)])
            assert abs(probs[parity == want].sum() - 1) < 1e-12, (edges, focal, theta)


def test_builders_refuse_what_the_reference_refuses_and_what_is_not_clifford():
    for not_a_tree in ([(0, 1), (1, 2), (2, 0)], [(0, 1), (2, 3)], [(0, 1), (1, 0)], []):
        with pytest.raises(ValueError, match="tree"):
            es.create_ghz_program(not_a_tree)
    for labels in ([(1, 2)], [(0, 2)], [("a", "b")]):
        with pytest.raises(ValueError, match="labels"):
            es.create_ghz_program(labels)
    with pytest.raises(ValueError, match="labels"):
        es.create_graph_state(([1, 2, 3], [(1, 2)]))
    with pytest.raises(ValueError, match="edge"):
        es.create_graph_state(([0, 1], [(0, 0)]))
    for theta in (0.3, math.pi / 4, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="Clifford"):
            es.measure_graph_state((RING_NODES, RING_EDGES), 0, theta=theta)
    with pytest.raises(ValueError, match="focal"):
        es.measure_graph_state((RING_NODES, RING_EDGES), 7)
