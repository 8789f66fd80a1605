"""GHZ and graph-state experiments (forest/benchmarking/entangled_states.py) from circuit to statistics.

``ghz_state_statistics`` (:36-51) counts the shots that are all zeros or all ones: bins 0 and n of the weight-kind histogram of
``fbx_bit_histogram``, counted on the device.  The program builders (``create_ghz_program`` :11-33, ``create_graph_state`` :54-96,
``measure_graph_state`` :99-121) return gate lists for ``fbx.clifford_circuit`` in place of pyquil programs: all three are Clifford
circuits, so their shots under gate noise and readout flips come from ``fbx_clifford_sample_shots`` at any width up to 64
(``simulate_ghz_statistics_batch``, ``simulate_graph_state_parities_batch``: circuit -> reference outcome -> shots -> statistics
without leaving the device).  Qubit labels must be 0 .. n-1.  ``compiled_parametric_graph_state`` and everything else that needs a
``QuantumComputer`` is not mirrored."""
import math

import numpy as np

from .utils import bitstring_histogram_batch

__all__ = ["ghz_state_statistics", "ghz_state_statistics_batch", "create_ghz_program", "create_graph_state", "measure_graph_state",
           "simulate_ghz_statistics_batch", "simulate_graph_state_parities_batch"]


def ghz_state_statistics_batch(bitstrings) -> dict:
    """``bitstrings [B, n_shots, n]`` -> ``{'bell': [B] int64, 'total': [B] int64}``; one launch."""
    bits = np.asarray(bitstrings)
    if bits.ndim != 3:
        raise ValueError("bitstrings must be [B, n_shots, n]")
    counts = bitstring_histogram_batch(bits, kind="weight")
    bell = counts[:, 0] + (counts[:, -1] if bits.shape[2] > 0 else 0)
    return {"bell": bell, "total": np.full(bits.shape[0], bits.shape[1], dtype=np.int64)}


def ghz_state_statistics(bitstrings) -> dict:
    """entangled_states.py:36-51: ``{'bell': shots consistent with a Bell / GHZ state, 'total': shots}`` as ints."""
    res = ghz_state_statistics_batch(np.asarray(bitstrings)[None])
    return {"bell": int(res["bell"][0]), "total": int(res["total"][0])}


# ------------------------------------------------------------------ the program builders, as gate lists
def _check_labels(nodes):
    """Nodes must be the ints 0 .. n-1 in some order (no relabelling in this version)."""
    ok = all(isinstance(q, (int, np.integer)) and not isinstance(q, bool) for q in nodes)
    if not ok or sorted(int(q) for q in nodes) != list(range(len(nodes))):
        raise ValueError(f"qubit labels must be the integers 0 .. n-1, not {list(nodes)!r}")
    if not 1 <= len(nodes) <= 64:
        raise ValueError("need 1..64 qubits")


def _tree_parts(tree):
    """(nodes in insertion order, successors dict) of a ``networkx.DiGraph`` or of a list of (parent, child) edges, whose nodes
    are inserted as the edges name them; a single int is the tree of one node without edges."""
    if hasattr(tree, "successors") and hasattr(tree, "nodes"):
        nodes = list(tree.nodes)
        return nodes, {q: list(tree.successors(q)) for q in nodes}
    if isinstance(tree, (int, np.integer)):
        return [int(tree)], {int(tree): []}
    nodes, succ = [], {}
    for parent, child in tree:
        for q in (parent, child):
            if q not in succ:
                nodes.append(q)
                succ[q] = []
        if child not in succ[parent]:
            succ[parent].append(child)
    return nodes, succ


def _is_tree(nodes, succ):
    """``networkx.is_tree`` for a directed graph: n - 1 edges and weakly connected."""
    if not nodes or sum(len(v) for v in succ.values()) != len(nodes) - 1:
        return False
    nbrs = {q: set() for q in nodes}
    for a, children in succ.items():
        for b in children:
            nbrs[a].add(b)
            nbrs[b].add(a)
    seen, todo = {nodes[0]}, [nodes[0]]
    while todo:
        for b in nbrs[todo.pop()]:
            if b not in seen:
                seen.add(b)
                todo.append(b)
    return len(seen) == len(nodes)


def _topological_sort(nodes, succ):
    """``networkx.topological_sort``: generation by generation, a generation in the order in which its members lost their last
    predecessor (the first one: the nodes without predecessors in insertion order)."""
    indegree = {q: 0 for q in nodes}
    for children in succ.values():
        for b in children:
            indegree[b] += 1
    generation, order = [q for q in nodes if indegree[q] == 0], []
    while generation:
        order += generation
        following = []
        for a in generation:
            for b in succ[a]:
                indegree[b] -= 1
                if indegree[b] == 0:
                    following.append(b)
        generation = following
    return order


def create_ghz_program(tree, skip_measurements=False):
    """entangled_states.py:11-33 as a gate list: ``[("H", (root,)), ("CNOT", (parent, child)), ...]``, the CNOTs in the reference's
    order -- the nodes in ``networkx.topological_sort`` order, each followed by its successors in edge order.  ``tree`` is a
    ``networkx.DiGraph`` or a list of (parent, child) edges (nodes are inserted as the edges name them; a single int is the tree
    of one qubit); anything ``networkx.is_tree`` rejects is refused with the reference's message.  The measurement of the
    reference's program is implicit here -- the samplers measure every qubit, column q = qubit q -- so ``skip_measurements``
    changes nothing."""
    del skip_measurements
    nodes, succ = _tree_parts(tree)
    if not _is_tree(nodes, succ):
        raise ValueError("Needs to be a tree")
    _check_labels(nodes)
    order = _topological_sort(nodes, succ)
    gates = [("H", (int(order[0]),))]
    for a in order:
        gates += [("CNOT", (int(a), int(b))) for b in succ[a]]
    return gates


def _graph_parts(graph):
    """(nodes, edges) of a ``networkx.Graph`` or of a ``(nodes, edges)`` pair, in insertion order."""
    if hasattr(graph, "nodes") and hasattr(graph, "edges"):
        nodes, edges = list(graph.nodes), [tuple(e) for e in graph.edges]
    else:
        nodes, edges = graph
        nodes, edges = list(nodes), [tuple(e) for e in edges]
    _check_labels(nodes)
    for e in edges:
        if len(e) != 2 or e[0] == e[1] or e[0] not in nodes or e[1] not in nodes:
            raise ValueError(f"not an edge between two different nodes of the graph: {e!r}")
    return [int(q) for q in nodes], [(int(a), int(b)) for a, b in edges]


def create_graph_state(graph):
    """entangled_states.py:54-96 as a gate list: H on every node in node order, then CZ on every edge in edge order.  ``graph`` is a
    ``networkx.Graph`` or a ``(nodes, edges)`` pair.  (``use_pragmas`` is a compiler hint and has no counterpart.)"""
    nodes, edges = _graph_parts(graph)
    return [("H", (q,)) for q in nodes] + [("CZ", e) for e in edges]


def measure_graph_state(graph, focal_node, theta=-math.pi / 2):
    """entangled_states.py:99-121: ``(gates, measured_qubits)`` -- ``RY(theta)`` on the focal node, then the focal node and its
    neighbours are read: ``measured_qubits = [focal_node] + sorted(neighbours)`` (the columns of a bit record that the reference
    puts into ``ro[0], ro[1], ...``).  The reference leaves theta a run-time parameter; here it must be a multiple of pi / 2 (up to
    1e-9), or the circuit is not Clifford and is refused: 0 -> no gate, +-pi / 2 -> ``RY(+-pi/2)``, +-pi -> ``Y``.

    WHICH SIGN MEASURES X.  A Z measurement after U = RY(theta) measures U^+ Z U.  By the conjugation table RY(pi/2) maps Z to X
    and X to -Z, so U^+ Z U = RY(-theta) Z RY(theta) is +X for theta = -pi / 2 and -X for theta = +pi / 2.  The graph state is
    stabilized by X_focal prod_{neighbours} Z, so with the default ``theta = -pi / 2`` the parity of the measured bits is EVEN on
    the ideal state (odd with +pi / 2, and a fair coin with 0 or pi)."""
    nodes, edges = _graph_parts(graph)
    focal = int(focal_node)
    if focal not in nodes:
        raise ValueError(f"focal node {focal_node!r} is not in the graph")
    quarter = float(theta) / (math.pi / 2)
    turns = round(quarter) if math.isfinite(quarter) else 0
    if not math.isfinite(quarter) or abs(quarter - turns) > 1e-9:
        raise ValueError(f"theta = {theta!r} is not a multiple of pi / 2: RY(theta) is not a Clifford gate")
    gate = {0: None, 1: "RY(pi/2)", 2: "Y", 3: "RY(-pi/2)"}[turns % 4]
    neighbours = sorted({b if a == focal else a for a, b in edges if focal in (a, b)})
    return ([] if gate is None else [(gate, (focal,))]), [focal] + neighbours


# ------------------------------------------------------------------ resident chains: circuit -> reference -> shots -> statistics
def _sample_resident(res, n, gates, B, K, d_ce, cls, d_flips, shots, key):
    """reference -> shots on the device for one circuit: the ``DeviceBuffer`` of the bit records [B, shots, n] and of the status."""
    from . import clifford_circuit as cc
    from . import _lib
    lib, ptr = _lib.lib(), _lib.devptr
    words = cc.encode_gates(gates, n)
    d_gates, d_cls = res.upload(words if words.size else np.zeros(1, dtype=np.uint32)), res.upload(cls)
    d_ref, d_bits, d_status = res.alloc(8), res.alloc(B * shots * n), res.alloc(4 * B)
    _lib.check(lib.fbx_clifford_reference_sample_dev(n, words.size, d_gates.ptr, d_ref.ptr))
    _lib.check(lib.fbx_clifford_sample_shots_dev(n, words.size, d_gates.ptr, ptr(d_cls), K, d_ref.ptr, B, shots, ptr(d_ce), ptr(d_flips),
                                                 key, 0, d_bits.ptr, None, d_status.ptr))
    return d_bits, d_status


def _raise_poisoned(status, who):
    bad = np.flatnonzero(status)
    if bad.size:
        raise ValueError(f"{who}: item {int(bad[0])} has a class_error or readout_flip value outside [0, 1] "
                         f"({bad.size} such item(s) in the batch)")


def simulate_ghz_statistics_batch(tree, shots, class_error=None, noise_class=None, readout_flip=None, seed=None) -> dict:
    """A GHZ experiment on up to 64 qubits from the tree to ``{'bell': [B] int64, 'total': [B] int64}`` without leaving the device:
    ``create_ghz_program(tree)`` -> ``fbx_clifford_reference_sample_dev`` -> ``fbx_clifford_sample_shots_dev`` (B items that differ
    in noise: ``class_error``, ``noise_class`` -- one class per gate of the program -- and ``readout_flip`` as in
    ``sampling.sample_clifford_circuit_batch``) -> the weight histogram of ``fbx_bit_histogram_dev``, whose bins 0 and n are the
    shots ``ghz_state_statistics`` counts.  Only the ``[B, n + 1]`` counts come back.  The shots are those of
    ``sample_clifford_circuit_batch`` on the same seed."""
    from . import _lib
    from . import clifford_circuit as cc
    from .operator_tools.random_operators import _stream_seed
    gates = create_ghz_program(tree)
    n = 1 + max(q for _, qs in gates for q in qs)
    B, K, ce, cls, flips = cc.frame_noise(n, len(gates), class_error, noise_class, readout_flip)
    shots, key = int(shots), _stream_seed(seed)
    if shots < 1:
        raise ValueError("need shots >= 1")
    with _lib.DeviceScope() as res:
        d_bits, d_status = _sample_resident(res, n, gates, B, K, res.upload(ce), cls, res.upload(flips), shots, key)
        d_counts = res.alloc(8 * B * (n + 1))
        _lib.check(_lib.lib().fbx_bit_histogram_dev(n, B, shots, d_bits.ptr, n, None, 1, None, _lib.HIST_WEIGHT, d_counts.ptr))
        counts = d_counts.to_array(np.int64, (B, n + 1))
        _raise_poisoned(d_status.to_array(np.int32, (B,)), "simulate_ghz_statistics_batch")
    return {"bell": counts[:, 0] + counts[:, n], "total": np.full(B, shots, dtype=np.int64)}


def simulate_graph_state_parities_batch(graph, shots, class_error=None, noise_class=None, readout_flip=None, seed=None,
                                        theta=-math.pi / 2) -> np.ndarray:
    """The graph-state experiment of the reference on up to 64 qubits: for every node of the graph, in node order, the circuit
    ``create_graph_state(graph) + measure_graph_state(graph, node, theta)`` is sampled with ``shots`` shots per item and the mean of
    (-1)^(focal bit + neighbour bits) is taken with ``fbx_shots_to_moments_dev`` -> ``[B, n_nodes]`` float64, 1.0 on the ideal state
    with the default theta (see ``measure_graph_state``).  One circuit per focal node, each on a stream of its own (the seed
    plus the node's position); nothing but the means leaves the device.  ``noise_class`` has one entry per gate of
    ``create_graph_state(graph)`` plus a last one for the measurement rotation (default: every gate class 0)."""
    from . import _lib
    from . import clifford_circuit as cc
    from .operator_tools.random_operators import _stream_seed
    nodes, _ = _graph_parts(graph)
    n = len(nodes)
    state = create_graph_state(graph)
    B, K, ce, cls, flips = cc.frame_noise(n, len(state) + 1, class_error, noise_class, readout_flip)
    shots, key = int(shots), _stream_seed(seed)
    if shots < 1:
        raise ValueError("need shots >= 1")
    out = np.zeros((B, n))
    with _lib.DeviceScope() as res:
        d_ce, d_flips = res.upload(ce), res.upload(flips)
        d_mean, d_var = res.alloc(8 * B * n), res.alloc(8 * B * n)
        status = []
        for i, focal in enumerate(nodes):
            rotation, measured = measure_graph_state(graph, focal, theta)
            gate_cls = cls if (cls is None or rotation) else cls[:-1]
            d_bits, d_status = _sample_resident(res, n, state + rotation, B, K, d_ce, gate_cls, d_flips, shots,
                                                (key + i) & (2 ** 64 - 1))
            mask = np.zeros((B, n), dtype=np.uint8)
            mask[:, measured] = 1
            _lib.check(_lib.lib().fbx_shots_to_moments_dev(n, B, shots, d_bits.ptr, res.upload(mask).ptr, None, 0,
                                                           d_mean.at(8 * B * i), d_var.at(8 * B * i)))
            status.append(d_status)
        out[:] = d_mean.to_array(np.float64, (n, B)).T
        for d_status in status:
            _raise_poisoned(d_status.to_array(np.int32, (B,)), "simulate_graph_state_parities_batch")
    return out
