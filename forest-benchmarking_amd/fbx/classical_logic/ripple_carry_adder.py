"""The analysis half of the ripple-carry adder benchmark (forest/benchmarking/classical_logic/ripple_carry_adder.py:317-384):
from the results of ``get_n_bit_adder_results`` -- for each of the 4^n pairs of n-bit summands the measured ``[n_shots, n + 1]``
register -- the probability that the sum came out right and the distribution of the Hamming weight of the error.  The reference
compares every shot with the expected answer in Python; here the expected answers are a host table (``adder_expected_bits``) and
the comparison is ONE weight-kind launch of ``fbx_bit_histogram`` over all pairs (of all experiments): bin w counts the shots that
differ from the answer in w bits, so the success probability is bin 0.

The acquisition half (:37-314) is simulated: ``adder`` builds the reference's circuit as a gate list with the summands as run-time
input bits, the register assignment works on a networkx graph where the reference asks a ``QuantumComputer`` for its topology, and
``simulate_n_bit_adder_results`` stands where ``get_n_bit_adder_results`` runs the programs -- the shots of the circuit under
depolarizing noise after every gate and readout flips, drawn on the GPU by ``fbx_reversible_sample_shots``.
``simulate_adder_statistics_batch`` keeps the records on the device and returns the statistics of a whole batch of noise
settings; ``predicted_adder_statistics`` computes the same two arrays exactly, without sampling.

``simulate_compiled_adder_results`` and ``compiled_adder_statistics_batch`` run the adder as the hardware would: compiled to native
gates by ``fbx.compilation.basic_compile`` -- the Toffoli as its 123-gate decomposition -- with an error after every native gate, on
a state vector (``fbx_native_trajectories``)."""
from typing import Sequence

import numpy as np

from ..utils import bitstring_histogram_batch
from . import reversible
from .primitives import CNOT_X_basis, majority_gate, unmajority_add_gate

__all__ = ["adder_expected_bits", "get_success_probabilities_from_results", "get_error_hamming_distributions_from_results",
           "get_success_probabilities_from_results_batch", "get_error_hamming_distributions_from_results_batch",
           "assign_registers_to_line_or_cycle", "get_qubit_registers_for_adder", "adder", "default_adder_registers",
           "simulate_n_bit_adder_results", "simulate_adder_statistics_batch", "predicted_adder_statistics",
           "compiled_adder_circuit", "simulate_compiled_adder_results", "compiled_adder_statistics_batch"]


def adder_expected_bits(n_bits: int) -> np.ndarray:
    """``[4^n, n + 1]`` uint8: row r = the bits of a + b (most significant first), where the 2n-bit number r spells a (high half)
    and b (low half) -- the order of ``all_bitstrings(2 * n_bits)`` in the reference's loops (:331-338)."""
    if n_bits < 1:
        raise ValueError("n_bits must be at least 1")
    r = np.arange(1 << (2 * n_bits), dtype=np.int64)
    ans = (r >> n_bits) + (r & ((1 << n_bits) - 1))
    return ((ans[:, None] >> np.arange(n_bits, -1, -1)) & 1).astype(np.uint8)


def _weight_frequencies(results):
    res = np.asarray(results)
    if res.ndim != 4 or res.shape[3] < 2 or res.shape[1] != 1 << (2 * (res.shape[3] - 1)):
        raise ValueError("results must be [E, 4^n, n_shots, n + 1]: for every pair of n-bit summands the measured n + 1 answer bits")
    E, pairs, n_shots, width = res.shape
    expected = np.broadcast_to(adder_expected_bits(width - 1), (E, pairs, width)).reshape(E * pairs, width)
    _, freq = bitstring_histogram_batch(res.reshape(E * pairs, n_shots, width), expected=expected, kind="weight", frequencies=True)
    return freq.reshape(E, pairs, width + 1)


def get_success_probabilities_from_results_batch(results) -> np.ndarray:
    """``results [E, 4^n, n_shots, n + 1]`` for E experiments -> ``[E, 4^n]`` success probabilities; one launch."""
    return np.ascontiguousarray(_weight_frequencies(results)[:, :, 0])


def get_error_hamming_distributions_from_results_batch(results) -> np.ndarray:
    """``results [E, 4^n, n_shots, n + 1]`` -> ``[E, 4^n, n + 2]``: the relative frequency of every error weight 0..n + 1."""
    return _weight_frequencies(results)


def get_success_probabilities_from_results(results: Sequence[Sequence[Sequence[int]]]) -> Sequence[float]:
    """ripple_carry_adder.py:317-347: the success probability of each of the 4^n additions, as a list."""
    return [float(p) for p in get_success_probabilities_from_results_batch(np.asarray(results)[None])[0]]


def get_error_hamming_distributions_from_results(results: Sequence[Sequence[Sequence[int]]]) -> Sequence[Sequence[float]]:
    """ripple_carry_adder.py:350-384: per addition the relative frequency of each Hamming weight of the error, as a list of lists."""
    return [[float(p) for p in row] for row in get_error_hamming_distributions_from_results_batch(np.asarray(results)[None])[0]]


# --------------------------------------------------------------------------------------------------
# The acquisition half: the circuit as a gate list, the register assignment, and the simulated experiment
# --------------------------------------------------------------------------------------------------
def assign_registers_to_line_or_cycle(start, graph, num_length):
    """ripple_carry_adder.py:37-87: walk the graph from ``start`` and assign the registers as they lie in the circuit diagram of
    [CDKM96] -- carry ancilla, then b_0, a_0, b_1, a_1, .., then the z ancilla.  ``graph`` must leave no choice from ``start``
    on (a line or a cycle).  Returns ``(register_a, register_b, carry_ancilla, z_ancilla)``, what ``adder`` takes."""
    import networkx as nx
    if 2 * num_length + 2 > nx.number_of_nodes(graph):
        raise ValueError("There are not enough qubits in the graph to support the computation.")
    graph = graph.copy()
    register_a, register_b = [], []
    node = carry_ancilla = start
    neighbors = list(graph.neighbors(node))
    for idx in range(2 * num_length):
        graph.remove_node(node)                       # never assigned twice
        if len(neighbors) == 0:
            raise ValueError("Encountered dead end; assignment failed.")
        node = neighbors[0]
        neighbors = list(graph.neighbors(node))
        (register_b if idx % 2 == 0 else register_a).append(node)
    if len(neighbors) == 0:
        raise ValueError("Encountered dead end; assignment failed.")
    return register_a, register_b, carry_ancilla, neighbors[0]         # z: a neighbour of the last a


def get_qubit_registers_for_adder(graph, num_length, qubits=None):
    """ripple_carry_adder.py:90-146 on a networkx graph of the qubit topology: find a path of ``2 num_length + 2`` qubits among
    ``qubits`` (default: all nodes) -- a monomorphism of the path into the graph, found as an isomorphism of line graphs as in
    the reference -- and assign the registers along it from one of its ends."""
    import networkx as nx
    graph = nx.Graph(graph)
    if qubits is not None:
        graph.remove_nodes_from([q for q in list(graph.nodes) if q not in set(qubits)])
    num_desired_nodes = 2 * num_length + 2
    if num_desired_nodes > graph.number_of_nodes():
        raise ValueError("There are not enough qubits in the graph to support the computation.")
    # networkx matches induced subgraphs; matching the EDGES of the path with edges of the graph is an isomorphism between
    # the line graph's subgraphs and a path with one node less
    matcher = nx.algorithms.isomorphism.GraphMatcher(nx.line_graph(graph), nx.path_graph(num_desired_nodes - 1))
    edge_iso = next(matcher.subgraph_isomorphisms_iter(), None)
    if edge_iso is None:
        raise ValueError("An appropriate layout for the qubits could not be found among the provided qubits.")
    subgraph = nx.Graph(graph.edge_subgraph(edge_iso.keys()))
    start = next(node for node in subgraph.nodes if subgraph.degree(node) == 1)
    return assign_registers_to_line_or_cycle(start, subgraph, num_length)


def default_adder_registers(n_bits):
    """The layout of the circuit diagram on qubits 0 .. 2n + 1: carry 0, b_j = 1 + 2j, a_j = 2 + 2j, z = 2n + 1."""
    n = int(n_bits)
    if not 1 <= n <= 31:
        raise ValueError("n_bits must be 1..31 (2 n_bits + 2 qubits, at most 64)")
    return [2 + 2 * j for j in range(n)], [1 + 2 * j for j in range(n)], 0, 2 * n + 1


def adder(register_a, register_b, carry_ancilla, z_ancilla, in_x_basis=False):
    """ripple_carry_adder.py:149-245 as a gate list for ``reversible.encode_reversible``, with the summands as run-time input:
    ``(gates, out_qubits)``.  The registers list the least significant bit first.  In the reference's order: the prep of
    ``register_a`` then ``register_b`` as ``XIN`` gates -- a_j reads input bit n + j and b_j bit j, so the input word r spells
    a in its high half and b in its low half, as ``adder_expected_bits`` assumes -- each followed by ``H`` in the X basis; there
    also ``H`` on both ancillas; the MAJ chain; CNOT of the top a onto ``z_ancilla``; the UMA chain in reverse; in the X basis
    ``H`` on every b and on z.  ``out_qubits = [z, b_{n-1}, .., b_0]``: column 0 of a record is the most significant bit of
    the answer, as ``ro`` in the reference.  ``8 n + 1`` gates in the Z basis, ``31 n + 6`` in the X basis."""
    register_a, register_b = [int(q) for q in register_a], [int(q) for q in register_b]
    n = len(register_a)
    if n != len(register_b):
        raise ValueError("Numbers being added must be equal length bitstrings")
    if n < 1:
        raise ValueError("the registers are empty")
    carry_ancilla, z_ancilla = int(carry_ancilla), int(z_ancilla)
    if len(set(register_a + register_b + [carry_ancilla, z_ancilla])) != 2 * n + 2:
        raise ValueError("the registers and ancillas must be 2 n + 2 different qubits")
    gates = []
    for reg, first_bit in ((register_a, n), (register_b, 0)):
        for j, q in enumerate(reg):
            gates.append(("XIN", (q, first_bit + j)))
            if in_x_basis:
                gates.append(("H", (q,)))
    if in_x_basis:
        gates += [("H", (carry_ancilla,)), ("H", (z_ancilla,))]
    undo_and_add = []
    carry = carry_ancilla
    for a, b in zip(register_a, register_b):
        gates += majority_gate(a, b, carry, in_x_basis)
        undo_and_add = unmajority_add_gate(a, b, carry, in_x_basis) + undo_and_add
        carry = a
    gates += CNOT_X_basis(register_a[-1], z_ancilla) if in_x_basis else [("CNOT", (register_a[-1], z_ancilla))]
    gates += undo_and_add
    if in_x_basis:
        gates += [("H", (q,)) for q in register_b] + [("H", (z_ancilla,))]
    return gates, [z_ancilla] + register_b[::-1]


def _expected_records(n_bits, inputs):
    """Packed expected records (bit j = column j, column 0 the most significant answer bit) of the input words ``inputs``."""
    inputs = np.asarray(inputs, dtype=np.uint64)
    n = np.uint64(n_bits)
    ans = (inputs >> n) + (inputs & ((np.uint64(1) << n) - np.uint64(1)))
    bits = (ans[:, None] >> np.arange(n_bits, -1, -1, dtype=np.uint64)) & np.uint64(1)
    return reversible.pack_records(bits)


def _adder_call(n_bits, registers, in_x_basis, gate_error, noise_class, class_error, inputs):
    """What the three public calls share: ``(words, n_qubits, out_qubits, noise_class, class_error [B, K], inputs, expected)``."""
    n_bits = int(n_bits)
    registers = default_adder_registers(n_bits) if registers is None else registers
    if len(registers[0]) != n_bits:
        raise ValueError("the registers do not hold n_bits qubits each")
    gates, out_qubits = adder(*registers, in_x_basis=in_x_basis)
    n_qubits = max(max(registers[0]), max(registers[1]), registers[2], registers[3]) + 1
    words = reversible.encode_reversible(gates, n_qubits)
    if noise_class is None:
        noise_class = reversible.gate_arity(words) - 1           # one-, two- and three-qubit gates
        if class_error is None:
            class_error = np.asarray(gate_error, dtype=np.float64).reshape(-1, 3)
    elif class_error is None:
        raise ValueError("noise_class comes with class_error")
    class_error = np.asarray(class_error, dtype=np.float64)
    class_error = class_error.reshape(1, -1) if class_error.ndim == 1 else class_error
    if inputs is None:
        if n_bits > 12:
            raise ValueError("all 4^n pairs are the default only up to n_bits = 12; pass a sample of input words")
        inputs = np.arange(1 << (2 * n_bits), dtype=np.uint64)
    inputs = np.ascontiguousarray(np.asarray(inputs, dtype=np.uint64).ravel())
    if inputs.size and int(inputs.max()) >> (2 * n_bits):
        raise ValueError("an input word spells a in bits n .. 2n - 1 and b in bits 0 .. n - 1: nothing above")
    return words, n_qubits, out_qubits, noise_class, class_error, inputs, _expected_records(n_bits, inputs)


def simulate_n_bit_adder_results(n_bits, registers=None, in_x_basis=False, num_shots=100, gate_error=(0.0, 0.0, 0.0),
                                 readout_flip=None, seed=0, noise_class=None, class_error=None) -> np.ndarray:
    """``get_n_bit_adder_results`` (ripple_carry_adder.py:248-314) on a simulated device: for each of the 4^n pairs of summands
    ``num_shots`` measured answers, ``[4^n, num_shots, n + 1]`` uint8 -- what ``get_success_probabilities_from_results`` and
    ``get_error_hamming_distributions_from_results`` take.  ``registers`` as ``adder`` takes them (default
    ``default_adder_registers``).  ``gate_error = (p1, p2, p3)``: the depolarizing probability after every one-, two- and
    three-qubit gate; ``noise_class`` [gates] with ``class_error`` [K] replace these classes (to give the Toffoli the error of
    its decomposition, say).  ``readout_flip`` [n + 1, 2] per answer column: P(read 1 | 0), P(read 0 | 1)."""
    words, n_qubits, out_qubits, cls, ce, inputs, _ = _adder_call(n_bits, registers, in_x_basis, gate_error, noise_class,
                                                                  class_error, None)
    if ce.shape[0] != 1:
        raise ValueError("one noise setting per call; simulate_adder_statistics_batch takes a batch")
    res = reversible.sample_reversible_shots(words, n_qubits, inputs, out_qubits, num_shots, ce, cls, readout_flip, seed)
    if res["status"][0]:
        raise ValueError("a probability is outside [0, 1]")
    return res["bits"][0]


def simulate_adder_statistics_batch(n_bits, class_error, registers=None, in_x_basis=False, num_shots=100, readout_flip=None, seed=0,
                                    noise_class=None, inputs=None, first_item=0, first_input=0):
    """B noise settings at once: ``class_error [B, K]`` (K = 3, the one-, two- and three-qubit gates, unless ``noise_class``
    says otherwise), ``readout_flip`` [n + 1, 2] or [B, n + 1, 2].  Returns ``(success [B, P], hamming [B, P, n + 2])`` -- per
    setting what ``get_success_probabilities_from_results`` and ``get_error_hamming_distributions_from_results`` make of its
    records, from the histogram the sampling kernel keeps: no record leaves the device.  ``inputs``: the input words r (a in the
    high half, b in the low half), default all 4^n pairs; for wide adders (``n_bits`` up to 31) a sample of pairs.  A poisoned
    setting (a probability outside [0, 1]) is a row of NaN."""
    class_error = np.asarray(class_error, dtype=np.float64)
    if class_error.ndim != 2:
        raise ValueError("class_error must be [B, K]")
    words, n_qubits, out_qubits, cls, ce, inputs, expected = _adder_call(n_bits, registers, in_x_basis, None,
                                                                         noise_class, class_error, inputs)
    if int(num_shots) < 1:
        raise ValueError("num_shots must be at least 1")
    res = reversible.sample_reversible_shots(words, n_qubits, inputs, out_qubits, num_shots, ce, cls, readout_flip, seed,
                                             first_item, first_input, expected=expected, bits=False, counts=True)
    hamming = res["counts"] / float(int(num_shots))
    hamming[res["status"] != 0] = np.nan
    return np.ascontiguousarray(hamming[:, :, 0]), hamming


def predicted_adder_statistics(n_bits, class_error, registers=None, in_x_basis=False, readout_flip=None, noise_class=None,
                               inputs=None):
    """The two arrays of ``simulate_adder_statistics_batch`` in the limit of infinitely many shots, exactly: the outcome
    distribution of every (setting, pair) from ``reversible.exact_distribution``, summed by the weight of the error.
    ``2 n_bits + 2 <= 12`` qubits."""
    class_error = np.asarray(class_error, dtype=np.float64)
    if class_error.ndim != 2:
        raise ValueError("class_error must be [B, K]")
    words, n_qubits, out_qubits, cls, ce, inputs, _ = _adder_call(n_bits, registers, in_x_basis, None, noise_class,
                                                                  class_error, inputs)
    m = n_bits + 1
    flips = None if readout_flip is None else np.broadcast_to(np.asarray(readout_flip, dtype=np.float64), (ce.shape[0], m, 2))
    outcome = np.arange(1 << m)
    hamming = np.zeros((ce.shape[0], inputs.size, m + 1))
    for r, word in enumerate(inputs.tolist()):
        answer = (word >> n_bits) + (word & ((1 << n_bits) - 1))
        weight = np.array([bin(v).count("1") for v in (outcome ^ answer).tolist()])
        for b in range(ce.shape[0]):
            dist = reversible.exact_distribution(words, n_qubits, word, ce[b], cls, None if flips is None else flips[b], out_qubits)
            hamming[b, r] = np.bincount(weight, weights=dist, minlength=m + 1)
    return np.ascontiguousarray(hamming[:, :, 0]), hamming


# --------------------------------------------------------------------------------------------------
# The adder on native gates: compiled, with an error after every native gate, on a state vector
# --------------------------------------------------------------------------------------------------
def compiled_adder_circuit(n_bits, registers=None, in_x_basis=False):
    """``adder`` compiled by ``basic_compile`` and encoded: ``(words, angles, n_qubits, out_qubits, noise_class)`` with the
    default classes of ``native_circuit.native_noise_classes`` (0: RX, 1: RZ, 2: CZ).  ``n_bits <= 5`` on the default registers
    (12 qubits); other registers must stay below qubit 13."""
    from .. import native_circuit
    from ..compilation import basic_compile
    n_bits = int(n_bits)
    if not 1 <= n_bits <= 5:
        raise ValueError("n_bits must be 1..5: the state vector of 2 n_bits + 2 qubits has to fit the LDS of one CU")
    registers = default_adder_registers(n_bits) if registers is None else registers
    if len(registers[0]) != n_bits:
        raise ValueError("the registers do not hold n_bits qubits each")
    gates, out_qubits = adder(*registers, in_x_basis=in_x_basis)
    n_qubits = max(max(registers[0]), max(registers[1]), registers[2], registers[3]) + 1
    words, angles = native_circuit.encode_native(basic_compile(gates), n_qubits)
    return words, angles, n_qubits, np.asarray(out_qubits, dtype=np.uint8), native_circuit.native_noise_classes(words)


def _compiled_class_error(class_error):
    ce = np.asarray(class_error, dtype=np.float64)
    ce = ce.reshape(1, -1) if ce.ndim == 1 else ce
    if ce.ndim != 2 or ce.shape[1] != 3:
        raise ValueError("class_error must be (p_rx, p_rz, p_cz) or [B, 3]")
    return np.ascontiguousarray(ce)


def _compiled_inputs(n_bits, inputs):
    if inputs is None:
        return np.arange(1 << (2 * n_bits), dtype=np.uint64)
    inputs = np.ascontiguousarray(np.asarray(inputs, dtype=np.uint64).ravel())
    if inputs.size and int(inputs.max()) >> (2 * n_bits):
        raise ValueError("an input word spells a in bits n .. 2n - 1 and b in bits 0 .. n - 1: nothing above")
    return inputs


def _compiled_marginals(dev, circuit, ce, inputs, trajectories, seed, first_item, first_input):
    """The resident front of both calls: upload, ``fbx_native_trajectories_dev``; the dict of device buffers it returns."""
    from .. import native_circuit
    words, angles, n_qubits, out_qubits, cls = circuit
    T = int(trajectories)
    if not 1 <= T < 2 ** 32:
        raise ValueError("need 1 <= trajectories < 2^32")
    return native_circuit.native_trajectories_dev(
        dev, n_qubits, words.size, dev.upload(words), dev.upload(angles), dev.upload(cls), 3, inputs.size, dev.upload(inputs),
        out_qubits.size, dev.upload(out_qubits), ce.shape[0], T, dev.upload(ce), seed, first_item, first_input)


def simulate_compiled_adder_results(n_bits, registers=None, in_x_basis=False, num_shots=100, class_error=(0.0, 0.0, 0.0),
                                    trajectories=256, readout_flip=None, seed=0) -> np.ndarray:
    """``get_n_bit_adder_results`` (ripple_carry_adder.py:248-314) on a simulated device that runs NATIVE gates: ``[4^n,
    num_shots, n + 1]`` uint8, for each pair of summands ``num_shots`` measured answers.  Resident on the device: ``adder`` ->
    ``basic_compile`` -> ``fbx_native_trajectories_dev`` (the mean outcome distribution of the answer qubits over
    ``trajectories`` Pauli-error trajectories per pair) -> ``fbx_sample_bitstrings_dev`` (the shots, and ``readout_flip`` [n + 1,
    2] per answer column).  ``class_error = (p_rx, p_rz, p_cz)``: the probability of a uniformly random Pauli after every RX
    pulse, every (virtual) RZ and every CZ.  The shots of a pair are drawn from the MEAN of its trajectories: exact without gate
    noise, and otherwise up to the sampling error of that mean (``1 / sqrt(trajectories)`` per probability)."""
    from .. import _lib
    from ..sampling import _noise, _raise_poisoned
    circuit = compiled_adder_circuit(n_bits, registers, in_x_basis)
    ce = _compiled_class_error(class_error)
    if ce.shape[0] != 1:
        raise ValueError("one noise setting per call; compiled_adder_statistics_batch takes a batch")
    inputs = _compiled_inputs(int(n_bits), None)
    P, m, key = int(inputs.size), int(n_bits) + 1, int(seed) & (2 ** 64 - 1)
    shots, _, flips, _ = _noise(P, m, num_shots, None, readout_flip)
    with _lib.DeviceScope() as dev:
        res = _compiled_marginals(dev, circuit, ce, inputs, trajectories, key, 0, 0)
        d_bits, d_status = dev.alloc(P * shots * m), dev.alloc(4 * P)
        _lib.check(_lib.lib().fbx_sample_bitstrings_dev(m, P, shots, res["probs_mean"].ptr, None, _lib.devptr(dev.upload(flips)), key, 0,
                                                        d_bits.ptr, d_status.ptr))
        if res["status"].to_array(np.int32, (1,))[0]:
            raise ValueError("a probability is outside [0, 1]")
        if shots:
            _raise_poisoned(d_status.to_array(np.int32, (P,)), 0, "simulate_compiled_adder_results")
        return d_bits.to_array(np.uint8, (P, shots, m))


def compiled_adder_statistics_batch(n_bits, class_error, registers=None, in_x_basis=False, trajectories=256, seed=0, inputs=None,
                                    first_item=0, first_input=0):
    """B noise settings ``class_error [B, 3]`` = (p_rx, p_rz, p_cz) of the compiled adder at once.  Returns ``(success [B, P],
    hamming [B, P, n + 2])`` in the layout of ``simulate_adder_statistics_batch``, from the mean marginals of
    ``fbx_native_trajectories_dev`` alone: the expectation over shots given the trajectories, without sampling -- entry w of
    ``hamming`` is the weight the mean distribution puts on the answers that differ from a + b in w bits.  ``inputs``: the input
    words r (default all 4^n pairs).  A poisoned setting is a row of NaN."""
    from .. import _lib
    n_bits = int(n_bits)
    circuit = compiled_adder_circuit(n_bits, registers, in_x_basis)
    ce = np.asarray(class_error, dtype=np.float64)
    if ce.ndim != 2:
        raise ValueError("class_error must be [B, 3]")
    ce = _compiled_class_error(ce)
    inputs = _compiled_inputs(n_bits, inputs)
    B, P, m = ce.shape[0], int(inputs.size), n_bits + 1
    with _lib.DeviceScope() as dev:
        res = _compiled_marginals(dev, circuit, ce, inputs, trajectories, seed, first_item, first_input)
        probs = res["probs_mean"].to_array(np.float64, (B, P, 1 << m))
    words = inputs.astype(np.int64)
    answer = (words >> n_bits) + (words & ((1 << n_bits) - 1))
    diff = answer[:, None] ^ np.arange(1 << m)[None, :]
    weight = np.zeros(diff.shape, dtype=np.int64)
    for j in range(m):
        weight += (diff >> j) & 1
    hamming = np.stack([np.where(weight[None] == w, probs, 0.0).sum(axis=2) for w in range(m + 1)], axis=2)
    hamming[np.isnan(probs).any(axis=2)] = np.nan
    return np.ascontiguousarray(hamming[:, :, 0]), hamming
