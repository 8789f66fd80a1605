"""Shared inputs of tests/test_frames_cpu.py and tests/test_frames_gpu.py: random Clifford circuits over all 15 opcodes with their
exact outcome distributions from a state-vector simulation, and the density-matrix simulation of ``dfe_cases`` read out as an
outcome distribution.  Dense convention: qubit q is tensor factor q, so qubit 0 is the most significant bit of an outcome index;
a packed outcome word has bit q = qubit q."""
import functools

import numpy as np

import dfe_cases as dc
from fbx import clifford_circuit as cc

SUPPORT_TOL = 1e-9                     # |amplitude|^2 above this: the outcome is in the support


def dense_probabilities(gates, n):
    """|<i| U |0..0>|^2 for every outcome index i (qubit 0 most significant), gate by gate on the state vector."""
    psi = np.zeros((2,) * n, dtype=complex)
    psi[(0,) * n] = 1.0
    for name, qubits in gates:
        k = len(qubits)
        u = dc.GATE[name].reshape((2,) * (2 * k))
        psi = np.moveaxis(np.tensordot(u, psi, axes=(list(range(k, 2 * k)), list(qubits))), list(range(k)), list(qubits))
    return np.abs(psi.reshape(-1)) ** 2


def index_to_word(i, n):
    """Outcome index (qubit 0 most significant) -> packed word (bit q = qubit q)."""
    return sum(((int(i) >> (n - 1 - q)) & 1) << q for q in range(n))


def words_to_indices(words, n):
    words = np.asarray(words, dtype=np.uint64)
    out = np.zeros(words.shape, dtype=np.int64)
    for q in range(n):
        out |= ((words >> np.uint64(q)) & np.uint64(1)).astype(np.int64) << (n - 1 - q)
    return out


@functools.lru_cache(maxsize=None)
def case_circuits():
    """200 random circuits, n = 1..8, up to 40 gates, as ``(n, gates, probabilities)``; together they use every opcode."""
    rng = np.random.default_rng(20240)
    out = []
    for i in range(200):
        n = 1 + i % 8
        gates = dc.random_circuit(rng, n, int(rng.integers(0, 41)))
        out.append((n, gates, dense_probabilities(gates, n)))
    assert {name for _, gates, _ in out for name, _ in gates} == set(cc.GATE_NAMES)
    return out


def support_indices(probs):
    return np.flatnonzero(probs > SUPPORT_TOL)


def noisy_probabilities(gates, n, noise_class, class_error):
    """The exact outcome distribution of the circuit with a depolarizing channel of its class's strength after every gate."""
    rho = np.zeros((2 ** n, 2 ** n), dtype=complex)
    rho[0, 0] = 1.0
    return np.real(np.diag(dc.noisy_channel(rho, gates, n, noise_class, class_error)))


def frequencies(words, n):
    """Relative frequencies of the outcome indices in one row of packed words."""
    return np.bincount(words_to_indices(words, n), minlength=2 ** n) / len(words)


def wide_circuit(n, n_gates, seed=0):
    """A random circuit for the mask edges: the two-qubit gates first visit the pairs that straddle bit 31 / 32 and the top bit."""
    pairs = [(a, b) for a, b in ((31, 32), (0, n - 1), (n - 2, n - 1), (30, 31)) if 0 <= a < n and 0 <= b < n and a != b]
    return dc.random_circuit(np.random.default_rng(7000 * n + n_gates + seed), n, n_gates, pairs)
