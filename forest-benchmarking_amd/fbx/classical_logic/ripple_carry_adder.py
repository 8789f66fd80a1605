"""The analysis half of the ripple-carry adder benchmark (forest/benchmarking/classical_logic/ripple_carry_adder.py:317-384):
from the results of ``get_n_bit_adder_results`` -- for each of the 4^n pairs of n-bit summands the measured ``[n_shots, n + 1]``
register -- the probability that the sum came out right and the distribution of the Hamming weight of the error.  The reference
compares every shot with the expected answer in Python; here the expected answers are a host table (``adder_expected_bits``) and
the comparison is ONE weight-kind launch of ``fbx_bit_histogram`` over all pairs (of all experiments): bin w counts the shots that
differ from the answer in w bits, so the success probability is bin 0.  The circuit builders and ``get_n_bit_adder_results`` need a
``QuantumComputer`` and are not mirrored."""
from typing import Sequence

import numpy as np

from ..utils import bitstring_histogram_batch

__all__ = ["adder_expected_bits", "get_success_probabilities_from_results", "get_error_hamming_distributions_from_results",
           "get_success_probabilities_from_results_batch", "get_error_hamming_distributions_from_results_batch"]


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
