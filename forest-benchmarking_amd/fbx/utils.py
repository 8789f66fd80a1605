"""Small host-side helpers under the reference's names (forest/benchmarking/utils.py)."""
import numpy as np


def transform_pauli_moments_to_bit(mean_p, var_p):
    """Mean and variance of a Pauli observable (on [-1, 1]) -> those of the bit it is read from (on [0, 1]); utils.py:431-443."""
    return (np.asarray(mean_p) + 1) / 2, np.asarray(var_p) / 4


def transform_bit_moments_to_pauli(mean_c, var_c):
    """Mean and variance of a bit (on [0, 1]) -> those of the Pauli observable (on [-1, 1]); utils.py:446-458."""
    return 2 * np.asarray(mean_c) - 1, 4 * np.asarray(var_c)
