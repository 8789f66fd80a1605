"""Inputs shared by test_rb_acquire_cpu.py and test_rb_acquire_gpu.py: three distinct noise channels per width (depolarizing,
amplitude damping = non-unital, coherent over-rotation), the sequence shapes at which fbx_rb_acquire's work split can go wrong,
and host references in plain numpy."""
import numpy as np

from fbx import clifford

SEED = (0x5EED << 32) + 0xACE1                       # above 2^32: both key words are in use
FLIPS = {1: np.array([[0.03, 0.08]]), 2: np.array([[0.03, 0.08], [0.05, 0.01]])}

# (depths, K): S K sequences per experiment against the 64 lanes of a wavefront and the 256 threads of a workgroup
SHAPES = {
    "partial_wavefront_15": ((2, 3, 7), 5),
    "full_wavefront_64": ((2, 3, 5, 9), 16),
    "two_units_70": ((2, 3, 4, 5, 6, 7, 9), 10),
    "past_a_workgroup_300": ((2, 5, 3), 100),
}


def depolarizing(n, p):
    out = np.eye(4 ** n) * p
    out[0, 0] = 1.0
    return out


def _damping_1q(gamma):
    s = np.sqrt(1.0 - gamma)
    return np.array([[1.0, 0, 0, 0], [0, s, 0, 0], [0, 0, s, 0], [gamma, 0, 0, 1.0 - gamma]])


def _rx_1q(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, c, -s], [0, 0, s, c]])


def _rz_1q(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[1.0, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1.0]])


def amplitude_damping(n, gamma):
    return _damping_1q(gamma) if n == 1 else np.kron(_damping_1q(gamma), _damping_1q(0.6 * gamma))


def over_rotation(n, theta):
    return _rx_1q(theta) if n == 1 else np.kron(_rx_1q(theta), _rz_1q(-0.7 * theta))


def channels(n, interleaved=False):
    """noise_ptms [3, G, D, D]: experiment 0 depolarizing, 1 amplitude damping, 2 a unitary over-rotation; with ``interleaved`` a
    second, different matrix of the same family follows the interleaved gate"""
    first = [depolarizing(n, 0.97), amplitude_damping(n, 0.04), over_rotation(n, 0.11)]
    if not interleaved:
        return np.array(first)[:, None]
    second = [depolarizing(n, 0.91), amplitude_damping(n, 0.09), over_rotation(n, -0.23)]
    return np.stack([np.array(first), np.array(second)], axis=1)


def interleaved_gate(n):
    """some element that is neither the identity nor an involution-free corner: index 7 of 24, index 4321 of 11520"""
    return clifford.from_index(n, 7 if n == 1 else 4321)


def dense_measurement(vector, n, digits, flips=None):
    """The outcome distribution of measuring the state with Pauli vector ``vector`` in the product basis ``digits`` (1, 2, 3 = X,
    Y, Z per qubit), through the density matrix and projectors, then one confusion matrix per qubit: the long way round that
    ``synthetic.rb_outcome_distributions`` is checked against."""
    from fbx.synthetic import pauli_matrix
    import itertools
    d = 2 ** n
    rho = sum(vector[k] * pauli_matrix(codes) for k, codes in enumerate(itertools.product(range(4), repeat=n))) / d
    p = np.empty(d)
    for o in range(d):
        proj = np.eye(1)
        for q in range(n):
            bit = (o >> (n - 1 - q)) & 1
            proj = np.kron(proj, (np.eye(2) + (-1) ** bit * pauli_matrix((digits[q],))) / 2)
        p[o] = np.trace(proj @ rho).real
    if flips is not None:
        conf = np.eye(1)
        for q in range(n):
            f0, f1 = flips[q]
            conf = np.kron(conf, np.array([[1 - f0, f1], [f0, 1 - f1]]))
        p = conf @ p
    return p


# the statistical test (GPU test 7), also evaluated on the host: 64 one-qubit experiments under depolarizing noise
STAT = dict(E=64, K=32, shots=200, depths=(2, 4, 8, 16, 32), p=0.98, flip=0.02, seed=20261020)


def stat_bounds():
    """(expected mean Z, five binomial standard deviations of the mean over E K N shots) per depth: a shot is +-1 with mean
    mu = (1 - 2 f) p^m, m = depth noisy steps, so the mean of E K N of them has variance (1 - mu^2) / (E K N)"""
    s = STAT
    mu = (1 - 2 * s["flip"]) * s["p"] ** np.array(s["depths"], dtype=np.float64)
    return mu, 5.0 * np.sqrt((1 - mu * mu) / (s["E"] * s["K"] * s["shots"]))
