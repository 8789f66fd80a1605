"""Pairs of states whose fidelity (and, where a spectrum is known, purity and Hilbert-Schmidt product) comes from no solver, and
the host restatements of the measures that are plain sums.  Shared by tests/test_state_measures_big_gpu.py; the generators of
tests/chernoff_cases.py are reused."""
import numpy as np

import chernoff_cases as cc


def pure_pure(d, rng):
    """F = |<psi|phi>|^2"""
    psi, phi = cc.random_vector(d, rng), cc.random_vector(d, rng)
    return np.outer(psi, psi.conj()), np.outer(phi, phi.conj()), {"fidelity": abs(np.vdot(psi, phi)) ** 2, "purity": 1.0}


def pure_mixed(d, rng):
    """pure rho, full-rank sigma: F = <psi|sigma|psi>"""
    psi = cc.random_vector(d, rng)
    sigma = cc.random_state(d, rng)
    return np.outer(psi, psi.conj()), sigma, {"fidelity": float(np.real(np.vdot(psi, sigma @ psi))), "purity": 1.0}


def _commuting(d, rng, a, b):
    u = cc.random_unitary(d, rng)
    exact = {"fidelity": float(np.sqrt(a * b).sum() ** 2), "purity": float((a * a).sum()), "hs_ip": float((a * b).sum())}
    return (u * a) @ u.conj().T, (u * b) @ u.conj().T, exact


def commuting(d, rng):
    """full-rank commuting pair in a random basis: F = (sum_i sqrt(a_i b_i))^2, purity sum a_i^2, hs_ip sum a_i b_i"""
    return _commuting(d, rng, cc.random_spectrum(d, rng), cc.random_spectrum(d, rng))


def identical(d, rng):
    rho = cc.random_state(d, rng)
    return rho, rho.copy(), {"fidelity": 1.0}


def orthogonal(d, rng):
    """mixed states on complementary subspaces: F = 0"""
    k = d // 2
    a = np.concatenate([cc.random_spectrum(k, rng), np.zeros(d - k)])
    b = np.concatenate([np.zeros(k), cc.random_spectrum(d - k, rng)])
    return _commuting(d, rng, a, b)


def rank_deficient(d, rng):
    """mixed / mixed, ranks 3d/4 with supports that overlap on d/2 directions of a common random basis; for one qubit (no room
    for two deficient ranks that overlap) a pure state and a full-rank one in a common basis"""
    if d == 2:
        return _commuting(d, rng, np.array([1.0, 0.0]), cc.random_spectrum(d, rng))
    q = d // 4
    a = np.concatenate([cc.random_spectrum(3 * q, rng), np.zeros(q)])
    b = np.concatenate([np.zeros(q), cc.random_spectrum(3 * q, rng)])
    return _commuting(d, rng, a, b)


FAMILIES = {"pure_pure": pure_pure, "pure_mixed": pure_mixed, "commuting": commuting, "identical": identical,
            "orthogonal": orthogonal, "rank_deficient": rank_deficient}


def family(name, n_qubits, count, seed=0):
    """`count` pairs of one family: rho [count, d, d], sigma [count, d, d], exact {measure: [count]}"""
    rng = np.random.default_rng([seed, n_qubits, sorted(FAMILIES).index(name)])
    items = [FAMILIES[name](2 ** n_qubits, rng) for _ in range(count)]
    exact = {k: np.array([it[2][k] for it in items]) for k in items[0][2]}
    return np.array([it[0] for it in items]), np.array([it[1] for it in items]), exact


def host_sums(rho, sigma):
    """the three measures that are sums and a maximum, in numpy: purity Re tr(rho rho), hs_ip Re tr(rho^H sigma) and the
    reference's trace distance (half the induced 1-norm)"""
    return {"purity": np.einsum("bij,bji->b", rho, rho).real,
            "hs_ip": np.einsum("bij,bij->b", rho.conj(), sigma).real,
            "trace_distance": 0.5 * np.abs(rho - sigma).sum(axis=1).max(axis=1)}


def full_rank_pairs(n_qubits, count, seed):
    rng = np.random.default_rng([seed, n_qubits])
    d = 2 ** n_qubits
    return (np.array([cc.random_state(d, rng) for _ in range(count)]),
            np.array([cc.random_state(d, rng) for _ in range(count)]))


def indefinite(n_qubits, count, seed):
    """random Hermitian trace-one matrices (about half of the spectrum negative)"""
    rng = np.random.default_rng([seed, n_qubits])
    d = 2 ** n_qubits
    h = rng.standard_normal((count, d, d)) + 1j * rng.standard_normal((count, d, d))
    h = h + h.conj().transpose(0, 2, 1)
    return h / np.trace(h, axis1=1, axis2=2).real[:, None, None]
