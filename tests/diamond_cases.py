"""Closed-form diamond-norm distances for the tests of diamond_norm_distance[_batch] (plain numpy, d = 2, 4, 8).

Choi matrices use the convention of the rest of the suite: J = sum_K vec(K) vec(K)^H with the column-stacking vec, so the first
tensor factor is the channel's input index and the second its output index.  The quantity every solver here computes is
2 max_rho tr[((1 (x) rho^1/2) J (1 (x) rho^1/2))_+] with rho on the SECOND factor (as the reference's SDP writes it).  For unital
pairs that is the diamond-norm distance; for the replacement channels below it is not, and the closed form says what it is.

Every constructor returns (choi0, choi1, exact)."""
import numpy as np
from scipy.linalg import expm

_PAULI1 = [np.eye(2, dtype=complex), np.array([[0, 1], [1, 0]], dtype=complex),
           np.array([[0, -1j], [1j, 0]]), np.diag([1.0 + 0j, -1.0])]


def kraus2choi(ks):
    ks = [ks] if np.ndim(ks) == 2 else ks
    out = 0
    for k in ks:
        v = np.asarray(k, dtype=complex).reshape(-1, 1, order="F")
        out = out + v @ v.conj().T
    return out


def paulis(nq):
    """The 4^nq n-qubit Pauli matrices (labels in itertools.product('IXYZ') order)."""
    out = [np.eye(1, dtype=complex)]
    for _ in range(nq):
        out = [np.kron(a, p) for a in out for p in _PAULI1]
    return out


def haar_unitary(d, rs):
    g = rs.randn(d, d) + 1j * rs.randn(d, d)
    q, r = np.linalg.qr(g)
    return q * (np.diag(r) / np.abs(np.diag(r)))


def random_hermitian(d, rs):
    h = rs.randn(d, d) + 1j * rs.randn(d, d)
    return (h + h.conj().T) / 2


def random_state(d, rs, rank=None):
    rank = d if rank is None else rank
    g = rs.randn(d, rank) + 1j * rs.randn(d, rank)
    r = g @ g.conj().T
    return r / np.trace(r).real


# ------------------------------------------------------------------------------------------------ unitary pairs
def unitary_exact(u, v):
    """Distance of the channels of U and V: with arc the shortest arc of the unit circle that holds every eigenphase of U^H V,
    2 sin(arc / 2) while arc < pi, else 2.  (The sine form: 2 sqrt(1 - cos^2) loses ~1e-10 relative at small angles.)"""
    ph = np.sort(np.angle(np.linalg.eigvals(u.conj().T @ v)))
    gaps = np.diff(np.concatenate([ph, [ph[0] + 2 * np.pi]]))
    arc = 2 * np.pi - gaps.max()
    return 2.0 * np.sin(arc / 2) if arc < np.pi else 2.0


def unitary_pair(u, v):
    return kraus2choi(u), kraus2choi(v), unitary_exact(u, v)


def unitary_perturbed(d, eps, rs):
    """Random U and V = U exp(-i eps H), H a normalised random Hermitian (spectral norm 1)."""
    u = haar_unitary(d, rs)
    h = random_hermitian(d, rs)
    h = h / np.abs(np.linalg.eigvalsh(h)).max()
    return unitary_pair(u, u @ expm(-1j * eps * h))


def unitary_one_phase(d, theta):
    """diag(e^{i theta}, 1, ..., 1) against the identity: the optimal input state has rank 2; exact 2 sin(|theta| / 2)."""
    v = np.eye(d, dtype=complex)
    v[0, 0] = np.exp(1j * theta)
    c0, c1, exact = unitary_pair(np.eye(d, dtype=complex), v)
    return c0, c1, exact


def unitary_wide(d, rs):
    """Random U and V = U W with W's eigenphases spread over more than pi: exact 2."""
    w = haar_unitary(d, rs)
    ph = np.linspace(-0.9 * np.pi, 0.9 * np.pi, d) if d > 2 else np.array([0.0, np.pi])
    u = haar_unitary(d, rs)
    v = u @ w @ np.diag(np.exp(1j * ph)) @ w.conj().T
    return unitary_pair(u, v)


# ------------------------------------------------------------------------------------------------ Pauli channels
def pauli_channel_choi(p):
    nq = int(round(np.log2(len(p)) / 2))
    return kraus2choi([np.sqrt(w) * P for w, P in zip(p, paulis(nq)) if w > 0]) if np.any(np.asarray(p) > 0) \
        else np.zeros((4 ** nq, 4 ** nq), dtype=complex)


def pauli_pair(p, q):
    """Pauli channels with probabilities p and q (length 4^n): exact sum |p_i - q_i|."""
    p, q = np.asarray(p, dtype=float), np.asarray(q, dtype=float)
    return pauli_channel_choi(p), pauli_channel_choi(q), float(np.abs(p - q).sum())


def random_pauli_probs(nq, rs, sparse=0):
    """Random probabilities on the 4^nq Paulis; with sparse > 0 only that many are non-zero."""
    n = 4 ** nq
    w = rs.rand(n)
    if sparse:
        w[rs.permutation(n)[sparse:]] = 0.0
    return w / w.sum()


def depolarizing_pair(d, p):
    """rho -> (1 - p) rho + p tr(rho) 1/d against the identity: exact 2 p (1 - 1/d^2)."""
    nq = int(round(np.log2(d)))
    probs = np.full(d * d, p / (d * d))
    probs[0] += 1 - p
    ident = np.zeros(d * d)
    ident[0] = 1.0
    c0, c1, _ = pauli_pair(probs, ident)
    assert c0.shape == (4 ** nq, 4 ** nq)
    return c0, c1, 2 * p * (1 - 1 / (d * d))


# ------------------------------------------------------------------------------------------------ replacement channels
def replacement_pair(sigma, tau):
    """rho -> tr(rho) sigma against rho -> tr(rho) tau; Choi kron(1_d, sigma).  With the input state on the second factor the
    optimum is rank 1 (the top eigenvector of sigma - tau) and the value 2 d lambda_max(sigma - tau): neither symmetric in the two
    channels nor bounded by 2."""
    d = sigma.shape[0]
    eye = np.eye(d)
    return np.kron(eye, sigma), np.kron(eye, tau), 2.0 * d * float(np.linalg.eigvalsh(sigma - tau).max())


def random_replacement(d, rs):
    """A replacement pair whose sigma - tau has a simple top eigenvalue (the optimal input state is unique)."""
    while True:
        sigma, tau = random_state(d, rs), random_state(d, rs, rank=1 + rs.randint(d))
        w = np.linalg.eigvalsh(sigma - tau)
        if w[-1] - w[-2] > 0.05:
            return replacement_pair(sigma, tau)


def replacement_top_state(sigma, tau):
    w, v = np.linalg.eigh(sigma - tau)
    return np.outer(v[:, -1], v[:, -1].conj())


# ------------------------------------------------------------------------------------------------ mixtures
def mixture(c0, c1, exact, k):
    """(c1 + t (c0 - c1), c1) with t = 2^-k: J scales by t exactly in floating point, so does the value."""
    t = 2.0 ** -k
    return c1 + t * (c0 - c1), c1, t * exact


# ------------------------------------------------------------------------------------------------ families
def families(nq, seed=0):
    """name -> list of (choi0, choi1, exact) at nq qubits: the cases the tests run."""
    d = 2 ** nq
    rs = np.random.RandomState(1000 + 17 * nq + seed)
    fam = {}
    fam["unitary"] = [unitary_perturbed(d, eps, rs) for eps in (1e-4, 1e-3, 1e-2, 1e-1, 1.0)] + \
                     [unitary_one_phase(d, th) for th in (1e-6, 1e-3, 0.5)] + [unitary_wide(d, rs)]
    n = d * d
    fam["pauli"] = [pauli_pair(random_pauli_probs(nq, rs), random_pauli_probs(nq, rs)),
                    pauli_pair(random_pauli_probs(nq, rs, sparse=2), random_pauli_probs(nq, rs, sparse=3)),
                    pauli_pair(np.eye(n)[0], random_pauli_probs(nq, rs, sparse=1 + n // 4)),
                    pauli_pair(*(2 * [random_pauli_probs(nq, rs)]))]
    fam["depolarizing"] = [depolarizing_pair(d, p) for p in (1e-6, 1e-3, 0.1, 1.0)]
    fam["replacement"] = [random_replacement(d, rs) for _ in range(3)]
    base = fam["unitary"][2], fam["pauli"][0], fam["replacement"][0]
    fam["mixture"] = [mixture(*c, k) for c, k in zip(base, (1, 3, 10))]
    return fam
