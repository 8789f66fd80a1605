"""Pairs of states whose quantum Chernoff bound is known exactly, for tests/test_chernoff_gpu.py and tests/test_chernoff_cpu.py.

The quantity (fbx.distance_measures.quantum_chernoff_bound_batch): with rho = V diag(a) V^H, sigma = W diag(b) W^H and
O_ij = |<v_i|w_j>|^2, Q(s) = sum_ij O_ij a_i^s b_j^(1-s) over the eigenvalues above zero_tol * lambda_max of their own matrix, and
qcb = min over s in [0, 1] of Q(s).  Every constructor returns (rho, sigma, exact) and is deterministic in its generator.
``mp_chernoff`` evaluates the same quantity for any pair in mpmath (used by tests/golden/make_chernoff_goldens.py).
"""
import mpmath as mp
import numpy as np


def random_unitary(d, rng):
    z = (rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))) / np.sqrt(2)
    q, r = np.linalg.qr(z)
    return q * (np.diag(r) / np.abs(np.diag(r)))


def random_spectrum(d, rng, rank=None):
    """unit-trace eigenvalues, the first `rank` positive (bounded away from zero), the rest exactly zero"""
    rank = d if rank is None else rank
    x = rng.uniform(0.1, 1.0, d)
    x[rank:] = 0.0
    return x / x.sum()


def random_state(d, rng, rank=None):
    u = random_unitary(d, rng)
    return (u * random_spectrum(d, rng, rank)) @ u.conj().T


def random_vector(d, rng):
    v = rng.standard_normal(d) + 1j * rng.standard_normal(d)
    return v / np.linalg.norm(v)


def commuting_min(a, b, dps=40):
    """min over s in [0, 1] of sum_i a_i^s b_i^(1-s) over the i with a_i, b_i > 0, in mpmath: (value, argmin)"""
    with mp.workdps(dps):
        terms = [(mp.mpf(float(x)), mp.mpf(float(y))) for x, y in zip(a, b) if x > 0 and y > 0]
        return _min_convex(terms, [mp.mpf(1)] * len(terms))


def _min_convex(terms, weights):
    """min over [0, 1] of sum_k w_k x_k^s y_k^(1-s) (convex): an endpoint when the derivative does not change sign, else
    bisection on the derivative to the working precision.  Returns (value, argmin) as mpf."""
    def q(s):
        return mp.fsum(w * x ** s * y ** (1 - s) for (x, y), w in zip(terms, weights))

    def dq(s):
        return mp.fsum(w * x ** s * y ** (1 - s) * (mp.log(x) - mp.log(y)) for (x, y), w in zip(terms, weights))
    if not terms:
        return mp.mpf(0), mp.mpf(0)
    if dq(mp.mpf(0)) >= 0:
        return q(mp.mpf(0)), mp.mpf(0)
    if dq(mp.mpf(1)) <= 0:
        return q(mp.mpf(1)), mp.mpf(1)
    lo, hi = mp.mpf(0), mp.mpf(1)
    for _ in range(int(mp.mp.prec) + 8):
        mid = (lo + hi) / 2
        if dq(mid) < 0:
            lo = mid
        else:
            hi = mid
    s = (lo + hi) / 2
    return q(s), s


def mp_chernoff(rho, sigma, zero_tol=1e-12, dps=40):
    """The device's quantity for one float64 pair, in mpmath at `dps` digits: lower triangles read, eigenvalues from mp.eighe,
    the zero_tol rule, the minimum of the convex Q.  Returns (value, argmin) as mpf."""
    with mp.workdps(dps):
        def herm(x):
            n = x.shape[0]
            m = mp.matrix(n, n)
            for r in range(n):
                for c in range(n):
                    z = x[r, c] if r >= c else np.conj(x[c, r])
                    m[r, c] = mp.mpc(float(z.real), float(z.imag) if r != c else 0.0)
            return m
        a, v = mp.eighe(herm(rho))
        b, w = mp.eighe(herm(sigma))
        n = rho.shape[0]
        amax, bmax = max(a), max(b)
        keep_a = [i for i in range(n) if a[i] > 0 and a[i] > zero_tol * amax]
        keep_b = [j for j in range(n) if b[j] > 0 and b[j] > zero_tol * bmax]
        terms, weights = [], []
        for i in keep_a:
            for j in keep_b:
                ip = mp.fsum(mp.conj(v[k, i]) * w[k, j] for k in range(n))
                o = abs(ip) ** 2
                if o > 0:
                    terms.append((a[i], b[j]))
                    weights.append(o)
        return _min_convex(terms, weights)


# ------------------------------------------------------------------------------------------------ exact families
def commuting(d, rng):
    """commuting pair rotated by one random unitary: a one-dimensional minimisation"""
    u = random_unitary(d, rng)
    a, b = random_spectrum(d, rng), random_spectrum(d, rng)
    rho = (u * a) @ u.conj().T
    sigma = (u * b) @ u.conj().T
    value, _ = commuting_min(a, b)
    return rho, sigma, float(value)


def pure_pure(d, rng):
    psi, phi = random_vector(d, rng), random_vector(d, rng)
    return np.outer(psi, psi.conj()), np.outer(phi, phi.conj()), float(abs(np.vdot(psi, phi)) ** 2)


def pure_mixed(d, rng):
    """pure rho, full-rank sigma: the minimum is at s = 0, <psi|sigma|psi>"""
    psi = random_vector(d, rng)
    sigma = random_state(d, rng)
    return np.outer(psi, psi.conj()), sigma, float(np.real(np.vdot(psi, sigma @ psi)))


def orthogonal(d, rng):
    """supports on complementary subspaces: Q = 0"""
    u = random_unitary(d, rng)
    k = d // 2
    a = np.zeros(d)
    b = np.zeros(d)
    a[:k] = rng.uniform(0.1, 1.0, k)
    b[k:] = rng.uniform(0.1, 1.0, d - k)
    return (u * (a / a.sum())) @ u.conj().T, (u * (b / b.sum())) @ u.conj().T, 0.0


def identical(d, rng):
    rho = random_state(d, rng)
    return rho, rho.copy(), 1.0


FAMILIES = {"commuting": commuting, "pure_pure": pure_pure, "pure_mixed": pure_mixed, "orthogonal": orthogonal,
            "identical": identical}


def family(name, n_qubits, count, seed=0):
    """`count` pairs of one family: rho [count, d, d], sigma [count, d, d], exact [count]"""
    rng = np.random.default_rng([seed, n_qubits, sorted(FAMILIES).index(name)])
    d = 2 ** n_qubits
    cases = [FAMILIES[name](d, rng) for _ in range(count)]
    return (np.array([c[0] for c in cases]), np.array([c[1] for c in cases]), np.array([c[2] for c in cases]))


# ------------------------------------------------------------------------------------------------ golden families
def golden_pair(kind, d, rng):
    """random full-rank ('full'), random low-rank ('lowrank': ranks about d / 2, overlapping supports) and nearly commuting
    ('near': sigma's eigenbasis turned by exp(1e-3 i H)) pairs"""
    if kind == "full":
        return random_state(d, rng), random_state(d, rng)
    if kind == "lowrank":
        k = max(1, d // 2)
        return random_state(d, rng, rank=k), random_state(d, rng, rank=min(d, k + 1))
    u = random_unitary(d, rng)
    h = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    h = (h + h.conj().T) / 2
    w, v = np.linalg.eigh(h)
    turn = (v * np.exp(1e-3j * w)) @ v.conj().T
    a, b = random_spectrum(d, rng), random_spectrum(d, rng)
    u2 = turn @ u
    return (u * a) @ u.conj().T, (u2 * b) @ u2.conj().T
