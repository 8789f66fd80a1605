"""References and pinned items for the device random operators (csrc/fbx_random.hip), shared by tests/test_random_cpu.py and
tests/test_random_exact_gpu.py.  Nothing here touches the GPU.

The device and the oracle (fbx_oracle.acquisition) draw the same fp64 Ginibre entries from one counter-based stream; what
differs is the arithmetic after them (Gram-Schmidt / Jacobi in LDS on the device, LAPACK in the oracle).  The references of this
file take those fp64 entries as exact numbers and do the rest in mpmath at MP_DPS digits, so they are the exact answer for the
numbers the device actually holds:

  mp_q_factor(G)   Q of G = Q R with diag(R) > 0 (haar_rand_unitary)
  mp_kraus(Gs)     K_j = G_j S^{-1/2}, S = sum_j G_j^H G_j (fbx_random_kraus)

Both return np.clongdouble arrays (64-bit mantissas: the rounding of the reference is 2^11 times below fp64's).

reference_bcsz_choi(X, dim) is the REFERENCE's way to a random CPTP map, restated from the description in
fbx/operator_tools/random_operators.py:72-79 (rho = X X^H, its partial trace, Q = red^{-1/2} (x) 1, Q rho Q): a construction
that shares nothing with the Kraus form but the claim, in the header of csrc/fbx_random.hip, that the two agree.

Error model of the bounds.  S^{-1/2} of a matrix known to relative accuracy u has relative accuracy of the order of
u kappa_2(S), and so has K_j = G_j S^{-1/2}, whose entries are at most 1 in modulus; the Q factor of G moves by u kappa_2(G)
under a relative perturbation u of G.  The oracle's own distance from mpmath in these units (ORACLE_C_S, ORACLE_C_Q, measured by
tests/test_random_cpu.py) is the yardstick: the device is allowed C_S = 4 ORACLE_C_S and C_Q = 4 ORACLE_C_Q, a factor 4 of
headroom for a different but backward-stable algorithm, times d for the length of its inner products.
"""
import functools

import mpmath as mp
import numpy as np

from fbx_oracle import acquisition as oa

U = 2.0 ** -53                                   # unit roundoff of fp64
MP_DPS = 50

# (seed, item) of the worst-conditioned S = G^H G (one d x d Ginibre matrix, K = 1) among items 0..19999 of the stream of seed 17
ILL = {2: (17, 12631), 4: (17, 12700), 8: (17, 9957)}
ILL_KAPPA_MIN = {2: 1e5, 4: 5e5, 8: 3e6}         # kappa_2(S) of those items is above this (recomputed by test_random_cpu.py)

# Worst |K_oracle - K_mp|_max / (u kappa_2(S)) and |Q_oracle - Q_mp|_max / (u kappa_2(G)) of the float64 oracle (numpy eigh / qr)
# over the ILL items and items 0..15 of seed 17 at d = 2, 4, 8 (K = 1 and K = d for the Kraus sets): the figures
# tests/test_random_cpu.py prints as `RANDDEV oracle ...` and asserts to lie at or below these, rounded up to two digits.
ORACLE_C_S = 1.9                                 # measured 1.83 (d = 2, item 13, K = 2: kappa_2(S) = 1.6)
ORACLE_C_Q = 2.2                                 # measured 2.11 (d = 2, item 8: kappa_2(G) = 1.8)
C_S = 4 * ORACLE_C_S
C_Q = 4 * ORACLE_C_Q


# ------------------------------------------------------------------------------------------------ the stream
def ginibre(seed, item, dim, K=1, tag=0):
    """[K][dim][dim] fp64 Ginibre matrices of one item, in the element order of fbx_random_kraus"""
    return oa.ginibre_entries(seed, item, K * dim * dim, tag).reshape(K, dim, dim)


def stacked(Gs):
    """[K d][d]: the G_j on top of each other; S = stacked^H stacked"""
    Gs = np.asarray(Gs)
    return Gs.reshape(-1, Gs.shape[-1])


def kappa_of(Gs):
    """kappa_2(S) of S = sum_j G_j^H G_j from the singular values of the stacked G_j (never from S itself)"""
    s = np.linalg.svd(stacked(Gs), compute_uv=False)
    return float((s[0] / s[-1]) ** 2)


def kappa_S(seed, item, dim, K):
    return kappa_of(ginibre(seed, item, dim, K))


def kappa_G(seed, item, dim, tag=0):
    s = np.linalg.svd(ginibre(seed, item, dim, 1, tag)[0], compute_uv=False)
    return float(s[0] / s[-1])


def bcsz_x(Gs):
    """X of the reference's construction: column j is the column-stacked G_j"""
    Gs = np.asarray(Gs)
    return np.stack([g.T.reshape(-1) for g in Gs], axis=1)


# ------------------------------------------------------------------------------------------------ mpmath
def _to_mp(a):
    a = np.asarray(a, dtype=np.complex128)
    return mp.matrix([[mp.mpc(float(z.real), float(z.imag)) for z in row] for row in a])


def _ld(x):
    return np.longdouble(mp.nstr(x, 25, strip_zeros=False))


def _from_mp(m):
    out = np.empty((m.rows, m.cols), dtype=np.clongdouble)
    for i in range(m.rows):
        for j in range(m.cols):
            z = mp.mpmathify(m[i, j])
            out[i, j] = _ld(mp.re(z)) + 1j * _ld(mp.im(z))
    return out


def mp_q_factor(G):
    """Q of G = Q R with diag(R) > 0: Gram-Schmidt at MP_DPS digits (it loses kappa_2(G) of them, which leaves 40 and more)"""
    with mp.workdps(MP_DPS):
        a = _to_mp(G)
        n = a.rows
        q = mp.matrix(n, n)
        for j in range(n):
            v = a[:, j].copy()
            for _ in range(2):
                for k in range(j):
                    c = mp.fsum(mp.conj(q[i, k]) * v[i] for i in range(n))
                    for i in range(n):
                        v[i] -= c * q[i, k]
            nrm = mp.sqrt(mp.fsum(mp.re(x) ** 2 + mp.im(x) ** 2 for x in v))
            for i in range(n):
                q[i, j] = v[i] / nrm
        return _from_mp(q)


def mp_kraus(Gs):
    """[K][d][d] K_j = G_j S^{-1/2} with S = sum_j G_j^H G_j through mp.eigh at MP_DPS digits"""
    Gs = np.asarray(Gs, dtype=np.complex128)
    with mp.workdps(MP_DPS):
        x = _to_mp(stacked(Gs))
        s = x.H * x
        lam, v = mp.eigh(s)
        d = s.rows
        w = v * mp.diag([1 / mp.sqrt(lam[i]) for i in range(d)]) * v.H
        return _from_mp(x * w).reshape(Gs.shape)


@functools.lru_cache(maxsize=None)
def mp_kraus_item(seed, item, dim, K):
    out = mp_kraus(ginibre(seed, item, dim, K))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mp_q_item(seed, item, dim, tag=0):
    out = mp_q_factor(ginibre(seed, item, dim, 1, tag)[0])
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ the reference's BCSZ route
def _inv_sqrt_psd(m):
    w, v = np.linalg.eigh(m)
    return (v / np.sqrt(w)) @ v.conj().T


def reference_bcsz_choi(X, dim):
    """Choi matrix of the map the reference builds from a Ginibre X [dim^2][K]: rho = X X^H, red = tr_2 rho (`iaja->ij`),
    Q = red^{-1/2} (x) 1, Q rho Q"""
    X = np.asarray(X, dtype=np.complex128)
    rho = X @ X.conj().T
    red = np.einsum("iaja->ij", rho.reshape(dim, dim, dim, dim))
    q = np.kron(_inv_sqrt_psd(red), np.eye(dim))
    return q @ rho @ q


# ------------------------------------------------------------------------------------------------ the bounds
def q_tol(dim, kappa_g):
    return C_Q * dim * U * kappa_g


def kraus_tol(dim, kappa_s):
    return C_S * dim * U * kappa_s + 32 * dim * U


def max_abs(a):
    return float(np.abs(np.asarray(a)).max())


def tp_defect(ks):
    """max |sum_j K_j^H K_j - 1| of one Kraus set [K][d][d], accumulated in long double"""
    ks = np.asarray(ks, dtype=np.clongdouble)
    return max_abs(np.einsum("kji,kjl->il", ks.conj(), ks) - np.eye(ks.shape[-1]))


# ------------------------------------------------------------------------------------------------ moments
# The moments of tests/test_random_exact_gpu.py, dim = 8: name -> (seed, expected value).  The seeds are fixed here, once, by one
# condition that does not involve the device: the ORACLE's stream of that seed lies within 3.5 standard errors of the expected
# value, for the first MOMENT_B_CPU items (asserted by tests/test_random_cpu.py) -- seed 6 of the Bures ensemble, at 2.9 sigma on
# 1500 items, was passed over for having little room left.
MOMENT_DIM = 8
MOMENT_B_GPU = 20000
MOMENT_B_CPU = 1500
MOMENT_ORACLE_SIGMA = 3.5
MOMENT_DEVICE_SIGMA = 5.0


def ginibre_purity_mean(d, k):
    return (d + k) / (d * k + 1.0)


def bures_purity_mean(d):
    return (5.0 * d * d + 1.0) / (2.0 * d * (d * d + 2.0))


MOMENTS = {
    "purity_rank1": (30, ginibre_purity_mean(MOMENT_DIM, 1)),
    "purity_rank3": (31, ginibre_purity_mean(MOMENT_DIM, 3)),
    "purity_rank8": (36, ginibre_purity_mean(MOMENT_DIM, 8)),
    "purity_bures": (34, bures_purity_mean(MOMENT_DIM)),
    "tr_u": (38, 1.0),
    "tr_u2": (38, 2.0),
}


def purity(rho):
    rho = np.asarray(rho)
    return np.einsum("bij,bji->b", rho, rho).real


def moment_sample(name, mats):
    """the per-item statistic of one MOMENTS entry from a batch [B][d][d] of states (purity_*) or unitaries (tr_u*)"""
    mats = np.asarray(mats)
    if name.startswith("purity"):
        return purity(mats)
    if name == "tr_u":
        return np.abs(np.trace(mats, axis1=1, axis2=2)) ** 2
    return np.abs(np.trace(mats @ mats, axis1=1, axis2=2)) ** 2


def moment_sigma(sample, want):
    """(mean - want) / (std / sqrt(n)): the distance of a sample mean from its expected value in standard errors"""
    sample = np.asarray(sample, dtype=np.float64)
    dev, se = sample.mean() - want, sample.std(ddof=1) / np.sqrt(sample.size)
    if se == 0.0:
        return 0.0 if dev == 0.0 else float(np.copysign(np.inf, dev))
    return float(dev / se)


# A standard error describes sampling only.  The statistic itself is computed in fp64 from fp64 entries that carry a few u of
# relative error each, d^2 products to a purity: an error of up to MOMENT_ROUNDING per item that no sample size averages away.
# For five of the six moments that is 1e-9 standard errors.  The sixth, the purity of a rank-1 state, is 1 for EVERY item: its
# sample spread is rounding alone (2e-16), its standard error 1e-18, and `moment_sigma` of it is 0 or +-80 according to whether
# a mean of doubles next to 1 rounds to 1.  So the moment checks allow |mean - want| <= n_sigma * SE + MOMENT_ROUNDING, and the
# deterministic case is checked item by item on top of that, which is more than any statistic of it.
MOMENT_ROUNDING = 64 * MOMENT_DIM * U
DETERMINISTIC_MOMENTS = ("purity_rank1",)


def check_moment(label, name, mats, n_sigma):
    """prints `RANDDEV <label> moment ...`, asserts the bound above, returns moment_sigma"""
    want = MOMENTS[name][1]
    x = moment_sample(name, mats)
    sigma = moment_sigma(x, want)
    se = x.std(ddof=1) / np.sqrt(x.size)
    print(f"RANDDEV {label} moment {name:13s} n {x.size:6d} mean {x.mean():.10f} want {want:.10f} sigma {sigma:+.2f}")
    assert abs(x.mean() - want) <= n_sigma * se + MOMENT_ROUNDING, (label, name, x.mean(), want, sigma)
    if name in DETERMINISTIC_MOMENTS:
        assert np.abs(x - want).max() <= MOMENT_ROUNDING, (label, name, float(np.abs(x - want).max()))
    return sigma


def oracle_moment_batch(name, seed, B):
    d = MOMENT_DIM
    if name == "purity_bures":
        return np.array([oa.bures_state(seed, b, d) for b in range(B)])
    if name.startswith("purity_rank"):
        return np.array([oa.ginibre_state(seed, b, d, int(name[len("purity_rank"):])) for b in range(B)])
    return np.array([oa.haar_unitary(seed, b, d) for b in range(B)])
