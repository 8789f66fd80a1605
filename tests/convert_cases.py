"""Inputs with known answers for the representation changes (fbx_convert, fbx_convert_general, fbx_apply_choi), for
tests/test_convert_exact_gpu.py and tests/test_convert_cases_cpu.py.  numpy and the oracle only.

Two families, every case rebuilt from a seed:

  gaussian integers  matrices [B, D, D] with real and imaginary parts in [-9, 9], Kraus sets [B, K, d, d] with parts in
                     [-3, 3].  Every conversion without the |C| step is a linear (from Kraus operators: bilinear) map whose
                     coefficients are entries of the Pauli matrices, {0, +-1, +-i}, times 1, 1/d or 1/d^2: on integers every
                     product and every partial sum is an integer far below 2^53 (at most D^2 terms of size 9 times the same
                     again, 2e8 at five qubits) and the scale is a power of two, so float64 gives THE answer in any summation
                     order, with or without fused multiply-add.  The expected value is the oracle on the same input;
                     tests/test_convert_cases_cpu.py holds the oracle itself to "exact" (integral after the scale, and equal
                     to an evaluation in int64 for one and two qubits).
  spectra            C = sum_i lambda_i |P_i>><<P_i| / d over the D Pauli matrices (vec of the oracle): the |P_i>> are
                     orthogonal with norm^2 d, so C has the eigenvalues lambda_i and the chi matrix of |C| is
                     diag(|lambda_i| if |lambda_i| > 1e-9 else 0) / d.  lambda = SPECTRUM padded with 0.1 and cut to D
                     entries, on a seeded permutation of the Paulis: both signs, a degenerate pair (and the cluster of the
                     padding), an exact zero, +-2e-9 (kept by the reference's cut at 1e-9) and +-5e-10 (dropped).  The same
                     spectra conjugated into a seeded Haar basis have no closed form: there the oracle's choi2chi is the
                     expected value.  The superoperator and Pauli-Liouville forms of each C are the oracle's linear maps of it.
"""
import functools

import numpy as np

from fbx_oracle import superops as so

SEED = 20261021
MATRIX_REPS = ("choi", "superop", "pauli_liouville", "chi")
# the nine matrix routes without the |C| step, and the four from Kraus operators
LINEAR_ROUTES = (("choi", "superop"), ("choi", "pauli_liouville"), ("superop", "choi"), ("superop", "pauli_liouville"),
                 ("pauli_liouville", "choi"), ("pauli_liouville", "superop"), ("chi", "choi"), ("chi", "superop"),
                 ("chi", "pauli_liouville"))
KRAUS_ROUTES = (("kraus", "choi"), ("kraus", "superop"), ("kraus", "pauli_liouville"), ("kraus", "chi"))
FIVE_QUBIT_ROUTES = (("choi", "pauli_liouville"), ("pauli_liouville", "superop"), ("superop", "choi"), ("chi", "choi"))
ORACLE = {("choi", "superop"): so.choi2superop, ("choi", "pauli_liouville"): so.choi2pauli_liouville,
          ("choi", "chi"): so.choi2chi,
          ("superop", "choi"): so.superop2choi, ("superop", "pauli_liouville"): so.superop2pauli_liouville,
          ("superop", "chi"): so.superop2chi,
          ("pauli_liouville", "choi"): so.pauli_liouville2choi, ("pauli_liouville", "superop"): so.pauli_liouville2superop,
          ("pauli_liouville", "chi"): so.pauli_liouville2chi,
          ("chi", "choi"): so.chi2choi, ("chi", "superop"): so.chi2superop, ("chi", "pauli_liouville"): so.chi2pauli_liouville,
          ("kraus", "choi"): so.kraus2choi, ("kraus", "superop"): so.kraus2superop,
          ("kraus", "pauli_liouville"): so.kraus2pauli_liouville, ("kraus", "chi"): so.kraus2chi}
# power of d that makes the oracle's output on integers integral: the basis change towards the Pauli side divides by d (a
# matrix) or by d^2 (Kraus -> chi), the one away from it multiplies by as much
SCALE_POWER = {("choi", "superop"): 0, ("superop", "choi"): 0, ("chi", "choi"): 0, ("chi", "superop"): 0,
               ("kraus", "choi"): 0, ("kraus", "superop"): 0,
               ("choi", "pauli_liouville"): 1, ("superop", "pauli_liouville"): 1, ("chi", "pauli_liouville"): 1,
               ("pauli_liouville", "choi"): 1, ("pauli_liouville", "superop"): 1, ("kraus", "pauli_liouville"): 1,
               ("kraus", "chi"): 2}
CUT = 1e-9
SPECTRUM = (0.4, -0.3, -5e-10, 2e-9, 0.25, 0.25, 0.0, -2e-9, 5e-10)     # the first four are what one qubit keeps
SPECTRUM_FAR_FROM_THE_CUT = (0.4, -0.3, 0.25, 0.25, 0.0)                # four qubits: see spectrum()


def _rs(*tag):
    return np.random.RandomState([SEED, *tag])


# ------------------------------------------------------------------ gaussian integers
def _gauss_int(rs, shape, bound):
    re = rs.randint(-bound, bound + 1, size=shape)
    im = rs.randint(-bound, bound + 1, size=shape)
    return (re + 1j * im).astype(np.complex128)


def int_matrices(D, B, tag=0):
    """[B, D, D] complex128, parts integers in [-9, 9]: no structure (not Hermitian, not real, not PSD)"""
    return _gauss_int(_rs(1, D, tag), (B, D, D), 9)


def int_kraus(d, K, B, tag=0):
    """[B, K, d, d] complex128, parts integers in [-3, 3]"""
    return _gauss_int(_rs(2, d, K, tag), (B, K, d, d), 3)


def int_states(d, B, tag=0):
    """[B, d, d] complex128, parts integers in [-9, 9], not Hermitian"""
    return _gauss_int(_rs(3, d, tag), (B, d, d), 9)


def oracle_batch(src, dst, x):
    """the oracle's src -> dst on every item of x"""
    f = ORACLE[(src, dst)]
    return np.array([f(list(v)) if src == "kraus" else f(v) for v in x])


@functools.lru_cache(maxsize=None)
def _exact_case(src, dst, n, B, K, tag):
    d = 2 ** n
    x = int_kraus(d, K, B, tag) if src == "kraus" else int_matrices(d * d, B, tag)
    want = oracle_batch(src, dst, x)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


def exact_case(src, dst, n, B, K=0, tag=0):
    """(input, the oracle's output), computed once per case and read-only"""
    return _exact_case(src, dst, n, B, K, tag)


def is_integral(x, scale):
    """largest deviation of x * scale from the integers (0.0 is what exactness means)"""
    y = np.asarray(x) * scale
    return float(max(np.abs(y.real - np.rint(y.real)).max(), np.abs(y.imag - np.rint(y.imag)).max()))


# ---- the same maps in int64, written from the definitions (nothing but the oracle's integer basis matrices is shared)
def _split(z):
    z = np.asarray(z)
    re, im = np.rint(z.real).astype(np.int64), np.rint(z.imag).astype(np.int64)
    assert np.array_equal(re, z.real) and np.array_equal(im, z.imag), "not a gaussian integer"
    return re, im


def _mul(a, b, spec):
    """complex product of int64 pairs through einsum"""
    return (np.einsum(spec, a[0], b[0]) - np.einsum(spec, a[1], b[1]), np.einsum(spec, a[0], b[1]) + np.einsum(spec, a[1], b[0]))


def _conj_t(a):
    return a[0].T.copy(), -a[1].T


def _reshuffle(a, d):
    """out[(p,q),(r,s)] = in[(s,q),(r,p)]"""
    return tuple(np.einsum("sqrp->pqrs", v.reshape(d, d, d, d)).reshape(d * d, d * d) for v in a)


def int64_route(src, dst, x):
    """d^SCALE_POWER times src -> dst of one gaussian-integer item, as an (re, im) pair of int64 arrays"""
    x = np.asarray(x)
    d = x.shape[-1] if src == "kraus" else int(round(np.sqrt(x.shape[-1])))
    P = _split(so.pauli2computational_basis_matrix(d))
    PH = _conj_t(P)
    to_pl = lambda s: _mul(_mul(PH, s, "ij,jk->ik"), P, "ij,jk->ik")        # d * superop2pauli_liouville
    from_pl = lambda m: _mul(_mul(P, m, "ij,jk->ik"), PH, "ij,jk->ik")      # d * pauli_liouville2superop; chi2choi
    if src == "kraus":
        ks = [_split(k) for k in x]
        D = d * d
        if dst == "superop" or dst == "pauli_liouville":
            s = (np.zeros((D, D), np.int64), np.zeros((D, D), np.int64))
            for k in ks:                                                    # conj(K) (x) K
                t = _mul((k[0], -k[1]), k, "ij,kl->ikjl")
                s = (s[0] + t[0].reshape(D, D), s[1] + t[1].reshape(D, D))
            return s if dst == "superop" else to_pl(s)
        c = (np.zeros((D, D), np.int64), np.zeros((D, D), np.int64))
        for k in ks:                                                        # vec(K) vec(K)^H, column stacking
            v = (k[0].T.reshape(D), k[1].T.reshape(D))
            if dst == "chi":                                                # d * computational2pauli vec(K)
                v = _mul(PH, v, "ij,j->i")
            t = _mul(v, (v[0], -v[1]), "i,j->ij")
            c = (c[0] + t[0], c[1] + t[1])
        return c
    a = _split(x)
    if src == "chi":
        choi = from_pl(a)
        return choi if dst == "choi" else _reshuffle(choi, d) if dst == "superop" else to_pl(_reshuffle(choi, d))
    if src == "choi":
        return _reshuffle(a, d) if dst == "superop" else to_pl(_reshuffle(a, d))
    if src == "superop":
        return _reshuffle(a, d) if dst == "choi" else to_pl(a)
    return from_pl(a) if dst == "superop" else _reshuffle(from_pl(a), d)


def apply_choi_exact(choi, rho):
    """apply_choi_matrix_2_state on batches, from the definition: out[o, p] = sum_{a, i} rho[a, i] choi[(a, o), (i, p)]"""
    d = rho.shape[-1]
    return np.einsum("bai,baoip->bop", rho, choi.reshape(-1, d, d, d, d))


# ------------------------------------------------------------------ spectra
def spectrum(n):
    """the eigenvalues of the spectra family for n qubits: D entries.  At four qubits the values near the cut are left out:
    that route is held to 1e-9 (an HBM-resident 256 x 256 Jacobi), where 5e-10 / d is not observable."""
    D = 4 ** n
    lam = list(SPECTRUM_FAR_FROM_THE_CUT if n >= 4 else SPECTRUM)
    lam = (lam + [0.1] * D)[:D]
    return np.array(lam)


def _haar(D, rs):
    z = rs.standard_normal((D, D)) + 1j * rs.standard_normal((D, D))
    q, r = np.linalg.qr(z)
    ph = np.diagonal(r) / np.abs(np.diagonal(r))
    return q * ph[None, :]


@functools.lru_cache(maxsize=None)
def spectra_cases(n, count=2):
    """{"diag": (choi [count, D, D], chi [count, D, D]), "basis": (choi, chi)}: the Pauli-diagonal matrices with their closed
    form and the same spectra in a Haar basis with the oracle's choi2chi.  Read-only."""
    d, D = 2 ** n, 4 ** n
    lam = spectrum(n)
    vp = np.hstack([so.vec(p) for p in so.n_qubit_pauli_matrices(n)])          # columns |P_i>>
    out = {"diag": ([], []), "basis": ([], [])}
    for k in range(count):
        rs = _rs(4, n, k)
        l = lam[rs.permutation(D)]
        c = (vp * l[None, :]) @ vp.conj().T / d
        out["diag"][0].append(c)
        out["diag"][1].append(np.diag(np.where(np.abs(l) > CUT, np.abs(l), 0.0)).astype(complex) / d)
        u = _haar(D, rs)
        cu = u @ c @ u.conj().T
        cu = (cu + cu.conj().T) / 2
        out["basis"][0].append(cu)
        out["basis"][1].append(so.choi2chi(cu))
    res = {}
    for fam, (c, x) in out.items():
        c, x = np.array(c), np.array(x)
        c.setflags(write=False)
        x.setflags(write=False)
        res[fam] = (c, x)
    return res


def as_source(src, choi):
    """the Choi matrices `choi` [B, D, D] in the representation `src` (choi, superop or pauli_liouville)"""
    if src == "choi":
        return np.array(choi)
    f = so.choi2superop if src == "superop" else so.choi2pauli_liouville
    return np.array([f(c) for c in choi])


def diagonal_int_choi(n, B):
    """B diagonal Choi matrices with signed integer diagonals that differ from item to item, and the exact chi of |C|:
    P^H |C| P / d^2 in integers"""
    d, D = 2 ** n, 4 ** n
    diag = ((np.arange(D)[None, :] * 7 + np.arange(B)[:, None] * 3) % 19 - 9).astype(np.float64)
    choi = np.zeros((B, D, D), complex)
    choi[:, np.arange(D), np.arange(D)] = diag
    P = so.pauli2computational_basis_matrix(d)
    chi = np.matmul(P.conj().T[None] * np.abs(diag)[:, None, :], P) / (d * d)
    return choi, chi
