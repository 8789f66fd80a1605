"""Structured Hermitian matrices for the generic eigensolver (fbx_eigh), for tests/test_linalg_gpu.py, tests/test_linalg_cpu.py
and tests/golden/make_linalg_goldens.py.

Every matrix is rebuilt from a seed (numpy.random.RandomState, whose streams do not change between numpy versions): the
matrices are too large to commit.  The fixture (tests/golden/linalg_cases.npz) records a SHA-256 of each matrix's bytes, and
every test checks it first, so a generator that drifts from the fixture is reported as that and not as a numerical failure.
To keep the bytes the same on every machine the builders use no BLAS / LAPACK call and no reduction whose order numpy may
choose: real and imaginary parts are separate float64 arrays, every step is one correctly rounded elementwise operation, and
every sum is a sequential numpy.add.accumulate.

A family is Q diag(spec) Q^H with a Haar-distributed Q (Gram-Schmidt of a complex Gaussian matrix) unless it says otherwise.
The LOWER triangle defines the matrix (numpy.linalg.eigh's convention, and the device's); ``hermitian`` mirrors it.
"""
import functools
import hashlib

import mpmath as mp
import numpy as np

DIRECT_SIZES = (2, 4, 8, 16, 32, 64, 66, 100, 130)          # sizes fbx_eigh_dev takes as they are
PADDED_SIZES = (1, 3, 5, 6, 9, 12, 27, 33, 63, 65, 129)     # sizes fbx_eigh embeds in the next one with zero rows / columns
DIRECT_FAMILIES = ("gaussian", "repeated", "cluster9", "cluster13", "rank1", "rankhalf", "graded", "diagonal", "realsym",
                   "imagoff", "oplus0", "zero", "scale_up", "scale_down", "upper_garbage")
PADDED_FAMILIES = ("gaussian", "rank1", "rep_zero", "mixed_zero", "oplus0", "zero")
_ALL = tuple(dict.fromkeys(DIRECT_FAMILIES + PADDED_FAMILIES))
EPS = 2.0 ** -52
SEED = 20261018


def _rs(name, N):
    return np.random.RandomState([SEED, N, _ALL.index(name)])


def _sum0(x):
    """sum over axis 0, strictly in index order"""
    return np.add.accumulate(x, axis=0)[-1]


def _sum1(x):
    return np.add.accumulate(x, axis=1)[:, -1]


def _cplx(re, im):
    out = np.empty(re.shape, dtype=np.complex128)
    out.real = re
    out.imag = im
    return out


def haar(N, rs):
    """(real, imaginary) parts of a Haar unitary: Gram-Schmidt (twice, for orthogonality at rounding level) of a complex
    Gaussian matrix, column by column"""
    zr, zi = rs.standard_normal((N, N)), rs.standard_normal((N, N))
    qr, qi = np.zeros((N, N)), np.zeros((N, N))
    for j in range(N):
        vr, vi = zr[:, j].copy(), zi[:, j].copy()
        for _ in range(2):
            if j == 0:
                break
            br, bi = qr[:, :j], qi[:, :j]
            cr = _sum0(br * vr[:, None] + bi * vi[:, None])          # c = Q^H v
            ci = _sum0(br * vi[:, None] - bi * vr[:, None])
            vr = vr - _sum1(br * cr - bi * ci)                       # v -= Q c
            vi = vi - _sum1(br * ci + bi * cr)
        nrm = np.sqrt(_sum0(vr * vr + vi * vi))
        qr[:, j], qi[:, j] = vr / nrm, vi / nrm
    return qr, qi


def from_spectrum(q, spec):
    """sum_k spec[k] q_k q_k^H, accumulated in the order of k: exactly Hermitian, with an exactly real diagonal"""
    qr, qi = q
    N = qr.shape[0]
    re, im = np.zeros((N, N)), np.zeros((N, N))
    for k in range(N):
        s = spec[k]
        if s == 0.0:
            continue
        a, b = qr[:, k], qi[:, k]
        re = re + s * (np.multiply.outer(a, a) + np.multiply.outer(b, b))
        im = im + s * (np.multiply.outer(b, a) - np.multiply.outer(a, b))
    return _cplx(re, im)


def _gaussian(N, rs):
    gr, gi = rs.standard_normal((N, N)), rs.standard_normal((N, N))
    return _cplx(gr + gr.T, gi - gi.T)


def _embed(block, N, at):
    """`block` on the coordinates `at` of an N x N zero matrix: the other coordinates are exactly decoupled"""
    out = np.zeros((N, N), dtype=np.complex128)
    at = np.asarray(at)
    out[at[:, None], at[None, :]] = block
    return out


def _distinct(N, rs):
    return rs.uniform(0.25, 2.0, N) * np.where(rs.randint(0, 2, N) == 0, -1.0, 1.0)


def _spec_repeated(N, rs):
    """multiplicities N/2, 3 and 2: a repeated positive, a repeated negative and a repeated exact zero eigenvalue"""
    spec = _distinct(N, rs)
    if N >= 10:
        groups = ((N // 2, 0.75), (3, -1.25), (2, 0.0))
    elif N == 8:
        groups = ((4, 0.75), (2, -1.25), (2, 0.0))
    elif N == 4:
        groups = ((2, -1.25), (2, 0.0))
    else:
        groups = ((2, -1.25),)
    k = 0
    for mult, val in groups:
        spec[k:k + mult] = val
        k += mult
    return spec[rs.permutation(N)]


def _spec_cluster(N, rs, gap):
    """triples lambda (1 + j gap), j = 0, 1, 2, of both signs among distinct eigenvalues"""
    spec = _distinct(N, rs)
    centres = (1.5, -0.625, 0.875)
    for g, lam in enumerate(centres):
        for j in range(3):
            if 3 * g + j < N and (3 * g + j < 2 or N >= 4):
                spec[3 * g + j] = lam * (1.0 + j * gap)
    return spec[rs.permutation(N)]


def _spec_graded(N):
    """logspace(-12, 12, N) with every third eigenvalue negative; the powers come from mpmath, not from the C library"""
    with mp.workdps(30):
        mag = [float(mp.power(10, mp.mpf(-12) + mp.mpf(24 * k) / max(N - 1, 1))) for k in range(N)]
    return np.array(mag) * np.where(np.arange(N) % 3 == 0, -1.0, 1.0)


def build(name, N):
    """the N x N complex128 matrix of one family, or None where the family does not exist at this size"""
    rs = _rs(name, N)
    if name == "gaussian":
        return _gaussian(N, rs)
    if name == "repeated":
        return from_spectrum(haar(N, rs), _spec_repeated(N, rs))
    if name == "cluster9":
        return from_spectrum(haar(N, rs), _spec_cluster(N, rs, 1e-9))
    if name == "cluster13":
        return from_spectrum(haar(N, rs), _spec_cluster(N, rs, 1e-13))
    if name == "rank1":                                   # a pure state |u><u|, ||u|| = 1
        ur, ui = rs.standard_normal(N), rs.standard_normal(N)
        nrm = np.sqrt(_sum0(ur * ur + ui * ui))
        ur, ui = ur / nrm, ui / nrm
        return _cplx(np.multiply.outer(ur, ur) + np.multiply.outer(ui, ui), np.multiply.outer(ui, ur) - np.multiply.outer(ur, ui))
    if name == "rankhalf":                                # PSD of rank N / 2 with trace 1
        spec = np.zeros(N)
        spec[:N // 2] = rs.uniform(0.1, 1.0, N // 2)
        spec = spec / _sum0(spec)
        return from_spectrum(haar(N, rs), spec)
    if name == "graded":
        return from_spectrum(haar(N, rs), _spec_graded(N))
    if name == "diagonal":                                # unsorted, with ties, a +0.0 and a -0.0
        vals = rs.randint(-3, 4, N) * 0.5
        vals[0] = -0.0
        if N >= 4:
            vals[N - 1] = 0.0
            vals[2] = vals[1]
        return _cplx(np.diag(vals), np.zeros((N, N)))
    if name == "realsym":
        g = rs.standard_normal((N, N))
        return _cplx(g + g.T, np.zeros((N, N)))
    if name == "imagoff":                                 # real diagonal, purely imaginary off-diagonal entries
        k = np.tril(rs.standard_normal((N, N)), -1)
        return _cplx(np.diag(rs.standard_normal(N)), k - k.T)
    if name == "oplus0":                                  # A' (+) [0]: the last coordinate is exactly decoupled
        if N < 2:
            return None
        return _embed(_gaussian(N - 1, rs), N, np.arange(N - 1))
    if name == "zero":
        return np.zeros((N, N), dtype=np.complex128)
    if name in ("scale_up", "scale_down"):                # the Gaussian case times 2^200 / 2^-200, exactly
        g = _gaussian(N, _rs("gaussian", N))
        e = 200 if name == "scale_up" else -200
        return _cplx(np.ldexp(g.real, e), np.ldexp(g.imag, e))
    if name == "upper_garbage":                           # the Gaussian case; the strictly upper triangle must not be read
        if N < 2:
            return None
        g = _gaussian(N, _rs("gaussian", N))
        junk = np.array([np.nan, np.inf, -np.inf, 1e300])
        r, c = np.triu_indices(N, 1)
        g.real[r, c] = junk[(r + 2 * c) % 4]
        g.imag[r, c] = junk[(3 * r + c + 1) % 4]
        return g
    if name == "rep_zero":                                # max(2, N / 2) zero eigenvalues of a dense matrix, the rest of both signs
        if N < 3:
            return None
        spec = _distinct(N, rs)
        spec[:max(2, N // 2)] = 0.0
        return from_spectrum(haar(N, rs), spec[rs.permutation(N)])
    if name == "mixed_zero":                              # eigenvalues of both signs and exactly decoupled zero coordinates
        if N < 3:                                         # (first and middle), so that the padding's zeros sort into the middle
            return None
        zeros = (0,) if N == 3 else (0, N // 2)
        at = np.array([k for k in range(N) if k not in zeros])
        m = len(at)
        spec = rs.uniform(0.25, 2.0, m) * np.where(np.arange(m) % 2 == 0, -1.0, 1.0)
        return _embed(from_spectrum(haar(m, rs), spec), N, at)
    raise KeyError(name)


def family_names(N):
    return DIRECT_FAMILIES if N in DIRECT_SIZES else PADDED_FAMILIES


@functools.lru_cache(maxsize=None)
def cases(N):
    """{family: matrix} at one size, in the order of the family list; built once per process, read-only"""
    out = {}
    for name in family_names(N):
        a = build(name, N)
        if a is not None:
            a.setflags(write=False)
            out[name] = a
    return out


def key(name, N):
    return f"n{N}_{name}"


def all_keys():
    return [key(name, N) for N in DIRECT_SIZES + PADDED_SIZES for name in cases(N)]


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.complex128).tobytes()).hexdigest()


def hermitian(a):
    """the matrix the solver sees: the lower triangle mirrored, the diagonal's imaginary part dropped"""
    low = np.tril(a, -1)
    return low + low.conj().T + np.diag(np.diag(a).real)


# ------------------------------------------------------------------------------------------------ the bounds of the tests
def eigenvalue_tol(N, norm2, normF, c_w):
    """1e-13 ||A||_F (the solver's stopping rule, sqrt(FBX_JACOBI_TOL2) ||A||_F) + c_w N eps ||A||_2 (LAPACK's measured error
    against mpmath, with its margin)"""
    return 1e-13 * normF + c_w * N * EPS * norm2


def residual_tol(N, normF, c_w):
    return 1e-13 * normF + c_w * N * EPS * normF


def orthogonality_tol(N):
    return 1e-12 if N <= 64 else 1e-12 * N


def residual(a, w, v):
    """||A V - V diag(w)||_F in long double"""
    al = hermitian(a).astype(np.clongdouble)
    vl = v.astype(np.clongdouble)
    r = al @ vl - vl * w.astype(np.longdouble)[None, :]
    return float(np.sqrt((r.real ** 2 + r.imag ** 2).sum()))


def orthogonality(v):
    N = v.shape[-1]
    return float(np.abs(v.conj().T @ v - np.eye(N)).max())
