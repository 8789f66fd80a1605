"""The generic primitives under everything that is not a fused kernel -- fbx_eigh (all six code paths), fbx_matmul and
fbx_partial_trace -- on structured inputs (tests/linalg_cases.py) against high-precision eigenvalues
(tests/golden/linalg_cases.npz, from tests/golden/make_linalg_goldens.py), exact integer products and long-double products;
with guard bytes around the outputs and the non-finite contract of include/fbx.h.

The bounds (tests/linalg_cases.py):
  eigenvalues    |w - w_ref| <= 1e-13 ||A||_F + c_w N eps ||A||_2   elementwise, both sorted
  residual       ||A V - V diag(w)||_F <= 1e-13 ||A||_F + c_w N eps ||A||_F   (in long double)
  orthogonality  max |V^H V - I| <= 1e-12 up to N = 64, 1e-12 N above
Eigenvalues that match with multiplicity, a small residual and near-orthonormal vectors together pin every invariant
subspace, so no reference eigenvectors are stored.  Each test prints the ratio of what it saw to its bound (pytest -s).
"""
import ctypes as C
import os

import numpy as np
import pytest

import linalg_cases as lc

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "linalg_cases.npz")
SENTINEL = np.uint64(0x7FF8DEADBEEFCAFE)        # a NaN with a payload no kernel produces
PAD = 64                                        # guard doubles on each side (512 bytes: the payload keeps its alignment)


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    keys = [str(k) for k in z["keys"]]
    return {"c_w": float(z["c_w"]), "sha": dict(zip(keys, (str(s) for s in z["sha256"]))),
            "norm2": dict(zip(keys, z["norm2"])), "normF": dict(zip(keys, z["normF"])), "w": {k: z["w_" + k] for k in keys}}


def check_hashes(N, gold):
    for name, a in lc.cases(N).items():
        assert lc.sha256(a) == gold["sha"][lc.key(name, N)], f"{lc.key(name, N)}: the generator no longer builds the fixture's matrix"


def shuffled_batch(N):
    names = list(lc.cases(N))
    order = np.random.RandomState([7, N]).permutation(len(names))
    names = [names[k] for k in order]
    return names, np.stack([lc.cases(N)[n] for n in names])


def check_item(label, name, N, a, w, v, gold):
    """every bound of the module docstring for one item; returns nothing, prints the ratios"""
    k = lc.key(name, N)
    norm2, normF, c_w = gold["norm2"][k], gold["normF"][k], gold["c_w"]
    assert np.isfinite(w).all() and np.isfinite(v).all(), (label, k)
    assert (np.diff(w) >= 0).all(), (label, k)
    e_err, e_tol = np.abs(w - gold["w"][k]).max(), lc.eigenvalue_tol(N, norm2, normF, c_w)
    r_err, r_tol = lc.residual(a, w, v), lc.residual_tol(N, normF, c_w)
    o_err, o_tol = lc.orthogonality(v), lc.orthogonality_tol(N)
    print(f"ratio {label:10s} {k:24s} eig {e_err / e_tol if e_tol else 0.0:.3f} res {r_err / r_tol if r_tol else 0.0:.3f} "
          f"orth {o_err / o_tol:.3f}")
    assert e_err <= e_tol, (label, k, e_err, e_tol)
    assert r_err <= r_tol, (label, k, r_err, r_tol)
    assert o_err <= o_tol, (label, k, o_err, o_tol)
    if name == "zero":
        assert np.all(w == 0) and np.array_equal(v, np.eye(N)), (label, k)
    if name == "diagonal":                                     # nothing to rotate: the sorted diagonal, exact zeros included
        assert np.array_equal(w, np.sort(np.diag(a).real)), (label, k)
    if name == "oplus0":                                       # the decoupled coordinate's eigenvalue is exactly 0
        assert np.count_nonzero(w == 0) == 1, (label, k, w)
    if name == "mixed_zero":
        assert np.count_nonzero(w == 0) == (1 if N == 3 else 2), (label, k, w)


def run_and_check(label, _lib, N, names, a, gold):
    """one call on the batch, one on the reversed batch (bit-identical per item), one without eigenvectors (bit-identical
    eigenvalues), and the bounds for every item"""
    w, v = _lib.eigh_batch(a)
    wr, vr = _lib.eigh_batch(a[::-1])
    assert np.array_equal(wr[::-1], w) and np.array_equal(vr[::-1], v), (label, N, "results depend on the item's place in the batch")
    assert np.array_equal(_lib.eigh_batch(a, eigenvectors=False), w), (label, N, "eigenvalue-only output differs")
    for b, name in enumerate(names):
        check_item(label, name, N, a[b], w[b], v[b], gold)
    return w, v


@pytest.mark.parametrize("N", lc.DIRECT_SIZES + lc.PADDED_SIZES)
def test_eigh_structured(gpu, gold, N):
    """All families of one size in one shuffled batch: eigh_kernel<N> for N = 2..64 (the generic block Jacobi, the one-wave
    16 x 16, the four-wave 32 x 32 and the role-split 64 x 64 solver), eigh_big_kernel above (the batch is larger than the
    cooperative kernel takes), and the host's zero padding for every other size."""
    check_hashes(N, gold)
    names, a = shuffled_batch(N)
    assert N < 128 or len(names) > 3
    label = "padded" if N in lc.PADDED_SIZES else "big" if N > 64 else f"lds{N}"
    run_and_check(label, gpu, N, names, a, gold)


@pytest.mark.parametrize("cooperative", [1, 0])
def test_eigh_130_few_matrices(gpu, gold, cooperative):
    """Batches of 1 and 3 matrices at N = 130 go to eigh_coop_kernel (one matrix over the whole chip), and with the option
    off to the one-workgroup kernel: eigenvectors included, same bounds, and every family passes through both."""
    N = 130
    check_hashes(N, gold)
    names, a = shuffled_batch(N)
    label = "coop" if cooperative else "big-few"
    with gpu.option("eigh_cooperative", cooperative):
        run_and_check(label, gpu, N, names[:1], a[:1], gold)
        for lo in range(0, len(names), 3):
            run_and_check(label, gpu, N, names[lo:lo + 3], a[lo:lo + 3], gold)


# ------------------------------------------------------------------------------------------------ guard bytes
class Guarded:
    """n doubles of device memory between two runs of sentinel words; read() checks that both runs are untouched"""

    def __init__(self, _lib, n):
        self._lib, self.n = _lib, int(n)
        host = np.full(self.n + 2 * PAD, SENTINEL, dtype=np.uint64)
        self.buf = _lib.DeviceBuffer.from_array(host)
        self.ptr = C.c_void_p(self.buf.ptr.value + 8 * PAD)

    def read(self):
        self._lib.synchronize()
        raw = self.buf.to_array(np.uint64, (self.n + 2 * PAD,))
        assert (raw[:PAD] == SENTINEL).all(), "bytes in front of the output were overwritten"
        assert (raw[PAD + self.n:] == SENTINEL).all(), "bytes behind the output were overwritten"
        return raw[PAD:PAD + self.n]

    def doubles(self):
        return self.read().view(np.float64)


@pytest.mark.parametrize("N", [2, 16, 64, 66])
def test_eigh_dev_writes_inside_its_outputs(gpu, N):
    B = 3
    a = np.stack([lc.cases(N)[n] for n in ("gaussian", "realsym", "repeated")])
    d_a = gpu.DeviceBuffer.from_array(a)
    w_g, v_g = Guarded(gpu, B * N), Guarded(gpu, B * N * N * 2)
    gpu.check(gpu.lib().fbx_eigh_dev(N, B, d_a.ptr, w_g.ptr, v_g.ptr))
    w, v = gpu.eigh_batch(a)
    assert np.array_equal(w_g.doubles().reshape(B, N), w)
    assert np.array_equal(v_g.doubles().view(np.complex128).reshape(B, N, N), v)
    w_only = Guarded(gpu, B * N)
    gpu.check(gpu.lib().fbx_eigh_dev(N, B, d_a.ptr, w_only.ptr, None))
    assert np.array_equal(w_only.doubles().reshape(B, N), w)


# ------------------------------------------------------------------------------------------------ non-finite items
def _poisoned(base, kind):
    a = base.copy()
    N = a.shape[0]
    if kind == "nan_diag":
        a[N // 2, N // 2] = np.nan
    elif kind == "inf_diag":
        a[0, 0] = np.inf
    elif kind == "nan_lower":
        a[N - 1, 0] = complex(np.nan, 0.0)
    elif kind == "inf_lower_imag":
        a[N // 2 + 1 if N > 2 else 1, N // 2 if N > 2 else 0] = complex(0.5, -np.inf)
    return a


NONFINITE = [(4, 1), (16, 1), (64, 1), (66, 1), (130, 1), (130, 0), (3, 1), (65, 1)]


@pytest.mark.parametrize("N,cooperative", NONFINITE)
def test_eigh_nonfinite_item_gives_nan_for_itself_only(gpu, N, cooperative):
    """include/fbx.h: an item with a NaN or Inf on its diagonal or in its strictly lower triangle returns all-NaN w and v, the
    call returns FBX_OK, and every other item is bit-identical to the same call with a finite matrix in that place.  Items
    with NaN / Inf only in the strictly upper triangle are ordinary items.  Direct sizes (every eigh_kernel<N>, the
    one-workgroup and the cooperative kernel at N = 130) and the padded sizes 3 and 65."""
    base = lc.build("gaussian", N)
    others = [lc.build("upper_garbage", N), lc.build("realsym", N)]
    with gpu.option("eigh_cooperative", cooperative):
        for place, kind in enumerate(("nan_diag", "nan_lower", "inf_lower_imag", "inf_diag")):
            place %= 3
            clean = others[:place] + [base] + others[place:]
            dirty = others[:place] + [_poisoned(base, kind)] + others[place:]
            w0, v0 = gpu.eigh_batch(np.stack(clean))
            assert np.isfinite(w0).all() and np.isfinite(v0).all(), (N, kind)
            w1, v1 = gpu.eigh_batch(np.stack(dirty))                            # raises unless FBX_OK
            assert np.isnan(w1[place]).all() and np.isnan(v1[place].real).all() and np.isnan(v1[place].imag).all(), (N, kind, w1[place])
            keep = [b for b in range(3) if b != place]
            assert np.array_equal(w1[keep], w0[keep]) and np.array_equal(v1[keep], v0[keep]), (N, kind)
            w2 = gpu.eigh_batch(np.stack(dirty), eigenvectors=False)
            assert np.isnan(w2[place]).all() and np.array_equal(w2[keep], w0[keep]), (N, kind)


# ------------------------------------------------------------------------------------------------ fbx_matmul
MATMUL_SIZES = (1, 15, 16, 17, 33, 70)
FLAGS = [(0, 0), (0, 1), (1, 0), (1, 1)]


def _op(x, conj_t):
    return x.conj().transpose(0, 2, 1) if conj_t else x


@pytest.mark.parametrize("N", MATMUL_SIZES)
def test_matmul_exact_on_integers(gpu, N):
    """Integer entries below 2^20 and power-of-two scales: every product and partial sum is exact in float64, so the device
    must equal an integer einsum bit for bit, for all four conj_t combinations, with and without scale.  Non-Hermitian
    operands with unrelated real and imaginary parts; three distinct items with distinct scale rows."""
    B = 3
    rs = np.random.RandomState([11, N])
    ar, ai, br, bi = (rs.randint(-2 ** 20 + 1, 2 ** 20, (B, N, N)).astype(np.int64) for _ in range(4))
    s4 = 2 ** rs.randint(0, 5, (B, N)).astype(np.int64)                  # 4 x scale: scale = 2^-2 .. 2^2
    a, b = ar + 1j * ai, br + 1j * bi
    for cta, ctb in FLAGS:
        xr, xi = (ar.transpose(0, 2, 1), -ai.transpose(0, 2, 1)) if cta else (ar, ai)
        yr, yi = (br.transpose(0, 2, 1), -bi.transpose(0, 2, 1)) if ctb else (br, bi)
        for scaled in (False, True):
            s = s4 if scaled else np.full((B, N), 4, dtype=np.int64)
            re = np.einsum("bik,bk,bkj->bij", xr, s, yr) - np.einsum("bik,bk,bkj->bij", xi, s, yi)
            im = np.einsum("bik,bk,bkj->bij", xr, s, yi) + np.einsum("bik,bk,bkj->bij", xi, s, yr)
            assert max(np.abs(re).max(), np.abs(im).max()) < 2 ** 53
            want = (re.astype(np.float64) + 1j * im.astype(np.float64)) / 4.0
            got = gpu.matmul_batch(a, b, conj_t_a=cta, conj_t_b=ctb, scale=s4 / 4.0 if scaled else None)
            assert np.array_equal(got, want), (N, cta, ctb, scaled, np.abs(got - want).max())


@pytest.mark.parametrize("N", MATMUL_SIZES)
def test_matmul_gaussian_against_long_double(gpu, N):
    """|out - ref|_ij <= (N + 2) eps (|op(a)| diag|s| |op(b)|)_ij, the dot-product bound, against a long-double product"""
    B = 3
    rs = np.random.RandomState([12, N])
    a = rs.standard_normal((B, N, N)) + 1j * rs.standard_normal((B, N, N))
    b = rs.standard_normal((B, N, N)) + 1j * rs.standard_normal((B, N, N))
    sc = rs.standard_normal((B, N))
    worst = 0.0
    for cta, ctb in FLAGS:
        x, y = _op(a, cta).astype(np.clongdouble), _op(b, ctb).astype(np.clongdouble)
        for scale in (None, sc):
            s = np.ones((B, N)) if scale is None else scale
            want = np.einsum("bik,bk,bkj->bij", x, s.astype(np.longdouble), y)
            bound = (N + 2) * lc.EPS * np.einsum("bik,bk,bkj->bij", np.abs(x), np.abs(s).astype(np.longdouble), np.abs(y))
            got = gpu.matmul_batch(a, b, conj_t_a=cta, conj_t_b=ctb, scale=scale)
            err = np.abs(got.astype(np.clongdouble) - want)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (N, cta, ctb, scale is not None, float((err / bound).max()))
    print(f"ratio matmul N={N} {worst:.3f}")


def test_matmul_dev_writes_inside_its_output(gpu):
    N, B = 17, 3
    rs = np.random.RandomState(13)
    a = rs.standard_normal((B, N, N)) + 1j * rs.standard_normal((B, N, N))
    b = rs.standard_normal((B, N, N)) + 1j * rs.standard_normal((B, N, N))
    sc = rs.standard_normal((B, N))
    d_a, d_b, d_s = (gpu.DeviceBuffer.from_array(x) for x in (a, b, sc))
    for cta, ctb in FLAGS:
        out = Guarded(gpu, B * N * N * 2)
        gpu.check(gpu.lib().fbx_matmul_dev(N, B, d_a.ptr, cta, d_s.ptr, d_b.ptr, ctb, out.ptr))
        got = out.doubles().view(np.complex128).reshape(B, N, N)
        assert np.array_equal(got, gpu.matmul_batch(a, b, conj_t_a=cta, conj_t_b=ctb, scale=sc)), (cta, ctb)


# ------------------------------------------------------------------------------------------------ fbx_partial_trace
DIM_PAIRS = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 4), (4, 3), (7, 9), (16, 16), (32, 8), (4, 64)]


@pytest.mark.parametrize("dim_a,dim_b", DIM_PAIRS)
def test_partial_trace_exact_on_integers(gpu, dim_a, dim_b):
    """complex entries with integer parts: both partial traces equal the einsum exactly; guard bytes around out"""
    B, n = 3, dim_a * dim_b
    rs = np.random.RandomState([14, dim_a, dim_b])
    x = rs.randint(-2 ** 20, 2 ** 20, (B, n, n)) + 1j * rs.randint(-2 ** 20, 2 ** 20, (B, n, n))
    t = x.reshape(B, dim_a, dim_b, dim_a, dim_b)
    d_x = gpu.DeviceBuffer.from_array(x)
    for keep, want in ((0, np.einsum("xajcj->xac", t)), (1, np.einsum("xiaic->xac", t))):
        m = dim_a if keep == 0 else dim_b
        out = Guarded(gpu, B * m * m * 2)
        gpu.check(gpu.lib().fbx_partial_trace_dev(dim_a, dim_b, keep, B, d_x.ptr, out.ptr))
        got = out.doubles().view(np.complex128).reshape(B, m, m)
        assert np.array_equal(got, want), (dim_a, dim_b, keep)
        host = np.empty((B, m, m), dtype=np.complex128)
        gpu.check(gpu.lib().fbx_partial_trace(dim_a, dim_b, keep, B, gpu.dptr(x.view(np.float64)), gpu.dptr(host.view(np.float64))))
        assert np.array_equal(host, want), (dim_a, dim_b, keep)


@pytest.mark.parametrize("dim_a,dim_b,keep", [(17, 241, 0), (4097, 1, 1), (3, 4, 2), (3, 4, -1)])
def test_partial_trace_refuses_and_leaves_out_untouched(gpu, dim_a, dim_b, keep):
    n = dim_a * dim_b
    x = np.zeros((1, n, n), dtype=np.complex128)
    m = dim_a if keep == 0 else dim_b if keep == 1 else max(dim_a, dim_b)        # what an accepted call would write
    out = np.full(2 * m * m, SENTINEL, dtype=np.uint64)
    rc = gpu.lib().fbx_partial_trace(dim_a, dim_b, keep, 1, gpu.dptr(x.view(np.float64)), gpu.dptr(out.view(np.float64)))
    assert rc != 0
    assert (out == SENTINEL).all()
    d_x = gpu.DeviceBuffer.from_array(x[:, :16, :16])          # never read: the call is refused before any launch
    d_out = Guarded(gpu, 2 * 16 * 16)
    assert gpu.lib().fbx_partial_trace_dev(dim_a, dim_b, keep, 1, d_x.ptr, d_out.ptr) != 0
    assert (d_out.read() == SENTINEL).all()
