"""The device random operators (csrc/fbx_random.hip) item by item: against the oracle's restatement of the counter-based stream
and against mpmath (tests/random_cases.py), past the grid caps of the three kernels, with both words of the seed and of the item
id in use, at every rank, at every Kraus count that takes another launch path, and on the worst-conditioned items of 20 000.

Bounds (u = 2^-53; kappa from the singular values of the fp64 Ginibre entries both sides hold):
  Ginibre entries          1e-13 absolute against the oracle (|z| <= 6.8, angle <= 2 pi: rounding is at 1e-14)
  Ginibre states           1e-13 against the oracle (entries <= 1 in modulus, no decomposition)
  U^H U - 1                1e-13, on every item checked
  U against mp_q_factor    C_Q d u kappa_2(G),                  C_Q = 4 ORACLE_C_Q = 8.8   (the oracle measures 2.11)
  K against mp_kraus, TP   C_S d u kappa_2(S) + 32 d u,         C_S = 4 ORACLE_C_S = 7.6   (the oracle measures 1.83)
  the same two bounds hold against the float64 oracle, whose own error is a fraction of them
  Bures states             1e-13 + 8 (tr M / tr P) C_Q d u kappa_2(G'): P = (1 + U) M (1 + U)^H / tr moves by at most
                           4 |dU| tr M / tr P for a change dU of U (|1 + U| <= 2, |M| <= tr M), twice that with its trace
  moments                  5 standard errors (random_cases.check_moment), seeds fixed by the oracle stream lying within 3.5 of them

Measured on an MI355X (the `RANDDEV device` lines; recorded, not used to set anything; also in include/fbx.h), as fractions of
the bound: U past the grid cap 0.150 / 0.038 / 0.010 at d = 2 / 4 / 8; Kraus sets against the oracle at most 0.064, against
mpmath 0.020, TP defect 0.111 (d = 2, K = 64); BCSZ Choi matrices 0.022; Ginibre and Bures states 0.004.  On the ILL items, as
multiples of d u kappa_2: |K - K_mp| 0.006 / 0.007 / 0.004, TP defect 0.013 / 0.015 / 0.009, |U - Q_mp| 0.020 / 0.004 / 0.006.
Moments: 0.00, +0.01, -0.13, +0.12, +0.15, +0.38 standard errors.

Before herm_inv_sqrt was made to sweep to 2^-52 ||S||_F (it stopped at the solver's default 1e-13 ||S||_F), this file failed at
test_kraus_past_the_grid_cap[4-2]: item 5 of seed 17, kappa_2(S) = 14, was 7.1e-14 from the oracle against a bound of 6.0e-14.
"""
import numpy as np
import pytest

import random_cases as rc
from fbx_oracle import acquisition as oa, superops as so

pytestmark = pytest.mark.gpu

DIMS = (2, 4, 8)
CAP = 256 * 32                                    # workgroups of the per-item kernels; x 256 threads for the Ginibre kernel
B_CAP = CAP + 67
GINIBRE_CAP_ELEMS = CAP * 256
KINDS = ("unitary", "state_vector", "ginibre_state", "bures_state")


@pytest.fixture(scope="module")
def ro(gpu):
    from fbx.operator_tools import random_operators
    return random_operators


def _cap_sample(B):
    return sorted(set(range(64)) | set(range(8160, 8259)) | set(range(0, B, 97)))


def _device(ro, kind, dim, B, seed, first, rank=None):
    if kind == "unitary":
        return ro.haar_rand_unitary_batch(dim, B, seed=seed, first_item=first)
    if kind == "state_vector":
        return ro.haar_rand_state_batch(dim, B, seed=seed, first_item=first)
    if kind == "ginibre_state":
        return ro.ginibre_state_matrix_batch(dim, rank, B, seed=seed, first_item=first)
    return ro.bures_measure_state_matrix_batch(dim, B, seed=seed, first_item=first)


def _bures_tol(seed, item, dim):
    a = rc.ginibre(seed, item, dim)[0]
    m = a @ a.conj().T
    w = np.eye(dim) + oa.haar_unitary(seed, item, dim, 1)
    amp = np.trace(m).real / np.trace(w @ m @ w.conj().T).real
    return 1e-13 + 8 * amp * rc.q_tol(dim, rc.kappa_G(seed, item, dim, 1))


def _check_item(kind, got, seed, item, dim, rank=None):
    """one item of one per-item kind against the oracle; returns err / tol"""
    if kind == "unitary":
        assert rc.max_abs(got.conj().T @ got - np.eye(dim)) < 1e-13, (kind, dim, seed, item)
        err, tol = rc.max_abs(got - oa.haar_unitary(seed, item, dim)), rc.q_tol(dim, rc.kappa_G(seed, item, dim))
    elif kind == "state_vector":
        err, tol = rc.max_abs(got[:, 0] - oa.haar_unitary(seed, item, dim)[:, 0]), rc.q_tol(dim, rc.kappa_G(seed, item, dim))
    elif kind == "ginibre_state":
        err, tol = rc.max_abs(got - oa.ginibre_state(seed, item, dim, rank)), 1e-13
    else:
        err, tol = rc.max_abs(got - oa.bures_state(seed, item, dim)), _bures_tol(seed, item, dim)
    assert err <= tol, (kind, dim, seed, item, err, tol)
    return err / tol


def _check_kraus(got, seed, item, dim, K, ref=None):
    """one Kraus set against the oracle (or `ref`) and its TP defect, both within kraus_tol; returns the two ratios"""
    kappa = rc.kappa_S(seed, item, dim, K)
    tol = rc.kraus_tol(dim, kappa)
    err = rc.max_abs(got - (oa.random_kraus(seed, item, dim, K) if ref is None else ref))
    tp = rc.tp_defect(got)
    assert err <= tol, ("kraus", dim, K, seed, item, err, tol, kappa)
    assert tp <= tol, ("kraus TP", dim, K, seed, item, tp, tol, kappa)
    return err / tol, tp / tol


def _pieces(fn, B, cuts):
    """the batch generated in pieces with first_item, joined"""
    edges = [0] + list(cuts) + [B]
    return np.concatenate([fn(hi - lo, lo) for lo, hi in zip(edges[:-1], edges[1:])])


# ------------------------------------------------------------------------------------------------ every item, past the grid caps
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", KINDS)
def test_per_item_kinds_past_the_grid_cap(ro, kind, dim):
    """B = 8192 + 67: the last 67 items are written by workgroups on their second trip round the stride loop"""
    seed, first, rank = 40 + dim, 1000, max(1, dim - 1)
    whole = _device(ro, kind, dim, B_CAP, seed, first, rank)
    worst = max(_check_item(kind, whole[b], seed, first + b, dim, rank) for b in _cap_sample(B_CAP))
    parts = _pieces(lambda n, lo: _device(ro, kind, dim, n, seed, first + lo, rank), B_CAP, (5000, 8200))
    assert np.array_equal(whole, parts), "an item depends on the batch it was generated in"
    print(f"RANDDEV device cap {kind:13s} d {dim} worst err / tol {worst:.3f}")


@pytest.mark.parametrize("dim,K", [(2, 1), (4, 2)])
def test_kraus_past_the_grid_cap(ro, dim, K):
    seed, first = 17, 12000 if dim == 2 else 0             # d = 2: the batch holds ILL item 12631
    whole = ro.random_kraus_batch(dim, K, B_CAP, seed=seed, first_item=first)
    sample = _cap_sample(B_CAP) + ([rc.ILL[2][1] - first] if dim == 2 else [])
    ratios = [_check_kraus(whole[b], seed, first + b, dim, K) for b in sample]
    parts = _pieces(lambda n, lo: ro.random_kraus_batch(dim, K, n, seed=seed, first_item=first + lo), B_CAP, (5000, 8200))
    assert np.array_equal(whole, parts), "an item depends on the batch it was generated in"
    print(f"RANDDEV device cap kraus d {dim} K {K} worst err / tol {max(r[0] for r in ratios):.3f} TP / tol {max(r[1] for r in ratios):.3f}")


def test_ginibre_past_the_grid_cap(ro):
    """16 x 11 x 12 001 = 2 112 176 elements > 8192 x 256: the last 15 024 are written on the second trip"""
    dim, k, B, seed = 16, 11, 12001, 11
    elems = dim * k
    assert B * elems > GINIBRE_CAP_ELEMS
    whole = ro.ginibre_matrix_complex_batch(dim, k, B, seed=seed)
    edge = GINIBRE_CAP_ELEMS // elems                         # the item that holds element 2 097 152
    assert edge * elems < GINIBRE_CAP_ELEMS < (edge + 1) * elems
    for b in sorted({0, B - 1, edge - 2, edge - 1, edge, edge + 1, edge + 2} | set(range(0, B, 97))):
        assert rc.max_abs(whole[b] - oa.ginibre_matrix(seed, b, dim, k)) < 1e-13, b
    parts = _pieces(lambda n, lo: ro.ginibre_matrix_complex_batch(dim, k, n, seed=seed, first_item=lo), B, (5000, edge + 1))
    assert np.array_equal(whole, parts)
    assert len(np.unique(whole.reshape(-1))) == whole.size, "two elements share a draw"


# ------------------------------------------------------------------------------------------------ high words
HIGH_SEEDS = (2 ** 32 + 11, 2 ** 63 + 5, 2 ** 64 - 1)
HIGH_FIRST = (2 ** 32 - 3, 2 ** 40 + 7)                    # a batch of 8 at 2^32 - 3 crosses the boundary


@pytest.mark.parametrize("first", HIGH_FIRST)
@pytest.mark.parametrize("seed", HIGH_SEEDS)
def test_high_words_of_seed_and_item_id(ro, seed, first):
    B, M = 8, 2 ** 32
    skip = max(first, M) - first                           # the items from `skip` on have a high word in their id

    def differs_mod(got, fn):
        """the items whose id has a high word are not those of the id mod 2^32, and no item is that of the seed mod 2^32"""
        assert not np.array_equal(got[skip:], fn(B - skip, seed, (first + skip) % M)), "the item id's high word is dropped"
        assert not np.array_equal(got, fn(B, seed % M, first)), "the seed's high word is dropped"

    for dim in DIMS:
        rank, K = max(1, dim // 2), 2
        for kind in KINDS:
            got = _device(ro, kind, dim, B, seed, first, rank)
            for b in range(B):
                _check_item(kind, got[b], seed, first + b, dim, rank)
            differs_mod(got, lambda n, sd, f0: _device(ro, kind, dim, n, sd, f0, rank))
        got = ro.random_kraus_batch(dim, K, B, seed=seed, first_item=first)
        for b in range(B):
            _check_kraus(got[b], seed, first + b, dim, K)
        differs_mod(got, lambda n, sd, f0: ro.random_kraus_batch(dim, K, n, seed=sd, first_item=f0))
    g = ro.ginibre_matrix_complex_batch(3, 5, B, seed=seed, first_item=first)
    for b in range(B):
        assert rc.max_abs(g[b] - oa.ginibre_matrix(seed, first + b, 3, 5)) < 1e-13
    differs_mod(g, lambda n, sd, f0: ro.ginibre_matrix_complex_batch(3, 5, n, seed=sd, first_item=f0))


def test_default_seed_is_a_64_bit_key_the_oracle_reproduces(ro):
    np.random.seed(1)
    key = ro._stream_seed(None)
    assert key >= 2 ** 32, "this numpy seed no longer gives a key with a high word: pick another"
    np.random.seed(1)
    u = ro.haar_rand_unitary_batch(4, 6)
    for b in range(6):
        _check_item("unitary", u[b], key, b, 4)
    np.random.seed(1)
    ks = ro.random_kraus_batch(4, 3, 6)
    for b in range(6):
        _check_kraus(ks[b], key, b, 4, 3)


# ------------------------------------------------------------------------------------------------ ranks and shapes
@pytest.mark.parametrize("dim", DIMS)
def test_every_rank(ro, dim):
    """the element index of A is r * rank + j: every rank draws differently"""
    B, seed = 32, 5
    seen = []
    for rank in range(1, dim + 1):
        rho = ro.ginibre_state_matrix_batch(dim, rank, B, seed=seed, first_item=7)
        for b in range(B):
            _check_item("ginibre_state", rho[b], seed, 7 + b, dim, rank)
        assert np.abs(np.trace(rho, axis1=1, axis2=2) - 1).max() < 1e-14
        w = np.linalg.eigvalsh(rho)
        assert w.min() > -1e-14 and (np.sum(w > 1e-12, axis=1) == rank).all(), (dim, rank)
        seen.append(rho)
    assert all(not np.array_equal(a, b) for i, a in enumerate(seen) for b in seen[:i])


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 5), (64, 64), (3, 1000)])
def test_ginibre_shapes(ro, shape):
    B, seed, first = 5, 11, 3
    g = ro.ginibre_matrix_complex_batch(shape[0], shape[1], B, seed=seed, first_item=first)
    assert g.shape == (B,) + shape
    for b in range(B):
        assert rc.max_abs(g[b] - oa.ginibre_matrix(seed, first + b, *shape)) < 1e-13, (shape, b)


# ------------------------------------------------------------------------------------------------ Kraus counts
@pytest.mark.parametrize("K", [1, 5, 17, 64])
@pytest.mark.parametrize("dim", DIMS)
def test_kraus_counts(ro, dim, K):
    """K = 64 at d = 8 needs 71 776 bytes of LDS: the launch goes through the opt-in past 64 KiB"""
    B, seed, first = (3 if (dim, K) == (8, 64) else 64), 17, 100
    ks = ro.random_kraus_batch(dim, K, B, seed=seed, first_item=first)
    ratios = [_check_kraus(ks[b], seed, first + b, dim, K) for b in range(B)]
    mp_ratios = [_check_kraus(ks[b], seed, first + b, dim, K, ref=rc.mp_kraus_item(seed, first + b, dim, K)) for b in (0, B - 1)]
    print(f"RANDDEV device kraus d {dim} K {K:2d} worst err / tol: oracle {max(r[0] for r in ratios):.3f} "
          f"mpmath {max(r[0] for r in mp_ratios):.3f} TP {max(r[1] for r in ratios):.3f}")
    if (dim, K) == (8, 64):
        small = ro.random_kraus_batch(2, 1, B, seed=seed, first_item=first)
        for b in range(B):
            _check_kraus(small[b], seed, first + b, 2, 1)
        assert np.array_equal(ro.random_kraus_batch(dim, K, B, seed=seed, first_item=first), ks), "the second opt-in launch differs"
    # the Choi matrices the device converts these sets to, against the reference's own construction from the same entries
    choi = ro.rand_map_with_BCSZ_dist_batch(dim, K, B, seed=seed, first_item=first)
    worst = 0.0
    for b in range(B):
        gs = rc.ginibre(seed, first + b, dim, K)
        # a Choi entry is sum_j K_j[a, i] conj(K_j[b, l]); sum_j |K_j[a, i]| <= sqrt(K) since a column of the stacked K_j has norm
        # 1, so it moves by at most 2 sqrt(K) times the change of the Kraus entries; the reference's own route is given the
        # 64 u kappa_2(S) it has on the CPU
        tol = 2 * np.sqrt(K) * rc.kraus_tol(dim, rc.kappa_of(gs)) + 64 * rc.U * rc.kappa_of(gs)
        err = rc.max_abs(choi[b] - rc.reference_bcsz_choi(rc.bcsz_x(gs), dim))
        assert err <= tol, ("bcsz", dim, K, b, err, tol)
        assert rc.max_abs(choi[b] - so.kraus2choi(list(ks[b]))) <= 4 * (K + 4) * rc.U, "the conversion is not the Kraus sets'"
        worst = max(worst, err / tol)
    print(f"RANDDEV device bcsz  d {dim} K {K:2d} worst err / tol {worst:.3f}")


# ------------------------------------------------------------------------------------------------ ill-conditioned items
@pytest.mark.parametrize("dim", DIMS)
def test_ill_conditioned_items(ro, dim):
    """K = 1 on the worst-conditioned S of 20 000 items: kappa_2(S) = 1.5e5, 7.6e5, 4.4e6.  K_1 = G (G^H G)^{-1/2} is the unitary
    polar factor of G."""
    seed, item = rc.ILL[dim]
    kappa_s, kappa_g = rc.kappa_S(seed, item, dim, 1), rc.kappa_G(seed, item, dim)
    assert kappa_s > rc.ILL_KAPPA_MIN[dim]
    ks = ro.random_kraus_batch(dim, 1, 2, seed=seed, first_item=item - 1)[1]
    err_mp, tp = _check_kraus(ks, seed, item, dim, 1, ref=rc.mp_kraus_item(seed, item, dim, 1))
    _check_kraus(ks, seed, item, dim, 1)
    k1 = ks[0].astype(np.clongdouble)
    unit = rc.max_abs(k1 @ k1.conj().T - np.eye(dim))
    assert unit <= rc.kraus_tol(dim, kappa_s), (dim, unit)
    u = ro.haar_rand_unitary_batch(dim, 2, seed=seed, first_item=item - 1)[1]
    assert rc.max_abs(u.conj().T @ u - np.eye(dim)) < 1e-13
    err_q = rc.max_abs(u - rc.mp_q_item(seed, item, dim))
    assert err_q <= rc.q_tol(dim, kappa_g), (dim, err_q, rc.q_tol(dim, kappa_g))
    duk = dim * rc.U * kappa_s
    print(f"RANDDEV device ill d {dim} item {item} kappa_2(S) {kappa_s:.3g}: |K - K_mp| {err_mp * rc.kraus_tol(dim, kappa_s) / duk:.3f} "
          f"TP {tp * rc.kraus_tol(dim, kappa_s) / duk:.3f} K K^H - 1 {unit / duk:.3f} (x d u kappa_2(S), C_S = {rc.C_S}); "
          f"|U - Q_mp| {err_q / (dim * rc.U * kappa_g):.3f} (x d u kappa_2(G), C_Q = {rc.C_Q})")


# ------------------------------------------------------------------------------------------------ moments
@pytest.mark.parametrize("name", list(rc.MOMENTS))
def test_moments_at_dim_8(ro, name):
    """E tr rho^2 = (d + k) / (d k + 1) for ranks 1, 3, 8; (5 d^2 + 1) / (2 d (d^2 + 2)) for the Bures measure; E |tr U|^2 = 1
    and E |tr U^2|^2 = 2: within 5 standard errors at B = 20 000.  The seeds are those of random_cases.MOMENTS, fixed by the
    condition that the ORACLE's stream of the seed lies within 3.5 standard errors on its first 1500 items
    (tests/test_random_cpu.py); the device has no say in them."""
    seed, d, B = rc.MOMENTS[name][0], rc.MOMENT_DIM, rc.MOMENT_B_GPU
    if name == "purity_bures":
        mats = ro.bures_measure_state_matrix_batch(d, B, seed=seed)
    elif name.startswith("purity_rank"):
        mats = ro.ginibre_state_matrix_batch(d, int(name[len("purity_rank"):]), B, seed=seed)
    else:
        mats = ro.haar_rand_unitary_batch(d, B, seed=seed)
    rc.check_moment("device", name, mats, rc.MOMENT_DEVICE_SIGMA)


# ------------------------------------------------------------------------------------------------ refusals
SENTINEL = 0xA5


def _sentinel(n):
    return np.full(n, SENTINEL, dtype=np.uint8).view(np.float64)


def _refused(gpu, rc_code, out):
    assert rc_code == gpu.FBX_ERR_BAD_ARG, rc_code
    assert len(gpu.lib().fbx_last_error()) > 0
    assert (out.view(np.uint8) == SENTINEL).all()


def test_refusals(gpu):
    lib = gpu.lib()
    out = _sentinel(8 * 64 * 2 * 8)
    dev = gpu.DeviceBuffer(out.nbytes)

    def operators(kind, dim, cols, B=1, first=0):
        _refused(gpu, lib.fbx_random_operators(kind, dim, cols, B, 1, first, gpu.dptr(out)), out)
        _refused(gpu, lib.fbx_random_operators_dev(kind, dim, cols, B, 1, first, dev.ptr), out)

    def kraus(n, K, B=1, first=0):
        _refused(gpu, lib.fbx_random_kraus(n, B, K, 1, first, gpu.dptr(out)), out)
        _refused(gpu, lib.fbx_random_kraus_dev(n, B, K, 1, first, dev.ptr), out)

    for K in (0, 65, -1):
        kraus(2, K)
    for n in (0, 4):
        kraus(n, 2)
    kraus(2, 2, first=-1)
    kraus(2, 2, B=-1)
    per_item = (gpu.RAND_UNITARY, gpu.RAND_STATE_VECTOR, gpu.RAND_GINIBRE_STATE, gpu.RAND_BURES_STATE)
    for kind in per_item:
        for dim in (1, 3, 16, 0, -2):
            operators(kind, dim, 1)
        operators(kind, 4, 1, first=-1)
        operators(kind, 4, 1, B=-1)
    for dim in DIMS:
        operators(gpu.RAND_GINIBRE_STATE, dim, 0)
        operators(gpu.RAND_GINIBRE_STATE, dim, dim + 1)
        operators(gpu.RAND_GINIBRE_STATE, dim, -1)
    # Ginibre: dim * cols > 2^30 -- refused before anything is sized from the shape
    for dim, cols in ((2 ** 15 + 1, 2 ** 15), (2 ** 30 + 1, 1), (1, 2 ** 30 + 1), (2 ** 16, 2 ** 16), (0, 3), (3, 0), (-1, 3)):
        operators(gpu.RAND_GINIBRE, dim, cols)
    operators(gpu.RAND_GINIBRE, 2, 2, first=-1)
    operators(5, 2, 2)
    operators(-1, 2, 2)
    # B = 0 is fine for every kind and writes nothing
    for kind in (gpu.RAND_GINIBRE,) + per_item:
        assert lib.fbx_random_operators(kind, 4, 2, 0, 1, 0, gpu.dptr(out)) == gpu.FBX_OK
        assert lib.fbx_random_operators_dev(kind, 4, 2, 0, 1, 0, dev.ptr) == gpu.FBX_OK
    assert lib.fbx_random_kraus(2, 0, 3, 1, 0, gpu.dptr(out)) == gpu.FBX_OK
    assert lib.fbx_random_kraus_dev(2, 0, 3, 1, 0, dev.ptr) == gpu.FBX_OK
    assert (out.view(np.uint8) == SENTINEL).all()
    # the shim's own refusals
    from fbx.operator_tools import random_operators as ro
    for bad in (lambda: ro.random_kraus_batch(4, 65, 2), lambda: ro.random_kraus_batch(4, 0, 2), lambda: ro.random_kraus_batch(3, 2, 2),
                lambda: ro.haar_rand_unitary_batch(16, 2), lambda: ro.haar_rand_unitary_batch(4, 2, first_item=-1),
                lambda: ro.ginibre_state_matrix_batch(4, 0, 2), lambda: ro.ginibre_state_matrix_batch(4, 5, 2),
                lambda: ro.ginibre_matrix_complex_batch(2 ** 15 + 1, 2 ** 15, 0)):
        with pytest.raises(ValueError):
            bad()
    # the refusals left the generators as they were
    u = ro.haar_rand_unitary_batch(4, 2, seed=3)
    _check_item("unitary", u[1], 3, 1, 4)
    dev.free()
