"""The references of tests/random_cases.py without a GPU: the pinned ill-conditioned items are what they are said to be, the
float64 oracle lies where the constants say against mpmath, the Kraus form of the BCSZ ensemble is the reference's construction,
the oracle stream uses both words of the item id and of the seed, and the seeds of the moment tests are sound.

The oracle's measured constants (the `RANDDEV oracle` lines; numpy 2.2 with its bundled LAPACK):

  |K_oracle - K_mp| / (u kappa_2(S))   worst 1.83  (d = 2, item 13, K = 2: kappa_2(S) = 1.6)      ORACLE_C_S = 1.9
  |Q_oracle - Q_mp| / (u kappa_2(G))   worst 2.11  (d = 2, item 8: kappa_2(G) = 1.8)              ORACLE_C_Q = 2.2
  on the ILL items (kappa_2(S) = 1.5e5, 7.6e5, 4.4e6) the same ratios are 0.02 .. 0.5: the worst cases are well-conditioned
  items, where a few u of plain rounding are divided by a kappa near 1.

tests/test_random_exact_gpu.py allows the device 4 times these, times d.
"""
import numpy as np
import pytest

import random_cases as rc
from fbx_oracle import acquisition as oa, superops as so

DIMS = (2, 4, 8)
SEED = 17


def _items(dim):
    return [rc.ILL[dim][1]] + list(range(16))


def test_pinned_items_are_ill_conditioned():
    """recomputed, not trusted: kappa_2(S) of the ILL items from the singular values of G"""
    for dim, (seed, item) in rc.ILL.items():
        kappa = rc.kappa_S(seed, item, dim, 1)
        print(f"RANDDEV pinned d {dim} seed {seed} item {item} kappa_2(S) {kappa:.4g} kappa_2(G) {rc.kappa_G(seed, item, dim):.4g}")
        assert kappa > rc.ILL_KAPPA_MIN[dim]
        assert abs(rc.kappa_G(seed, item, dim) ** 2 / kappa - 1) < 1e-9          # K = 1: S = G^H G


def test_mpmath_references_are_what_they_claim():
    """Q is unitary with G = Q R, R upper triangular with a positive diagonal; sum K^H K = 1 and K_j = G_j W with one Hermitian
    positive W for all j -- in long double, to 2^-60"""
    for dim in DIMS:
        seed, item = rc.ILL[dim]
        g = rc.ginibre(seed, item, dim)[0].astype(np.clongdouble)
        q = rc.mp_q_item(seed, item, dim)
        r = q.conj().T @ g
        assert rc.max_abs(q.conj().T @ q - np.eye(dim)) < 2.0 ** -60
        assert rc.max_abs(np.tril(r, -1)) < 2.0 ** -58 * rc.max_abs(g) and (np.diagonal(r).real > 0).all()
        assert rc.max_abs(np.diagonal(r).imag) < 2.0 ** -58 * rc.max_abs(g)
        for K in (1, 3):
            gs = rc.ginibre(seed, item, dim, K)
            ks = rc.mp_kraus_item(seed, item, dim, K)
            assert rc.tp_defect(ks) < 2.0 ** -60
            w = np.linalg.solve(gs[0], ks[0].astype(np.complex128))              # W = G_0^{-1} K_0, to fp64 with kappa(G_0)
            tol = 64 * dim * rc.U * np.linalg.cond(gs[0]) * rc.max_abs(w)
            assert rc.max_abs(w - w.conj().T) < tol and np.linalg.eigvalsh((w + w.conj().T) / 2).min() > 0
            for j in range(K):
                assert rc.max_abs(gs[j] @ w - ks[j]) < tol * rc.max_abs(gs[j]) * dim


def test_oracle_against_mpmath_sets_the_constants():
    """the oracle's worst distances from mpmath in units of u kappa: printed, and at or below ORACLE_C_S / ORACLE_C_Q"""
    worst_s, worst_q, worst_tp = (0.0, None), (0.0, None), (0.0, None)
    for dim in DIMS:
        for item in _items(dim):
            for K in (1, dim):
                kappa = rc.kappa_S(SEED, item, dim, K)
                ko = oa.random_kraus(SEED, item, dim, K)
                r = rc.max_abs(ko - rc.mp_kraus_item(SEED, item, dim, K)) / (rc.U * kappa)
                worst_s = max(worst_s, (r, (dim, item, K, kappa)))
                worst_tp = max(worst_tp, (rc.tp_defect(ko) / (rc.U * kappa), (dim, item, K, kappa)))
                if item == rc.ILL[dim][1] and K == 1:
                    print(f"RANDDEV oracle ill d {dim} item {item} kappa_2(S) {kappa:.3g} |K - K_mp| / (u kappa) {r:.3f} "
                          f"TP defect {rc.tp_defect(ko):.2e} = {rc.tp_defect(ko) / (rc.U * kappa):.3f} u kappa")
            kg = rc.kappa_G(SEED, item, dim)
            r = rc.max_abs(oa.haar_unitary(SEED, item, dim) - rc.mp_q_item(SEED, item, dim)) / (rc.U * kg)
            worst_q = max(worst_q, (r, (dim, item, kg)))
    print(f"RANDDEV oracle c_S {worst_s[0]:.3f} at (d, item, K, kappa_2(S)) = {worst_s[1]}")
    print(f"RANDDEV oracle c_Q {worst_q[0]:.3f} at (d, item, kappa_2(G)) = {worst_q[1]}")
    print(f"RANDDEV oracle TP defect / (u kappa_2(S)) {worst_tp[0]:.3f} at {worst_tp[1]}")
    assert worst_s[0] <= rc.ORACLE_C_S and worst_q[0] <= rc.ORACLE_C_Q
    # the device's allowance holds the oracle's own TP defect too: the bound is attainable without the code under test
    for dim in DIMS:
        for item in _items(dim):
            for K in (1, dim):
                assert rc.tp_defect(oa.random_kraus(SEED, item, dim, K)) <= rc.kraus_tol(dim, rc.kappa_S(SEED, item, dim, K))


@pytest.mark.parametrize("dim", DIMS)
def test_kraus_form_is_the_references_bcsz_construction(dim):
    """kraus2choi(K_j = G_j S^{-1/2}) = (red^{-1/2} (x) 1) X X^H (red^{-1/2} (x) 1) for X[:, j] = vec(G_j), to 64 u kappa_2(S)"""
    for K in (1, 3, dim * dim):
        for item in (0, 1, rc.ILL[dim][1]):
            gs = rc.ginibre(SEED, item, dim, K)
            kappa = rc.kappa_of(gs)
            got = so.kraus2choi(list(oa.random_kraus(SEED, item, dim, K)))
            want = rc.reference_bcsz_choi(rc.bcsz_x(gs), dim)
            err = rc.max_abs(got - want)
            print(f"RANDDEV oracle bcsz d {dim} K {K} item {item} kappa_2(S) {kappa:.3g} err / (64 u kappa) {err / (64 * rc.U * kappa):.3f}")
            assert err <= 64 * rc.U * kappa, (dim, K, item, err)
            # and what makes it a channel: trace over the output index is the identity
            pt = np.einsum("iaja->ij", want.reshape(dim, dim, dim, dim))
            assert rc.max_abs(pt - np.eye(dim)) <= 64 * rc.U * kappa


def test_oracle_stream_uses_the_high_words():
    assert not np.array_equal(oa.ginibre_entries(11, 2 ** 32, 8), oa.ginibre_entries(11, 0, 8))
    assert not np.array_equal(oa.ginibre_entries(11 + 2 ** 32, 0, 8), oa.ginibre_entries(11, 0, 8))
    # item 2^32 + 5 of seed 2^32 + 11, counter and key written out: (item low, item high, element, tag), (seed low, seed high)
    n = 6
    ctr = np.array([[5, 1, e, 0] for e in range(n)], dtype=np.uint32)
    key = np.array([[11, 1]] * n, dtype=np.uint32)
    x = oa.philox4x32_10(ctr, key).astype(np.float64)
    u1, u2 = (x[:, 0] + 0.5) * 2.0 ** -32, (x[:, 1] + 0.5) * 2.0 ** -32
    want = np.sqrt(-2.0 * np.log(u1)) * np.exp(1j * 6.283185307179586476925 * u2)
    got = oa.ginibre_entries(2 ** 32 + 11, 2 ** 32 + 5, n)
    assert np.abs(got - want).max() < 1e-14
    # Philox4x32-10 itself, on the known-answer vectors of the Random123 distribution (kat_vectors)
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for c, k, out in kat:
        got = oa.philox4x32_10(np.array([c], dtype=np.uint32), np.array([k], dtype=np.uint32))[0]
        assert tuple(int(v) for v in got) == out


@pytest.mark.parametrize("name", list(rc.MOMENTS))
def test_moment_seeds_are_sound_on_the_oracle_stream(name):
    """the condition the seeds of the GPU moment tests were chosen by: the oracle's first MOMENT_B_CPU items of that seed lie
    within 3.5 standard errors of the expected value"""
    seed = rc.MOMENTS[name][0]
    sigma = rc.check_moment("oracle", name, rc.oracle_moment_batch(name, seed, rc.MOMENT_B_CPU), rc.MOMENT_ORACLE_SIGMA)
    assert name in rc.DETERMINISTIC_MOMENTS or abs(sigma) <= rc.MOMENT_ORACLE_SIGMA


def test_moment_sigma():
    x = np.array([1.0, 2.0, 3.0, 4.0])
    assert abs(rc.moment_sigma(x, 2.0) - 0.5 / (np.sqrt(5.0 / 3.0) / 2.0)) < 1e-15
    assert rc.moment_sigma(np.ones(5), 1.0) == 0.0 and rc.moment_sigma(np.ones(5), 2.0) == -np.inf
    # a batch that repeats every other item (a stride loop that wrote one stream twice) keeps each moment but is caught exactly;
    # a batch of the WRONG ensemble is what the moments catch: rank 2 in place of rank 3 is 30 standard errors off at n = 1500
    wrong = np.array([oa.ginibre_state(31, b, rc.MOMENT_DIM, 2) for b in range(rc.MOMENT_B_CPU)])
    assert abs(rc.moment_sigma(rc.purity(wrong), rc.MOMENTS["purity_rank3"][1])) > 30
