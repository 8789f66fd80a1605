"""What tests/test_state_dispatch_gpu.py and tests/test_state_measures_small_gpu.py rely on, checked with the oracle alone (no
device): the designs of tests/state_cases.py have the sizes that place the dispatch, every design and mode gives a finite
estimate, the converge mode stops where a comparison of iteration counts means something, and the oracle's own errors that serve
as yardsticks (fidelity on exact families, the spread of an estimate when the list of results is permuted).

Converge mode (state_cases.CONVERGE): maxiter 2000 and (epsilon, tol) = (0.5, 1e-6) / (1.0, 1e-4) / (0.5, 1e-3) for 1 / 2 / 3
qubits (with epsilon 0.5 and tol 1e-6 the oracle needs some 900 iterations at two qubits and does not finish in 2000 at three).
Iteration counts of the oracle per row, unit then signed coefficients:

    row (n, design, B)      unit                                  signed
    1 with_identity 5       38 52 39 33 45                        121 147 187 149 185
    2 with_identity 5       50 88 56 49 42                        90 144 116 189 146
    1 standard 33           25 .. 39                              90 .. 138
    2 standard 9            46 91 61 54 49 51 38 58 41            150 141 109 153 101 167 142 208 100
    1 d_plus_1 4            48 46 45 32                           31 49 49 41
    2 d_plus_1 4            53 78 47 58                           95 207 151 108
    1 twice 4               31 32 22 34                           100 158 105 101
    2 twice 4               33 55 60 78                           87 144 86 136
    1 sixty_four 4          33 38 25 26                           29 40 42 51
    2 sixty_four 4          30 81 35 92                           48 106 69 67
    3 standard 3            30 85 61                              45 101 1
    3 with_identity 3       18 90 52                              19 100 2

Largest change of the oracle's plain estimate (maxiter 40) when the results are listed in another order, per design with
repeated observables, three orders each: 1.1e-16 to 3.4e-16 for every one of them (1-2 qubits twice, d_plus_1, sixty_four,
sixty_five; 3 qubits twice).  No bound of tests/test_state_dispatch_gpu.py is widened by it.

Oracle fidelity errors on the exact families (12 pairs, either argument order): at most 4e-15 for commuting, identical and
orthogonal pairs, 1e-8 to 3e-8 for pure_pure, pure_mixed and rank_deficient (the square root of a zero eigenvalue's rounding)."""
import warnings

import numpy as np
import pytest

import state_cases as sc
import state_measure_cases as smc
from fbx_oracle import estimators as oe

SIGNED = pytest.mark.parametrize("signed", [False, True], ids=["unit", "signed"])


def oracle_mle(des, e, c, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return oe.iterative_mle_state_estimate(des, e, c, return_stats=True, **kw)


def test_design_sizes_sit_on_the_switches():
    sizes = {(n, kind): len(sc.design_variant(n, kind)[0]) for n in (1, 2, 3) for kind in sc.KINDS[n]}
    assert [sizes[n, "standard"] for n in (1, 2, 3)] == [3, 15, 63]
    assert [sizes[n, "with_identity"] for n in (1, 2, 3)] == [4, 16, 64]               # m = D at n = 1, 2; m = 64 at n = 3
    assert [sizes[n, "twice"] for n in (1, 2, 3)] == [6, 30, 126]
    assert [sizes[n, "d_plus_1"] for n in (1, 2)] == [5, 17]                           # m = D + 1
    assert [sizes[n, "sixty_four"] for n in (1, 2)] == [64, 64] and [sizes[n, "sixty_five"] for n in (1, 2)] == [65, 65]
    for n in (1, 2, 3):
        for kind in sc.KINDS[n]:
            p, cf = sc.design_variant(n, kind)
            assert np.all(cf == 1.0) and p.dtype == np.uint8 and p.shape == (sizes[n, kind], n)
            assert (p.max(axis=1) == 0).sum() == (kind == "with_identity")             # the identity, once, there only
            p2, cf2 = sc.design_variant(n, kind, signed=True)
            assert np.array_equal(p, p2) and set(np.abs(cf2)) <= {0.5, 1.0} and (cf2 < 0).any() and (np.abs(cf2) == 0.5).any()
            if kind == "with_identity":
                assert not p[0].any() and cf2[0] == -0.5
            e, c = sc.data(n, p2, cf2, 4, 3)
            assert np.all(np.abs(e) <= np.abs(cf2)) and np.all(c == 500)
            assert np.array_equal(sc.data(n, p2, cf2, 2, 3)[0], e[:2])                 # a smaller batch is a prefix


@pytest.mark.parametrize("n", [1, 2, 3])
@SIGNED
def test_every_design_and_fixed_length_mode_is_finite(n, signed):
    """plain (maxiter 40), hedged and max-entropy (maxiter 12) on two items, a quiet and a noisy one; the converge mode has
    test_converge_mode_stops_where_counts_can_be_compared"""
    for kind in sc.KINDS[n]:
        p, cf, e, c = sc.case(n, kind, signed, 2)
        des = sc.oracle_design(n, p, cf)
        for mode in ("plain", "hedged", "maxent"):
            for b in range(2):
                rho, st = oracle_mle(des, e[b], c[b], **sc.mode_kwargs(mode, n, len(p)))
                assert np.isfinite(rho).all() and st["hit_max"], (n, kind, mode, b)
                assert abs(np.trace(rho) - 1) < 1e-12


CONVERGE_ROWS = [(n, kind, B) for n, kind, B, modes in sc.ROWS if "converge" in modes]


@pytest.mark.parametrize("n,kind,B", CONVERGE_ROWS)
@SIGNED
def test_converge_mode_stops_where_counts_can_be_compared(n, kind, B, signed):
    """every item stops before maxiter; within the batch the counts differ by a factor of 1.5 at least; and no item's last step
    lies within 1 % of tol, where rounding would decide whether it is the last"""
    p, cf, e, c = sc.case(n, kind, signed, B)
    des = sc.oracle_design(n, p, cf)
    kw = sc.mode_kwargs("converge", n, len(p))
    counts = []
    for b in range(B):
        rho, st = oracle_mle(des, e[b], c[b], **kw)
        k = st["iterations"]
        assert np.isfinite(rho).all() and not st["hit_max"] and k < kw["maxiter"], (b, k)
        before, _ = oracle_mle(des, e[b], c[b], **dict(kw, maxiter=k))                   # k - 1 updates: the state before the last
        step = np.linalg.norm(rho - before, "fro")
        assert step < 0.99 * kw["tol"], (b, k, step)
        counts.append(k)
    print(f"oracle iterations, {n} qubits, {kind}, {'signed' if signed else 'unit'}: {counts}")
    assert max(counts) >= 1.5 * min(counts), counts
    assert max(counts) <= (1500 if n == 1 else 700), counts


@pytest.mark.parametrize("n,kind", [(n, kind) for n in (1, 2, 3) for kind in sc.KINDS[n] if kind not in ("standard", "with_identity")])
def test_permutation_spread_of_the_oracle(n, kind):
    """designs with repeated observables: the device adds the repeats of a Pauli operator in another order than the reference's
    loop over the list, so the oracle's own sensitivity to the order is the scale of an honest difference"""
    p, cf, e, c = sc.case(n, kind, True, 2)
    kw = sc.mode_kwargs("plain", n, len(p))
    base = [oracle_mle(sc.oracle_design(n, p, cf), e[b], c[b], **kw)[0] for b in range(2)]
    spread = 0.0
    for seed in range(3):
        p2, cf2, e2, c2 = sc.permuted(p, cf, e, c, seed)
        des = sc.oracle_design(n, p2, cf2)
        for b in range(2):
            spread = max(spread, np.abs(oracle_mle(des, e2[b], c2[b], **kw)[0] - base[b]).max())
    print(f"permutation spread of the oracle, {n} qubits, {kind}: {spread:.3e}")
    assert spread < 1e-12


@pytest.mark.parametrize("nq", [1, 2, 3])
@pytest.mark.parametrize("name", sorted(smc.FAMILIES))
def test_oracle_fidelity_error_on_exact_families(name, nq):
    """every family is defined from one qubit on, and the oracle's error is the yardstick of the kernel's"""
    from fbx_oracle import measures as om
    rho, sigma, exact = smc.family(name, nq, 12)
    sums = smc.host_sums(rho, sigma)
    for key in ("purity", "hs_ip"):
        if key in exact:
            assert np.abs(sums[key] - exact[key]).max() < 1e-13
    worst = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for b in range(12):
            assert abs(np.trace(rho[b]) - 1) < 1e-13 and abs(np.trace(sigma[b]) - 1) < 1e-13
            assert np.linalg.eigvalsh(rho[b]).min() > -1e-15 and np.linalg.eigvalsh(sigma[b]).min() > -1e-15
            for a, s in ((rho[b], sigma[b]), (sigma[b], rho[b])):
                worst = max(worst, abs(np.real(om.fidelity(a, s)) - exact["fidelity"][b]))
    print(f"oracle fidelity error, {name}, {nq} qubits: {worst:.3e}")
    assert worst < (1e-13 if name in ("commuting", "identical", "orthogonal") else 1e-6)


def test_rank_deficient_is_unchanged_from_two_qubits_on():
    """the one-qubit form must not move the generator's stream for d >= 4"""
    rng = np.random.default_rng(5)
    rho, sigma, exact = smc.rank_deficient(4, rng)
    assert np.linalg.matrix_rank(rho, tol=1e-12) == 3 and np.linalg.matrix_rank(sigma, tol=1e-12) == 3
    rho1, sigma1, exact1 = smc.rank_deficient(2, np.random.default_rng(5))
    assert np.linalg.matrix_rank(rho1, tol=1e-12) == 1 and np.linalg.matrix_rank(sigma1, tol=1e-12) == 2
    assert abs(exact1["fidelity"] - np.real(np.trace(rho1 @ sigma1))) < 1e-14
