"""Every branch of the dispatch in fbx_mle_state_dev (csrc/fbx_state.hip), item by item against the oracle on the same list of
results, with unit coefficients and with coefficients from {1, -1, 0.5, -0.5}; and fbx_linv_state, fbx_r_operator and
fbx_state_log_likelihood on the same designs.  The designs and data are those of tests/state_cases.py, whose conditions
tests/test_state_cases_cpu.py checks with the oracle alone.

With D = 4^n, m settings, and "plain" for no entropy penalty and no hedging, the dispatch reads

    n >= 4                                   mle_state_big_kernel<n>
    packed = plain && n <= 2 && m <= D       mle_state_packed_kernel<n>      16 / 4 items per wavefront
    n == 3 && plain && m <= 64               mle_state_plain3_kernel
    otherwise                                mle_state_kernel<n>             m <= 64: r_operator_resident (a setting per lane),
                                                                             m > 64: r_operator_strided (staged in LDS)

and the tests reach

    test                                        n, design (m)                                        kernel
    test_packed_at_m_equal_D                    1, 2 with_identity (4, 16 = D)                       mle_state_packed_kernel<1, 2>
    test_packed_partial_and_full_waves          1, 2 standard (3, 15), B around 16 / 4 per wave      mle_state_packed_kernel<1, 2>
    test_one_setting_per_lane                   1, 2 d_plus_1 (D + 1), twice (6, 30), sixty_four     mle_state_kernel<1, 2>, r_operator_resident
    test_first_staged_design                    1, 2 sixty_five (65)                                 mle_state_kernel<1, 2>, r_operator_strided
    test_three_qubit_variants                   3 standard (63), with_identity (64), hedged/maxent   mle_state_kernel<3>, r_operator_resident
    test_three_qubit_plain                      3 standard (63), with_identity (64)                  mle_state_plain3_kernel
    test_four_qubit_coefficients                4 standard (255), signed                             mle_state_big_kernel<4>
    test_linear_inversion_r_and_likelihood      every design above, and 3 twice (126)                linv_state_kernel, r_operator_kernel,
                                                                                                     loglik_kernel, state_big_kernel<4>

Bounds are the ones the suite already holds these kernels to: 1e-11 for plain runs of a fixed length, 1e-10 hedged and
max-entropy, 1e-9 converged with the oracle's iteration count, 1e-12 linear inversion, 1e-10 the R operator, 1e-9 relative the
log-likelihood.  None is widened: on an MI355X the largest difference from the oracle over all rows is 9.4e-16 in plain, 6.7e-16 in
converged, 3.1e-16 in hedged and 3.6e-16 in max-entropy runs, and every iteration count is the oracle's; the oracle itself moves
by 1e-16 to 3e-16 when a list with repeated observables is permuted (tests/test_state_cases_cpu.py)."""
import functools
import warnings

import numpy as np
import pytest

import state_cases as sc
import state_measure_cases as smc

pytestmark = pytest.mark.gpu

SIGNED = pytest.mark.parametrize("signed", [False, True], ids=["unit", "signed"])
ROW_B = {(n, kind): B for n, kind, B, _ in sc.ROWS}


@functools.lru_cache(maxsize=None)
def oracle_estimates(n, kind, signed, B, mode, maxiter=None):
    """[(rho, stats)] per item; computed once per case"""
    from fbx_oracle import estimators as oe
    p, cf, e, c = sc.case(n, kind, signed, B)
    des = sc.oracle_design(n, p, cf)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return [oe.iterative_mle_state_estimate(des, e[b], c[b], return_stats=True, **sc.mode_kwargs(mode, n, len(p), maxiter))
                for b in range(B)]


def device_estimates(n, kind, signed, B, mode, maxiter=None, items=None):
    from fbx import tomography as T
    p, cf, e, c = sc.case(n, kind, signed, B)
    if items is not None:
        e, c = e[items], c[items]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return T.iterative_mle_state_estimate_batch(sc.device_design(n, p, cf), e, c, return_stats=True,
                                                    **sc.mode_kwargs(mode, n, len(p), maxiter))


def against_the_oracle(n, kind, signed, B, mode, maxiter=None, take=None):
    """the first `take` items of the case (all of them by default) on the device, each against the oracle"""
    take = B if take is None else take
    got, st = device_estimates(n, kind, signed, B, mode, maxiter, items=slice(0, take))
    want = oracle_estimates(n, kind, signed, B, mode, maxiter)
    worst = 0.0
    for b in range(take):
        rho, wst = want[b]
        err = np.abs(got[b] - rho).max()
        worst = max(worst, err)
        assert err < sc.MLE_BOUND[mode], (n, kind, signed, mode, b, err)
        assert st["iterations"][b] == wst["iterations"] and bool(st["hit_max"][b]) == wst["hit_max"], (n, kind, mode, b)
        assert wst["hit_max"] == (mode != "converge")
    print(f"{n} qubits, {kind}, {'signed' if signed else 'unit'}, {mode}: largest error {worst:.2e} of {sc.MLE_BOUND[mode]:.0e}")
    return got, st


# ------------------------------------------------------------------------------------------------ several items per wavefront
@pytest.mark.parametrize("mode", ["plain", "converge"])
@pytest.mark.parametrize("n", [1, 2])
@SIGNED
def test_packed_at_m_equal_D(gpu, n, signed, mode):
    """the all-identity observable makes m = D, the last design the packed kernel takes: lane t = D - 1 of a group holds a setting"""
    against_the_oracle(n, "with_identity", signed, ROW_B[n, "with_identity"], mode)


@pytest.mark.parametrize("n,sizes", [(1, (1, 15, 16, 17, 33)), (2, (1, 3, 4, 5, 9))])
@SIGNED
def test_packed_partial_and_full_waves(gpu, n, sizes, signed):
    """16 / 4 items share a wavefront and the groups that have converged idle until the last one has: batches that end inside a
    wavefront, fill one exactly and spill one item into the next, of items that stop at very different iterations -- each
    against the oracle, and bit for bit (iteration counts included) what it is when it runs alone"""
    B = ROW_B[n, "standard"]
    assert max(sizes) == B
    alone = [device_estimates(n, "standard", signed, B, "converge", items=slice(b, b + 1)) for b in range(B)]
    for size in sizes:
        got, st = against_the_oracle(n, "standard", signed, B, "converge", take=size)
        assert got.shape[0] == size
        for b in range(size):
            assert np.array_equal(got[b], alone[b][0][0]), (n, size, b)
            assert st["iterations"][b] == alone[b][1]["iterations"][0] and st["hit_max"][b] == alone[b][1]["hit_max"][0]
    # a wavefront in reverse order: every item in another group of lanes, next to other neighbours
    got, st = device_estimates(n, "standard", signed, B, "converge", items=slice(None, None, -1))
    for b in range(B):
        assert np.array_equal(got[B - 1 - b], alone[b][0][0]) and st["iterations"][B - 1 - b] == alone[b][1]["iterations"][0]


# ------------------------------------------------------------------------------------------------ one wavefront per item
@pytest.mark.parametrize("mode", ["plain", "converge"])
@pytest.mark.parametrize("kind", ["d_plus_1", "twice", "sixty_four"])
@pytest.mark.parametrize("n", [1, 2])
@SIGNED
def test_one_setting_per_lane(gpu, n, kind, signed, mode):
    """D < m <= 64 without variants: mle_state_kernel<1, 2> with the settings in registers (r_operator_resident); several lanes add
    to the weight of the same Pauli operator"""
    against_the_oracle(n, kind, signed, ROW_B[n, kind], mode)


@pytest.mark.parametrize("n", [1, 2])
@SIGNED
def test_first_staged_design(gpu, n, signed):
    """m = 65: the first design whose settings no longer fit the lanes (r_operator_strided, staged in LDS)"""
    against_the_oracle(n, "sixty_five", signed, ROW_B[n, "sixty_five"], "plain")


@pytest.mark.parametrize("mode", ["hedged", "maxent"])
@pytest.mark.parametrize("kind", ["standard", "with_identity"])
@SIGNED
def test_three_qubit_variants(gpu, kind, signed, mode):
    """hedging and the entropy penalty at 3 qubits with at most 64 settings: mle_state_kernel<3> on r_operator_resident with
    PauliTables<3>, which nothing else launches; with_identity fills all 64 lanes"""
    against_the_oracle(3, kind, signed, ROW_B[3, kind], mode)


@pytest.mark.parametrize("mode", ["plain", "converge"])
@pytest.mark.parametrize("kind", ["standard", "with_identity"])
@SIGNED
def test_three_qubit_plain(gpu, kind, signed, mode):
    """mle_state_plain3_kernel, also run until tol is reached, with the oracle's iteration counts"""
    against_the_oracle(3, kind, signed, ROW_B[3, kind], mode)


@pytest.mark.parametrize("mode,maxiter", [("plain", 10), ("hedged", 6)])
def test_four_qubit_coefficients(gpu, mode, maxiter):
    """the coefficient branch of r_operator_strided over a workgroup"""
    against_the_oracle(4, "standard", True, ROW_B[4, "standard"], mode, maxiter)


# ------------------------------------------------------------------------------------------------ the other entry points
DESIGNS = sorted(set((n, kind) for n, kind, _, _ in sc.ROWS) | {(3, "twice")})


@pytest.mark.parametrize("n,kind", DESIGNS)
@SIGNED
def test_linear_inversion_r_and_likelihood(gpu, n, kind, signed):
    """linv_state_kernel, r_operator_kernel and loglik_kernel (state_big_kernel at 4 qubits) with coefficients, repeated
    observables and the identity among them.  The identity's row gives the reference's linear inversion a second multiple of
    I / d next to the one it always adds: the kernel has to reproduce that."""
    from fbx import tomography as T
    from fbx_oracle import estimators as oe
    B = 3
    p, cf, e, c = sc.case(n, kind, signed, B)
    dev, ora = sc.device_design(n, p, cf), sc.oracle_design(n, p, cf)
    got = T.linear_inv_state_estimate_batch(dev, e)
    for b in range(B):
        assert np.abs(got[b] - oe.linear_inv_state_estimate(ora, e[b])).max() < 1e-12, b
    states = smc.full_rank_pairs(n, B, 97)[0]
    r = T._R_batch(states, dev, e)
    ll = T.state_log_likelihood_batch(states, dev, e, c)
    for b in range(B):
        assert np.abs(r[b] - oe.R_operator(states[b], ora, e[b])).max() < 1e-10, b
        want = oe.state_log_likelihood(states[b], ora, e[b], c[b])
        assert abs(ll[b] - want) < 1e-9 * abs(want), (b, ll[b], want)
