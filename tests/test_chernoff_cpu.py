"""The exact constructors of tests/chernoff_cases.py and the mpmath brackets of tests/golden/chernoff_exact.npz, checked on the host
(numpy / mpmath only, no GPU)."""
import os

import mpmath as mp
import numpy as np
import pytest

import chernoff_cases as cc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chernoff_exact.npz")


def host_q(rho, sigma, s, zero_tol=1e-12):
    """Q(s) in float64 with numpy's eigh and the support rule of the device"""
    a, v = np.linalg.eigh(rho)
    b, w = np.linalg.eigh(sigma)
    ka = (a > 0) & (a > zero_tol * a.max())
    kb = (b > 0) & (b > zero_tol * b.max())
    o = np.abs(v.conj().T @ w) ** 2
    fa = np.where(ka, np.abs(a), 1.0) ** s * ka
    fb = np.where(kb, np.abs(b), 1.0) ** (1 - s) * kb
    return float(fa @ o @ fb)


@pytest.mark.parametrize("nq", [1, 2, 3])
@pytest.mark.parametrize("name", sorted(cc.FAMILIES))
def test_constructors_are_states_with_their_value(name, nq):
    rho, sigma, exact = cc.family(name, nq, 4)
    for b in range(4):
        for x in (rho[b], sigma[b]):
            assert np.abs(x - x.conj().T).max() <= 1e-15
            assert abs(np.trace(x) - 1) <= 1e-14
            assert np.linalg.eigvalsh(x).min() >= -1e-15
        grid = np.linspace(0, 1, 201)
        qs = np.array([host_q(rho[b], sigma[b], s) for s in grid])
        assert qs.min() >= exact[b] - 1e-12                          # nothing on a grid beats the exact minimum
        assert qs.min() <= exact[b] + 1e-3                           # and the grid gets near it


def test_commuting_minimum_is_stationary():
    rng = np.random.default_rng(5)
    a, b = cc.random_spectrum(4, rng), cc.random_spectrum(4, rng)
    value, s = cc.commuting_min(a, b)
    with mp.workdps(40):
        dq = mp.fsum(mp.mpf(x) ** s * mp.mpf(y) ** (1 - s) * (mp.log(x) - mp.log(y)) for x, y in zip(a, b))
        assert abs(dq) < mp.mpf(10) ** -30
        assert 0 < s < 1


def test_goldens_bracket_the_float64_objective():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) <= 300 * 1024
    total = 0
    for nq in (1, 2, 3, 4, 5):
        lo, hi, s = g[f"q{nq}_lo"], g[f"q{nq}_hi"], g[f"q{nq}_s"]
        rho, sigma = g[f"q{nq}_rho"], g[f"q{nq}_sigma"]
        assert rho.shape[1:] == (2 ** nq, 2 ** nq) and len(lo) >= 3
        assert set(g[f"q{nq}_family"]) == {"full", "lowrank", "near"}
        assert np.all(lo < hi) and np.all(hi - lo <= 5e-16 * hi)
        for b in range(len(lo)):
            q = host_q(rho[b], sigma[b], s[b])                       # float64 at the mpmath argmin
            assert abs(q - lo[b]) <= 1e-12 * hi[b], (nq, b, q, lo[b])
        total += len(lo)
    assert total >= 30


def test_golden_bracket_recomputes():
    """one pair per size up to three qubits recomputed in mpmath lands in its stored bracket"""
    g = np.load(GOLDEN)
    for nq in (1, 2, 3):
        value, _ = cc.mp_chernoff(g[f"q{nq}_rho"][0], g[f"q{nq}_sigma"][0], dps=40)
        assert mp.mpf(g[f"q{nq}_lo"][0]) <= value <= mp.mpf(g[f"q{nq}_hi"][0])
