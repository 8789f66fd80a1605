"""The closed forms of tests/diamond_cases.py and the brackets of tests/golden/diamond_exact.npz on the host: the constructors
give the channels they claim, the host solver (distance_measures.diamond_norm_distance, the comparator of
tests/test_diamond_gpu.py) reproduces the closed forms, and every golden bracket contains its closed form."""
import os

import numpy as np
import pytest

import diamond_cases as dc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diamond_exact.npz")


def ptrace_out(choi, d):
    """Tr over the output (second) factor: sum_K K^T conj(K) in this convention; the identity for a trace-preserving map."""
    return np.einsum("iaja->ij", choi.reshape(d, d, d, d))


def is_cp(choi, atol=1e-12):
    return np.linalg.eigvalsh((choi + choi.conj().T) / 2).min() >= -atol and np.abs(choi - choi.conj().T).max() <= atol


@pytest.mark.parametrize("nq", [1, 2, 3])
def test_constructors_are_channels(nq):
    d = 2 ** nq
    fam = dc.families(nq)
    for name, cases in fam.items():
        for c0, c1, exact in cases:
            assert c0.shape == c1.shape == (d * d, d * d)
            assert np.isfinite(exact) and exact >= 0
            for c in (c0, c1):
                assert is_cp(c), name
                assert np.allclose(ptrace_out(c, d), np.eye(d), atol=1e-12), name
    # a unitary's Choi matrix is rank 1, a Pauli channel's is diagonal in the Bell-Pauli basis with its probabilities
    u0, _, _ = fam["unitary"][0]
    assert np.linalg.matrix_rank(u0, tol=1e-10) == 1
    p = dc.random_pauli_probs(nq, np.random.RandomState(3))
    vecs = np.array([P.reshape(-1, order="F") for P in dc.paulis(nq)]) / np.sqrt(d)
    c = dc.pauli_channel_choi(p)
    assert np.allclose(vecs.conj() @ c @ vecs.T, np.diag(p) * d, atol=1e-12)
    # the replacement channel's Choi matrix is kron(1, sigma): it sends every input state to sigma
    sigma = dc.random_state(d, np.random.RandomState(4))
    c0, _, _ = dc.replacement_pair(sigma, sigma)
    rho = dc.random_state(d, np.random.RandomState(5))
    out = np.einsum("iajb,ij->ab", c0.reshape(d, d, d, d), rho)      # Phi(rho) = Tr_in[(rho^T (x) 1) J]
    assert np.allclose(out, sigma, atol=1e-14)


def test_closed_form_identities():
    """Two families give the same value by different routes; the unitary formula at its edges."""
    for d in (2, 4, 8):
        for p in (1e-6, 0.3):
            c0, c1, exact = dc.depolarizing_pair(d, p)
            probs = np.full(d * d, p / (d * d))
            probs[0] += 1 - p
            assert abs(dc.pauli_pair(probs, np.eye(d * d)[0])[2] - exact) <= 1e-15 * max(exact, 1)
        assert dc.unitary_one_phase(d, 1e-8)[2] == pytest.approx(1e-8, rel=1e-14)
        assert dc.unitary_one_phase(d, -0.5)[2] == pytest.approx(2 * np.sin(0.25), rel=1e-14)
        assert dc.unitary_wide(d, np.random.RandomState(d))[2] == 2.0
        assert dc.unitary_pair(np.eye(d), np.eye(d))[2] == 0.0


@pytest.mark.parametrize("nq", [1, 2])
def test_host_solver_against_closed_forms(nq):
    from fbx import distance_measures as dm
    for name, cases in dc.families(nq).items():
        for c0, c1, exact in cases:
            got = dm.diamond_norm_distance(c0, c1)
            assert abs(got - exact) <= 1e-9 * max(exact, 1e-6), (name, got, exact)


def test_replacement_is_not_symmetric():
    """The quantity puts the input state on the second factor: for replacement channels it is 2 d lambda_max(sigma - tau), which
    differs between the two orders and exceeds 2."""
    from fbx import distance_measures as dm
    rs = np.random.RandomState(9)                            # (at d = 2, sigma - tau is traceless with two eigenvalues: symmetric)
    sigma, tau = dc.random_state(4, rs, rank=1), dc.random_state(4, rs)
    ab = dc.replacement_pair(sigma, tau)
    ba = dc.replacement_pair(tau, sigma)
    assert abs(dm.diamond_norm_distance(ab[0], ab[1]) - ab[2]) <= 1e-9 * ab[2]
    assert abs(dm.diamond_norm_distance(ba[0], ba[1]) - ba[2]) <= 1e-9 * ba[2]
    assert abs(ab[2] - ba[2]) > 1e-3 and max(ab[2], ba[2]) > 2


def test_golden_brackets_hold():
    g = np.load(GOLDEN)
    families = set()
    for nq in (1, 2, 3):
        p = f"q{nq}_"
        d = 2 ** nq
        L, U, width, exact = g[p + "lower"], g[p + "upper"], g[p + "width"], g[p + "exact"]
        names = g[p + "family"]
        c0, c1, T = g[p + "choi0"], g[p + "choi1"], g[p + "T"]
        assert len(L) >= (4 if nq == 3 else 12), nq
        assert c0.shape == c1.shape == (len(L), d * d, d * d) and T.shape == (len(L), d, d)
        assert np.all(L <= U) and np.all(width <= 1e-10) and np.all(np.abs((U - L) - width * U) <= 1e-15 * U + 1e-30)
        known = np.isfinite(exact)
        assert known.sum() >= 2 and (~known).sum() >= 2, nq
        # the closed form lies inside its bracket (to the rounding of the float64 inputs)
        assert np.all(L[known] <= exact[known] * (1 + 1e-13) + 1e-15), nq
        assert np.all(U[known] >= exact[known] * (1 - 1e-13) - 1e-15), nq
        for name, a, b in zip(names, c0, c1):                # completely positive maps (non_tp: trace non-increasing)
            assert is_cp(a) and is_cp(b), name
            tp = np.linalg.eigvalsh(ptrace_out(a, d)).max()
            assert tp <= 1 + 1e-12 if name == "non_tp" else abs(tp - 1) <= 1e-12, (name, tp)
        families.update(names)
    assert {"non_tp", "random_cptp", "amplitude_damping", "near_identical", "unitary", "pauli", "replacement"} <= families
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_golden_lower_bounds_at_float64():
    """L is 2 g at the stored input state: float64 evaluation agrees to rounding (the mpmath value is the stored one)."""
    g = np.load(GOLDEN)
    for nq in (1, 2):
        p = f"q{nq}_"
        for c0, c1, T, L in zip(g[p + "choi0"], g[p + "choi1"], g[p + "T"], g[p + "lower"]):
            d = T.shape[0]
            J = (c0 - c1 + (c0 - c1).conj().T) / 2
            S = np.kron(np.eye(d), T / np.sqrt(np.real(np.trace(T @ T))))
            lam = np.linalg.eigvalsh(S @ J @ S)
            assert abs(2 * lam[lam > 0].sum() - L) <= 1e-13 * max(L, 1e-6)
