"""The 1-3 qubit state kernels behind fbx_state_measures and fbx_proj_state_physical (state_measures_kernel<1, 2, 3>,
proj_state_kernel<1, 2, 3>: one wavefront per item): the counterpart of tests/test_state_measures_big_gpu.py.  Answers that come
from no solver, the oracle, projections whose eigenvectors are not the identity, products that tie the three instantiations to
each other and to the 4-qubit kernel, the batch geometry bit for bit, and non-finite items.

Fidelity on exact families is held to the oracle's own error (fbx_oracle.measures.fidelity, the reference's formula on scipy) on
the same pairs: per family and size every error of the kernel stays within max(4 E, 1e-11), E the oracle's largest error in that
family -- the factor and the floor of the 4-5 qubit test.  A square root turns the 1e-17 rounding of a zero eigenvalue into 3e-9,
so no absolute bound exists for pure and rank-deficient pairs.  Largest errors on an MI355X, (kernel, oracle), 12 pairs each,
the larger of the two argument orders:

    family            1 qubit               2 qubits              3 qubits
    commuting         (1.2e-15, 1.8e-15)    (2.6e-15, 2.2e-15)    (3.6e-15, 2.0e-15)
    identical         (1.8e-15, 2.0e-15)    (1.3e-15, 3.6e-15)    (3.3e-15, 2.7e-15)
    orthogonal        (2.7e-16, 2.0e-16)    (1.1e-16, 6.1e-16)    (1.2e-16, 4.5e-16)
    pure_mixed        (1.2e-08, 1.5e-08)    (9.1e-09, 2.4e-08)    (7.0e-09, 1.3e-08)
    pure_pure         (1.6e-08, 1.9e-08)    (6.7e-09, 2.9e-08)    (9.8e-09, 1.7e-08)
    rank_deficient    (1.3e-08, 1.1e-08)    (7.3e-09, 3.2e-08)    (7.2e-09, 2.4e-08)

The non-finite contract is the one of the big kernels: an item with a NaN or an infinity anywhere in the pair gives NaN in every
measure asked for (in every entry of its projection) and leaves its neighbours' bits alone.  The small kernels did not hold it
before test_non_finite_items came with its guard in them: the column maximum of the trace distance (fmax) drops a NaN, the
clipped square roots of the fidelity turn NaN eigenvalues into zeros (a finite fidelity of 0), and the projection takes an item
whose eigenvalues are all NaN for physical and returns it with its finite entries in place."""
import warnings

import numpy as np
import pytest

import chernoff_cases as cc
import state_measure_cases as sc
from test_state_measures_big_gpu import ALL, measures, project, raw_measures, raw_project

pytestmark = pytest.mark.gpu

SMALL = (1, 2, 3)


def oracle_fidelity(rho, sigma):
    from fbx_oracle import measures as om
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.array([np.real(om.fidelity(r, s)) for r, s in zip(rho, sigma)])


# ------------------------------------------------------------------------------------------------ answers from no solver
@pytest.mark.parametrize("nq", SMALL)
@pytest.mark.parametrize("name", sorted(sc.FAMILIES))
def test_exact_families(gpu, name, nq):
    rho, sigma, exact = sc.family(name, nq, 12)
    got = measures(rho, sigma)
    want = sc.host_sums(rho, sigma)
    assert np.abs(got["purity"] - want["purity"]).max() < 1e-13
    assert np.abs(got["hs_ip"] - want["hs_ip"]).max() < 1e-13
    assert np.abs(got["trace_distance"] - want["trace_distance"]).max() < 1e-14
    for key in ("purity", "hs_ip"):
        if key in exact:
            assert np.abs(got[key] - exact[key]).max() < 1e-13, key
    # rho's root is taken; the other way round it is sigma's (a different computation on a different matrix)
    for label, a, b in (("", rho, sigma), (" swapped", sigma, rho)):
        f = got["fidelity"] if a is rho else measures(a, b, ("fidelity",))["fidelity"]
        err_new = np.abs(f - exact["fidelity"])
        err_old = np.abs(oracle_fidelity(a, b) - exact["fidelity"])
        print(f"fidelity error, {name}{label}, {nq} qubits: kernel max {err_new.max():.3e}, oracle max {err_old.max():.3e}")
        assert np.all(np.isfinite(f))
        assert np.all(err_new <= max(4 * err_old.max(), 1e-11)), (name, nq, label, err_new.max(), err_old.max())


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("nq", SMALL)
def test_measures_against_the_oracle(gpu, nq):
    from fbx_oracle import measures as om
    rho, sigma = sc.full_rank_pairs(nq, 12, 41)
    got = measures(rho, sigma)
    for b in range(12):
        assert abs(got["fidelity"][b] - np.real(om.fidelity(rho[b], sigma[b]))) < 1e-11, b
        assert abs(got["purity"][b] - np.real(om.purity(rho[b]))) < 1e-13, b
        assert abs(got["trace_distance"][b] - om.trace_distance(rho[b], sigma[b])) < 1e-13, b
        assert abs(got["hs_ip"][b] - np.real(om.hilbert_schmidt_ip(rho[b], sigma[b]))) < 1e-13, b


def against_the_oracle_projection(x):
    from fbx_oracle import superops as so
    got = project(x)
    for b in range(len(x)):
        assert np.abs(got[b] - so.project_state_matrix_to_physical(x[b])).max() < 1e-12, b
    return got


@pytest.mark.parametrize("nq", SMALL)
def test_projection_of_indefinite_matrices(gpu, nq):
    h = sc.indefinite(nq, 12, 43)
    got = against_the_oracle_projection(h)
    for b in range(12):
        assert np.linalg.eigvalsh(got[b]).min() > -1e-12 and abs(np.trace(got[b]) - 1) < 1e-12, b
    assert np.abs(project(got) - got).max() < 1e-12
    # a complex trace: the division comes first
    against_the_oracle_projection(h * (0.37 - 1.2j))


# eigenvalues and what the redistribution of Smolin, Gambetta and Smith makes of them (the most negative ones are set to zero and
# their sum is spread evenly over the others, until none is negative); the first of the 8 x 8 ones is Fig. 1 of the paper
SPECTRA = {1: [([1.2, -0.2], [1.0, 0.0]), ([0.5, 0.5], [0.5, 0.5])],
           2: [([3 / 5, 1 / 2, 7 / 20, -9 / 20], [9 / 20, 7 / 20, 1 / 5, 0]), ([0.9, 0.4, -0.1, -0.2], [0.75, 0.25, 0, 0])],
           3: [([-11 / 20, 1 / 10, 7 / 20, 1 / 2, 3 / 5, 0, 0, 0], [0, 0, 1 / 5, 7 / 20, 9 / 20, 0, 0, 0]),
               ([0.5, 0.4, 0.3, 0.2, 0.15, -0.15, -0.2, -0.2], [0.39, 0.29, 0.19, 0.09, 0.04, 0, 0, 0])]}


@pytest.mark.parametrize("nq", SMALL)
def test_projection_of_known_spectra(gpu, nq):
    """in random unitary bases, where the eigenvectors have to be put back (the diagonal case of tests/test_state_gpu.py leaves
    them the identity)"""
    d = 2 ** nq
    rng = np.random.default_rng([47, nq])
    for eigs, want in SPECTRA[nq]:
        eigs, want = np.array(eigs, dtype=float), np.array(want, dtype=float)
        assert abs(eigs.sum() - 1) < 1e-15 and abs(want.sum() - 1) < 1e-15
        us = [cc.random_unitary(d, rng) for _ in range(6)]
        x = np.array([(u * eigs) @ u.conj().T for u in us])
        got = against_the_oracle_projection(x)
        for u, g in zip(us, got):
            assert np.abs(g - (u * want) @ u.conj().T).max() < 1e-12


@pytest.mark.parametrize("nq", SMALL)
def test_physical_inputs_come_back_divided_by_their_trace(gpu, nq):
    """The reference returns rho / tr(rho) itself when the eigenvalues are non-negative.  With a diagonal of multiples of 2^-20
    that add up to one (exactly, in any order) and a trace of +-2^k or +-i 2^k, every product and the division are exact:
    x / tr(x) is rho to the last bit, whatever the order of the sums and with or without fused multiply-adds."""
    d = 2 ** nq
    rho, _ = sc.full_rank_pairs(nq, 8, 53)
    rho = rho.copy()
    for b in range(8):
        diag = np.round(rho[b].diagonal().real * 2 ** 20) / 2 ** 20
        diag[-1] = 1.0 - diag[:-1].sum()
        rho[b][np.arange(d), np.arange(d)] = diag
        assert np.linalg.eigvalsh(rho[b]).min() > 1e-3
    scale = np.array([2, -0.5, 4j, -0.25j, 1, -8, 0.125j, -1j])[:, None, None]
    got = project(rho * scale)
    assert np.array_equal(got, rho)
    # an upper triangle that is not the adjoint of the lower one comes back as it went in, where a rebuilt matrix would be
    # Hermitian
    junk = np.tril(rho) + np.triu(np.full_like(rho, 0.25 - 0.5j), 1)
    assert np.array_equal(project(junk * scale), junk)


@pytest.mark.parametrize("nq", SMALL)
def test_projection_reads_the_lower_triangle(gpu, nq):
    """on the branch that rebuilds the matrix: what scipy.linalg.eigh reads in the reference, and the oracle with it"""
    h = sc.indefinite(nq, 12, 57)
    h = h[np.linalg.eigvalsh(h).min(axis=1) < -1e-3]                            # (a 2 x 2 one may happen to be physical)
    assert len(h) >= 4
    clean = project(h)
    low = np.tril(h) + np.triu(np.full_like(h, 7 + 3j), 1)
    got = against_the_oracle_projection(low)
    assert np.array_equal(got, clean)
    assert np.abs(got - got.conj().transpose(0, 2, 1)).max() < 1e-13


# ------------------------------------------------------------------------------------------------ invariances
@pytest.mark.parametrize("ka,kb", [(1, 1), (1, 2), (2, 2)])
def test_tensor_products_of_smaller_pairs(gpu, ka, kb):
    """F, purity and hs_ip are multiplicative: 1 + 1 -> 2, 1 + 2 -> 3 and 2 + 2 -> 4 qubits tie the three small instantiations
    to each other and to the 4-qubit kernel"""
    ra, sa = sc.full_rank_pairs(ka, 12, 59)
    rb, sb = sc.full_rank_pairs(kb, 12, 61)
    a, b = measures(ra, sa), measures(rb, sb)
    big = measures(np.array([np.kron(x, y) for x, y in zip(ra, rb)]), np.array([np.kron(x, y) for x, y in zip(sa, sb)]))
    assert np.abs(big["fidelity"] - a["fidelity"] * b["fidelity"]).max() < 1e-10
    for key in ("purity", "hs_ip"):
        assert np.abs(big[key] - a[key] * b[key]).max() < 1e-13, key


@pytest.mark.parametrize("nq", SMALL)
def test_unitary_conjugation_symmetry_and_fuchs_van_de_graaf(gpu, nq):
    rho, sigma = sc.full_rank_pairs(nq, 12, 67)
    base = measures(rho, sigma)
    u = cc.random_unitary(2 ** nq, np.random.default_rng([71, nq]))
    rot = measures(u @ rho @ u.conj().T, u @ sigma @ u.conj().T)
    for key in ("fidelity", "purity", "hs_ip"):
        assert np.abs(rot[key] - base[key]).max() < 1e-10, key
    swapped = measures(sigma, rho, ("fidelity",))["fidelity"]
    assert np.abs(swapped - base["fidelity"]).max() < 1e-10
    t = 0.5 * np.abs(np.linalg.eigvalsh(rho - sigma)).sum(axis=1)               # the true trace distance: half the nuclear norm
    f = base["fidelity"]
    assert np.all(1 - np.sqrt(f) <= t + 1e-10) and np.all(t <= np.sqrt(1 - f) + 1e-10)


# ------------------------------------------------------------------------------------------------ batch geometry
BATCHES = (1, 63, 64, 65, 257)


def mixed_items(nq):
    """five pairs: full rank, a pure / mixed one, a rank-deficient one"""
    rho, sigma = sc.full_rank_pairs(nq, 3, 73)
    pr, ps, _ = sc.family("pure_mixed", nq, 1)
    dr, ds, _ = sc.family("rank_deficient", nq, 1)
    return np.concatenate([rho, pr, dr]), np.concatenate([sigma, ps, ds])


@pytest.mark.parametrize("nq", SMALL)
def test_measures_do_not_depend_on_the_batch(gpu, nq):
    rho, sigma = mixed_items(nq)
    n = len(rho)
    alone = [measures(rho[b:b + 1], sigma[b:b + 1]) for b in range(n)]
    for B in BATCHES:
        idx = (np.arange(B) * 3 + 1) % n
        got = measures(rho[idx], sigma[idx])
        for key in ALL:
            want = np.array([alone[b][key][0] for b in idx])
            assert np.array_equal(got[key], want), (nq, B, key)
    # any subset of the outputs (NULL for the rest): the same bits in those that are asked for
    full = measures(rho, sigma)
    for mask in range(1, 15):
        which = tuple(k for i, k in enumerate(ALL) if mask >> i & 1)
        got = measures(rho, sigma, which)
        assert set(got) == set(which)
        for key in which:
            assert np.array_equal(got[key], full[key]), (nq, which, key)
    # rho enters through its lower triangle where it is diagonalised; the cheap outputs see the whole matrix
    low = np.tril(rho) + np.triu(np.full_like(rho, 7 + 3j), 1)
    assert np.array_equal(measures(low, sigma, ("fidelity",))["fidelity"], full["fidelity"])


@pytest.mark.parametrize("nq", SMALL)
def test_projection_does_not_depend_on_the_batch(gpu, nq):
    h = np.concatenate([sc.indefinite(nq, 3, 79), sc.full_rank_pairs(nq, 2, 83)[0]])
    n = len(h)
    alone = np.array([project(h[b:b + 1])[0] for b in range(n)])
    for B in BATCHES:
        idx = (np.arange(B) * 3 + 1) % n
        assert np.array_equal(project(h[idx]), alone[idx]), (nq, B)


@pytest.mark.parametrize("nq", SMALL)
def test_empty_batch_touches_nothing(gpu, nq):
    lib = gpu.lib()
    d = 2 ** nq
    rc, outs = raw_measures(lib, nq, np.zeros((0, d, d)), np.zeros((0, d, d)))
    assert rc == 0 and all(v.shape == (0,) for v in outs.values())
    rc, out = raw_project(lib, nq, np.zeros((0, d, d)))
    assert rc == 0 and out.shape == (0, d, d)
    # B = 0 with buffers behind the pointers: they keep what they held
    from fbx import _lib
    x = np.ascontiguousarray(sc.full_rank_pairs(nq, 2, 87)[0])
    keep = {k: np.full(2, -7.0) for k in ALL}
    rc = lib.fbx_state_measures(nq, 0, _lib.dptr(x.view(np.float64)), _lib.dptr(x.view(np.float64)), _lib.dptr(keep["purity"]),
                                _lib.dptr(keep["fidelity"]), _lib.dptr(keep["trace_distance"]), _lib.dptr(keep["hs_ip"]))
    assert rc == 0 and all(np.all(v == -7.0) for v in keep.values())
    out = np.full_like(x, -7.0)
    rc = lib.fbx_proj_state_physical(nq, 0, _lib.dptr(x.view(np.float64)), _lib.dptr(out.view(np.float64)))
    assert rc == 0 and np.all(out == -7.0)


@pytest.mark.parametrize("nq", SMALL)
def test_non_finite_items(gpu, nq):
    """the contract of test_empty_batch_and_non_finite_items for the big kernels: NaN in every output of the item, its
    neighbours bit-identical to a clean run"""
    rho, sigma = mixed_items(nq)
    want = measures(rho, sigma)
    d = 2 ** nq
    for bad_value in (np.nan, np.inf):
        bad = rho.copy()
        bad[3, d - 1, 0] = bad_value
        got = measures(bad, sigma)
        keep = np.arange(len(rho)) != 3
        for key in ALL:
            assert np.array_equal(got[key][keep], want[key][keep]), (nq, key)
            assert not np.isfinite(got[key][3]), (nq, key, got[key][3])
        bad_s = sigma.copy()
        bad_s[2, 0, 0] = bad_value
        got = measures(rho, bad_s, ("fidelity", "hs_ip", "trace_distance"))
        for key in ("fidelity", "hs_ip", "trace_distance"):
            assert not np.isfinite(got[key][2]), (nq, key, got[key][2])
            assert np.array_equal(np.delete(got[key], 2), np.delete(want[key], 2))
    h = sc.indefinite(nq, 5, 89)
    want = project(h)
    for bad_value in (np.nan, np.inf):
        bad = h.copy()
        bad[4, 1, 0] = bad_value
        got = project(bad)
        assert np.array_equal(np.delete(got, 4, axis=0), np.delete(want, 4, axis=0))
        assert not np.isfinite(got[4]).any()
