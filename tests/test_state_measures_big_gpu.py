"""The 4- and 5-qubit state kernels behind fbx_state_measures and fbx_proj_state_physical (state_measures_big_kernel,
proj_state_big_kernel) and the resident bootstrap tomography.state_measure_variance_batch: the C entry points, answers that come
from no solver, the oracle, invariances that tie the kernels to the 1-3 qubit ones, the batch geometry bit for bit, and the
bootstrap against its hand composition.

Fidelity on exact families is held to the error of the composition of generic primitives the kernels replace
(distance_measures._state_measures_large) on the same inputs: per family and size, every error of the kernel stays within
max(4 E, 1e-11), E the largest error of the composition in that family -- a square root turns the 1e-17 rounding of a zero
eigenvalue into 3e-9, so no absolute bound can be fixed for rank-deficient inputs.  Both largest errors are printed."""
import warnings

import numpy as np
import pytest

import chernoff_cases as cc
import state_measure_cases as sc

pytestmark = pytest.mark.gpu

ALL = ("purity", "fidelity", "trace_distance", "hs_ip")
BIG = (4, 5)


def measures(rho, sigma, which=ALL):
    from fbx import distance_measures as dm
    return dm.state_measures_batch(rho, sigma, which)


def project(x):
    from fbx.operator_tools.project_state_matrix import project_state_matrix_to_physical_batch
    return project_state_matrix_to_physical_batch(x)


def raw_measures(lib, nq, rho, sigma, which=ALL):
    """fbx_state_measures through ctypes: (return code, {name: values})"""
    from fbx import _lib
    rho, sigma = np.ascontiguousarray(rho, dtype=np.complex128), np.ascontiguousarray(sigma, dtype=np.complex128)
    B = rho.shape[0]
    outs = {k: np.full(B, -7.0) for k in which}
    rc = lib.fbx_state_measures(nq, B, _lib.dptr(rho.view(np.float64)), _lib.dptr(sigma.view(np.float64)),
                                _lib.dptr(outs.get("purity")), _lib.dptr(outs.get("fidelity")),
                                _lib.dptr(outs.get("trace_distance")), _lib.dptr(outs.get("hs_ip")))
    return rc, outs


def raw_project(lib, nq, x):
    from fbx import _lib
    x = np.ascontiguousarray(x, dtype=np.complex128)
    out = np.full_like(x, -7.0)
    rc = lib.fbx_proj_state_physical(nq, x.shape[0], _lib.dptr(x.view(np.float64)), _lib.dptr(out.view(np.float64)))
    return rc, out


# ------------------------------------------------------------------------------------------------ the C entry points
@pytest.mark.parametrize("nq", BIG)
def test_c_entry_points_accept_four_and_five_qubits(gpu, nq):
    lib = gpu.lib()
    rho, sigma, exact = sc.family("commuting", nq, 5)
    rc, got = raw_measures(lib, nq, rho, sigma)
    assert rc == 0
    want = sc.host_sums(rho, sigma)
    assert np.abs(got["fidelity"] - exact["fidelity"]).max() < 1e-11
    assert np.abs(got["purity"] - exact["purity"]).max() < 1e-13
    assert np.abs(got["hs_ip"] - exact["hs_ip"]).max() < 1e-13
    assert np.abs(got["trace_distance"] - want["trace_distance"]).max() < 1e-14
    h = sc.indefinite(nq, 5, 3)
    rc, p = raw_project(lib, nq, h)
    assert rc == 0
    for b in range(5):
        w = np.linalg.eigvalsh(p[b])
        assert w.min() > -1e-12 and abs(np.trace(p[b]) - 1) < 1e-12
    assert np.abs(p - p.conj().transpose(0, 2, 1)).max() < 1e-13


def test_six_qubits_stay_an_argument_error(gpu):
    lib = gpu.lib()
    x = np.zeros((1, 64, 64), dtype=np.complex128)
    x[0] = np.eye(64) / 64
    rc, _ = raw_measures(lib, 6, x, x)
    assert rc == gpu.FBX_ERR_BAD_ARG
    rc, _ = raw_project(lib, 6, x)
    assert rc == gpu.FBX_ERR_BAD_ARG
    for nq in (0, -1):
        assert raw_measures(lib, nq, x, x)[0] == gpu.FBX_ERR_BAD_ARG
        assert raw_project(lib, nq, x)[0] == gpu.FBX_ERR_BAD_ARG


def test_bootstraps_run_on_a_four_qubit_design(gpu):
    from fbx import synthetic, tomography
    design, rhos, e, c = synthetic.state_batch(4, 2, shots=2000, mixed=0.1)
    mean, var, q = tomography.state_chernoff_variance_batch(design, e, c, rhos, n_resamples=4, seed=2, estimator="linv",
                                                            project_to_physical=True, return_samples=True)
    assert q.shape == (4, 2) and np.all((q > 0.3) & (q <= 1 + 1e-9)) and np.all(var >= 0)
    mean, var, f = tomography.state_measure_variance_batch(design, e, c, rhos, "fidelity", n_resamples=4, seed=2,
                                                           estimator="linv", return_samples=True)
    assert f.shape == (4, 2) and np.all((f > 0.3) & (f <= 1 + 1e-9)) and np.all(var >= 0)
    mean, var = tomography.state_measure_variance_batch(design, e, c, measure="purity", n_resamples=4, seed=2, estimator="linv")
    assert mean.shape == (2,) and np.all((mean > 0.3) & (mean <= 1 + 1e-9))


# ------------------------------------------------------------------------------------------------ answers from no solver
@pytest.mark.parametrize("nq", BIG)
@pytest.mark.parametrize("name", sorted(sc.FAMILIES))
def test_exact_families(gpu, name, nq):
    from fbx import distance_measures as dm
    rho, sigma, exact = sc.family(name, nq, 12)
    got = measures(rho, sigma)
    old = dm._state_measures_large(rho, sigma, ALL)
    want = sc.host_sums(rho, sigma)
    assert np.abs(got["purity"] - want["purity"]).max() < 1e-13
    assert np.abs(got["hs_ip"] - want["hs_ip"]).max() < 1e-13
    assert np.abs(got["trace_distance"] - want["trace_distance"]).max() < 1e-14
    for key in ("purity", "hs_ip"):
        if key in exact:
            assert np.abs(got[key] - exact[key]).max() < 1e-13, key
    err_new = np.abs(got["fidelity"] - exact["fidelity"])
    err_old = np.abs(old["fidelity"] - exact["fidelity"])
    print(f"fidelity error, {name}, {nq} qubits: kernel max {err_new.max():.3e}, composition max {err_old.max():.3e}")
    assert np.all(np.isfinite(got["fidelity"]))
    assert np.all(err_new <= max(4 * err_old.max(), 1e-11)), (name, nq, err_new.max(), err_old.max())
    # the other way round: sigma's root is taken (a different computation on a different matrix)
    back = measures(sigma, rho, ("fidelity",))["fidelity"]
    old_back = dm._state_measures_large(sigma, rho, ("fidelity",))["fidelity"]
    err_new, err_old = np.abs(back - exact["fidelity"]), np.abs(old_back - exact["fidelity"])
    print(f"fidelity error, {name} swapped, {nq} qubits: kernel max {err_new.max():.3e}, composition max {err_old.max():.3e}")
    assert np.all(err_new <= max(4 * err_old.max(), 1e-11)), (name, nq, "swapped", err_new.max(), err_old.max())


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("nq", BIG)
def test_measures_against_the_oracle(gpu, nq):
    from fbx_oracle import measures as om
    rho, sigma = sc.full_rank_pairs(nq, 64, 41)
    got = measures(rho, sigma)
    for b in range(64):
        assert abs(got["fidelity"][b] - om.fidelity(rho[b], sigma[b])) < 1e-11, b
        assert abs(got["purity"][b] - om.purity(rho[b])) < 1e-13, b
        assert abs(got["trace_distance"][b] - om.trace_distance(rho[b], sigma[b])) < 1e-14, b
        assert abs(got["hs_ip"][b] - om.hilbert_schmidt_ip(rho[b], sigma[b])) < 1e-13, b


@pytest.mark.parametrize("nq", BIG)
def test_projection_against_the_oracle(gpu, nq):
    from fbx_oracle import superops as so
    h = sc.indefinite(nq, 64, 43)
    got = project(h)
    for b in range(64):
        assert np.abs(got[b] - so.project_state_matrix_to_physical(h[b])).max() < 1e-11, b
        assert np.linalg.eigvalsh(got[b]).min() > -1e-12 and abs(np.trace(got[b]) - 1) < 1e-12, b
    again = project(got)
    assert np.abs(again - got).max() < 1e-12


@pytest.mark.parametrize("nq", BIG)
def test_projection_of_known_spectra(gpu, nq):
    """Fig. 1 of Smolin-Gambetta-Smith, the diagonal case of tests/test_state_gpu.py, in a random basis of 16 / 32 dimensions"""
    d = 2 ** nq
    rng = np.random.default_rng([47, nq])
    eigs, want = np.zeros(d), np.zeros(d)
    eigs[:5] = [-11.0 / 20, 1.0 / 10, 7.0 / 20, 1.0 / 2, 3.0 / 5]
    want[:5] = [0, 0, 1.0 / 5, 7.0 / 20, 9.0 / 20]
    us = [np.eye(d)] + [cc.random_unitary(d, rng) for _ in range(5)]
    x = np.array([(u * eigs) @ u.conj().T for u in us])
    got = project(x)
    for u, g in zip(us, got):
        assert np.abs(g - (u * want) @ u.conj().T).max() < 1e-13


@pytest.mark.parametrize("nq", BIG)
def test_physical_inputs_come_back_rescaled(gpu, nq):
    rho, _ = sc.full_rank_pairs(nq, 8, 53)
    scale = np.arange(1, 9)[:, None, None] * 0.37
    got = project(rho * scale)
    assert np.abs(got - rho * scale / np.trace(rho * scale, axis1=1, axis2=2)[:, None, None]).max() < 1e-14
    # the reference returns rho / tr(rho) itself when the eigenvalues of its lower triangle are non-negative: an upper
    # triangle that is not the adjoint of the lower one comes back as it went in, where a rebuilt matrix would be Hermitian
    junk = np.tril(rho) + np.triu(np.full_like(rho, 0.25 - 0.5j), 1)
    got = project(junk)
    assert np.abs(got - junk / np.trace(junk, axis1=1, axis2=2)[:, None, None]).max() < 1e-14


# ------------------------------------------------------------------------------------------------ invariances
@pytest.mark.parametrize("nq", BIG)
def test_tensor_products_of_smaller_pairs(gpu, nq):
    """F, purity and hs_ip are multiplicative: a 3-qubit pair times a 1-qubit (4 qubits) or 2-qubit (5 qubits) pair, the
    factors from the 1-3 qubit kernels"""
    k = nq - 3
    r3, s3 = sc.full_rank_pairs(3, 10, 59)
    rk, sk = sc.full_rank_pairs(k, 10, 61)
    a, b = measures(r3, s3), measures(rk, sk)
    big = measures(np.array([np.kron(x, y) for x, y in zip(r3, rk)]), np.array([np.kron(x, y) for x, y in zip(s3, sk)]))
    for key in ("fidelity", "purity", "hs_ip"):
        assert np.abs(big[key] - a[key] * b[key]).max() < 1e-10, key


@pytest.mark.parametrize("nq", BIG)
def test_unitary_conjugation_symmetry_and_fuchs_van_de_graaf(gpu, nq):
    rho, sigma = sc.full_rank_pairs(nq, 10, 67)
    base = measures(rho, sigma)
    u = cc.random_unitary(2 ** nq, np.random.default_rng([71, nq]))
    rot = measures(u @ rho @ u.conj().T, u @ sigma @ u.conj().T)
    for key in ("fidelity", "purity", "hs_ip"):
        assert np.abs(rot[key] - base[key]).max() < 1e-10, key
    swapped = measures(sigma, rho, ("fidelity",))["fidelity"]
    assert np.abs(swapped - base["fidelity"]).max() < 1e-10
    t = 0.5 * np.abs(np.linalg.eigvalsh(rho - sigma)).sum(axis=1)               # half the nuclear norm
    f = base["fidelity"]
    assert np.all(1 - np.sqrt(f) <= t + 1e-10) and np.all(t <= np.sqrt(1 - f) + 1e-10)


# ------------------------------------------------------------------------------------------------ batch geometry
def mixed_items(nq):
    """seven pairs: full rank, a pure / mixed one, rank-deficient ones"""
    rho, sigma = sc.full_rank_pairs(nq, 3, 73)
    pr, ps, _ = sc.family("pure_mixed", nq, 2)
    dr, ds, _ = sc.family("rank_deficient", nq, 2)
    return np.concatenate([rho, pr, dr]), np.concatenate([sigma, ps, ds])


@pytest.mark.parametrize("nq", BIG)
def test_measures_do_not_depend_on_the_batch(gpu, nq):
    rho, sigma = mixed_items(nq)
    n = len(rho)
    alone = [measures(rho[b:b + 1], sigma[b:b + 1]) for b in range(n)]
    for B in (3, 257, 4099):
        idx = (np.arange(B) * 3 + 1) % n
        got = measures(rho[idx], sigma[idx])
        for key in ALL:
            want = np.array([alone[b][key][0] for b in idx])
            assert np.array_equal(got[key], want), (nq, B, key)
    # any subset of the outputs: the same bits in those that are asked for
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


@pytest.mark.parametrize("nq", BIG)
def test_projection_does_not_depend_on_the_batch(gpu, nq):
    h = np.concatenate([sc.indefinite(nq, 5, 79), sc.full_rank_pairs(nq, 2, 83)[0]])
    n = len(h)
    alone = np.array([project(h[b:b + 1])[0] for b in range(n)])
    for B in (3, 257, 4099):
        idx = (np.arange(B) * 3 + 1) % n
        assert np.array_equal(project(h[idx]), alone[idx]), (nq, B)
    low = np.tril(h[:5]) + np.triu(np.full_like(h[:5], 7 + 3j), 1)             # not physical: rebuilt from the lower triangle
    assert np.array_equal(project(low), alone[:5])


@pytest.mark.parametrize("nq", BIG)
def test_empty_batch_and_non_finite_items(gpu, nq):
    lib = gpu.lib()
    d = 2 ** nq
    rc, outs = raw_measures(lib, nq, np.zeros((0, d, d)), np.zeros((0, d, d)))
    assert rc == 0 and all(v.shape == (0,) for v in outs.values())
    assert raw_project(lib, nq, np.zeros((0, d, d)))[0] == 0
    rho, sigma = mixed_items(nq)
    want = measures(rho, sigma)
    for bad_value in (np.nan, np.inf):
        bad = rho.copy()
        bad[3, 5, 2] = bad_value
        got = measures(bad, sigma)
        keep = np.arange(len(rho)) != 3
        for key in ALL:
            assert np.array_equal(got[key][keep], want[key][keep]), (nq, key)
            assert not np.isfinite(got[key][3]), (nq, key)
        bad_s = sigma.copy()
        bad_s[2, 0, 0] = bad_value
        got = measures(rho, bad_s, ("fidelity", "hs_ip"))
        assert not np.isfinite(got["fidelity"][2]) and not np.isfinite(got["hs_ip"][2])
        assert np.array_equal(np.delete(got["fidelity"], 2), np.delete(want["fidelity"], 2))
    h = sc.indefinite(nq, 6, 89)
    want = project(h)
    bad = h.copy()
    bad[4, 1, 0] = np.nan
    got = project(bad)
    assert np.array_equal(np.delete(got, 4, axis=0), np.delete(want, 4, axis=0))
    assert not np.isfinite(got[4]).any()


# ------------------------------------------------------------------------------------------------ bootstrap
@pytest.mark.parametrize("nq,R,B", [(2, 6, 3), (4, 4, 2)])
@pytest.mark.parametrize("estimator,project_flag", [("mle", True), ("linv", False)])
def test_bootstrap_is_the_hand_composition(gpu, nq, R, B, estimator, project_flag):
    from fbx import synthetic, tomography
    design, rhos, e, c = synthetic.state_batch(nq, B, shots=2000, mixed=0.05)
    m = design.m
    target = rhos if nq == 4 else cc.random_state(2 ** nq, np.random.default_rng(31))
    e_rs = tomography.resample_expectations_with_beta_batch(e, c, R, seed=5).reshape(R * B, m)
    c_rs = np.ascontiguousarray(np.broadcast_to(c, (R, B, m))).reshape(R * B, m)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if estimator == "mle":
            est = tomography.iterative_mle_state_estimate_batch(design, e_rs, c_rs)
        else:
            est = tomography.linear_inv_state_estimate_batch(design, e_rs)
    if project_flag:
        est = project(est)
    tgt = np.ascontiguousarray(np.broadcast_to(target, (R, B) + est.shape[-2:])).reshape(est.shape)
    want = measures(tgt, est)
    values = {}
    for measure in ("fidelity", "trace_distance", "hs_ip", "infidelity"):
        mean, var, v = tomography.state_measure_variance_batch(design, e, c, target, measure, n_resamples=R, seed=5,
                                                               estimator=estimator, project_to_physical=project_flag,
                                                               return_samples=True)
        values[measure] = v
        if measure != "infidelity":
            assert np.array_equal(v, want[measure].reshape(R, B)), (nq, measure)
        assert np.array_equal(mean, v.mean(axis=0)) and np.array_equal(var, v.var(axis=0))
    assert np.array_equal(values["infidelity"], 1 - values["fidelity"])
    mean, var, v = tomography.state_measure_variance_batch(design, e, c, None, "purity", n_resamples=R, seed=5,
                                                           estimator=estimator, project_to_physical=project_flag,
                                                           return_samples=True)
    assert np.array_equal(v, measures(est, None, ("purity",))["purity"].reshape(R, B))
    if project_flag:
        assert np.all((values["fidelity"] > 0.3) & (values["fidelity"] <= 1 + 1e-9))


def test_estimate_variance_agrees_at_the_same_seed(gpu):
    """estimate_variance on a 4-qubit experiment (its projection and measures now the fused kernels) against the resident
    bootstrap with the same seed: the same resamples, estimates and measures, averaged on the host in both"""
    from fbx import distance_measures as dm, synthetic, tomography as T
    from fbx.observable_estimation import ExperimentResult
    design, rhos, e, c = synthetic.state_batch(4, 1, shots=2000, mixed=0.1)
    qubits = [0, 1, 2, 3]
    settings = T.generate_state_tomography_settings(qubits)
    res = [ExperimentResult(setting=s, expectation=float(e[0, k]), total_counts=int(c[0, k]), std_err=0.0)
           for k, s in enumerate(settings)]
    for est, name, R in ((T.iterative_mle_state_estimate, "mle", 6), (T.linear_inv_state_estimate, "linv", 16)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mean, var = T.estimate_variance(res, qubits, est, dm.fidelity, target_state=rhos[0], n_resamples=R,
                                            project_to_physical=True, seed=9)
        m2, v2 = T.state_measure_variance_batch(design, e, c, rhos[0], "fidelity", n_resamples=R, seed=9, estimator=name)
        assert abs(mean - m2[0]) <= 1e-12 and abs(var - v2[0]) <= 1e-12, (name, mean, m2, var, v2)
