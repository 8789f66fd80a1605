"""fbx_chernoff_bound against exact and high-precision answers: the closed forms of tests/chernoff_cases.py, the mpmath brackets of
tests/golden/chernoff_exact.npz, inequalities against other kernels, invariances, parity with the host function and the reference's
recorded values, the batch geometry of the fused (1-3 qubits) and composed (4-5 qubits) paths, and the resident bootstrap.  The
promise checked is the one of include/fbx.h: lower is a lower bound and qcb an upper bound of the exact minimum, for every item
whether certified or not, and certified items are within tol.  The slack is at the rounding level (1e-12 relative), never tol."""
import ctypes
import os
import warnings

import numpy as np
import pytest

import chernoff_cases as cc

pytestmark = pytest.mark.gpu

RT, AT = 1e-12, 1e-15                 # rounding slack: relative, absolute
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "chernoff_exact.npz")
EXTRAS = os.path.join(HERE, "golden", "extras.npz")
# floor on the share of certified items (iters >= 0) at tol 1e-10, every exact family and the goldens, 1-5 qubits
CERTIFIED_FLOOR = 1.0


def run(rho, sigma, tol=1e-10, max_iters=100, zero_tol=1e-12):
    from fbx import distance_measures as dm
    return dm.quantum_chernoff_bound_batch(rho, sigma, tol=tol, max_iters=max_iters, zero_tol=zero_tol, return_bounds=True)


def sandwich(lo, hi, qcb, lower, where):
    """lo <= exact <= hi known: lower must not exceed hi, qcb must not fall below lo (to rounding)"""
    assert np.all(lower <= hi * (1 + RT) + AT), (where, np.max(lower - hi))
    assert np.all(qcb >= lo * (1 - RT) - AT), (where, np.min(qcb - lo))
    assert np.all(lower <= qcb), where


def gap_rule(qcb, lower, iters, tol, where):
    ok = iters >= 0
    assert np.all(qcb[ok] - lower[ok] <= tol * np.maximum(qcb[ok], 1e-12)), where
    return ok.mean()


def overlap(a, b, where):
    """two runs on inputs with the same exact value: each bracket [lower, qcb] meets the other"""
    qa, _, la, _ = a
    qb, _, lb, _ = b
    assert np.all(la <= qb * (1 + RT) + AT) and np.all(lb <= qa * (1 + RT) + AT), where


def random_pairs(nq, count, seed):
    rng = np.random.default_rng([seed, nq])
    d = 2 ** nq
    kinds = ["full", "lowrank", "near"]
    pairs = [cc.golden_pair(kinds[k % 3], d, rng) for k in range(count)]
    return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])


# ------------------------------------------------------------------------------------------------ exact answers
EXACT_CASES = [(name, nq) for name in sorted(cc.FAMILIES) for nq in (1, 2, 3)] + \
              [(name, nq) for name in ("commuting", "pure_mixed", "orthogonal") for nq in (4, 5)]


@pytest.mark.parametrize("name,nq", EXACT_CASES)
def test_exact_families(gpu, name, nq):
    rho, sigma, exact = cc.family(name, nq, 8 if nq <= 3 else 3)
    for tol in (1e-4, 1e-10):
        qcb, s, lower, iters = run(rho, sigma, tol=tol)
        sandwich(exact, exact, qcb, lower, (name, nq, tol))
        share = gap_rule(qcb, lower, iters, tol, (name, nq, tol))
        if tol == 1e-10:
            assert share >= CERTIFIED_FLOOR, (name, nq, share, iters)
        assert np.all((s >= 0) & (s <= 1))
    if name == "pure_mixed":
        assert np.all(s == 0.0)                                     # the minimum sits at the endpoint


def test_pure_rho_mixed_sigma_against_the_host_function(gpu):
    """<psi|sigma|psi> at s = 0: the device within rounding; the host function's miss is measured and reported."""
    from fbx import distance_measures as dm
    misses = []
    for nq in (1, 2, 3):
        rho, sigma, exact = cc.family("pure_mixed", nq, 8)
        qcb, s, lower, iters = run(rho, sigma)
        assert np.all(np.abs(qcb - exact) <= RT * exact), nq
        for b in range(len(exact)):
            q, _ = dm.quantum_chernoff_bound(rho[b], sigma[b])
            misses.append(abs(float(q) - exact[b]) / exact[b])
    print(f"host quantum_chernoff_bound on pure rho / mixed sigma: relative miss max {max(misses):.2e}, "
          f"median {np.median(misses):.2e}")


def test_trivial_answers_stop_at_once(gpu):
    """orthogonal supports in a common eigenbasis: Q = 0 exactly, both bounds 0 with no search; rho = sigma: 1"""
    for nq in (1, 2, 3, 4, 5):
        d = 2 ** nq
        a = np.zeros(d)
        b = np.zeros(d)
        a[: d // 2] = 2.0 / d
        b[d // 2:] = 2.0 / d
        qcb, s, lower, iters = run(np.diag(a).astype(complex), np.diag(b).astype(complex))
        assert qcb[0] == 0.0 and lower[0] == 0.0 and iters[0] == 0, nq
        rho, _, _ = cc.family("identical", min(nq, 3), 1)
        x = np.eye(d, dtype=complex) / d if nq > 3 else rho[0]
        qcb, s, lower, iters = run(x, x)
        assert abs(qcb[0] - 1.0) <= RT and lower[0] <= 1.0 + RT and iters[0] >= 0, nq


@pytest.mark.parametrize("nq", [1, 2, 3, 4, 5])
def test_golden_brackets(gpu, nq):
    g = np.load(GOLDEN)
    rho, sigma, lo, hi = g[f"q{nq}_rho"], g[f"q{nq}_sigma"], g[f"q{nq}_lo"], g[f"q{nq}_hi"]
    for tol in (1e-4, 1e-10, 1e-13):
        qcb, s, lower, iters = run(rho, sigma, tol=tol)
        sandwich(lo, hi, qcb, lower, (nq, tol))
        share = gap_rule(qcb, lower, iters, tol, (nq, tol))
        if tol == 1e-10:
            assert share >= CERTIFIED_FLOOR, (nq, share, iters)
            assert np.all(np.abs(s - g[f"q{nq}_s"]) <= 1e-4), (nq, s, g[f"q{nq}_s"])
    qcb, s, lower, iters = run(rho, sigma, max_iters=0)
    sandwich(lo, hi, qcb, lower, (nq, "max_iters=0"))
    assert np.all(np.abs(iters) <= 1) and np.all(np.isin(s, (0.0, 1.0)))


def host_endpoints(rho, sigma):
    """Q and Q' at s = 0 and 1 in float64 (numpy's eigh, every eigenvalue above 1e-12 lambda_max kept)"""
    a, v = np.linalg.eigh(rho)
    b, w = np.linalg.eigh(sigma)
    ka, kb = a > 1e-12 * a.max(), b > 1e-12 * b.max()
    a, v, b, w = a[ka], v[:, ka], b[kb], w[:, kb]
    o = np.abs(v.conj().T @ w) ** 2
    g = np.log(a)[:, None] - np.log(b)[None, :]
    q0, q1 = (o * b[None, :]).sum(), (o * a[:, None]).sum()
    return q0, (o * b[None, :] * g).sum(), q1, (o * a[:, None] * g).sum()


@pytest.mark.parametrize("nq", [1, 2, 3, 4])
def test_endpoint_tangents_at_max_iters_zero(gpu, nq):
    """With no search the lower bound is the best combination of the two endpoint tangents: where the slopes have opposite
    signs, the height of their intersection (to the rounding shift)."""
    g = np.load(GOLDEN)
    rho, sigma = g[f"q{nq}_rho"], g[f"q{nq}_sigma"]
    qcb, s, lower, iters = run(rho, sigma, max_iters=0)
    checked = 0
    for b in range(len(rho)):
        q0, d0, q1, d1 = host_endpoints(rho[b], sigma[b])
        assert abs(qcb[b] - min(q0, q1)) <= 1e-12 * qcb[b]
        if d0 < -1e-6 and d1 > 1e-6:
            t = (q1 - d1 - q0) / (d0 - d1)
            want = q0 + d0 * t
            assert abs(lower[b] - want) <= 1e-10 * qcb[b], (b, lower[b], want)
            checked += 1
    assert checked >= 1


def test_lower_bound_holds_exactly_on_diagonal_pairs(gpu):
    """Diagonal pairs: the eigensolver is exact, so the only error is the rounding of the search itself, and the shifted
    lower bound must not exceed the exact minimum (mpmath) by a single ulp."""
    rng = np.random.default_rng(37)
    for nq in (1, 2, 3):
        d = 2 ** nq
        a = np.array([cc.random_spectrum(d, rng) for _ in range(24)])
        b = np.array([cc.random_spectrum(d, rng) for _ in range(24)])
        rho = np.array([np.diag(x) for x in a]).astype(complex)
        sigma = np.array([np.diag(x) for x in b]).astype(complex)
        qcb, s, lower, iters = run(rho, sigma, tol=1e-14, max_iters=200)
        for k in range(24):
            value, _ = cc.commuting_min(a[k], b[k])
            hi = np.nextafter(float(value), np.inf)
            assert lower[k] <= hi, (nq, k, lower[k], float(value))
            assert abs(qcb[k] - float(value)) <= 1e-13 * qcb[k], (nq, k)


# ------------------------------------------------------------------------------------------------ inequalities
@pytest.mark.parametrize("nq", [1, 2, 3])
def test_trace_distance_and_fidelity_inequalities(gpu, nq):
    """1 - T <= qcb <= sqrt(F): T the trace distance (Schatten 1-norm on the host), F from the state-measures kernel"""
    from fbx import distance_measures as dm
    rho, sigma = random_pairs(nq, 30, 7)
    qcb, s, lower, iters = run(rho, sigma)
    t = 0.5 * np.abs(np.linalg.eigvalsh(rho - sigma)).sum(axis=1)
    assert np.all(1 - t <= qcb * (1 + RT) + AT), np.max(1 - t - qcb)
    f = dm.state_measures_batch(rho, sigma, ("fidelity",))["fidelity"]
    assert np.all(lower <= np.sqrt(f) * (1 + RT) + AT), np.max(lower - np.sqrt(f))


# ------------------------------------------------------------------------------------------------ invariances
@pytest.mark.parametrize("nq", [1, 2, 3, 4])
def test_joint_unitary_and_swap(gpu, nq):
    rho, sigma = random_pairs(nq, 9, 11)
    base = run(rho, sigma, tol=1e-13)
    u = cc.random_unitary(2 ** nq, np.random.default_rng([3, nq]))
    rot = run(u @ rho @ u.conj().T, u @ sigma @ u.conj().T, tol=1e-13)
    overlap(base, rot, (nq, "unitary"))
    sw = run(sigma, rho, tol=1e-13)
    overlap(base, sw, (nq, "swap"))
    inner = (base[1] > 1e-3) & (base[1] < 1 - 1e-3)                 # a unique interior minimum: full-rank / nearly commuting pairs
    assert inner.sum() >= 3
    assert np.all(np.abs(base[1][inner] - (1 - sw[1][inner])) <= 1e-6), (base[1], sw[1])


@pytest.mark.parametrize("nq", [1, 2, 3])
def test_tensoring_with_a_common_state(gpu, nq):
    """Q(rho (x) tau, sigma (x) tau) = Q(rho, sigma) tr tau: crosses 1 -> 2, 2 -> 3 and 3 -> 4 qubits (fused against composed)"""
    rho, sigma = random_pairs(nq, 6, 13)
    tau = cc.random_state(2, np.random.default_rng([17, nq]))
    base = run(rho, sigma)
    big = run(np.array([np.kron(r, tau) for r in rho]), np.array([np.kron(x, tau) for x in sigma]))
    overlap(base, big, nq)


@pytest.mark.parametrize("nq", [1, 3, 4])
def test_power_of_two_scaling(gpu, nq):
    rho, sigma = random_pairs(nq, 6, 19)
    base = run(rho, sigma)
    for k in (-3, 5):
        q, s, lo, it = run(rho * 2.0 ** k, sigma * 2.0 ** k)
        overlap(base, (q / 2.0 ** k, s, lo / 2.0 ** k, it), (nq, k))


# ------------------------------------------------------------------------------------------------ parity
def test_reference_recorded_values(gpu):
    """the reference's qcb / argmin on the pairs of tests/golden/extras.npz, with the host function's support rule (zero_tol 0)"""
    g = np.load(EXTRAS)
    for d in (2, 4):
        want = g[f"qcb{d}"]
        qcb, s, lower, iters = run(g[f"qcb{d}_rho"], g[f"qcb{d}_sigma"], zero_tol=0.0)
        assert np.all(qcb <= want[:, 0] + 1e-12) and np.all(qcb >= want[:, 0] - 1e-9), (qcb, want[:, 0])
        assert np.all(np.abs(s - want[:, 1]) <= 1e-4), (s, want[:, 1])


@pytest.mark.parametrize("nq", [1, 2, 3])
def test_host_function_parity(gpu, nq):
    from fbx import distance_measures as dm
    rng = np.random.default_rng([23, nq])
    d = 2 ** nq
    rho = np.array([cc.random_state(d, rng) for _ in range(6)])
    sigma = np.array([cc.random_state(d, rng) for _ in range(6)])
    qcb, s, lower, iters = run(rho, sigma, zero_tol=0.0)
    for b in range(6):
        q, x = dm.quantum_chernoff_bound(rho[b], sigma[b])
        assert qcb[b] <= float(q) + 1e-12 and qcb[b] >= float(q) - 1e-9, (b, qcb[b], q)
        assert abs(s[b] - float(x)) <= 1e-4, (b, s[b], x)


# ------------------------------------------------------------------------------------------------ batch geometry
def mixed_batch(nq, count, seed=29):
    rho, sigma = random_pairs(nq, count, seed)
    pr, ps, _ = cc.family("pure_mixed", nq, 2)
    return np.concatenate([rho, pr]), np.concatenate([sigma, ps])


@pytest.mark.parametrize("nq", [1, 2, 3, 4, 5])
def test_alone_in_batch_and_shared_are_bitwise_equal(gpu, nq):
    rho, sigma = mixed_batch(nq, 6)
    n = len(rho)
    reps = 4100 // n + 1 if nq == 4 else 3            # 4 qubits: past the composed path's 4096-pair pass
    big = run(np.tile(rho, (reps, 1, 1)), np.tile(sigma, (reps, 1, 1)))
    for b in range(n):
        alone = run(rho[b], sigma[b][None])
        for k, name in enumerate(("qcb", "s", "lower", "iters")):
            col = big[k].reshape(reps, n)[:, b]
            assert np.all(col == alone[k][0]), (nq, b, name)
    shared = run(rho, sigma[2])
    tiled = run(rho, np.broadcast_to(sigma[2], rho.shape))
    for a, c in zip(shared, tiled):
        assert np.array_equal(a, c), nq
    # the lower triangle is what is read
    low = run(np.tril(rho) + np.triu(np.full_like(rho, 7 + 3j), 1), sigma)
    for a, c in zip(low, run(rho, sigma)):
        assert np.array_equal(a, c), nq


def test_one_qubit_batch_past_the_grid_cap(gpu):
    """2^20 + 64 one-qubit pairs: the wavefronts stride over the batch; items past the cap equal one-item calls.  Seven distinct
    pairs, so that a wavefront's second item differs from its first."""
    rho, sigma = mixed_batch(1, 5)
    n = len(rho)
    B = (1 << 20) + 64
    idx = np.arange(B) % n
    qcb, s, lower, iters = run(rho[idx], sigma[idx])
    for b in range(n):
        alone = run(rho[b], sigma[b][None])
        for k, arr in enumerate((qcb, s, lower, iters)):
            assert np.all(arr[idx == b] == alone[k][0]), (b, k)


@pytest.mark.parametrize("nq", [2, 4])
def test_device_entry_with_offset_pointers(gpu, nq):
    from fbx import _lib
    d = 2 ** nq
    B, off = 5, 3
    rho, sigma = mixed_batch(nq, B + off - 2)
    want = run(rho[off:], sigma[off:])
    lib, DB = _lib.lib(), _lib.DeviceBuffer
    dr, ds = DB.from_array(rho.view(np.float64)), DB.from_array(sigma.view(np.float64))
    n = B + off
    dq, dl, dsv, di = DB(n * 8), DB(n * 8), DB(n * 8), DB(n * 4)
    at = lambda buf, k, size: ctypes.c_void_p(buf.ptr.value + k * size)  # noqa: E731
    _lib.check(lib.fbx_chernoff_bound_dev(nq, B, at(dr, off, d * d * 16), at(ds, off, d * d * 16), 0, 1e-10, 100, 1e-12,
                                          at(dq, off, 8), at(dl, off, 8), at(dsv, off, 8), at(di, off, 4)))
    _lib.synchronize()
    got = (dq.to_array(np.float64, (n,))[off:], dsv.to_array(np.float64, (n,))[off:], dl.to_array(np.float64, (n,))[off:],
           di.to_array(np.int32, (n,))[off:])
    for name, a, b in zip(("qcb", "s", "lower", "iters"), got, want):
        assert np.array_equal(a, b), name


@pytest.mark.parametrize("nq", [1, 3, 4])
def test_non_finite_item_is_isolated(gpu, nq):
    rho, sigma = mixed_batch(nq, 6)
    want = run(rho, sigma)
    bad_r = rho.copy()
    bad_r[3, 1, 0] = np.nan
    got = run(bad_r, sigma)
    keep = np.arange(len(rho)) != 3
    for a, b in zip(got, want):
        assert np.array_equal(a[keep], b[keep]), nq
    assert np.isnan(got[0][3]) and np.isnan(got[1][3]) and np.isnan(got[2][3]) and got[3][3] < 0
    bad_s = sigma[0].copy()
    bad_s[0, 0] = np.inf
    got = run(rho, bad_s)
    assert np.all(np.isnan(got[0])) and np.all(got[3] < 0)


def test_argument_errors(gpu):
    import fbx
    from fbx import _lib, distance_measures as dm
    lib = _lib.lib()
    x = np.eye(2, dtype=complex).view(np.float64)
    out = np.zeros(1)
    for nq in (0, 6):
        assert lib.fbx_chernoff_bound(nq, 1, _lib.dptr(x), _lib.dptr(x), 0, 0.0, 10, 0.0, _lib.dptr(out), None, None,
                                      None) == _lib.FBX_ERR_UNSUPPORTED
    assert lib.fbx_chernoff_bound(1, 1, None, _lib.dptr(x), 0, 0.0, 10, 0.0, _lib.dptr(out), None, None, None) == \
        _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_chernoff_bound(1, 1, _lib.dptr(x), _lib.dptr(x), 0, 0.0, 10, 0.0, None, None, None, None) == \
        _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_chernoff_bound(1, -1, _lib.dptr(x), _lib.dptr(x), 0, 0.0, 10, 0.0, _lib.dptr(out), None, None, None) == \
        _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_chernoff_bound(1, 1, _lib.dptr(x), _lib.dptr(x), 0, 0.0, -1, 0.0, _lib.dptr(out), None, None, None) == \
        _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_chernoff_bound(1, 1, _lib.dptr(x), _lib.dptr(x), 0, 0.0, 10, 1.0, _lib.dptr(out), None, None, None) == \
        _lib.FBX_ERR_BAD_ARG
    with pytest.raises(ValueError):
        dm.quantum_chernoff_bound_batch(np.eye(3), np.eye(3))
    with pytest.raises(ValueError):
        dm.quantum_chernoff_bound_batch(np.zeros((2, 2, 2)), np.zeros((3, 2, 2)))
    with pytest.raises(ValueError):
        dm.quantum_chernoff_bound_batch(np.zeros((2, 2, 3)), np.zeros((2, 2)))
    with pytest.raises(fbx.FbxError):
        dm.quantum_chernoff_bound_batch(np.eye(64), np.eye(64))
    q, s = dm.quantum_chernoff_bound_batch(np.zeros((0, 2, 2)), np.eye(2))
    assert q.shape == (0,) and s.shape == (0,)


# ------------------------------------------------------------------------------------------------ bootstrap
@pytest.mark.parametrize("estimator,project", [("mle", True), ("linv", False)])
def test_bootstrap_is_the_hand_composition(gpu, estimator, project):
    from fbx import distance_measures as dm, synthetic, tomography
    from fbx.operator_tools.project_state_matrix import project_state_matrix_to_physical_batch
    design, _, e, c = synthetic.state_batch(2, 3, mixed=0.05)
    R, B, m = 6, 3, design.m
    target = cc.random_state(4, np.random.default_rng(31))
    mean, var, q = tomography.state_chernoff_variance_batch(design, e, c, target, n_resamples=R, seed=5, estimator=estimator,
                                                            project_to_physical=project, return_samples=True)
    e_rs = tomography.resample_expectations_with_beta_batch(e, c, R, seed=5).reshape(R * B, m)
    c_rs = np.ascontiguousarray(np.broadcast_to(c, (R, B, m))).reshape(R * B, m)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if estimator == "mle":
            rhos = tomography.iterative_mle_state_estimate_batch(design, e_rs, c_rs)
        else:
            rhos = tomography.linear_inv_state_estimate_batch(design, e_rs)
    if project:
        rhos = project_state_matrix_to_physical_batch(rhos)
    want, _ = dm.quantum_chernoff_bound_batch(rhos, target)
    assert np.array_equal(q, want.reshape(R, B))
    assert np.array_equal(mean, q.mean(axis=0)) and np.array_equal(var, q.var(axis=0))
    assert np.all((q > 0) & (q <= 1 + 1e-9))
