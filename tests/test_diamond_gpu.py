"""Batched diamond-norm distance on the device (fbx_diamond_norm, distance_measures.diamond_norm_distance_batch) against the
reference's known answers, the host solver (distance_measures.diamond_norm_distance) and its own certificate."""
import numpy as np
import pytest
from scipy.linalg import expm, fractional_matrix_power as matpow

pytestmark = pytest.mark.gpu

X = np.array([[0, 1], [1, 0]], dtype=complex)
Y = np.array([[0, -1j], [1j, 0]])
Z = np.diag([1.0 + 0j, -1.0])
I2 = np.eye(2, dtype=complex)
H = np.array([[1, 1], [1, -1]], dtype=complex) / np.sqrt(2)


def kraus2choi(ks):
    ks = [ks] if np.ndim(ks) == 2 else ks
    out = 0
    for k in ks:
        v = np.asarray(k).reshape(-1, 1, order="F")
        out = out + v @ v.conj().T
    return out


def superop2choi(sop, d=2):
    return sop.reshape([d] * 4).swapaxes(0, 3).reshape(d * d, d * d)


def random_channel(d, rank, rs):
    g = rs.randn(d * rank, d) + 1j * rs.randn(d * rank, d)
    q, _ = np.linalg.qr(g)
    return kraus2choi([q[j * d:(j + 1) * d] for j in range(rank)])


def near_unitary(d, rs, scale=1e-2):
    h = rs.randn(d, d) + 1j * rs.randn(d, d)
    u = expm(-1j * scale * (h + h.conj().T))
    p = scale * rs.rand()
    return (1 - p) * kraus2choi(u) + p * np.eye(d * d) / d


def host_g2(choi0, choi1, rho):
    """2 g(rho) = 2 tr[((1 (x) rho^1/2) J (1 (x) rho^1/2))_+] on the host."""
    delta = choi0 - choi1
    J = (delta + delta.conj().T) / 2
    w, v = np.linalg.eigh((rho + rho.conj().T) / 2)
    s = (v * np.sqrt(np.clip(w, 0, None))) @ v.conj().T
    S = np.kron(np.eye(rho.shape[0]), s)
    lam = np.linalg.eigvalsh(S @ J @ S)
    return 2 * lam[lam > 0].sum()


def pairs(nq, count, seed):
    rs = np.random.RandomState(seed)
    d = 2 ** nq
    out = []
    for i in range(count):
        if i % 2 == 0:
            out.append((random_channel(d, 1 + i % 3, rs), random_channel(d, 2, rs)))
        else:
            out.append((near_unitary(d, rs), kraus2choi(np.eye(d))))
    return np.array([a for a, _ in out]), np.array([b for _, b in out])


def test_reference_known_answers(gpu):
    from fbx import distance_measures as dm
    cases = [(kraus2choi(I2), kraus2choi(X), 2.0, 1e-6)]
    for turns, target in [[1e-3, 3.141591e-3], [3.1e-3, 9.738899e-3], [1e-2, 3.141463e-2], [3.1e-2, 9.735089e-2],
                          [1e-1, 3.128689e-1], [3.1e-1, 9.358596e-1]]:
        cases.append((kraus2choi(X), kraus2choi(matpow(X, 1 + turns)), target, 1e-5))
    for p, target in [[1e-3, 2e-3], [3.1e-3, 6.2e-3], [1e-2, 2e-2], [3.1e-2, 6.2e-2], [1e-1, 2e-1], [3.1e-1, 6.2e-1]]:
        c0 = superop2choi(np.kron(I2.conj(), I2) * (1 - p) + np.kron(H.conj(), H) * p)
        cases.append((c0, superop2choi(np.kron(I2.conj(), I2)), target, 1e-6))
    cases.append((kraus2choi(I2), kraus2choi(matpow(Y, 0.5)), np.sqrt(2), 1e-6))
    cases.append((kraus2choi(I2), kraus2choi(expm(-0.2j * X)), 0.3973386615692544, 1e-6))
    c0 = np.array([c[0] for c in cases])
    c1 = np.array([c[1] for c in cases])
    got, upper, iters = dm.diamond_norm_distance_batch(c0, c1, return_bounds=True)
    for (_, _, want, rtol), g, u in zip(cases, got, upper):
        assert np.isclose(g, want, rtol=rtol), (g, want)
        assert u >= g
    # closed forms to 1e-9
    assert abs(got[0] - 2.0) < 1e-9
    assert abs(got[-2] - np.sqrt(2)) < 1e-9
    for k, p in enumerate([1e-3, 3.1e-3, 1e-2, 3.1e-2, 1e-1, 3.1e-1]):
        assert abs(got[7 + k] - 2 * p) < 1e-9
    theta = 0.3
    u2 = expm(-1j * theta * np.kron(Z, Z))
    d2 = dm.diamond_norm_distance_batch(kraus2choi(np.eye(4, dtype=complex)), kraus2choi(u2))
    assert abs(d2[0] - 2 * np.sin(theta)) < 1e-9
    same = dm.diamond_norm_distance_batch(kraus2choi(H), kraus2choi(H))
    assert abs(same[0]) < 1e-9


@pytest.mark.parametrize("nq,count", [(1, 12), (2, 12), (3, 8)])
def test_against_the_host_solver(gpu, nq, count):
    from fbx import distance_measures as dm
    c0, c1 = pairs(nq, count, seed=10 + nq)
    tol = 1e-7
    dist, upper, iters, rho = dm.diamond_norm_distance_batch(c0, c1, tol=tol, return_bounds=True, return_inputs=True)
    rs = np.random.RandomState(5)
    d = 2 ** nq
    for b in range(count):
        host = dm.diamond_norm_distance(c0[b], c1[b])
        assert dist[b] >= host - 1e-9 * max(1.0, host), (b, dist[b], host)
        assert upper[b] >= host - 1e-12 * max(1.0, host), (b, upper[b], host)
        for _ in range(3):                                   # the certificate bounds 2 g of any input state
            g = rs.randn(d, d) + 1j * rs.randn(d, d)
            r = g @ g.conj().T
            assert upper[b] >= host_g2(c0[b], c1[b], r / np.trace(r).real) - 1e-12
        if iters[b] >= 0:
            assert upper[b] - dist[b] <= tol * max(dist[b], 1e-12)
        # the returned input state
        w = np.linalg.eigvalsh((rho[b] + rho[b].conj().T) / 2)
        assert w.min() > -1e-12 and abs(np.trace(rho[b]) - 1) < 1e-12
        assert abs(host_g2(c0[b], c1[b], rho[b]) - dist[b]) < 1e-10
    assert (iters >= 0).mean() >= 0.75, iters


def test_plumbing(gpu):
    from fbx import distance_measures as dm
    c0, c1 = pairs(2, 1000, seed=21)
    tgt = kraus2choi(np.eye(4))
    shared = dm.diamond_norm_distance_batch(c0[:64], tgt)
    explicit = dm.diamond_norm_distance_batch(c0[:64], np.broadcast_to(tgt, (64, 16, 16)))
    assert np.array_equal(shared, explicit)
    full, up_full, it_full = dm.diamond_norm_distance_batch(c0, c1, return_bounds=True)
    for b in (0, 1, 517, 999):
        alone, up, it = dm.diamond_norm_distance_batch(c0[b:b + 1], c1[b:b + 1], return_bounds=True)
        assert alone[0] == full[b] and up[0] == up_full[b] and it[0] == it_full[b]
    # d(a, b) = d(b, a) holds for unital pairs (the odd items): like the reference, the input state acts on the SECOND tensor
    # factor of the Choi matrix, and for non-unital pairs that quantity is neither symmetric nor bounded by 2
    ab = dm.diamond_norm_distance_batch(c0[1:32:2], c1[1:32:2])
    ba = dm.diamond_norm_distance_batch(c1[1:32:2], c0[1:32:2])
    assert np.all(np.abs(ab - ba) <= 1e-7 * np.maximum(ab, 1e-12) + 1e-12)
    bad = c0[:8].copy()
    bad[3, 2, 5] = np.nan
    got = dm.diamond_norm_distance_batch(bad, c1[:8])
    assert np.isnan(got[3])
    keep = [0, 1, 2, 4, 5, 6, 7]
    assert np.array_equal(got[keep], full[keep])
    with pytest.raises(ValueError):
        dm.diamond_norm_distance_batch(c0[:2, :15, :15], c1[:2, :15, :15])
    with pytest.raises(ValueError):
        dm.diamond_norm_distance_batch(c0[:2], c1[:3])
    with pytest.raises(Exception):                           # 4 qubits: FBX_ERR_UNSUPPORTED
        dm.diamond_norm_distance_batch(np.eye(256)[None], np.eye(256))


def test_bootstrap_is_the_hand_composition(gpu):
    from fbx import _lib, distance_measures as dm, synthetic, tomography
    design, _, e, c = synthetic.process_batch(1, "pauli", 3)
    target = kraus2choi(I2)
    R, seed = 5, 11
    mean, var, samples = tomography.process_diamond_distance_variance_batch(design, e, c, target, n_resamples=R, seed=seed,
                                                                             return_samples=True)
    B, m = e.shape[0], design.m
    lib, DB = _lib.lib(), _lib.DeviceBuffer
    d_e, d_c = DB.from_array(np.ascontiguousarray(e, dtype=np.float64)), DB.from_array(np.ascontiguousarray(c, dtype=np.float64))
    d_er, d_cr = DB(R * B * m * 8), DB(R * B * m * 8)
    _lib.check(lib.fbx_beta_resample_dev(B * m, R, d_e.ptr, d_c.ptr, 1.0, seed, d_er.ptr, d_cr.ptr))
    er = d_er.to_array(np.float64, (R * B, m))
    cr = d_cr.to_array(np.float64, (R * B, m))
    choi = tomography.pgdb_process_estimate_batch(design, er, cr)
    want = dm.diamond_norm_distance_batch(choi, target).reshape(R, B)
    assert np.array_equal(samples, want)
    point = dm.diamond_norm_distance_batch(tomography.pgdb_process_estimate_batch(design, e, c), target)
    assert np.all(np.abs(mean - point) < 5 * np.sqrt(var) + 0.05)
    assert np.all((samples >= 0) & (samples <= 2 + 1e-12))


def test_walkthrough_reports_the_diamond_distance(gpu):
    import importlib.util
    import os
    from fbx import distance_measures as dm
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "process_tomography_walkthrough.py")
    spec = importlib.util.spec_from_file_location("walkthrough_diamond", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main()
    v = out["diamond_norm_to_ideal"]
    assert 0.0 <= v <= 2.0
    assert abs(v - dm.diamond_norm_distance(out["choi_estimate"], out["choi_ideal"])) < 1e-7
    assert out["diamond_norm_to_ideal_std"] >= 0.0
