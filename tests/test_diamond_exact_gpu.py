"""fbx_diamond_norm against exact and high-precision answers: the closed forms of tests/diamond_cases.py, the mpmath brackets
[L, U] of tests/golden/diamond_exact.npz (make_diamond_goldens.py), invariances of the quantity at 3 qubits, and the batch
geometry of both launch paths (the 1-2-qubit grid cap of 2^20 items, the 512 resident 3-qubit workgroups that stride over the
batch).  The promise checked is the one of include/fbx.h: dist is a lower bound, upper an upper bound, for every item whether
certified or not, and certified items are within tol.  The slack is at the rounding level, never tol."""
import ctypes
import os

import numpy as np
import pytest

import diamond_cases as dc

pytestmark = pytest.mark.gpu

RT, AT = 1e-12, 1e-15                 # rounding slack: relative, absolute
TOLS = [1e-3, 1e-7, 1e-10]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diamond_exact.npz")

# floors on the share of certified items (iters >= 0) at tol = 1e-7 per (family, qubits).  Measured on an MI355X: every closed-form
# family at 1, 2 and 3 qubits 1.000; the golden pairs 15 / 16 (the amplitude-damping pair stops uncertified), 13 / 13 and 5 / 5.
# A certificate that is valid but loose (a wrong tensor factor for S, a shorter eps scan) leaves these at 0.0-0.4.
CERTIFIED_FLOOR = {(name, nq): 1.0 for name in ("unitary", "pauli", "depolarizing", "replacement", "mixture", "golden")
                   for nq in (1, 2, 3)}
CERTIFIED_FLOOR[("golden", 1)] = 0.93


def run(c0, c1, tol=1e-7, max_iters=200):
    from fbx import distance_measures as dm
    return dm.diamond_norm_distance_batch(c0, c1, tol=tol, max_iters=max_iters, return_bounds=True, return_inputs=True)


def host_g2(choi0, choi1, rho):
    """2 g(rho) = 2 tr[((1 (x) rho^1/2) J (1 (x) rho^1/2))_+] on the host (float64; J is formed as the kernel forms it)."""
    delta = choi0 - choi1
    J = (delta + delta.conj().T) / 2
    w, v = np.linalg.eigh((rho + rho.conj().T) / 2)
    s = (v * np.sqrt(np.clip(w, 0, None))) @ v.conj().T
    S = np.kron(np.eye(rho.shape[0]), s)
    lam = np.linalg.eigvalsh(S @ J @ S)
    return 2 * lam[lam > 0].sum()


def check_state(c0, c1, dist, rho, where):
    d = rho.shape[-1]
    for b in range(len(dist)):
        r = rho[b]
        assert np.abs(r - r.conj().T).max() <= 1e-15, (where, b)
        assert np.linalg.eigvalsh((r + r.conj().T) / 2).min() >= -1e-15 and abs(np.trace(r) - 1) <= 1e-13 * d, (where, b)
        g2 = host_g2(c0[b], c1[b], r)
        assert abs(g2 - dist[b]) <= RT * dist[b] + AT, (where, b, g2, dist[b])


def sandwich(lo, hi, dist, upper, where):
    """lo <= value <= hi known; dist must not exceed hi, upper must not fall below lo (to rounding)."""
    assert np.all(dist <= hi * (1 + RT) + AT), (where, np.max(dist - hi))
    assert np.all(upper >= lo * (1 - RT) - AT), (where, np.min(upper - lo))
    assert np.all(upper >= dist), where


def closed_form_batch(nq):
    fam = dc.families(nq)
    names, c0, c1, ex = [], [], [], []
    for name, cases in fam.items():
        for a, b, e in cases:
            names.append(name); c0.append(a); c1.append(b); ex.append(e)
    return np.array(names), np.array(c0), np.array(c1), np.array(ex)


def share_report(tag, names, iters):
    out = {n: float((iters[names == n] >= 0).mean()) for n in dict.fromkeys(names)}
    print(f"\ncertified share {tag}: " + ", ".join(f"{k} {v:.3f}" for k, v in out.items()))
    return out


# ------------------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("nq", [1, 2, 3])
def test_closed_forms(gpu, nq):
    names, c0, c1, exact = closed_form_batch(nq)
    for tol in TOLS:
        dist, upper, iters, rho = run(c0, c1, tol=tol)
        where = f"{nq}q tol={tol}"
        sandwich(exact, exact, dist, upper, where)
        cert = iters >= 0
        slack = tol * np.maximum(exact, 1e-12) + RT * exact + AT
        assert np.all((upper - exact)[cert] <= slack[cert]), (where, names[cert][np.argmax((upper - exact - slack)[cert])])
        check_state(c0, c1, dist, rho, where)
        d = 2 ** nq
        for b in np.flatnonzero(names == "replacement"):    # the returned state is close to the top eigenvector of sigma - tau:
            sigma, tau = c0[b][:d, :d], c1[b][:d, :d]       # dist / 2d <= lam_1 - (lam_1 - max(lam_2, 0)) (1 - F)
            lam = np.linalg.eigvalsh(sigma - tau)
            fid = np.real(np.trace(dc.replacement_top_state(sigma, tau) @ rho[b]))
            bound = (exact[b] - dist[b]) / (2 * d * (lam[-1] - max(lam[-2], 0.0)))
            assert 1 - fid <= bound + 1e-12, (where, b, fid, bound)
        if tol == 1e-7:
            share = share_report(where, names, iters)
            for n, v in share.items():
                assert v >= CERTIFIED_FLOOR[(n, nq)], (where, n, v)
        exact_start = (names == "pauli") | (names == "depolarizing")
        assert np.all(iters[exact_start] == 0), (where, iters[exact_start])


@pytest.mark.parametrize("nq", [1, 2, 3])
def test_no_steps_still_bounds(gpu, nq):
    """max_iters = 0: the certificate at rho = 1/d and the eps scan only.  The bounds still hold; Pauli channels are exact at
    rho = 1/d, so they are certified with zero steps."""
    names, c0, c1, exact = closed_form_batch(nq)
    dist, upper, iters, rho = run(c0, c1, tol=1e-7, max_iters=0)
    where = f"{nq}q max_iters=0"
    sandwich(exact, exact, dist, upper, where)
    assert np.all((iters == 0) | (iters == -1)), iters
    exact_start = (names == "pauli") | (names == "depolarizing")
    assert np.all(iters[exact_start] == 0), iters[exact_start]
    assert np.all(np.abs(dist - exact)[exact_start] <= RT * exact[exact_start] + AT)
    gap = (upper - exact)[iters == 0]
    assert np.all(gap <= 1e-7 * np.maximum(exact[iters == 0], 1e-12) + RT * exact[iters == 0] + AT)
    check_state(c0, c1, dist, rho, where)


# ------------------------------------------------------------------------------------------------ high-precision brackets
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("nq", [1, 2, 3])
def test_golden_brackets(gpu, golden, nq):
    p = f"q{nq}_"
    c0, c1, L, U = golden[p + "choi0"], golden[p + "choi1"], golden[p + "lower"], golden[p + "upper"]
    names = golden[p + "family"]
    assert len(L) >= (4 if nq == 3 else 12)
    for tol in TOLS + [None]:
        dist, upper, iters, rho = run(c0, c1, tol=tol or 1e-7, max_iters=0 if tol is None else 200)
        where = f"golden {nq}q tol={tol}"
        sandwich(L, U, dist, upper, where)
        cert = iters >= 0
        t = tol or 1e-7
        slack = t * np.maximum(L, 1e-12) + (U - L) + RT * U + AT
        assert np.all((upper - L)[cert] <= slack[cert]), (where, names[cert][np.argmax((upper - L - slack)[cert])])
        check_state(c0, c1, dist, rho, where)
        if tol == 1e-7:
            share = float(cert.mean())
            print(f"\ncertified share {where}: {share:.3f} ({', '.join(names[~cert])})")
            assert share >= CERTIFIED_FLOOR[("golden", nq)], (where, share, names[~cert])


# ------------------------------------------------------------------------------------------------ invariances
def random_pairs(nq, count, seed):
    rs = np.random.RandomState(seed)
    d = 2 ** nq

    def channel(rank):
        g = rs.randn(d * rank, d) + 1j * rs.randn(d * rank, d)
        q, _ = np.linalg.qr(g)
        return dc.kraus2choi([q[j * d:(j + 1) * d] for j in range(rank)])
    c0 = np.array([channel(1 + i % 4) for i in range(count)])
    c1 = np.array([channel(1 + (i + 2) % 4) for i in range(count)])
    return c0, c1, rs


def overlap(a, b, where):
    (d0, u0), (d1, u1) = a, b
    lo, hi = np.maximum(d0, d1), np.minimum(u0, u1)
    assert np.all(lo <= hi * (1 + RT) + AT), (where, np.max(lo - hi))


@pytest.mark.parametrize("nq", [2, 3])
def test_invariances(gpu, nq):
    count = 6 if nq == 3 else 12
    c0, c1, rs = random_pairs(nq, count, seed=40 + nq)
    d = 2 ** nq
    base = run(c0, c1)
    ref = (base[0], base[1])
    # the same local unitary A (x) B on both Choi matrices
    ab = np.array([np.kron(dc.haar_unitary(d, rs), dc.haar_unitary(d, rs)) for _ in range(count)])
    conj = lambda c: ab @ c @ ab.conj().transpose(0, 2, 1)              # noqa: E731
    got = run(conj(c0), conj(c1))
    overlap(ref, (got[0], got[1]), f"{nq}q A(x)B")
    # an anti-Hermitian part on choi0 changes nothing (only the Hermitian part of the difference enters)
    k = rs.randn(count, d * d, d * d) + 1j * rs.randn(count, d * d, d * d)
    got = run(c0 + (k - k.conj().transpose(0, 2, 1)) / 4, c1)
    overlap(ref, (got[0], got[1]), f"{nq}q anti-Hermitian")
    # scaling both inputs by a power of two scales the quantity by it, bit for bit: the kernel's arithmetic is homogeneous (its
    # thresholds are relative) and no intermediate leaves the normal range at these scales
    for e in (-30, 20):
        s = 2.0 ** e
        got = run(c0 * s, c1 * s)
        overlap((ref[0] * s, ref[1] * s), (got[0], got[1]), f"{nq}q 2^{e}")
        assert np.array_equal(got[0], base[0] * s) and np.array_equal(got[1], base[1] * s), (nq, e)
        assert np.array_equal(got[2], base[2]) and np.array_equal(got[3], base[3]), (nq, e)


# ------------------------------------------------------------------------------------------------ batch geometry
def tiled(nq, B, shared):
    """B items made of a few distinct pairs: random channels, a unitary pair, a replacement pair; per-item or shared target."""
    d = 2 ** nq
    c0, c1, rs = random_pairs(nq, 3, seed=70 + nq)
    fam = dc.families(nq, seed=2)
    u = fam["unitary"][3]
    r = fam["replacement"][0]
    c0 = np.concatenate([c0, [u[0], r[0]]])
    c1 = np.concatenate([c1, [u[1], r[1]]])
    if shared:
        c1 = np.broadcast_to(dc.kraus2choi(np.eye(d)), c0.shape)
    idx = np.arange(B) % len(c0)
    return c0, c1, idx


def assert_tiles(c0, c1, idx, got, shared, where):
    from fbx import distance_measures as dm
    for k in range(len(c0)):
        tgt = c1[k] if shared else c1[k:k + 1]
        one = dm.diamond_norm_distance_batch(c0[k:k + 1], tgt, return_bounds=True, return_inputs=True)
        sel = idx == k
        for name, a, b in zip(("dist", "upper", "iters", "rho"), got, one):
            assert np.array_equal(a[sel], np.broadcast_to(b[0], a[sel].shape)), (where, k, name)


@pytest.mark.parametrize("shared", [False, True])
def test_strided_3q_batch_is_item_by_item(gpu, shared):
    """B = 2 * 512 + 37 at 3 qubits: every workgroup solves two or three items in turn in the same LDS and HBM work block."""
    from fbx import distance_measures as dm
    B = 2 * 512 + 37
    c0, c1, idx = tiled(3, B, shared)
    tgt = c1[0] if shared else c1[idx]
    got = dm.diamond_norm_distance_batch(c0[idx], tgt, return_bounds=True, return_inputs=True)
    assert_tiles(c0, c1, idx, got, shared, f"3q B={B} shared={shared}")


def test_past_the_grid_cap_1q(gpu):
    """B = 2^20 + 3 at 1 qubit with a shared target: the grid is capped at 2^20 workgroups, the last items are each a second
    item of a workgroup."""
    from fbx import distance_measures as dm
    B = (1 << 20) + 3
    c0, c1, idx = tiled(1, B, True)
    got = dm.diamond_norm_distance_batch(c0[idx], c1[0], return_bounds=True, return_inputs=True)
    assert_tiles(c0, c1, idx, got, True, f"1q B={B}")


@pytest.mark.parametrize("nq", [1, 3])
def test_non_finite_items(gpu, nq):
    from fbx import distance_measures as dm
    B = 9
    c0, c1, idx = tiled(nq, B, False)
    a0, a1 = c0[idx].copy(), c1[idx].copy()
    clean = dm.diamond_norm_distance_batch(a0, a1, return_bounds=True, return_inputs=True)
    a0[2, 1, 3] = np.nan
    a1[6, 0, 0] = np.inf
    got = dm.diamond_norm_distance_batch(a0, a1, return_bounds=True, return_inputs=True)
    bad = np.zeros(B, bool)
    bad[[2, 6]] = True
    assert np.all(np.isnan(got[0][bad])) and np.all(np.isnan(got[1][bad])) and np.all(got[2][bad] < 0)
    assert np.all(np.isnan(got[3][bad]))
    for a, b in zip(got, clean):
        assert np.array_equal(a[~bad], b[~bad])
    tgt = c1[0].copy()
    tgt[3, 2] = np.nan
    got = dm.diamond_norm_distance_batch(c0[idx], tgt, return_bounds=True, return_inputs=True)
    assert np.all(np.isnan(got[0])) and np.all(np.isnan(got[1])) and np.all(got[2] < 0) and np.all(np.isnan(got[3]))


@pytest.mark.parametrize("nq", [1, 3])
def test_device_entry_with_offset_pointers(gpu, nq):
    """fbx_diamond_norm_dev on sub-ranges of resident buffers (pointers offset by whole items) equals the host entry point."""
    from fbx import _lib, distance_measures as dm
    d = 2 ** nq
    D = d * d
    B, off = 7, 3
    c0, c1, idx = tiled(nq, B + off, False)
    a0 = np.ascontiguousarray(c0[idx]).view(np.float64)
    a1 = np.ascontiguousarray(c1[idx]).view(np.float64)
    want = dm.diamond_norm_distance_batch(c0[idx][off:], c1[idx][off:], return_bounds=True, return_inputs=True)
    lib, DB = _lib.lib(), _lib.DeviceBuffer
    d0, d1 = DB.from_array(a0), DB.from_array(a1)
    n = B + off
    dd, du, dr, di = DB(n * 8), DB(n * 8), DB(n * d * d * 16), DB(n * 4)
    at = lambda buf, k, size: ctypes.c_void_p(buf.ptr.value + k * size)  # noqa: E731
    _lib.check(lib.fbx_diamond_norm_dev(nq, B, at(d0, off, D * D * 16), at(d1, off, D * D * 16), 0, 1e-7, 200,
                                        at(dd, off, 8), at(du, off, 8), at(dr, off, d * d * 16), at(di, off, 4)))
    got = (dd.to_array(np.float64, (n,))[off:], du.to_array(np.float64, (n,))[off:],
           di.to_array(np.int32, (n,))[off:], dr.to_array(np.complex128, (n, d, d))[off:])
    for name, a, b in zip(("dist", "upper", "iters", "rho"), got, want):
        assert np.array_equal(a, b), name
    # shared target through the device entry
    _lib.check(lib.fbx_diamond_norm_dev(nq, B, at(d0, off, D * D * 16), at(d1, off, D * D * 16), 1, 1e-7, 200,
                                        at(dd, off, 8), None, None, None))
    want = dm.diamond_norm_distance_batch(c0[idx][off:], c1[idx][off])
    assert np.array_equal(dd.to_array(np.float64, (n,))[off:], want)
