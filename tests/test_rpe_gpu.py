"""fbx_rpe_phase / fbx_rpe_from_shots / fbx_circular_stats on the GPU: against the reference's phases, bloch data and stopping depths
(tests/golden/rpe_cases.npz), against answers that are known exactly, against the composed path on the same bits, and against a
numpy bootstrap.

Tolerance of a phase (TOL).  The recursion is performed operation for operation, so the device and the reference differ through
atan2 alone, and the phase is fixed modulo 2 pi / k by the LAST used iteration (k = 2^j): a deviation of A ulp in that atan2 moves
theta_j by at most A / k units of 2 pi 2^-53, and on each side the window arithmetic of that iteration rounds five times on values
below 8 (theta - pi / k; theta_j - low; the + width of the %; offset + low; the + 2 pi of the final %), at most 0.64 units each:
|phase_dev - phase_ref| <= (A / k + 7) 2 pi 2^-53.  The ROCm documentation installed next to the compiler states no ulp bound for
atan2, so A is not taken from it: as the issue prescribes for that case, the largest circular deviation from the reference over
the 200 golden sets was measured on an MI355X -- MEASURED_MAX = 8.88e-16 (4 ulp of a phase between 2 and 4; reached at K = 1 and
K = 2, 2.2e-16 at K = 5, 0 at K = 12) -- and TOL is 8 x that, 7.1e-15, to allow for rounding patterns the 200 sets do not hit; far
under the 1e-12 cap (a condition, not a measurement).  For comparison the formula with the 6 ulp that the OpenCL C specification
allows a double-precision atan2 gives 9.1e-15 at k = 1.  test_goldens prints the largest deviation it sees as an RPEDEV line.
depth_reached must match exactly.  The radius of a bloch row is a correctly rounded sqrt of a two-term sum on both sides (2 ulp are allowed); its angle is theta_est * k, so k TOL.

The stored sets, and every moment set generated here, keep each offset 1e-9 of the window's width away from the window's ends and
|r - r_std| >= 1e-9 r (asserted before the device is consulted): at those boundaries the estimator is discontinuous.  The sets of
test_from_shots keep the r margin only: their phases are compared between two device paths that run the same atan2 on the same
moments, so a window's end moves both alike, and only depth_reached -- which r < r_std alone decides -- is compared with numpy."""
import ctypes as C
import math
import os
import warnings

import numpy as np
import pytest

import rpe_cases as rc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rpe_cases.npz")
MEASURED_MAX = 8.881784197001252e-16      # largest circular deviation from the reference over the golden sets, on an MI355X
TOL = min(8 * MEASURED_MAX, 1e-12)
U8 = C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def phase_call(lib_mod, x, y, xe, ye, variances=0, partners=None, post=0, phase=True, depth=True, bloch=True):
    """fbx_rpe_phase with the outputs asked for; returns (phase, depth, bloch), None where not asked"""
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, xe, ye) + tuple(partners or ())]
    B, K = arrs[0].shape
    p = np.empty(B) if phase else None
    d = np.empty(B, dtype=np.int32) if depth else None
    bl = np.empty((B, K, 2)) if bloch else None
    ptr = [lib_mod.dptr(a) for a in arrs] + [None] * (8 - len(arrs))
    lib_mod.check(lib_mod.lib().fbx_rpe_phase(B, K, ptr[0], ptr[1], ptr[2], ptr[3], variances, ptr[4], ptr[5], ptr[6], ptr[7], post,
                                              lib_mod.dptr(p), lib_mod.iptr(d), lib_mod.dptr(bl)))
    return p, d, bl


@pytest.mark.parametrize("K", rc.GOLDEN_DEPTHS)
def test_goldens(gpu, gold, K):
    """1. phase by circular distance, depth_reached exactly, bloch rows"""
    from fbx import robust_phase_estimation as rpe
    x, y, xe, ye = (gold[f"k{K}_{n}"] for n in ("x", "y", "x_err", "y_err"))
    assert all(rc.safe(m) for m in rc.estimate_batch(x, y, xe, ye)[3])           # before the device is consulted
    phase, stats = rpe.estimate_phase_from_moments_batch(x, y, xe, ye, return_stats=True)
    dev = rc.circ_dist(phase, gold[f"k{K}_phase"])
    want_b, got_b = gold[f"k{K}_bloch"], stats["bloch"]
    k = 2.0 ** np.arange(K)
    print(f"RPEDEV K = {K}: largest circular deviation {dev.max():.3e} (TOL {TOL:.3e}), "
          f"bloch radius {np.nanmax(np.abs(got_b[..., 0] - want_b[..., 0]) / want_b[..., 0], initial=0):.3e} relative, "
          f"angle {np.nanmax(np.abs(got_b[..., 1] - want_b[..., 1]) / k, initial=0):.3e} / k")
    assert np.array_equal(stats["depth_reached"], gold[f"k{K}_depth_reached"])
    assert dev.max() <= TOL
    assert np.all((phase >= 0) & (phase < rc.TWO_PI))
    assert np.array_equal(np.isnan(got_b), np.isnan(want_b))
    live = ~np.isnan(want_b[..., 0])
    assert np.all(np.abs(got_b[..., 0] - want_b[..., 0])[live] <= 4 * rc.U_ROUND * want_b[..., 0][live])
    assert np.all((np.abs(got_b[..., 1] - want_b[..., 1]) / k)[live] <= TOL)
    # the reference's signature, item by item: value, bloch_data list and the warning's text
    for b in range(0, 50, 7):
        rows = []
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            got = rpe.estimate_phase_from_moments(list(x[b]), list(y[b]), list(xe[b]), list(ye[b]), rows)
        used = int(gold[f"k{K}_depth_reached"][b])
        assert got == phase[b] and len(rows) == used and all(isinstance(r, tuple) for r in rows)
        assert np.array_equal(np.asarray(rows).reshape(used, 2), got_b[b, :used])
        if used < K:
            assert len(w) == 1 and str(w[0].message) == (
                "Decoherence limited estimate of phase {0:.3f} to depth {1:d}. You may want to increase the additive_error and/or "
                "multiplicative_factor and try again.".format(got, 2 ** used // 2))
        else:
            assert not w


def test_exact_answers(gpu):
    """2. ==, no tolerance"""
    for K in (1, 2, 7, 62):
        one, zero, err = np.ones((1, K)), np.zeros((1, K)), np.full((1, K), 0.01)
        p, d, bl = phase_call(gpu, one, zero, err, err)                          # phase 0
        assert p[0] == 0.0 and d[0] == K and np.array_equal(bl[0], np.stack([np.ones(K), np.zeros(K)], axis=1))
        xs = np.ones((1, K)); xs[0, 0] = -1.0                                    # phase pi: cos(2^j pi) as exact +-1
        for y0 in (0.0, -0.0):
            p, d, _ = phase_call(gpu, xs, np.full((1, K), y0), err, err)
            assert p[0] == math.pi and d[0] == K, (K, y0, p[0])
    p, d, bl = phase_call(gpu, [[0.5]], [[0.0]], [[0.3]], [[0.4]])                # r == r_std = 0.5 does not stop the item
    assert d[0] == 1 and p[0] == 0.0 and bl[0, 0, 0] == 0.5
    p, d, bl = phase_call(gpu, [[np.nextafter(0.5, 0)]], [[0.0]], [[0.3]], [[0.4]])   # just below: stopped at iteration 0
    assert d[0] == 0 and p[0] == 0.0 and np.isnan(bl).all()
    p, d, bl = phase_call(gpu, [[0.0, 1.0, 1.0]], [[0.0, 0.0, 0.0]], [[1.0, 0.1, 0.1]], [[1.0, 0.1, 0.1]])
    assert d[0] == 0 and p[0] == 0.0 and np.isnan(bl).all()                     # stopped at iteration 0: later moments are not used
    p, d, _ = phase_call(gpu, [[0.0]], [[1.0]], [[0.1]], [[0.1]])                 # K = 1: atan2(1, 0)
    want = rc.estimate([0.0], [1.0], [0.1], [0.1])
    assert d[0] == 1 and abs(p[0] - want[0]) <= TOL
    # errors given as variances, and the post-selected combinations
    x, y, xe, ye, _ = rc.moment_sets(np.random.default_rng(5), 9, 4)
    a = phase_call(gpu, x, y, xe, ye)
    b = phase_call(gpu, x, y, xe * xe, ye * ye, variances=1)
    assert np.array_equal(a[1], b[1]) and rc.circ_dist(a[0], b[0]).max() <= TOL
    half = [0.5 * x, 0.5 * y, xe / math.sqrt(2), ye / math.sqrt(2)]
    want = rc.estimate_batch(x, y, np.sqrt((xe / math.sqrt(2)) ** 2 * 2), np.sqrt((ye / math.sqrt(2)) ** 2 * 2))
    assert all(rc.safe(m) for m in want[3])
    plus = phase_call(gpu, *half, partners=half, post=0)                          # x/2 + x/2
    minus = phase_call(gpu, half[0], half[1], half[2], half[3], partners=[-half[0], -half[1], half[2], half[3]], post=1)
    for got in (plus, minus):
        assert np.array_equal(got[1], want[1]) and rc.circ_dist(got[0], want[0]).max() <= TOL


def test_batch_geometry(gpu):
    """3. item b equals the same item alone, bit for bit; B = 0; every output NULL in turn; _dev = host"""
    from fbx import robust_phase_estimation as rpe
    K = 6
    x, y, xe, ye, _ = rc.moment_sets(np.random.default_rng(11), 7, K)
    alone = [phase_call(gpu, x[b:b + 1], y[b:b + 1], xe[b:b + 1], ye[b:b + 1]) for b in range(7)]
    assert len({int(a[1][0]) for a in alone}) > 1                                 # cut and uncut items are both present
    for B in (1, 63, 64, 65, 257):
        sel = (np.arange(B) * 3) % 7
        got = phase_call(gpu, x[sel], y[sel], xe[sel], ye[sel])
        for b in range(B):
            for k in range(3):
                assert np.array_equal(got[k][b], alone[sel[b]][k][0], equal_nan=True), (B, b, k)
    assert rpe.estimate_phase_from_moments_batch(x[:0], y[:0], xe[:0], ye[:0]).shape == (0,)
    full = phase_call(gpu, x, y, xe, ye)
    for skip in range(3):
        flags = [k != skip for k in range(3)]
        part = phase_call(gpu, x, y, xe, ye, phase=flags[0], depth=flags[1], bloch=flags[2])
        for k in range(3):
            assert (part[k] is None) if k == skip else np.array_equal(part[k], full[k], equal_nan=True)
    lib, DB = gpu.lib(), gpu.DeviceBuffer
    d_in = [DB.from_array(a) for a in (x, y, xe, ye)]
    d_p, d_d, d_b = DB(7 * 8), DB(7 * 4), DB(7 * K * 16)
    gpu.check(lib.fbx_rpe_phase_dev(7, K, d_in[0].ptr, d_in[1].ptr, d_in[2].ptr, d_in[3].ptr, 0, None, None, None, None, 0,
                                    d_p.ptr, d_d.ptr, d_b.ptr))
    gpu.synchronize()
    assert np.array_equal(d_p.to_array(np.float64, (7,)), full[0]) and np.array_equal(d_d.to_array(np.int32, (7,)), full[1])
    assert np.array_equal(d_b.to_array(np.float64, (7, K, 2)), full[2], equal_nan=True)


def _composed(gpu, xb, yb, col, zcol, post):
    """fbx_shots_to_moments_dev -> fbx_rpe_phase_dev on the same bits, resident"""
    lib, DB = gpu.lib(), gpu.DeviceBuffer
    B, K, shots, n = xb.shape
    masks = np.zeros((2, B * K, n), dtype=np.uint8)
    masks[:, :, col] = 1
    if zcol is not None:
        masks[1, :, zcol] = 1
    d_bits = [DB.from_array(xb), DB.from_array(yb)]
    d_masks = [DB.from_array(masks[0]), DB.from_array(masks[1])]
    moments = []
    for which in range(2 if zcol is not None else 1):
        for bits in d_bits:
            m, v = DB(B * K * 8), DB(B * K * 8)
            gpu.check(lib.fbx_shots_to_moments_dev(n, B * K, shots, bits.ptr, d_masks[which].ptr, None, 0, m.ptr, v.ptr))
            moments.append((m, v))
    (xm, xv), (ym, yv) = moments[:2]
    part = [None] * 4 if zcol is None else [moments[2][0].ptr, moments[3][0].ptr, moments[2][1].ptr, moments[3][1].ptr]
    d_p, d_d = DB(B * 8), DB(B * 4)
    gpu.check(lib.fbx_rpe_phase_dev(B, K, xm.ptr, ym.ptr, xv.ptr, yv.ptr, 1, part[0], part[1], part[2], part[3], post,
                                    d_p.ptr, d_d.ptr, None))
    gpu.synchronize()
    return d_p.to_array(np.float64, (B,)), d_d.to_array(np.int32, (B,))


@pytest.mark.parametrize("n_qubits", [1, 2, 3])
@pytest.mark.parametrize("shots", [1, 15, 16, 17, 500, 1337])
def test_from_shots(gpu, shots, n_qubits):
    """4. moments equal a direct numpy count, exactly; phase and depth_reached equal the composed path on the same bits.  Records
    of an odd number of bytes put every later record off the 16-byte grid (the byte-wise heads and tails)."""
    from fbx import robust_phase_estimation as rpe
    K = 3
    rng = np.random.default_rng(1000 * shots + n_qubits)
    # (col, zcol, post_select, B): no partner, a partner column before col and one after it, both signs, every batch size
    cases = {1: [(0, None, 0, 260), (0, None, 0, 1), (0, None, 0, 3), (0, None, 0, 5)],
             2: [(1, None, 0, 260), (1, 0, 0, 1), (1, 0, 1, 3), (0, 1, 0, 5), (0, 1, 1, 260)],
             3: [(1, None, 0, 260), (1, 0, 0, 1), (1, 0, 1, 3), (1, 2, 0, 5), (1, 2, 1, 260)]}[n_qubits]
    assert {c[3] for c in cases} == {1, 3, 5, 260}
    lib = gpu.lib()
    for col, zcol, ps, B in cases:
        # a few spare items: with few shots the counts can make r equal r_std exactly; such an item is drawn again
        xb, yb = rc.shot_records(rng, B + 16, K, shots, n_qubits, col, zcol, rng.uniform(0, rc.TWO_PI, B + 16), visibility=0.5)
        xb = xb | 2 * (xb ^ 1)                                                   # only bit 0 of a byte is read
        want = rc.moments_from_shots(xb, yb, col, zcol, ps)
        ok = [i for i, w in enumerate(want) if rc.estimate(w[:, 0], w[:, 1], w[:, 2], w[:, 3])[3][1] >= rc.MARGIN][:B]
        assert len(ok) == B
        xb, yb, want = np.ascontiguousarray(xb[ok]), np.ascontiguousarray(yb[ok]), want[ok]
        ref = rc.estimate_batch(want[..., 0], want[..., 1], want[..., 2], want[..., 3])
        assert all(m[1] >= rc.MARGIN for m in ref[3])                            # |r - r_std| >= 1e-9 r, before the device is consulted
        phase, depth, bloch, moments = np.empty(B), np.empty(B, dtype=np.int32), np.empty((B, K, 2)), np.empty((B, K, 4))
        gpu.check(lib.fbx_rpe_from_shots(n_qubits, B, K, shots, xb.ctypes.data_as(U8), yb.ctypes.data_as(U8), col,
                                         -1 if zcol is None else zcol, ps, gpu.dptr(phase), gpu.iptr(depth), gpu.dptr(bloch),
                                         gpu.dptr(moments)))
        assert np.array_equal(moments, want), (shots, n_qubits, col, zcol, ps, B)
        cp, cd = _composed(gpu, xb, yb, col, zcol, ps)
        assert np.array_equal(depth, cd) and np.array_equal(depth, ref[1])
        assert rc.circ_dist(phase, cp).max() <= TOL
        assert np.array_equal(np.isnan(bloch[..., 0]), np.arange(K)[None] >= depth[:, None])
        # without the moments the deeper records of a cut item are not read: the same answers
        assert np.array_equal(rpe.robust_phase_estimate_from_shots_batch(xb & 1, yb, col, zcol=zcol, post_select=ps), phase)


def test_from_shots_wide_records_and_dev_form(gpu):
    """4. (the other record widths, 4..8 qubits, and the _dev form against the host form)"""
    from fbx import robust_phase_estimation as rpe
    rng = np.random.default_rng(77)
    for n, col, zcol in ((4, 2, 0), (5, 0, 4), (6, 5, 2), (7, 3, 6), (8, 7, 0)):
        xb, yb = rc.shot_records(rng, 6, 2, 333, n, col, zcol, rng.uniform(0, rc.TWO_PI, 6))
        for ps in (0, 1):
            p, st = rpe.robust_phase_estimate_from_shots_batch(xb, yb, col, zcol=zcol, post_select=ps, return_stats=True)
            assert np.array_equal(st["moments"], rc.moments_from_shots(xb, yb, col, zcol, ps)), (n, ps)
    lib, DB = gpu.lib(), gpu.DeviceBuffer
    d_x, d_y, d_p, d_m = DB.from_array(xb), DB.from_array(yb), DB(6 * 8), DB(6 * 2 * 4 * 8)
    gpu.check(lib.fbx_rpe_from_shots_dev(8, 6, 2, 333, d_x.ptr, d_y.ptr, 7, 0, 1, d_p.ptr, None, None, d_m.ptr))
    gpu.synchronize()
    assert np.array_equal(d_p.to_array(np.float64, (6,)), p) and np.array_equal(d_m.to_array(np.float64, (6, 2, 4)), st["moments"])
    assert rpe.robust_phase_estimate_from_shots_batch(xb[:0], yb[:0], 7).shape == (0,)


@pytest.mark.parametrize("name", rc.RESULT_STRUCTURES)
def test_robust_phase_estimate(gpu, gold, name):
    """5. the golden two-qubit structures: number and order of the phases as the reference's, values within the tolerance"""
    from fbx import robust_phase_estimation as rpe
    results, qubits = rc.fbx_results(gold, name)
    for item in rpe._phase_inputs(results, qubits):
        assert rc.safe(rc.estimate(*item)[3])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = rpe.robust_phase_estimate(results, qubits)
    want = gold[f"{name}_phases"]
    assert isinstance(got, list) and len(got) == len(want)
    assert rc.circ_dist(got, want).max() <= TOL
    x_only = [[res for res in depth if res.setting.observable[1] in "XY" and res.setting.observable[0] == "I"] for depth in results]
    one = rpe.robust_phase_estimate(x_only, [1])                                  # one qubit: a float
    assert isinstance(one, float) and 0 <= one < rc.TWO_PI


def test_non_finite_moments_poison_their_own_item_only(gpu):
    """6. NaN / inf in item 2 of 6: that item NaN, the other five bit-identical to a clean run"""
    x, y, xe, ye, _ = rc.moment_sets(np.random.default_rng(21), 6, 5, decay_range=(1.0, 4.0))
    clean = phase_call(gpu, x, y, xe, ye)
    assert clean[1][2] == 5
    keep = [0, 1, 3, 4, 5]
    for which in range(4):
        for poison in (np.nan, np.inf, -np.inf):
            arrs = [a.copy() for a in (x, y, xe, ye)]
            arrs[which][2, 3] = poison
            got = phase_call(gpu, *arrs)
            for k in range(3):
                assert np.array_equal(got[k][keep], clean[k][keep], equal_nan=True), (which, poison, k)
            assert np.isnan(got[0][2]) and np.isnan(got[2][2]).all() and got[1][2] == 3
    arrs = [a.copy() for a in (x, y, xe, ye)]                                     # beyond the cut a moment is not used
    arrs[0][2, 1], arrs[2][2, 1], arrs[0][2, 3] = 0.0, 1.0, np.nan
    got = phase_call(gpu, *arrs)
    assert got[1][2] == 1 and not np.isnan(got[0][2])


def test_circular_stats(gpu):
    """7a. fbx_circular_stats against numpy (exactly rounded sums, math.fsum) on angles straddling 0 / 2 pi.  With the angles of an
    item spread uniformly over +-1 rad, Rbar is near 0.84 and std^2 = -2 ln Rbar near 0.35: an error dR of Rbar moves std by
    dR / (Rbar std^2) = 3.4 dR relatively; the sums are exact to 2 ulp on the device (compensated) and exact in the partner, sin and
    cos average to ~1 ulp, the division, the sqrt and the log add one each: inside 64 x 2^-53 relative on both sides together, and
    64 x 2^-53 of 2 pi for the mean."""
    from fbx import robust_phase_estimation as rpe
    rng = np.random.default_rng(3)
    R, B = 257, 70
    centre = np.where(np.arange(B) % 2 == 0, rng.uniform(-0.2, 0.2, B), rng.uniform(0, rc.TWO_PI, B))
    angles = (centre[None] + rng.uniform(-1, 1, (R, B))) % rc.TWO_PI
    angles[rng.random((R, B)) < 0.05] = np.nan
    angles[:, 5] = np.nan                                                      # nothing left: NaN results, everything counted
    angles[:, 6] = 0.3                                                         # no spread
    mean, std, skipped = rpe.circular_stats(angles)
    assert np.array_equal(skipped, np.isnan(angles).sum(axis=0)) and skipped[5] == R and 0 < skipped.sum() - R < R * B // 5
    assert np.isnan(mean[5]) and np.isnan(std[5])
    for b in [i for i in range(B) if i != 5]:
        a = angles[~np.isnan(angles[:, b]), b]
        ms, mc = math.fsum(np.sin(a)) / len(a), math.fsum(np.cos(a)) / len(a)
        wmean = math.atan2(ms, mc) % rc.TWO_PI
        rbar = math.hypot(ms, mc)
        wstd = math.sqrt(-2 * math.log(rbar)) if rbar < 1 else 0.0
        assert rc.circ_dist(mean[b], wmean) <= 64 * rc.U_ROUND * rc.TWO_PI, (b, mean[b], wmean)
        if b == 6:
            assert std[b] <= 1e-7                                               # sqrt of a rounding residue of ln(1 - 1e-16)
        else:
            assert abs(std[b] - wstd) <= 64 * rc.U_ROUND * wstd, (b, std[b], wstd)
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(rpe.circular_stats(angles), (mean, std, skipped)))
    lib = gpu.lib()
    only = np.empty(B)
    gpu.check(lib.fbx_circular_stats(R, B, gpu.dptr(np.ascontiguousarray(angles)), None, gpu.dptr(only), None))
    assert np.array_equal(only, std, equal_nan=True)
    assert rpe.circular_stats(np.zeros((0, 3)))[2].tolist() == [0, 0, 0]


def test_phase_variance_batch(gpu):
    """7b. R = 2000 against a numpy bootstrap of the reference's estimator on the same moments: the two circular standard deviations
    agree within 5 / sqrt(2 R) = 7.9 % relative (the sampling error of a standard deviation from R draws at five sigma); same seed ->
    identical bits; an item's result does not depend on its position in the batch."""
    from fbx import robust_phase_estimation as rpe
    R, K, shots, B = 2000, 6, 500, 4
    depth = 2.0 ** np.arange(K)
    phi = np.array([0.4, 2.0, 3.3, 6.1])
    x, y = 0.9 * np.cos(depth[None] * phi[:, None]), 0.9 * np.sin(depth[None] * phi[:, None])
    xe, ye = np.sqrt((1 - x * x) / shots), np.sqrt((1 - y * y) / shots)
    mean, var, skipped, samples = rpe.phase_variance_batch(x, y, xe, ye, shots, n_resamples=R, seed=7, return_samples=True)
    assert samples.shape == (B, R) and not skipped.any()
    rng = np.random.default_rng(99)
    for b in range(B):
        xr = 2 * rng.beta((x[b] + 1) / 2 * shots + 1, shots - (x[b] + 1) / 2 * shots + 1, size=(R, K)) - 1
        yr = 2 * rng.beta((y[b] + 1) / 2 * shots + 1, shots - (y[b] + 1) / 2 * shots + 1, size=(R, K)) - 1
        ph = rc.estimate_vec(xr, yr, np.broadcast_to(xe[b], (R, K)), np.broadcast_to(ye[b], (R, K)))
        rbar = math.hypot(np.sin(ph).mean(), np.cos(ph).mean())
        wstd = math.sqrt(-2 * math.log(rbar))
        print(f"RPEBOOT item {b}: device std {math.sqrt(var[b]):.4e}, numpy {wstd:.4e}, mean off by {rc.circ_dist(mean[b], phi[b]):.2e}")
        assert abs(math.sqrt(var[b]) - wstd) <= 5 / math.sqrt(2 * R) * wstd
        assert rc.circ_dist(mean[b], phi[b]) <= 5 * wstd / math.sqrt(R) + 1e-3
    again = rpe.phase_variance_batch(x, y, xe, ye, shots, n_resamples=R, seed=7)
    assert all(np.array_equal(u, v) for u, v in zip(again, (mean, var, skipped)))
    other = rpe.phase_variance_batch(x, y, xe, ye, shots, n_resamples=R, seed=8)
    assert not np.array_equal(other[0], mean)
    order = [2, 0]
    moved = rpe.phase_variance_batch(x[order], y[order], xe[order], ye[order], shots, n_resamples=R, seed=7)
    assert np.array_equal(moved[0], mean[order]) and np.array_equal(moved[1], var[order])
