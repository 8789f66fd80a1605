"""The wave reductions of csrc/fbx_common.hpp by themselves: wave_sum (four DPP levels with a zero `old` operand, the four row sums
through v_readlane), the lean form of the one-wave PGDB kernels (bound_ctrl levels, the rows through row_bcast:15 / row_bcast:31,
one readlane of lane 63) and wave_sum_n<N> (N values level by level) must give the SAME BITS, and those of the stated tree

    v += v[lane ^ 1]; v += v[lane ^ 2]; v += v[half-row mirror]; v += v[row mirror]; (r0 + r1) + (r2 + r3)

evaluated in numpy.  One launch of one wavefront (csrc/test/fbx_wave_reduce_test.hip -> libfbx_wavered.so, built by build()) runs
all of them on [16][64] doubles per input set.  If row_bcast did not deliver the row sums on this hardware, the lean columns would
hold wrong VALUES here -- nothing can fault: the kernel reads its input and writes 88 doubles per set from lane 0.
(The sums replace np.sum / np.linalg.norm of the reference's loops, tomography.py:542-594 and project_superoperators.py:87-144.)"""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "forest-benchmarking_amd", "libfbx_wavered.so")
LANES = np.arange(64)
NAN_LANES = (0, 15, 16, 31, 47, 63)


def tree_sum(rows):
    """The stated tree on rows[..., 64] (float64): partner + own at every level, every lane keeps a running value."""
    v = np.array(rows, dtype=np.float64)
    with np.errstate(all="ignore"):
        for partner in (LANES ^ 1, LANES ^ 2, (LANES & ~7) | (7 - (LANES & 7)), (LANES & ~15) | (15 - (LANES & 15))):
            v = v[..., partner] + v
        return (v[..., 0] + v[..., 16]) + (v[..., 32] + v[..., 48])


def tree_max(rows):
    v = np.array(rows, dtype=np.float64)
    for partner in (LANES ^ 1, LANES ^ 2, (LANES & ~7) | (7 - (LANES & 7)), (LANES & ~15) | (15 - (LANES & 15))):
        v = np.fmax(v, v[..., partner])
    return np.fmax(np.fmax(v[..., 0], v[..., 16]), np.fmax(v[..., 32], v[..., 48]))


def input_sets():
    """name -> [16][64] doubles; `loose` names the sets whose sums may be NaN (NaN-ness and the finite entries are compared)."""
    rs = np.random.RandomState(12)
    sets = {}
    # mixed magnitude 1e-300 .. 1e300 (row k spans k-dependent decades), every second lane nearly cancels its neighbour
    mag = 10.0 ** rs.uniform(-300, 300, (16, 64))
    mag[8:] = 10.0 ** rs.uniform(-8, 8, (8, 64))
    x = mag * rs.choice([-1.0, 1.0], (16, 64))
    x[:, 1::2] = -x[:, 0::2] * (1.0 + rs.randint(-4, 5, (16, 32)) * 2.0 ** -52)
    x[12:] = x[12:, rs.permutation(64)]                       # cancellation across quads, half rows and rows
    sets["mixed"] = x
    # denormals (and sums that leave / stay in the denormal range)
    den = rs.randint(1, 2 ** 40, (16, 64)).astype(np.float64) * 5e-324 * rs.choice([-1.0, 1.0], (16, 64))
    den[8:] += rs.choice([0.0, 2.2250738585072014e-308], (8, 64))
    sets["denormal"] = den
    # +-0: row k of the set makes the 16-lane rows named by the bits of k sum to -0 (every lane -0); the other rows of lanes hold
    # +0 / -0 mixtures that sum to +0.  The total is -0 only for k = 15.
    z = np.zeros((16, 64))
    for k in range(16):
        for r in range(4):
            if k >> r & 1:
                z[k, 16 * r:16 * r + 16] = -0.0
            else:
                z[k, 16 * r:16 * r + 16] = np.where(rs.rand(16) < 0.5, -0.0, 0.0)
                z[k, 16 * r + rs.randint(16)] = 0.0
    sets["zeros"] = z
    # +-inf: one +inf, one -inf, both (NaN), inf beside huge finite values, inf in the lanes the row sums pass through
    f = rs.uniform(-1e300, 1e300, (16, 64)) / 64
    for k, (lane, val) in enumerate(((0, np.inf), (63, -np.inf), (15, np.inf), (16, -np.inf), (31, np.inf), (47, -np.inf), (5, np.inf), (40, -np.inf))):
        f[k, lane] = val
    f[8, 3] = np.inf; f[8, 60] = -np.inf                      # noqa: E702   inf - inf across rows
    f[9, 17] = np.inf; f[9, 18] = -np.inf                     # noqa: E702   inside a quad
    f[10, :] = np.inf
    f[11, :] = -np.inf
    f[12, ::2] = np.inf
    sets["inf"] = f
    # one NaN in lane 0, 15, 16, 31, 47, 63 in turn (rows 0 .. 5); the other rows stay finite
    n = rs.randn(16, 64)
    for k, lane in enumerate(NAN_LANES):
        n[k, lane] = np.nan
    sets["nan"] = n
    # the lane index itself and functions of it: a wrong or missing partner changes the bits
    li = np.zeros((16, 64))
    L = LANES.astype(np.float64)
    li[0] = L; li[1] = 2.0 ** L; li[2] = 3.0 ** L; li[3] = L * L; li[4] = (-2.0) ** L; li[5] = 1.0 / (1.0 + L)      # noqa: E702
    li[6] = 2.0 ** (-L); li[7] = L + 2.0 ** 53; li[8] = np.sqrt(L); li[9] = 1e16 * (L % 2) + L                       # noqa: E702
    for k in range(10, 16):
        li[k] = (L == 4 * (k - 10) + 3) * 1.0 + (L == 63 - (k - 10)) * 2.0 ** -60       # two lanes only
    sets["lane"] = li
    # all-equal values
    sets["equal"] = np.tile(np.array([0.1, 1.0 / 3.0, 1e300, 1e-310, -0.0, 1.0, -7.25, 2.0 ** -1074, 1e-300, np.pi, 1.7e306, -1e-5,
                                      3.0, 2.0 ** 52 + 1, 1e22, 5e-324])[:, None], (1, 64))
    return sets, ("inf", "nan")


def same(a, b, loose):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if loose:                                                 # NaN-ness and the non-NaN entries; not the payload
        return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_numpy_tree_is_the_stated_tree():
    """The numpy evaluation itself, on the CPU: exact where every order gives the same sum, equal to the tree written out by hand
    where the order decides the bits, and -0 only when every lane is -0."""
    L = LANES.astype(np.float64)
    assert tree_sum(L) == 2016.0
    assert tree_sum(np.where(LANES < 53, 2.0 ** L, 0.0)) == 2.0 ** 53 - 1          # exact: every partial sum is representable
    x = np.random.RandomState(1).randn(64) * 10.0 ** np.random.RandomState(2).uniform(-12, 12, 64)

    def quad(q):                                              # lanes 4 q .. 4 q + 3 as lane 4 q sees them: (x1 + x0), then (x3 + x2) + that
        return float((x[4 * q + 3] + x[4 * q + 2]) + (x[4 * q + 1] + x[4 * q]))

    def row(r):                                               # half-row mirror: lane 0 takes lane 7; row mirror: lane 0 takes lane 15
        h0 = float(np.float64(quad(4 * r + 1)) + np.float64(quad(4 * r)))
        h1 = float(np.float64(quad(4 * r + 2)) + np.float64(quad(4 * r + 3)))     # lane 15 of the row: own quad 3, partner quad 2
        return float(np.float64(h1) + np.float64(h0))
    by_hand = (np.float64(row(0)) + np.float64(row(1))) + (np.float64(row(2)) + np.float64(row(3)))
    assert np.float64(tree_sum(x)).view(np.uint64) == np.float64(by_hand).view(np.uint64)
    z = np.full(64, -0.0)
    assert np.signbit(tree_sum(z))
    z[37] = 0.0
    assert not np.signbit(tree_sum(z)) and tree_sum(z) == 0.0
    sets, loose = input_sets()
    assert np.signbit(tree_sum(sets["zeros"])).tolist() == [False] * 15 + [True]
    assert np.isnan(tree_sum(sets["nan"])).tolist() == [True] * 6 + [False] * 10
    assert tree_max(L) == 63.0 and tree_max(-L) == 0.0


@pytest.mark.gpu
def test_lean_and_level_by_level_reductions_match_wave_sum_bit_for_bit(gpu):
    assert os.path.exists(LIB), "libfbx_wavered.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(LIB)
    lib.fbx_test_wave_reduce.restype = ctypes.c_int
    lib.fbx_test_wave_reduce.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    sets, loose_names = input_sets()
    names = list(sets)
    x = np.ascontiguousarray(np.stack([sets[k] for k in names]), dtype=np.float64)
    out = np.full((len(names), 88), 123.0)
    assert lib.fbx_test_wave_reduce(x.ctypes.data, len(names), out.ctypes.data) == 0
    bad = []
    for s, name in enumerate(names):
        loose = name in loose_names
        ref, lean, n2, n6, n16 = out[s, 0:16], out[s, 16:32], out[s, 32:34], out[s, 34:40], out[s, 40:56]
        want = tree_sum(x[s])
        print(name, "wave_sum", ref[:4], "lean", lean[:4], "numpy", want[:4])
        for label, got, exp in (("wave_sum vs numpy", ref, want), ("lean vs wave_sum", lean, ref), ("lean vs numpy", lean, want),
                                ("n2 vs wave_sum", n2, ref[:2]), ("n6 vs wave_sum", n6, ref[:6]), ("n16 vs wave_sum", n16, ref),
                                ("n16 vs numpy", n16, want)):
            # NaN payloads aside, the device forms are compared as raw bits with each other even in the loose sets
            if not same(got, exp, loose):
                bad.append((name, label, got.tolist(), np.asarray(exp).tolist()))
        mx, mxl = out[s, 56:72], out[s, 72:88]
        if not same(mxl, mx, loose):
            bad.append((name, "wave_max_lean vs wave_max", mxl.tolist(), mx.tolist()))
        if name in ("mixed", "denormal", "lane", "equal") and not same(mx, tree_max(x[s]), False):     # (no +0 against -0 in these)
            bad.append((name, "wave_max vs numpy", mx.tolist(), tree_max(x[s]).tolist()))
    assert not bad, bad
