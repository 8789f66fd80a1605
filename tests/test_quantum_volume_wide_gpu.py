"""fbx_qv_heavy_outputs_wide / fbx_qv_count_heavy_wide / fbx_qv_wide_plan on the GPU (widths 14..26): against the numpy restatement
of tests/qv_cases.py, against the numpy mirror of the planner, and against circuits whose answers are known exactly.

Tolerances are the derived ones of tests/test_quantum_volume_gpu.py: |dp[i]| <= qc.prob_bound(p_ref[i], L), the same bound at the
median, heavy tables equal (the drawn circuits have a relative middle gap of at least 1e-7 against a bound of about 3e-14 relative
at width 20), heavy_prob within the sum of the bounds over the heavy set.  The restatement runs once per module (`drawn`)."""
import ctypes as C

import numpy as np
import pytest

import qv_cases as qc

pytestmark = pytest.mark.gpu
KEYS = ("probabilities", "median", "mask", "heavy_prob", "heavy_count")
PAIRINGS = ("reference", "disjoint")


def _draw(n, count, seed, pairings=PAIRINGS):
    """qc.random_circuits's recipe, keeping the simulated distributions: permutations [count, n, n], gates [count, n, n // 2, 4, 4],
    {pairing: probabilities [count, 2^n]}, every circuit with a relative middle gap of at least 1e-7 under every pairing asked for"""
    rng = np.random.default_rng(seed)
    perms, gates, probs = [], [], {p: [] for p in pairings}
    while len(perms) < count:
        p = np.stack([rng.permutation(n) for _ in range(n)])
        z = rng.standard_normal((n, n // 2, 4, 4)) + 1j * rng.standard_normal((n, n // 2, 4, 4))
        q, r = np.linalg.qr(z)
        d = np.diagonal(r, axis1=-2, axis2=-1)
        g = q * (d / np.abs(d))[..., None, :]
        sims = {pairing: qc.simulate(n, qc.pairs_of(p, pairing), g.reshape(-1, 4, 4)) for pairing in pairings}
        if all(qc.middle_gap(s) >= 1e-7 for s in sims.values()):
            perms.append(p); gates.append(g)
            for pairing in pairings:
                probs[pairing].append(sims[pairing])
    return np.stack(perms), np.stack(gates), {k: np.stack(v) for k, v in probs.items()}


@pytest.fixture(scope="module")
def drawn():
    """{width: (permutations, gates, {pairing: reference probabilities})}: three circuits each at widths 14..17, one at width 20"""
    out = {n: _draw(n, 3, seed=1000 + n) for n in (14, 15, 16, 17)}
    out[20] = _draw(20, 1, seed=1020, pairings=("reference",))
    return out


@pytest.fixture(scope="module")
def device_results(gpu, drawn):
    """the device's results for `drawn` at the default tile, shared by the tests that compare other runs with them"""
    from fbx import quantum_volume as qv
    res = {}
    for n, (perms, gates, probs) in drawn.items():
        for pairing in probs:
            pairs, flat = _flat(qv, perms, gates, pairing)
            res[n, pairing] = qv.heavy_outputs_flat_wide(n, pairs, flat)
    return res


def _flat(qv, perms, gates, pairing):
    B, n = perms.shape[:2]
    L = n * (n // 2)
    return qv.layer_pairs(perms, pairing).reshape(B, L, 2), gates.reshape(B, L, 4, 4)


def _same(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k]) for k in keys)


def _check_against(n, L, r, want_p, label):
    from fbx import quantum_volume as qv
    heavy = qv.unpack_heavy_mask(r["mask"], n)
    for b in range(len(want_p)):
        wmed, wheavy = qc.heavy_of(want_p[b])
        err, bound = np.abs(r["probabilities"][b] - want_p[b]), qc.prob_bound(want_p[b], L)
        hp_err, hp_bound = abs(r["heavy_prob"][b] - want_p[b][wheavy].sum()), bound[wheavy].sum()
        print(f"{label} width {n} item {b}: max |dp| {err.max():.3e} (bound at max p {bound.max():.3e}), max |dp| / bound "
              f"{(err / bound).max():.3e}, |dmedian| {abs(r['median'][b] - wmed):.3e} (bound {qc.prob_bound(wmed, L):.3e}), "
              f"|dheavy_prob| {hp_err:.3e} (bound {hp_bound:.3e}), heavy table differs at {np.count_nonzero(heavy[b] != wheavy)}")
        assert np.all(err <= bound), (label, n, b)
        assert abs(r["median"][b] - wmed) <= qc.prob_bound(wmed, L), (label, n, b)
        assert np.array_equal(heavy[b], wheavy), (label, n, b)
        assert r["heavy_count"][b] == wheavy.sum()
        assert hp_err <= hp_bound, (label, n, b)


@pytest.mark.parametrize("pairing", PAIRINGS)
@pytest.mark.parametrize("n", [14, 15, 16, 17])
def test_restatement(gpu, drawn, device_results, n, pairing):
    """1. widths 14..17, both pairings, B = 3, default tile, against the numpy restatement"""
    from fbx import quantum_volume as qv
    perms, gates, probs = drawn[n]
    _check_against(n, n * (n // 2), device_results[n, pairing], probs[pairing], pairing)
    heavy, p, stats = qv.collect_heavy_outputs_wide_batch(perms, gates, pairing=pairing, return_probabilities=True, return_stats=True)
    assert np.array_equal(heavy, np.stack([qc.heavy_of(w)[1] for w in probs[pairing]]))
    r = device_results[n, pairing]
    assert np.array_equal(p, r["probabilities"]) and all(np.array_equal(stats[k], r[k]) for k in ("median", "heavy_prob", "heavy_count"))
    assert np.array_equal(qv.ideal_heavy_output_probability_wide_batch(perms, gates, pairing=pairing), r["heavy_prob"])


def test_restatement_width_20(gpu, drawn, device_results):
    """1. one width-20 circuit, reference pairing: a 16 MiB state, larger than the L2 of one XCD"""
    from fbx import quantum_volume as qv
    perms, gates, probs = drawn[20]
    _check_against(20, 200, device_results[20, "reference"], probs["reference"], "reference")
    assert np.array_equal(qv.collect_heavy_outputs_wide_batch(perms, gates), qc.heavy_of(probs["reference"][0])[1][None])


@pytest.mark.parametrize("tile_bits", [8, 12, 13])
def test_planner(gpu, drawn, tile_bits):
    """2. fbx_qv_wide_plan equals plan_wide_passes, integer for integer, for the circuits of test 1"""
    from fbx import _lib, quantum_volume as qv
    lib = _lib.lib()
    for n, (perms, gates, probs) in drawn.items():
        for pairing in probs:
            pairs, _ = _flat(qv, perms, gates, pairing)
            B, L = pairs.shape[:2]
            n_passes = np.full(B, -7, dtype=np.int32)
            first = np.full((B, L + 1), -7, dtype=np.int32)
            masks = np.full((B, L), 0xFFFFFFFF, dtype=np.uint32)
            _lib.check(lib.fbx_qv_wide_plan(n, B, L, pairs.ctypes.data_as(C.POINTER(C.c_uint8)), tile_bits, _lib.iptr(n_passes),
                                            _lib.iptr(first), masks.ctypes.data_as(C.POINTER(C.c_uint32))))
            want = qv.plan_wide_passes(n, pairs, tile_bits)
            print(f"plan width {n} {pairing} tile {tile_bits}: passes {n_passes.tolist()} of {L} gates")
            assert np.array_equal(n_passes, want[0]) and np.array_equal(first, want[1]) and np.array_equal(masks, want[2])


@pytest.mark.parametrize("n", [14, 15])
def test_tiling_invariance(gpu, drawn, device_results, n):
    """3. every tile size gives the same bits: the plan moves data, it changes neither the gate order nor a group's arithmetic"""
    from fbx import quantum_volume as qv
    perms, gates, _ = drawn[n]
    for pairing in PAIRINGS:
        pairs, flat = _flat(qv, perms, gates, pairing)
        for tile_bits in (8, 10, 12, 13):
            r = qv.heavy_outputs_flat_wide(n, pairs, flat, tile_bits=tile_bits)
            for k in KEYS:
                assert np.array_equal(r[k], device_results[n, pairing][k]), (n, pairing, tile_bits, k)


@pytest.mark.parametrize("n", [14, 17])
def test_exact_known_answers(gpu, n):
    """4. ==, no tolerance: the bit order on both sides of the always-local bits, the matrix index order, ties are not heavy"""
    from fbx import quantum_volume as qv
    N = 1 << n
    e0 = np.zeros(N); e0[0] = 1.0
    r = qv.heavy_outputs_flat_wide(n, np.zeros((2, 0, 2), dtype=np.uint8), np.zeros((2, 0, 4, 4), dtype=complex))
    ident_pairs = np.asarray([[(q, (q + 1) % n) for q in range(n)]] * 2)
    ri = qv.heavy_outputs_flat_wide(n, ident_pairs, np.broadcast_to(np.eye(4, dtype=complex), (2, n, 4, 4)).copy())
    for res in (r, ri):
        for b in range(2):
            assert np.array_equal(res["probabilities"][b], e0) and res["median"][b] == 0.0 and res["heavy_prob"][b] == 1.0
            assert res["heavy_count"][b] == 1 and np.flatnonzero(qv.unpack_heavy_mask(res["mask"], n)[b]).tolist() == [0]
    cases = qc.basis_state_cases(n)
    for L in sorted({len(p) for _, p, _, _ in cases}):                      # one launch per circuit length
        group = [c for c in cases if len(c[1]) == L]
        res = qv.heavy_outputs_flat_wide(n, np.stack([c[1] for c in group]), np.stack([c[2] for c in group]))
        heavy = qv.unpack_heavy_mask(res["mask"], n)
        for b, (name, _, _, idx) in enumerate(group):
            want = np.zeros(N); want[idx] = 1.0
            assert np.array_equal(res["probabilities"][b], want), (n, name, np.flatnonzero(res["probabilities"][b]), idx)
            assert res["median"][b] == 0.0 and res["heavy_prob"][b] == 1.0 and res["heavy_count"][b] == 1
            assert np.flatnonzero(heavy[b]).tolist() == [idx], (n, name)
    for kind in ["all"] + (["all_but_last"] if n % 2 == 0 else []):
        pairs, gates, probs, med, heavy = qc.hadamard_case(n, kind)
        res = qv.heavy_outputs_flat_wide(n, pairs[None], gates[None])
        assert np.array_equal(res["probabilities"][0], probs), (n, kind)
        assert res["median"][0] == med, (n, kind, res["median"][0], med)
        assert np.array_equal(qv.unpack_heavy_mask(res["mask"], n)[0], heavy), (n, kind)
        assert res["heavy_count"][0] == heavy.sum() and res["heavy_prob"][0] == probs[heavy].sum()
        if n % 2 == 0 and kind == "all":
            assert not heavy.any() and med == 2.0 ** -n                      # all equal: an EMPTY heavy set, heavy probability 0


def test_batch_geometry(gpu, drawn, device_results):
    """5. width 14: an item's bits do not depend on B or on the chunking; every output NULL in turn; _dev = host"""
    from fbx import _lib, quantum_volume as qv
    n, L = 14, 98
    perms, gates, _ = drawn[n]
    pairs3, flat3 = _flat(qv, perms, gates, "reference")
    full = device_results[n, "reference"]
    for B in (1, 3, 17):
        sel = np.arange(B) % 3
        r = qv.heavy_outputs_flat_wide(n, pairs3[sel], flat3[sel])
        for b in range(B):
            for k in KEYS:
                assert np.array_equal(r[k][b], full[k][sel[b]]), (B, b, k)
    sel = np.arange(5) % 3
    with _lib.option("qv_wide_workspace_mib", 1.0):                          # 1 MiB: three circuits per chunk, two when the probabilities live in the workspace too
        r = qv.heavy_outputs_flat_wide(n, pairs3[sel], flat3[sel])
        rp = qv.heavy_outputs_flat_wide(n, pairs3[sel], flat3[sel], probabilities=False)    # the probabilities in the workspace
    assert _lib.get_option("qv_wide_workspace_mib") == 128.0
    for k in KEYS:
        assert np.array_equal(r[k], full[k][sel]), k
        assert k == "probabilities" or np.array_equal(rp[k], full[k][sel]), k
    empty = qv.heavy_outputs_flat_wide(n, pairs3[:0], flat3[:0])
    assert empty["probabilities"].shape == (0, 1 << n) and empty["mask"].shape == (0, (1 << n) // 64)
    for skip in KEYS:
        part = qv.heavy_outputs_flat_wide(n, pairs3, flat3, **{k: k != skip for k in KEYS})
        assert skip not in part and _same(part, full, [k for k in KEYS if k != skip]), skip
    for only in KEYS:
        one = qv.heavy_outputs_flat_wide(n, pairs3, flat3, **{k: k == only for k in KEYS})
        assert list(one) == [only] and np.array_equal(one[only], full[only])
    lib = _lib.lib()
    N, W = 1 << n, (1 << n) // 64
    d_pairs, d_gates = _lib.DeviceBuffer.from_array(pairs3.astype(np.uint8)), _lib.DeviceBuffer.from_array(flat3)
    d_p, d_m, d_k = _lib.DeviceBuffer(3 * N * 8), _lib.DeviceBuffer(3 * 8), _lib.DeviceBuffer(3 * W * 8)
    d_hp, d_hc = _lib.DeviceBuffer(3 * 8), _lib.DeviceBuffer(3 * 4)
    _lib.check(lib.fbx_qv_heavy_outputs_wide_dev(n, 3, L, d_pairs.ptr, d_gates.ptr, 0, d_p.ptr, d_m.ptr, d_k.ptr, d_hp.ptr, d_hc.ptr))
    _lib.synchronize()
    assert np.array_equal(d_p.to_array(np.float64, (3, N)), full["probabilities"])
    assert np.array_equal(d_m.to_array(np.float64, (3,)), full["median"])
    assert np.array_equal(d_k.to_array(np.uint64, (3, W)), full["mask"])
    assert np.array_equal(d_hp.to_array(np.float64, (3,)), full["heavy_prob"])
    assert np.array_equal(d_hc.to_array(np.int32, (3,)), full["heavy_count"])


def test_dispatch_below_14(gpu):
    """6. widths up to 13 go to the narrow entry points unchanged"""
    from fbx import quantum_volume as qv
    n = 10
    perms, gates = qc.random_circuits(n, 3, seed=610, min_gap=0.0)
    pairs, flat = _flat(qv, perms, gates, "reference")
    assert _same(qv.heavy_outputs_flat_wide(n, pairs, flat), qv.heavy_outputs_flat(n, pairs, flat))
    assert _same(qv.heavy_outputs_flat_wide(n, pairs, flat, tile_bits=9), qv.heavy_outputs_flat(n, pairs, flat))
    assert np.array_equal(qv.collect_heavy_outputs_wide_batch(perms, gates), qv.collect_heavy_outputs_batch(perms, gates))
    assert np.array_equal(qv.ideal_heavy_output_probability_wide_batch(perms, gates), qv.ideal_heavy_output_probability_batch(perms, gates))
    bits = np.random.default_rng(6).integers(0, 2, size=(3, 100, n), dtype=np.uint8)
    heavy = qv.collect_heavy_outputs_batch(perms, gates)
    assert np.array_equal(qv.count_heavy_hitters_sampled_wide_batch(bits, heavy), qv.count_heavy_hitters_sampled_batch(bits, heavy))


def test_errors_and_isolation(gpu, drawn):
    """7. widths, tile sizes, bad pairs; a NaN / Inf gate entry poisons its own item only"""
    from fbx import _lib, quantum_volume as qv
    lib = _lib.lib()
    u8 = C.POINTER(C.c_uint8)
    eye = np.eye(4, dtype=complex)[None, None].copy()
    out = np.zeros(1 << 14)
    ok_pair = np.asarray([[(0, 1)]], dtype=np.uint8)
    for n in (13, 27):
        rc = lib.fbx_qv_heavy_outputs_wide(n, 1, 1, ok_pair.ctypes.data_as(u8), _lib.dptr(eye.view(np.float64)), 0, None, _lib.dptr(out),
                                           None, None, None)
        assert rc == _lib.FBX_ERR_UNSUPPORTED and b"14..26" in lib.fbx_last_error()
    for t in (7, 14):
        rc = lib.fbx_qv_heavy_outputs_wide(14, 1, 1, ok_pair.ctypes.data_as(u8), _lib.dptr(eye.view(np.float64)), t, _lib.dptr(out),
                                           None, None, None, None)
        assert rc == _lib.FBX_ERR_BAD_ARG
    for bad in ([(1, 1)], [(0, 14)]):
        pr = np.asarray([bad], dtype=np.uint8)
        rc = lib.fbx_qv_heavy_outputs_wide(14, 1, 1, pr.ctypes.data_as(u8), _lib.dptr(eye.view(np.float64)), 0, _lib.dptr(out), None,
                                           None, None, None)
        assert rc == _lib.FBX_ERR_BAD_ARG
        rc = lib.fbx_qv_wide_plan(14, 1, 1, pr.ctypes.data_as(u8), 0, _lib.iptr(np.zeros(1, dtype=np.int32)),
                                  _lib.iptr(np.zeros(2, dtype=np.int32)), np.zeros(1, dtype=np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)))
        assert rc == _lib.FBX_ERR_BAD_ARG
    n, L = 14, 98
    perms, gates, _ = drawn[n]
    sel = np.arange(5) % 3
    pairs, flat = _flat(qv, perms[sel], gates[sel], "reference")
    clean = qv.heavy_outputs_flat_wide(n, pairs, flat)
    keep = [0, 1, 3, 4]
    for poison in (np.nan, np.inf):
        dirty = flat.copy()
        dirty[2, L // 2, 1, 2] = poison
        r = qv.heavy_outputs_flat_wide(n, pairs, dirty)
        for k in KEYS:
            assert np.array_equal(r[k][keep], clean[k][keep]), (poison, k)
        assert np.isnan(r["probabilities"][2]).all() and np.isnan(r["median"][2]) and np.isnan(r["heavy_prob"][2])
        assert r["heavy_count"][2] == 0 and not r["mask"][2].any()
    # the _dev form cannot check the pairs: a bad pair poisons its item, and the state is never indexed with it
    bad_pairs = pairs.astype(np.uint8).copy()
    bad_pairs[2, L // 3] = (200, 3)
    N, W = 1 << n, (1 << n) // 64
    d_pairs, d_gates = _lib.DeviceBuffer.from_array(bad_pairs), _lib.DeviceBuffer.from_array(flat)
    d_p, d_m, d_k, d_hc = _lib.DeviceBuffer(5 * N * 8), _lib.DeviceBuffer(5 * 8), _lib.DeviceBuffer(5 * W * 8), _lib.DeviceBuffer(5 * 4)
    _lib.check(lib.fbx_qv_heavy_outputs_wide_dev(n, 5, L, d_pairs.ptr, d_gates.ptr, 0, d_p.ptr, d_m.ptr, d_k.ptr, None, d_hc.ptr))
    _lib.synchronize()
    p, m, k, hc = d_p.to_array(np.float64, (5, N)), d_m.to_array(np.float64, (5,)), d_k.to_array(np.uint64, (5, W)), d_hc.to_array(np.int32, (5,))
    assert np.isnan(p[2]).all() and np.isnan(m[2]) and not k[2].any() and hc[2] == 0
    assert np.array_equal(p[keep], clean["probabilities"][keep]) and np.array_equal(k[keep], clean["mask"][keep])
    assert np.array_equal(m[keep], clean["median"][keep]) and np.array_equal(hc[keep], clean["heavy_count"][keep])


@pytest.mark.parametrize("n", [14, 17])
def test_heavy_counts(gpu, drawn, device_results, n):
    """8. counts equal a direct numpy evaluation of the reference's loop, with the masks of test 1; the chain on device pointers"""
    from fbx import _lib, quantum_volume as qv
    mask = device_results[n, "reference"]["mask"]
    heavy = qv.unpack_heavy_mask(mask, n)
    rng = np.random.default_rng(800 + n)
    for shots in (1, 15, 16, 17, 1000):
        bits = rng.integers(0, 2, size=(3, shots, n), dtype=np.uint8)
        want = qc.count_heavy_direct(bits, heavy)
        got = qv.count_heavy_hitters_sampled_wide_batch(bits, mask)
        assert got.dtype == np.int64 and np.array_equal(got, want), (n, shots, got, want)
        assert np.array_equal(qv.count_heavy_hitters_sampled_wide_batch(bits, heavy), want)
    noisy, got = np.ascontiguousarray(bits | 0xA2), np.zeros(3, dtype=np.int64)                       # only bit 0 of a byte is read
    _lib.check(_lib.lib().fbx_qv_count_heavy_wide(n, 3, 1000, noisy.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                  mask.ctypes.data_as(C.POINTER(C.c_uint64)), got.ctypes.data_as(C.POINTER(C.c_int64))))
    assert np.array_equal(got, want)
    assert qv.count_heavy_hitters_sampled_wide_batch(bits[:, :0], mask).tolist() == [0, 0, 0]
    # heavy outputs -> counts without leaving the device
    lib = _lib.lib()
    perms, gates, _ = drawn[n]
    pairs, flat = _flat(qv, perms, gates, "reference")
    L, W = pairs.shape[1], (1 << n) // 64
    d_pairs, d_gates, d_bits = _lib.DeviceBuffer.from_array(pairs), _lib.DeviceBuffer.from_array(flat), _lib.DeviceBuffer.from_array(bits)
    d_mask, d_counts = _lib.DeviceBuffer(3 * W * 8), _lib.DeviceBuffer(3 * 8)
    _lib.check(lib.fbx_qv_heavy_outputs_wide_dev(n, 3, L, d_pairs.ptr, d_gates.ptr, 0, None, None, d_mask.ptr, None, None))
    _lib.check(lib.fbx_qv_count_heavy_wide_dev(n, 3, 1000, d_bits.ptr, d_mask.ptr, d_counts.ptr))
    _lib.synchronize()
    assert np.array_equal(d_mask.to_array(np.uint64, (3, W)), mask)
    assert np.array_equal(d_counts.to_array(np.int64, (3,)), want)
