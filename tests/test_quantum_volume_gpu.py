"""fbx_qv_heavy_outputs / fbx_qv_count_heavy on the GPU: against the reference's heavy lists (tests/golden/qv_cases.npz, widths 2..10),
against the numpy restatement of tests/qv_cases.py (widths 11..13; pinned to the same goldens in tests/test_quantum_volume_cpu.py),
and against circuits whose answers are known exactly.

Tolerance (derived, not tuned): one gate application computes four length-4 complex dot products; its rounding error in the 2-norm
of the state is at most about 17 u (u = 2^-53; |U| of a 4 x 4 unitary has 2-norm <= 2), on the device and in numpy alike.  After L
gates two simulations differ by at most delta_L = 64 L u in the 2-norm, hence |p_dev[i] - p_ref[i]| <= 2 sqrt(p_ref[i]) delta_L +
delta_L^2 element by element (qv_cases.prob_bound), the same with the median in place of p, and |sum(p_dev) - 1| <= 2 delta_L.  At
width 13 (L = 78) that is 1e-14 at the median against a smallest permitted middle gap of 8e-12 (1e-7 of a median near ln 2 / 2^13),
which is why the heavy tables are compared with ==."""
import ctypes as C
import os

import numpy as np
import pytest

import qv_cases as qc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qv_cases.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def check_against(n, L, r, want_p, want_heavy=None, label=""):
    """device result dict r of one circuit batch against reference probabilities [B, N]"""
    from fbx import quantum_volume as qv
    heavy = qv.unpack_heavy_mask(r["mask"], n)
    for b in range(len(want_p)):
        wmed, wheavy = qc.heavy_of(want_p[b])
        if want_heavy is not None:
            assert np.array_equal(wheavy, want_heavy[b])
        err = np.abs(r["probabilities"][b] - want_p[b])
        bound = qc.prob_bound(want_p[b], L)
        print(f"{label} width {n} item {b}: max |dp| {err.max():.3e} (bound at max p {bound.max():.3e}), "
              f"|dmedian| {abs(r['median'][b] - wmed):.3e} (bound {qc.prob_bound(wmed, L):.3e}), "
              f"|sum - 1| {abs(r['probabilities'][b].sum() - 1):.3e}")
        assert np.all(err <= bound), (label, n, b)
        assert abs(r["median"][b] - wmed) <= qc.prob_bound(wmed, L), (label, n, b)
        assert abs(r["probabilities"][b].sum() - 1) <= 2 * qc.delta(L)
        assert np.array_equal(heavy[b], wheavy), (label, n, b, np.flatnonzero(heavy[b] != wheavy))
        assert r["heavy_count"][b] == wheavy.sum()
        hp = r["probabilities"][b][heavy[b]].sum()
        assert abs(r["heavy_prob"][b] - hp) <= (1 << n) * qc.U_ROUND          # two summation orders of at most 2^n / 2 terms, sum <= 1


@pytest.mark.parametrize("n", range(2, 11))
def test_goldens(gpu, gold, n):
    """1. heavy tables equal the reference's, every circuit; probabilities and medians within the bound"""
    from fbx import quantum_volume as qv
    perms, gates = gold[f"w{n}_permutations"], gold[f"w{n}_gates"]
    pairs = qv.layer_pairs(perms).reshape(len(perms), -1, 2)
    r = qv.heavy_outputs_flat(n, pairs, gates.reshape(len(perms), -1, 4, 4))
    check_against(n, pairs.shape[1], r, gold[f"w{n}_probabilities"], gold[f"w{n}_heavy"], "golden")
    assert abs(r["median"] - gold[f"w{n}_median"]).max() <= qc.prob_bound(gold[f"w{n}_median"], pairs.shape[1]).max()
    heavy, probs, stats = qv.collect_heavy_outputs_batch(perms, gates, return_probabilities=True, return_stats=True)
    assert np.array_equal(heavy, gold[f"w{n}_heavy"]) and np.array_equal(probs, r["probabilities"])
    assert np.array_equal(stats["median"], r["median"]) and np.array_equal(stats["heavy_count"], r["heavy_count"])
    assert np.array_equal(qv.ideal_heavy_output_probability_batch(perms, gates), r["heavy_prob"])
    for b in range(len(perms)):                                          # the reference's signature: a sorted list of ints
        got = qv.collect_heavy_outputs(None, list(perms[b]), gates[b])
        assert got == [int(i) for i in np.flatnonzero(gold[f"w{n}_heavy"][b])]


@pytest.mark.parametrize("pairing", ["reference", "disjoint"])
@pytest.mark.parametrize("n", [11, 12, 13])
def test_restatement_above_the_goldens(gpu, n, pairing):
    """2. widths 11, 12, 13, both pairings, against the numpy restatement"""
    from fbx import quantum_volume as qv
    perms, gates = qc.random_circuits(n, 4, seed=100 + n)
    L = n * (n // 2)
    want = []
    for b in range(4):
        p = qc.simulate(n, qc.pairs_of(perms[b], pairing), gates[b].reshape(-1, 4, 4))
        assert qc.middle_gap(p) >= 1e-7                                   # asserted before the device is consulted
        want.append(p)
    pairs = qv.layer_pairs(perms, pairing).reshape(4, L, 2)
    assert np.array_equal(pairs, np.stack([qc.pairs_of(perms[b], pairing) for b in range(4)]))
    r = qv.heavy_outputs_flat(n, pairs, gates.reshape(4, L, 4, 4))
    check_against(n, L, r, np.stack(want), None, pairing)
    heavy = qv.collect_heavy_outputs_batch(perms, gates, pairing=pairing)
    assert np.array_equal(heavy, np.stack([qc.heavy_of(p)[1] for p in want]))


@pytest.mark.parametrize("pairing", ["reference", "disjoint"])
@pytest.mark.parametrize("n", [3, 6, 7, 10])
def test_restatement_small_widths_both_pairings(gpu, n, pairing):
    """2. (odd and even widths below the goldens' limit, for the disjoint pairing the goldens do not hold)"""
    from fbx import quantum_volume as qv
    perms, gates = qc.random_circuits(n, 4, seed=200 + n)
    L = n * (n // 2)
    want = np.stack([qc.simulate(n, qc.pairs_of(perms[b], pairing), gates[b].reshape(-1, 4, 4)) for b in range(4)])
    assert all(qc.middle_gap(p) >= 1e-7 for p in want)
    r = qv.heavy_outputs_flat(n, qv.layer_pairs(perms, pairing).reshape(4, L, 2), gates.reshape(4, L, 4, 4))
    check_against(n, L, r, want, None, pairing)


@pytest.mark.parametrize("n", range(2, 14))
def test_exact_known_answers(gpu, n):
    """4. ==, no tolerance: the bit order, the matrix index order and the strict inequality"""
    from fbx import quantum_volume as qv
    N = 1 << n
    e0 = np.zeros(N); e0[0] = 1.0
    # L = 0 and all-identity gates
    r = qv.heavy_outputs_flat(n, np.zeros((2, 0, 2), dtype=np.uint8), np.zeros((2, 0, 4, 4), dtype=complex))
    ident_pairs = np.asarray([[(q, (q + 1) % n) for q in range(n)]] * 2)
    ri = qv.heavy_outputs_flat(n, ident_pairs, np.broadcast_to(np.eye(4, dtype=complex), (2, n, 4, 4)).copy())
    for res in (r, ri):
        for b in range(2):
            assert np.array_equal(res["probabilities"][b], e0) and res["median"][b] == 0.0 and res["heavy_prob"][b] == 1.0
            assert res["heavy_count"][b] == 1 and np.flatnonzero(qv.unpack_heavy_mask(res["mask"], n)[b]).tolist() == [0]
    # permutation matrices: one non-zero probability at an index computed by hand
    for name, pairs, gates, idx in qc.basis_state_cases(n):
        res = qv.heavy_outputs_flat(n, pairs[None], gates[None])
        want = np.zeros(N); want[idx] = 1.0
        assert np.array_equal(res["probabilities"][0], want), (n, name, np.flatnonzero(res["probabilities"][0]), idx)
        assert res["median"][0] == 0.0 and res["heavy_prob"][0] == 1.0 and res["heavy_count"][0] == 1
        assert np.flatnonzero(qv.unpack_heavy_mask(res["mask"], n)[0]).tolist() == [idx], (n, name)
    # H (x) H on disjoint pairs: exact dyadic probabilities, ties are not heavy
    kinds = ["all"] + (["all_but_last"] if n % 2 == 0 else [])
    for kind in kinds:
        pairs, gates, probs, med, heavy = qc.hadamard_case(n, kind)
        res = qv.heavy_outputs_flat(n, pairs[None], gates[None])
        assert np.array_equal(res["probabilities"][0], probs), (n, kind)
        assert res["median"][0] == med, (n, kind, res["median"][0], med)
        assert np.array_equal(qv.unpack_heavy_mask(res["mask"], n)[0], heavy), (n, kind)
        assert res["heavy_count"][0] == heavy.sum() and res["heavy_prob"][0] == probs[heavy].sum()
    if n % 2 == 0:
        pairs, gates, probs, med, heavy = qc.hadamard_case(n, "all")
        assert not heavy.any() and med == 2.0 ** -n                      # all equal: an EMPTY heavy set, heavy probability 0


@pytest.mark.parametrize("n", [2, 5, 8, 9, 12, 13])
def test_closed_form_one_layer(gpu, n):
    """5. one layer of Haar gates on the disjoint pairs in natural order: Kronecker product of |U_k[:, 0]|^2 (x) (1, 0) for odd n"""
    from fbx import quantum_volume as qv
    _, g = qc.random_circuits(max(n, 2), 1, seed=300 + n, min_gap=0.0)
    gates = g[0, 0]                                                       # n // 2 Haar gates
    pairs = np.asarray([(2 * k, 2 * k + 1) for k in range(n // 2)])
    want = np.ones(1)
    for k in range(n // 2):
        want = np.kron(want, np.abs(gates[k][:, 0]) ** 2)
    if n % 2:
        want = np.kron(want, np.array([1.0, 0.0]))
    r = qv.heavy_outputs_flat(n, pairs[None], gates[None])
    err = np.abs(r["probabilities"][0] - want)
    bound = qc.prob_bound(want, n // 2)                                   # the bound of the tolerance section, L = n / 2 gates
    print(f"closed form width {n}: max |dp| {err.max():.3e}, bound {bound.max():.3e}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("n", [4, 7, 10, 13])
def test_covariance_under_relabelling(gpu, n):
    """6. renaming the qubits permutes the output indices by the corresponding bit permutation"""
    from fbx import quantum_volume as qv
    perms, gates = qc.random_circuits(n, 2, seed=400 + n)
    L = n * (n // 2)
    pairs = qv.layer_pairs(perms).reshape(2, L, 2)
    flat = gates.reshape(2, L, 4, 4)
    pi = np.random.default_rng(n).permutation(n)
    a = qv.heavy_outputs_flat(n, pairs, flat)
    b = qv.heavy_outputs_flat(n, qc.relabel(pairs, pi), flat)
    new = qc.relabel_index_map(n, pi)
    ha, hb = qv.unpack_heavy_mask(a["mask"], n), qv.unpack_heavy_mask(b["mask"], n)
    for k in range(2):
        assert np.array_equal(hb[k][new], ha[k])
        assert abs(a["median"][k] - b["median"][k]) <= qc.prob_bound(a["median"][k], L)
        assert np.all(np.abs(b["probabilities"][k][new] - a["probabilities"][k]) <= qc.prob_bound(a["probabilities"][k], L))


@pytest.mark.parametrize("n", [3, 9, 13])
def test_batch_geometry(gpu, n):
    """7. item b of a batch equals the same circuit run alone, bit for bit; B = 0; every output NULL in turn; _dev = host"""
    from fbx import _lib, quantum_volume as qv
    L = n * (n // 2)
    perms, gates = qc.random_circuits(n, 5, seed=500 + n, min_gap=0.0)
    pairs5 = qv.layer_pairs(perms).reshape(5, L, 2)
    flat5 = gates.reshape(5, L, 4, 4)
    alone = [qv.heavy_outputs_flat(n, pairs5[b:b + 1], flat5[b:b + 1]) for b in range(5)]
    keys = ("probabilities", "median", "mask", "heavy_prob", "heavy_count")
    for B in (1, 3, 64, 257):
        sel = np.arange(B) % 5
        r = qv.heavy_outputs_flat(n, pairs5[sel], flat5[sel])
        for b in (range(B) if B <= 64 else (0, 1, 63, 64, 128, 255, 256)):
            for k in keys:
                assert np.array_equal(r[k][b], alone[sel[b]][k][0]), (n, B, b, k)
    empty = qv.heavy_outputs_flat(n, pairs5[:0], flat5[:0])
    assert empty["probabilities"].shape == (0, 1 << n) and empty["mask"].shape == (0, max(1, (1 << n) // 64))
    assert qv.collect_heavy_outputs_batch(perms[:0], gates[:0]).shape == (0, 1 << n)
    full = qv.heavy_outputs_flat(n, pairs5, flat5)
    for skip in keys:
        flags = {k: k != skip for k in keys}
        part = qv.heavy_outputs_flat(n, pairs5, flat5, **flags)
        assert skip not in part
        for k in keys:
            if k != skip:
                assert np.array_equal(part[k], full[k]), (skip, k)
    for only in keys:
        one = qv.heavy_outputs_flat(n, pairs5, flat5, **{k: k == only for k in keys})
        assert list(one) == [only] and np.array_equal(one[only], full[only])
    # _dev form
    lib = _lib.lib()
    N, W = 1 << n, max(1, (1 << n) // 64)
    d_pairs = _lib.DeviceBuffer.from_array(pairs5.astype(np.uint8))
    d_gates = _lib.DeviceBuffer.from_array(flat5)
    d_p, d_m, d_k = _lib.DeviceBuffer(5 * N * 8), _lib.DeviceBuffer(5 * 8), _lib.DeviceBuffer(5 * W * 8)
    d_hp, d_hc = _lib.DeviceBuffer(5 * 8), _lib.DeviceBuffer(5 * 4)
    _lib.check(lib.fbx_qv_heavy_outputs_dev(n, 5, L, d_pairs.ptr, d_gates.ptr, d_p.ptr, d_m.ptr, d_k.ptr, d_hp.ptr, d_hc.ptr))
    _lib.synchronize()
    assert np.array_equal(d_p.to_array(np.float64, (5, N)), full["probabilities"])
    assert np.array_equal(d_m.to_array(np.float64, (5,)), full["median"])
    assert np.array_equal(d_k.to_array(np.uint64, (5, W)), full["mask"])
    assert np.array_equal(d_hp.to_array(np.float64, (5,)), full["heavy_prob"])
    assert np.array_equal(d_hc.to_array(np.int32, (5,)), full["heavy_count"])


def _count_case(n, shots, B, seed):
    from fbx import synthetic
    rng = np.random.default_rng(seed)
    p = rng.exponential(size=(B, 1 << n)); p /= p.sum(axis=1, keepdims=True)
    heavy = p > np.median(p, axis=1, keepdims=True)
    heavy[0] = False                                                    # an empty heavy set
    if B > 1:
        heavy[1] = False; heavy[1, (1 << n) - 1] = True                 # an all-but-empty one
    return synthetic.qv_shots(p, shots, depolarizing=0.2, seed=seed), heavy


@pytest.mark.parametrize("shots", [1, 1000, 1337])
@pytest.mark.parametrize("n", [2, 5, 6, 7, 13])
def test_heavy_counts(gpu, n, shots):
    """8. counts equal a direct numpy evaluation of the reference's loop (bit_array_to_int + membership)"""
    from fbx import quantum_volume as qv
    for B in (7, 2):                                                    # a wavefront per circuit, a workgroup per circuit
        bits, heavy = _count_case(n, shots, B, seed=n * 10 + B)
        want = qc.count_heavy_direct(bits, heavy)
        got = qv.count_heavy_hitters_sampled_batch(bits, heavy)
        assert got.dtype == np.int64 and np.array_equal(got, want), (n, shots, B, got, want)
        assert got[0] == 0
        assert np.array_equal(qv.count_heavy_hitters_sampled_batch(bits, qv.pack_heavy_mask(heavy)), want)
        lists = [[int(i) for i in np.flatnonzero(h)] for h in heavy]
        assert list(qv.count_heavy_hitters_sampled(iter(bits), iter(lists))) == [int(w) for w in want]
    assert qv.count_heavy_hitters_sampled_batch(bits[:0], heavy[:0]).shape == (0,)


def test_heavy_counts_long_records(gpu):
    from fbx import quantum_volume as qv
    for n in (3, 8, 13):
        bits, heavy = _count_case(n, 20011, 3, seed=n)
        assert np.array_equal(qv.count_heavy_hitters_sampled_batch(bits, heavy), qc.count_heavy_direct(bits, heavy))


@pytest.mark.parametrize("n", [4, 11])
def test_resident_pipeline(gpu, n):
    """9. gates generated on the device, simulated and counted through the _dev entry points without a copy in between"""
    from fbx import _lib, quantum_volume as qv, synthetic
    lib = _lib.lib()
    B, L, N, W, shots = 6, n * (n // 2), 1 << n, max(1, (1 << n) // 64), 500
    perms = np.stack([np.stack([np.random.default_rng([n, b, k]).permutation(n) for k in range(n)]) for b in range(B)])
    pairs = qv.layer_pairs(perms).reshape(B, L, 2)
    d_gates = _lib.DeviceBuffer(B * L * 16 * 16)
    _lib.check(lib.fbx_random_operators_dev(_lib.RAND_UNITARY, 4, 0, B * L, 1234, 0, d_gates.ptr))
    d_pairs = _lib.DeviceBuffer.from_array(pairs)
    d_mask, d_hp, d_counts = _lib.DeviceBuffer(B * W * 8), _lib.DeviceBuffer(B * 8), _lib.DeviceBuffer(B * 8)
    _lib.check(lib.fbx_qv_heavy_outputs_dev(n, B, L, d_pairs.ptr, d_gates.ptr, None, None, d_mask.ptr, d_hp.ptr, None))
    # host form on the downloaded gates
    _lib.synchronize()
    gates = d_gates.to_array(np.complex128, (B, L, 4, 4))
    assert np.abs(gates @ gates.conj().transpose(0, 1, 3, 2) - np.eye(4)).max() < 1e-12
    host = qv.heavy_outputs_flat(n, pairs, gates)
    bits = synthetic.qv_shots(host["probabilities"], shots, depolarizing=0.1, seed=n)
    d_bits = _lib.DeviceBuffer.from_array(bits)
    _lib.check(lib.fbx_qv_count_heavy_dev(n, B, shots, d_bits.ptr, d_mask.ptr, d_counts.ptr))
    _lib.synchronize()
    assert np.array_equal(d_mask.to_array(np.uint64, (B, W)), host["mask"])
    assert np.array_equal(d_hp.to_array(np.float64, (B,)), host["heavy_prob"])
    want = qv.count_heavy_hitters_sampled_batch(bits, host["mask"])
    assert np.array_equal(d_counts.to_array(np.int64, (B,)), want)
    assert np.array_equal(want, qc.count_heavy_direct(bits, qv.unpack_heavy_mask(host["mask"], n)))
    p2, g2 = qv.generate_abstract_qv_circuits_batch(n, 3, seed=9, first_item=2)
    p5, g5 = qv.generate_abstract_qv_circuits_batch(n, 5, seed=9)
    assert p2.shape == (3, n, n) and g2.shape == (3, n, n // 2, 4, 4)
    assert np.array_equal(p2, p5[2:]) and np.array_equal(g2, g5[2:])   # a circuit depends on (seed, id) only
    assert np.all(np.sort(p5, axis=-1) == np.arange(n))


def test_errors(gpu):
    """10. unsupported widths, bad pairs, wrong shapes; a NaN gate poisons its own item only"""
    import fbx
    from fbx import _lib, quantum_volume as qv
    lib = _lib.lib()
    for n in (1, 14):
        out = np.zeros(1 << n)
        rc = lib.fbx_qv_heavy_outputs(n, 1, 0, None, None, _lib.dptr(out), None, None, None, None)
        assert rc == _lib.FBX_ERR_UNSUPPORTED and b"2..13" in lib.fbx_last_error()
        rc = lib.fbx_qv_count_heavy(n, 1, 1, np.zeros(16, dtype=np.uint8).ctypes.data_as(C.POINTER(C.c_uint8)),
                                    np.zeros(256, dtype=np.uint64).ctypes.data_as(C.POINTER(C.c_uint64)),
                                    np.zeros(1, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64)))
        assert rc == _lib.FBX_ERR_UNSUPPORTED
    with pytest.raises(fbx.FbxError) as ei:
        qv.collect_heavy_outputs_batch(np.arange(14)[None, None].repeat(14, 1), np.broadcast_to(np.eye(4, dtype=complex), (1, 14, 7, 4, 4)))
    assert ei.value.code == _lib.FBX_ERR_UNSUPPORTED
    eye = np.eye(4, dtype=complex)[None, None]
    u8 = C.POINTER(C.c_uint8)
    for bad in ([(1, 1)], [(0, 3)]):                                     # equal qubits; an index out of range -- also in the C ABI
        with pytest.raises(ValueError):
            qv.heavy_outputs_flat(3, [bad], eye)
        pr = np.asarray([bad], dtype=np.uint8)
        out = np.zeros(8)
        rc = lib.fbx_qv_heavy_outputs(3, 1, 1, pr.ctypes.data_as(u8), _lib.dptr(eye.copy().view(np.float64)), _lib.dptr(out), None, None, None, None)
        assert rc == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_qv_heavy_outputs(3, 1, 0, None, None, None, None, None, None, None) == _lib.FBX_ERR_BAD_ARG      # no output at all
    assert lib.fbx_qv_heavy_outputs(3, 1, 1, None, None, _lib.dptr(np.zeros(8)), None, None, None, None) == _lib.FBX_ERR_BAD_ARG
    with pytest.raises(ValueError):
        qv.heavy_outputs_flat(3, [[(0, 1)]], np.zeros((1, 1, 4, 3), dtype=complex))
    for n in (5, 10):
        perms, gates = qc.random_circuits(n, 6, seed=600 + n, min_gap=0.0)
        L = n * (n // 2)
        pairs, flat = qv.layer_pairs(perms).reshape(6, L, 2), gates.reshape(6, L, 4, 4).copy()
        clean = qv.heavy_outputs_flat(n, pairs, flat)
        for poison in (np.nan, np.inf):
            dirty = flat.copy()
            dirty[2, L // 2, 1, 2] = poison
            r = qv.heavy_outputs_flat(n, pairs, dirty)
            keep = [0, 1, 3, 4, 5]
            for k in r:
                assert np.array_equal(r[k][keep], clean[k][keep]), (n, k)
            assert np.isnan(r["probabilities"][2]).all() and np.isnan(r["median"][2]) and np.isnan(r["heavy_prob"][2])
            assert r["heavy_count"][2] == 0 and not r["mask"][2].any()
