"""The wide quantum-volume tier (widths 14..26) without a device: the numpy mirror of the pass planner, a numpy executor of its
plans against the restatement of tests/qv_cases.py, and the argument checks that are made before a device is needed."""
import numpy as np
import pytest

import qv_cases as qc

LOW = 0b111                                                  # index bits 0..2 are always local


def _random_pairs(n, pairing, seed, layers=None):
    rng = np.random.default_rng(seed)
    perms = np.stack([rng.permutation(n) for _ in range(layers or n)])
    return qc.pairs_of(perms, pairing)


def _bits(n, pair):
    return (1 << (n - 1 - int(pair[0]))) | (1 << (n - 1 - int(pair[1])))


@pytest.mark.parametrize("tile_bits", [8, 12, 13])
@pytest.mark.parametrize("pairing", ["reference", "disjoint"])
@pytest.mark.parametrize("n", [14, 17])
def test_plan_properties(n, pairing, tile_bits):
    from fbx import quantum_volume as qv
    for seed in range(6):
        pairs = _random_pairs(n, pairing, 1000 * n + seed)
        L = len(pairs)
        n_passes, first, masks = qv.plan_wide_passes(n, pairs, tile_bits)
        assert first.shape == (L + 1,) and masks.shape == (L,) and first.dtype == np.int32 and masks.dtype == np.uint32
        # the passes partition 0..L in order; entries past the last pass are L and 0
        assert 1 <= n_passes <= L and first[0] == 0 and np.all(first[n_passes:] == L) and np.all(masks[n_passes:] == 0)
        assert np.all(np.diff(first[:n_passes + 1]) >= 1)
        for k in range(n_passes):
            m = int(masks[k])
            assert bin(m).count("1") == tile_bits and m < (1 << n) and m & LOW == LOW
            need = LOW
            for l in range(first[k], first[k + 1]):
                assert _bits(n, pairs[l]) & ~m == 0, (k, l)
                need |= _bits(n, pairs[l])
            if k + 1 < n_passes:                             # maximal: the next pass's first gate does not fit beside these targets
                assert bin(need | _bits(n, pairs[first[k + 1]])).count("1") > tile_bits, k
    # the batched form is the single form, circuit by circuit; L = 0 is no pass at all
    stack = np.stack([_random_pairs(n, pairing, 77 + b) for b in range(3)])
    nb, fb, mb = qv.plan_wide_passes(n, stack, tile_bits)
    for b in range(3):
        n1, f1, m1 = qv.plan_wide_passes(n, stack[b], tile_bits)
        assert nb[b] == n1 and np.array_equal(fb[b], f1) and np.array_equal(mb[b], m1)
    n0, f0, m0 = qv.plan_wide_passes(n, np.zeros((0, 2), dtype=np.int64), tile_bits)
    assert n0 == 0 and f0.tolist() == [0] and m0.shape == (0,)


def test_plan_default_tile_and_argument_checks():
    from fbx import quantum_volume as qv
    pairs = _random_pairs(14, "reference", 5)
    a, b = qv.plan_wide_passes(14, pairs), qv.plan_wide_passes(14, pairs, 13)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    for bad in ([(3, 3)], [(0, 14)]):
        with pytest.raises(ValueError):
            qv.plan_wide_passes(14, bad, 12)
    for n, t in ((13, 12), (27, 12), (14, 7), (14, 14)):
        with pytest.raises(ValueError):
            qv.plan_wide_passes(n, pairs[:0], t)


def _deposit(v, mask):
    """bits of v (array), lowest first, on the set bits of mask, lowest first"""
    out = np.zeros_like(v)
    k = 0
    for p in range(32):
        if (mask >> p) & 1:
            out |= ((v >> k) & 1) << p
            k += 1
    return out


def _execute_plan(n, T, pairs, gates, plan):
    """the circuit run pass by pass, tile by tile, as the device does it: gather a tile, apply the pass's gates on LOCAL bit
    positions, scatter it back"""
    n_passes, first, masks = plan
    N = 1 << n
    state = np.zeros(N, dtype=np.complex128)
    state[0] = 1.0
    for k in range(n_passes):
        m = int(masks[k])
        tiles = _deposit(np.arange(N >> T, dtype=np.int64), ~m & (N - 1))
        local = _deposit(np.arange(1 << T, dtype=np.int64), m)
        idx = tiles[:, None] | local[None, :]
        assert np.array_equal(np.sort(idx.reshape(-1)), np.arange(N))           # the tiles partition the state
        assert np.all(np.diff(idx.reshape(-1, 8), axis=1) == 1)                # runs of 8 amplitudes are contiguous
        t = state[idx].reshape((N >> T,) + (2,) * T)                            # axis 1 + a = local bit T - 1 - a
        for l in range(first[k], first[k + 1]):
            ax = []
            for q in pairs[l]:
                p = n - 1 - int(q)
                ax.append(1 + T - 1 - bin(m & ((1 << p) - 1)).count("1"))
            u = np.asarray(gates[l], dtype=np.complex128).reshape(2, 2, 2, 2)
            t = np.moveaxis(np.tensordot(u, t, axes=((2, 3), ax)), (0, 1), ax)
        state[idx] = t.reshape(N >> T, 1 << T)
    return np.abs(state) ** 2


@pytest.mark.parametrize("pairing", ["reference", "disjoint"])
def test_numpy_executor_of_the_plan_reproduces_the_simulation(pairing):
    from fbx import quantum_volume as qv
    n, T = 14, 8
    perms, gates = qc.random_circuits(n, 1, seed=1400, min_gap=0.0)
    pairs, flat = qc.pairs_of(perms[0], pairing), gates[0].reshape(-1, 4, 4)
    want = qc.simulate(n, pairs, flat)
    got = _execute_plan(n, T, pairs, flat, qv.plan_wide_passes(n, pairs, T))
    err, bound = np.abs(got - want), qc.prob_bound(want, len(pairs))
    print(f"plan executor width {n} tile {T} {pairing}: max |dp| {err.max():.3e}, bound at max p {bound.max():.3e}")
    assert np.all(err <= bound)


def test_python_layer_checks():
    import fbx
    from fbx import _lib, quantum_volume as qv
    assert (qv.MIN_WIDTH, qv.MAX_WIDTH) == (2, 13)
    for name in ("heavy_outputs_flat_wide", "collect_heavy_outputs_wide_batch", "ideal_heavy_output_probability_wide_batch",
                 "count_heavy_hitters_sampled_wide_batch", "plan_wide_passes"):
        assert name in qv.__all__ and callable(getattr(qv, name))
    eye = np.eye(4, dtype=complex)
    with pytest.raises(fbx.FbxError) as ei:                                     # width 27: refused before anything is allocated
        qv.heavy_outputs_flat_wide(27, np.zeros((1, 0, 2), dtype=np.uint8), np.zeros((1, 0, 4, 4), dtype=complex))
    assert ei.value.code == _lib.FBX_ERR_UNSUPPORTED
    with pytest.raises(fbx.FbxError) as ei:
        qv.collect_heavy_outputs_wide_batch(np.arange(27)[None, None], np.broadcast_to(eye, (1, 1, 13, 4, 4)))
    assert ei.value.code == _lib.FBX_ERR_UNSUPPORTED
    with pytest.raises(fbx.FbxError) as ei:
        qv.count_heavy_hitters_sampled_wide_batch(np.zeros((1, 1, 27), dtype=np.uint8), np.zeros((1, 1 << 21), dtype=np.uint64))
    assert ei.value.code == _lib.FBX_ERR_UNSUPPORTED
    for t in (7, 14, -1):
        with pytest.raises(ValueError):
            qv.heavy_outputs_flat_wide(14, [[(0, 1)]], eye[None, None], tile_bits=t)
    with pytest.raises(ValueError):
        qv.heavy_outputs_flat_wide(14, [[(0, 1, 2)]], eye[None, None])           # pairs must be [B, L, 2]
    with pytest.raises(ValueError):
        qv.heavy_outputs_flat_wide(14, [[(0, 1)]], np.zeros((1, 1, 4, 3), dtype=complex))
    with pytest.raises(ValueError):
        qv.heavy_outputs_flat_wide(14, [[(0, 14)]], eye[None, None])             # out of range
    with pytest.raises(ValueError):
        qv.heavy_outputs_flat_wide(14, [[(5, 5)]], eye[None, None])              # equal qubits
    with pytest.raises(ValueError):
        qv.heavy_outputs_flat_wide(14, [[(0, 1)]], eye[None, None], probabilities=False, median=False, mask=False,
                                   heavy_prob=False, heavy_count=False)
    with pytest.raises(ValueError):
        qv.count_heavy_hitters_sampled_wide_batch(np.zeros((1, 4, 14), dtype=np.uint8), np.zeros((1, 3), dtype=np.uint64))
    with pytest.raises(ValueError):
        qv.count_heavy_hitters_sampled_wide_batch(np.full((1, 4, 14), 2), np.zeros((1, 256), dtype=np.uint64))


def test_wide_abi_refuses_other_widths_without_a_device():
    """widths 13 and 27 through the _wide C ABI: FBX_ERR_UNSUPPORTED with the range in the message, before a device is looked for"""
    import ctypes as C
    from fbx import _lib
    lib = _lib.lib()
    out = np.zeros(1)
    u8, u64, i64 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
    for n in (13, 27):
        rc = lib.fbx_qv_heavy_outputs_wide(n, 1, 0, None, None, 0, None, _lib.dptr(out), None, None, None)
        assert rc == _lib.FBX_ERR_UNSUPPORTED and b"14..26" in lib.fbx_last_error()
        rc = lib.fbx_qv_heavy_outputs_wide_dev(n, 1, 0, None, None, 0, None, out.ctypes.data_as(C.c_void_p), None, None, None)
        assert rc == _lib.FBX_ERR_UNSUPPORTED and b"14..26" in lib.fbx_last_error()
        rc = lib.fbx_qv_count_heavy_wide(n, 1, 1, np.zeros(32, dtype=np.uint8).ctypes.data_as(u8),
                                         np.zeros(1, dtype=np.uint64).ctypes.data_as(u64), np.zeros(1, dtype=np.int64).ctypes.data_as(i64))
        assert rc == _lib.FBX_ERR_UNSUPPORTED and b"14..26" in lib.fbx_last_error()
        rc = lib.fbx_qv_wide_plan(n, 1, 0, None, 0, _lib.iptr(np.zeros(1, dtype=np.int32)), _lib.iptr(np.zeros(1, dtype=np.int32)), None)
        assert rc == _lib.FBX_ERR_UNSUPPORTED and b"14..26" in lib.fbx_last_error()
    for t in (7, 14):
        rc = lib.fbx_qv_heavy_outputs_wide(14, 1, 0, None, None, t, None, _lib.dptr(out), None, None, None)
        assert rc == _lib.FBX_ERR_BAD_ARG and b"tile_bits" in lib.fbx_last_error()
    assert lib.fbx_qv_heavy_outputs_wide(14, 1, 0, None, None, 0, None, None, None, None, None) == _lib.FBX_ERR_BAD_ARG
    v = C.c_double()
    assert lib.fbx_get_option(b"qv_wide_workspace_mib", C.byref(v)) == 0 and v.value == 128.0
    assert lib.fbx_set_option(b"qv_wide_workspace_mib", C.c_double(0.5)) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_set_option(b"qv_wide_workspace_mib", C.c_double(1e6)) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_get_option(b"qv_wide_workspace_mib", C.byref(v)) == 0 and v.value == 128.0
