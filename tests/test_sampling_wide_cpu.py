"""fbx_sample_bitstrings_wide without a device: the seven-block restatement of its stream against the four-block one, the argument
checks of the two C entry points (which come before any device work), the workspace option and the dispatch of the Python
functions on the width."""
import ctypes as C

import numpy as np
import pytest

import sampling_cases as sc
import sampling_wide_cases as swc

KAT_ZERO = [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]           # Random123: philox4x32_10, counter 0 0 0 0, key 0 0


def test_both_symbols_exist():
    from fbx import _lib
    lib = _lib.lib()
    assert callable(lib.fbx_sample_bitstrings_wide) and callable(lib.fbx_sample_bitstrings_wide_dev)
    assert "fbx_sample_bitstrings_wide" in _lib.PROTOTYPES and "fbx_sample_bitstrings_wide_dev" in _lib.PROTOTYPES


def test_word_layout_by_hand():
    """4 ceil((2 + n) / 4) words per shot, block t = words 4 t .. 4 t + 3, and column j reads word 2 + j: at width 26 the last
    column reads word 27 = the last word of block 6."""
    assert [swc.words(0, 0, 1, n).shape[1] for n in (14, 15, 18, 19, 22, 23, 26)] == [16, 20, 20, 24, 24, 28, 28]
    x = swc.words(0, 0, 3, 26)
    assert x.shape == (3, 28) and x.dtype == np.uint32
    assert [int(v) for v in x[0, :4]] == KAT_ZERO
    for t in range(7):
        assert np.array_equal(x[2, 4 * t:4 * t + 4], sc.block(0, 0, 2, t)[0])
    assert np.array_equal(x[:, :16], sc.words(0, 0, 3))                 # widths up to 13 read the same words as before
    y = swc.words(7, (5 << 32) | 9, 2, 17)
    assert np.array_equal(y[1, 16:20], sc.block(7, (5 << 32) | 9, 1, 4)[0])
    # column 25 of a width-26 record whose drawn bits are all 0 flips iff x_27 2^-32 is below its threshold
    r27 = float(x[1, 27]) * 2.0 ** -32
    flip = np.zeros((26, 2))
    flip[25, 0] = np.nextafter(r27, 1.0)
    assert sc.apply_flips(np.zeros((3, 26), dtype=np.uint8), flip, x)[1].tolist() == [0] * 25 + [1]
    flip[25, 0] = r27
    assert sc.apply_flips(np.zeros((3, 26), dtype=np.uint8), flip, x)[1].tolist() == [0] * 26


def test_dyadic_weights_cross_the_blocks():
    p = swc.dyadic_weights_wide(14, 2, seed=3)
    N = p.shape[1]
    for i in (0, N - 1, 4095, 4096, N - 4097, N - 4096):
        assert np.all(p[:, i] == 0.0)
    assert np.all(p[:, 8192:12288] == 0.0) and np.all(p[:, 4097:8192].sum(axis=1) > 0.0)
    assert 0.25 < (p == 0.0).mean() < 0.6
    assert np.all(p * 2.0 ** 30 == np.round(p * 2.0 ** 30))
    w = sc.weights(p[0], 0.25)
    assert np.all(w * 2.0 ** 32 == np.round(w * 2.0 ** 32)) and np.cumsum(w)[-1] == 1.0
    bits, drawn, _ = swc.restate(p[0], 3000, 0.0, seed=5, g=2)
    assert np.all(p[0][drawn] > 0.0) and np.array_equal(sc.from_bits(bits), drawn)


def _call(lib, n, B, shots, first_item=0, dev=False):
    """a call with valid (host) buffers of the smallest shape that fits a legal (n, B, shots); the _dev form gets no buffers"""
    if dev:
        return lib.fbx_sample_bitstrings_wide_dev(n, B, shots, None, None, None, 7, first_item, None, None)
    N = 1 << max(min(n, 14), 1)
    p = np.full((max(B, 1), N), 1.0 / N)
    bits = np.zeros(max(B, 1) * max(min(shots, 4), 1) * max(n, 1), dtype=np.uint8)
    return lib.fbx_sample_bitstrings_wide(n, B, shots, p.ctypes.data_as(C.POINTER(C.c_double)), None, None, 7, first_item,
                                          bits.ctypes.data_as(C.POINTER(C.c_uint8)), None)


def test_widths_outside_14_to_26_are_unsupported():
    from fbx import _lib
    lib = _lib.lib()
    for n in (0, 13, 27, -3):
        assert _call(lib, n, 1, 4) == _lib.FBX_ERR_UNSUPPORTED
        assert b"14..26" in lib.fbx_last_error()
        assert _call(lib, n, 1, 4, dev=True) == _lib.FBX_ERR_UNSUPPORTED          # before any buffer is looked at


def test_bad_sizes_and_null_buffers_are_bad_arguments():
    from fbx import _lib
    lib = _lib.lib()
    assert _call(lib, 14, 1, 2 ** 32) == _lib.FBX_ERR_BAD_ARG
    assert b"2^32" in lib.fbx_last_error()
    assert _call(lib, 14, -1, 4) == _lib.FBX_ERR_BAD_ARG
    assert _call(lib, 14, 1, -4) == _lib.FBX_ERR_BAD_ARG
    assert _call(lib, 14, 1, 4, first_item=-1) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_sample_bitstrings_wide(14, 1, 4, None, None, None, 7, 0, None, None) == _lib.FBX_ERR_BAD_ARG
    assert _call(lib, 14, 1, 4, dev=True) == _lib.FBX_ERR_BAD_ARG
    assert _call(lib, 20, 2 ** 62, 2 ** 31, dev=True) == _lib.FBX_ERR_BAD_ARG      # NULL buffers, and B * n_shots * n overflows
    with pytest.raises(ValueError):
        _lib.check(_call(lib, 14, 1, 2 ** 32))


def test_empty_calls_behave_as_the_narrow_entry_point():
    """B == 0 or n_shots == 0: nothing to do; with or without a device the wide form answers what the narrow one answers"""
    from fbx import _lib
    lib = _lib.lib()
    for B, shots in ((0, 4), (1, 0), (0, 0)):
        narrow = lib.fbx_sample_bitstrings_dev(3, B, shots, None, None, None, 7, 0, None, None)
        assert narrow in (_lib.FBX_OK, _lib.FBX_ERR_NO_DEVICE)
        assert _call(lib, 14, B, shots, dev=True) == narrow
        assert _call(lib, 14, B, shots) == narrow


def test_workspace_option():
    from fbx import _lib
    lib = _lib.lib()
    v = C.c_double(0.0)
    assert lib.fbx_get_option(b"sample_wide_workspace_mib", C.byref(v)) == 0 and v.value == 128.0
    assert lib.fbx_set_option(b"sample_wide_workspace_mib", C.c_double(0.5)) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_set_option(b"sample_wide_workspace_mib", C.c_double(1e6)) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_get_option(b"sample_wide_workspace_mib", C.byref(v)) == 0 and v.value == 128.0
    with _lib.option("sample_wide_workspace_mib", 1.0):
        assert _lib.get_option("sample_wide_workspace_mib") == 1.0
    assert _lib.get_option("sample_wide_workspace_mib") == 128.0
    assert _lib.get_option("qv_wide_workspace_mib") == 128.0              # its neighbour is another option


def test_python_functions_dispatch_on_the_width(monkeypatch):
    """below 14 qubits the wide functions ARE the narrow ones: same arguments in, their result out"""
    import fbx
    from fbx import _lib, quantum_volume as qv, sampling, synthetic
    assert "sample_bitstrings_wide_batch" in sampling.__all__
    assert "simulate_heavy_output_counts_wide_batch" in qv.__all__
    seen = []
    monkeypatch.setattr(sampling, "sample_bitstrings_batch", lambda *a, **k: seen.append((a, k)) or "narrow")
    p = np.full((2, 8), 0.125)
    assert sampling.sample_bitstrings_wide_batch(p, 5, 0.1, None, 3, 4, True) == "narrow"
    (a, k), = seen
    assert a[0] is p or np.array_equal(a[0], p)
    assert a[1:] == (5, 0.1, None, 3, 4, True) and not k
    assert synthetic.qv_shots_wide_batch(p, 5, seed=9) == "narrow"
    monkeypatch.setattr(qv, "simulate_heavy_output_counts_batch", lambda *a, **k: ("narrow", a[2:], k))
    perms = np.stack([np.stack([np.random.default_rng(l).permutation(5) for l in range(5)])])
    gates = np.broadcast_to(np.eye(4, dtype=np.complex128), (1, 5, 2, 4, 4))
    got = qv.simulate_heavy_output_counts_wide_batch(perms, gates, 10, 0.2, None, 4, "disjoint", tile_bits=12, max_resident_mib=1)
    assert got == ("narrow", (10, 0.2, None, 4, "disjoint"), {})
    # the arguments of the wide tier are checked whatever the width
    with pytest.raises(ValueError):
        qv.simulate_heavy_output_counts_wide_batch(perms, gates, 10, tile_bits=5)
    with pytest.raises(ValueError):
        qv.simulate_heavy_output_counts_wide_batch(perms, gates, 10, max_resident_mib=0)
    with pytest.raises(ValueError):
        sampling.sample_bitstrings_wide_batch(np.full((2, 6), 1.0), 4)
    with pytest.raises(ValueError):
        sampling.sample_bitstrings_wide_batch(np.full((1, 1 << 14), 1.0), 4, readout_flip=np.zeros((13, 2)))
    with pytest.raises(fbx.FbxError) as ei:
        sampling.sample_bitstrings_wide_batch(np.broadcast_to(np.float64(1.0), (1, 1 << 27)), 1, seed=1)
    assert ei.value.code == _lib.FBX_ERR_UNSUPPORTED


def test_no_device_fails_loudly():
    """Without a GPU a valid wide call reports FBX_ERR_NO_DEVICE -- there is no host sampler behind it."""
    import fbx
    from fbx import _lib, sampling, synthetic
    if fbx.device_count() > 0:
        pytest.skip("a GPU is visible")
    assert _call(_lib.lib(), 14, 1, 4) == _lib.FBX_ERR_NO_DEVICE
    for call in (lambda: sampling.sample_bitstrings_wide_batch(np.full((1, 1 << 14), 1.0), 4, seed=1),
                 lambda: synthetic.qv_shots_wide_batch(np.full((1, 1 << 14), 1.0), 4)):
        with pytest.raises(fbx.FbxError) as ei:
            call()
        assert ei.value.code == _lib.FBX_ERR_NO_DEVICE
