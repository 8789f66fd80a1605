"""fbx_sample_bitstrings without a device: the host restatement of its stream against the Random123 known answers, and the
argument checks of the C entry points (which come before any device work)."""
import ctypes as C

import numpy as np
import pytest

import sampling_cases as sc

# Random123 kat_vectors, philox4x32_10 <counter> <key> -> <output> (the vectors of tests/test_resample_cpu.py)
KAT_ZERO = [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]                       # counter 0 0 0 0, key 0 0
KAT_ONES = [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]                       # counter ffffffff x 4, key ffffffff x 2
KAT_PI = [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]      # counter 243f6a88 85a308d3 13198a2e 03707344, key a4093822 299f31d0


def test_counter_and_key_layout_against_the_known_answers():
    """counter = (g low, g high, s, t), key = (seed low, seed high): the three vectors, read as (seed, g, s, t)"""
    assert [int(v) for v in sc.block(0, 0, 0, 0)[0]] == KAT_ZERO
    assert [int(v) for v in sc.block(0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)[0]] == KAT_ONES
    assert [int(v) for v in sc.block(0x299f31d0a4093822, 0x85a308d3243f6a88, 0x13198a2e, 0x03707344)[0]] == KAT_PI
    # shot 0 of item 0 under seed 0 is the first vector; its block 0 is words 0..3 of the shot
    x = sc.words(0, 0, 3)
    assert x.shape == (3, 16) and [int(v) for v in x[0, :4]] == KAT_ZERO
    assert [int(v) for v in x[2, 4:8]] == [int(v) for v in sc.block(0, 0, 2, 1)[0]]


def test_draw_and_flip_words_by_hand():
    """u = k 2^-53 with k = ((x_0 >> 5) << 26) | (x_1 >> 6), worked out by hand for the three vectors:
         6627e8d5 >> 5 = 0x3313f46, e169c58d >> 6 = 0x385a716  ->  k = 0x3313f46 * 2^26 + 0x385a716
         408f276d >> 5 = 0x204793b, 41c83b0e >> 6 = 0x10720ec
         d16cfe09 >> 5 = 0x68b67f0, 94fdcceb >> 6 = 0x253f733
    and the flip word of column j is x_{2 + j}: columns 0 and 1 read words 2 and 3 of block 0."""
    by_hand = [(KAT_ZERO, 0x3313f46, 0x385a716), (KAT_ONES, 0x204793b, 0x10720ec), (KAT_PI, 0x68b67f0, 0x253f733)]
    for x, hi, lo in by_hand:
        k = hi * 2 ** 26 + lo
        arr = np.array([x + [0] * 12], dtype=np.uint32)
        assert int(sc.draw_integers(arr)[0]) == k
        u = sc.uniforms(arr)[0]
        assert 0.0 <= u < 1.0 and u == k / 2.0 ** 53 and int(u * 2 ** 53) == k
    x = sc.words(0, 0, 1)
    assert sc.uniforms(x)[0] == (0x3313f46 * 2 ** 26 + 0x385a716) / 2.0 ** 53
    # 0xbc57ac4c / 2^32 = 0.7357...: column 0 (drawn 0) flips for a threshold of 0.75 and not for 0.5; 0x9b00dbd8 / 2^32 = 0.6054...
    bits = np.zeros((1, 2), dtype=np.uint8)
    assert sc.apply_flips(bits, np.array([[0.75, 0.0], [0.5, 0.0]]), x).tolist() == [[1, 0]]
    assert sc.apply_flips(bits, np.array([[0.5, 1.0], [0.625, 1.0]]), x).tolist() == [[0, 1]]
    assert sc.apply_flips(1 - bits, np.array([[0.0, 0.75], [0.0, 0.5]]), x).tolist() == [[0, 1]]


def test_restatement_never_draws_a_weightless_outcome_and_follows_the_distribution():
    p = sc.dyadic_weights(4, 3, seed=11)
    assert p[0, 0] == 0.0 and p[0, -1] == 0.0
    for lam in (0.0, 0.25):
        bits, drawn = sc.restate(p[0], 20000, lam, seed=5, g=9)
        w = sc.weights(p[0], lam)
        assert np.all(w[drawn] > 0.0) and np.array_equal(sc.from_bits(bits), drawn)
        freq = np.bincount(drawn, minlength=16) / 20000.0
        assert np.abs(freq - w).max() < 5.0 * np.sqrt(0.25 / 20000.0)


def _call(lib, n, B, shots, first_item=0):
    """a call with valid buffers of the smallest shape that fits a legal (n, B, shots)"""
    N = 1 << max(min(n, 13), 1)
    p = np.full((max(B, 1), N), 1.0 / N)
    bits = np.zeros(max(B, 1) * max(min(shots, 4), 1) * max(n, 1), dtype=np.uint8)
    return lib.fbx_sample_bitstrings(n, B, shots, p.ctypes.data_as(C.POINTER(C.c_double)), None, None, 7, first_item,
                                     bits.ctypes.data_as(C.POINTER(C.c_uint8)), None)


def test_widths_outside_1_to_13_are_unsupported():
    from fbx import _lib
    lib = _lib.lib()
    for n in (0, 14, -3):
        assert _call(lib, n, 1, 4) == _lib.FBX_ERR_UNSUPPORTED
        assert b"1..13" in lib.fbx_last_error()
        assert lib.fbx_sample_bitstrings_dev(n, 1, 4, None, None, None, 7, 0, None, None) == _lib.FBX_ERR_UNSUPPORTED


def test_bad_sizes_and_null_buffers_are_bad_arguments():
    from fbx import _lib
    lib = _lib.lib()
    assert _call(lib, 3, 1, 2 ** 32) == _lib.FBX_ERR_BAD_ARG
    assert b"2^32" in lib.fbx_last_error()
    assert _call(lib, 3, -1, 4) == _lib.FBX_ERR_BAD_ARG
    assert _call(lib, 3, 1, -4) == _lib.FBX_ERR_BAD_ARG
    assert _call(lib, 3, 1, 4, first_item=-1) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_sample_bitstrings(3, 1, 4, None, None, None, 7, 0, None, None) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_sample_bitstrings_dev(3, 1, 4, None, None, None, 7, 0, None, None) == _lib.FBX_ERR_BAD_ARG
    with pytest.raises(ValueError):
        _lib.check(_call(lib, 3, 1, 2 ** 32))


def test_front_end_checks_shapes_without_a_device():
    from fbx import sampling
    p = np.full((2, 8), 0.125)
    for kwargs in ({"depolarizing": [0.1, 0.2, 0.3]}, {"readout_flip": np.zeros((4, 2))}, {"readout_flip": np.zeros((3, 3, 2))},
                   {"first_item": -1}):
        with pytest.raises(ValueError):
            sampling.sample_bitstrings_batch(p, 4, **kwargs)
    with pytest.raises(ValueError):
        sampling.sample_bitstrings_batch(p, -1)
    with pytest.raises(ValueError):
        sampling.sample_bitstrings_batch(np.full((2, 6), 1.0), 4)


def test_no_device_fails_loudly():
    """Without a GPU a valid call reports FBX_ERR_NO_DEVICE -- there is no host sampler behind it."""
    import fbx
    from fbx import _lib, sampling, synthetic
    if fbx.device_count() > 0:
        pytest.skip("a GPU is visible")
    assert _call(_lib.lib(), 3, 1, 4) == _lib.FBX_ERR_NO_DEVICE
    for call in (lambda: sampling.sample_bitstrings_batch(np.full((2, 8), 0.125), 4, seed=1),
                 lambda: synthetic.qv_shots_batch(np.full((2, 8), 0.125), 4),
                 lambda: synthetic.readout_shots_batch(np.eye(4), 4)):
        with pytest.raises(fbx.FbxError) as ei:
            call()
        assert ei.value.code == _lib.FBX_ERR_NO_DEVICE
