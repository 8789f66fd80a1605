"""fbx_bit_histogram / fbx_counts_to_frequencies on the GPU against the numpy model of tests/readout_cases.py (np.bincount on the
packed index; pinned to the reference by tests/test_readout_cpu.py).  Counts are integers and are compared EXACTLY; frequencies are
compared bit for bit with numpy's counts / n_shots (one IEEE division on either side).

Shapes: every column count with a load path of its own (1, 2, 4, 8: whole vectors; 3, 5: packed; 11: byte-wise), shot counts with
no vector at all, a head and a tail (1, 15, 16, 17, 1000, 4099), batches around the four records of a workgroup (1, 3, 4, 5), records
whose size is no multiple of 16 bytes (every record after the first starts misaligned), a device buffer at a 1-byte offset, one record
on each side of the launcher's wavefront / workgroup switch (_lib.HIST_WAVE_BYTES, csrc/fbx_histogram.hip), and more records than the
capped grid has wavefronts (4 x 256 x 16), which runs the grid-stride loop and catches bins that are not cleared between records."""
import ctypes as C

import numpy as np
import pytest

import readout_cases as rc

pytestmark = pytest.mark.gpu
U8 = C.POINTER(C.c_uint8)
I64 = C.POINTER(C.c_int64)
KINDS = {rc.JOINT: 0, rc.WEIGHT: 1}
GRID_WAVEFRONTS = 4 * 256 * 16


def n_bins(k, kind):
    return 1 << k if kind == rc.JOINT else k + 1


def prepared(bits, cols, expected):
    bits = np.ascontiguousarray(bits, dtype=np.uint8)
    B = bits.shape[0]
    c = None if cols is None else np.ascontiguousarray(cols, dtype=np.uint8)
    k = bits.shape[2] if c is None else c.shape[-1]
    e = None if expected is None else np.ascontiguousarray(np.broadcast_to(np.asarray(expected, dtype=np.uint8), (B, k)))
    return bits, c, k, e


def host_hist(lib_mod, bits, cols=None, expected=None, kind=rc.JOINT):
    bits, c, k, e = prepared(bits, cols, expected)
    B, n_shots, n_cols = bits.shape
    out = np.full((B, n_bins(k, kind)), -7, dtype=np.int64)
    lib_mod.check(lib_mod.lib().fbx_bit_histogram(n_cols, B, n_shots, bits.ctypes.data_as(U8), k, None if c is None else c.ctypes.data_as(U8),
                                                  int(c is None or c.ndim == 1), None if e is None else e.ctypes.data_as(U8), KINDS[kind],
                                                  out.ctypes.data_as(I64)))
    return out


def dev_hist(lib_mod, bits, cols=None, expected=None, kind=rc.JOINT, offset=0):
    """the _dev form on caller-owned buffers; the record buffer starts `offset` bytes into its allocation"""
    bits, c, k, e = prepared(bits, cols, expected)
    B, n_shots, n_cols = bits.shape
    lib = lib_mod.lib()
    d_bits = lib_mod.DeviceBuffer(bits.nbytes + 16)
    lib_mod.check(lib.fbx_memcpy_h2d(d_bits.ptr.value + offset, bits.ctypes.data, bits.nbytes))
    d_c = None if c is None else lib_mod.DeviceBuffer.from_array(c)
    d_e = None if e is None else lib_mod.DeviceBuffer.from_array(e)
    d_out = lib_mod.DeviceBuffer(B * n_bins(k, kind) * 8)
    lib_mod.check(lib.fbx_bit_histogram_dev(n_cols, B, n_shots, d_bits.ptr.value + offset, k, None if d_c is None else d_c.ptr,
                                            int(c is None or c.ndim == 1), None if d_e is None else d_e.ptr, KINDS[kind], d_out.ptr))
    lib_mod.synchronize()
    out = d_out.to_array(np.int64, (B, n_bins(k, kind)))
    for buf in (d_bits, d_c, d_e, d_out):
        if buf is not None:
            buf.free()
    return out


def agree(lib_mod, bits, cols=None, expected=None, kind=rc.JOINT, tag=None):
    want = rc.histogram(bits, cols, expected, kind)
    got = host_hist(lib_mod, bits, cols, expected, kind)
    assert got.dtype == np.int64 and np.array_equal(got, want), (tag, kind, bits.shape, np.argwhere(got != want)[:4])
    assert (got.sum(axis=1) == bits.shape[1]).all()
    return got


@pytest.mark.parametrize("n_cols", [1, 2, 3, 4, 5, 8, 11])
def test_load_paths_heads_and_tails(gpu, n_cols):
    rng = np.random.default_rng(100 + n_cols)
    k = min(n_cols, 10)
    for n_shots in (1, 15, 16, 17, 1000, 4099):
        for B in (1, 3, 4, 5):
            bits = rc.random_bits(rng, B, n_shots, n_cols, high_bits=True)          # bytes 0..3: only bit 0 counts
            cols = None if n_cols <= 10 else rng.permutation(n_cols)[:k]
            agree(gpu, bits, cols, None, rc.JOINT, tag=(n_shots, B))
            wcols = rng.permutation(n_cols)
            agree(gpu, bits, wcols, rng.integers(0, 2, size=(B, n_cols)), rc.WEIGHT, tag=(n_shots, B))


@pytest.mark.parametrize("n_cols", [1, 2, 3, 5, 8, 11])
def test_dev_form_at_a_one_byte_offset_and_against_the_host_form(gpu, n_cols):
    rng = np.random.default_rng(200 + n_cols)
    for n_shots, B in ((17, 5), (1000, 4), (4099, 3)):
        bits = rc.random_bits(rng, B, n_shots, n_cols, high_bits=True)
        k = min(n_cols, 10)
        cols = rng.permutation(n_cols)[:k]
        for kind in (rc.JOINT, rc.WEIGHT):
            expected = rng.integers(0, 2, size=(B, k))
            want = rc.histogram(bits, cols, expected, kind)
            host = host_hist(gpu, bits, cols, expected, kind)
            for offset in (0, 1):
                assert np.array_equal(dev_hist(gpu, bits, cols, expected, kind, offset=offset), want), (n_shots, kind, offset)
            assert np.array_equal(host, want)


def test_both_sides_of_the_wavefront_workgroup_switch(gpu):
    rng = np.random.default_rng(3)
    limit = gpu.HIST_WAVE_BYTES
    for n_cols in (1, 3, 11):
        below = (limit - 1) // n_cols                                   # the longest record a wavefront takes
        above = -(-limit // n_cols)                                     # the shortest one a workgroup takes
        assert below * n_cols < limit <= above * n_cols
        for n_shots in (below, above):
            bits = rc.random_bits(rng, 4, n_shots, n_cols)
            agree(gpu, bits, None if n_cols <= 10 else np.arange(10), None, rc.JOINT, tag=n_shots)
            agree(gpu, bits, None, rng.integers(0, 2, size=(4, n_cols)), rc.WEIGHT, tag=n_shots)
    bits = rc.random_bits(rng, 3, 1000, 2)                              # fewer than four records: a workgroup each, however short
    agree(gpu, bits)


def test_more_records_than_wavefronts(gpu):
    rng = np.random.default_rng(4)
    B = GRID_WAVEFRONTS + 5
    bits = rc.random_bits(rng, B, 16, 2)
    bits[1::2] = 1                                                      # every other record entirely in the last bin
    got = agree(gpu, bits)
    assert (got[1::2, 3] == 16).all() and (got[1::2, :3] == 0).all()
    agree(gpu, bits, [1, 0], rng.integers(0, 2, size=(B, 2)), rc.WEIGHT)


@pytest.mark.parametrize("k", [1, 3, 10])
def test_every_shot_in_one_bin(gpu, k):
    """maximal contention: that bin holds n_shots, all others 0 -- from a wavefront (4 short records) and from a workgroup"""
    rng = np.random.default_rng(50 + k)
    for B, n_shots in ((4, 4099), (2, 20011)):
        pattern = rng.integers(0, 2, size=(B, 1, k), dtype=np.uint8)
        bits = np.broadcast_to(pattern, (B, n_shots, k)) | rng.integers(0, 2, size=(B, n_shots, k), dtype=np.uint8) << 1
        got = agree(gpu, bits)
        target = (pattern[:, 0, :].astype(np.int64) << np.arange(k - 1, -1, -1)).sum(axis=1)
        assert (got[np.arange(B), target] == n_shots).all() and (got.sum(axis=1) == n_shots).all()
    if k == 10:                                                         # ten selected columns of an 8-column record: the table path
        bits = np.broadcast_to(rng.integers(0, 2, size=(4, 1, 8), dtype=np.uint8), (4, 4099, 8))
        got = agree(gpu, bits, [0, 1, 2, 3, 4, 5, 6, 7, 0, 1])
        assert (got.max(axis=1) == 4099).all()


def test_joint_k10_with_every_bin_hit(gpu):
    rng = np.random.default_rng(6)
    table = (np.arange(1024)[:, None] >> np.arange(9, -1, -1)) & 1
    records = [table[rng.permutation(np.tile(np.arange(1024), 3))].astype(np.uint8) for _ in range(4)]
    got = agree(gpu, np.stack(records))
    assert (got == 3).all()
    long_record = table[rng.permutation(np.tile(np.arange(1024), 20))].astype(np.uint8)[None]      # 204 800 bytes: a workgroup
    assert (agree(gpu, long_record) == 20).all()
    small = (np.arange(32)[:, None] >> np.arange(4, -1, -1)) & 1                                     # the table path, k = 5
    got = agree(gpu, np.stack([small[rng.permutation(np.tile(np.arange(32), 7))].astype(np.uint8) for _ in range(4)]))
    assert (got == 7).all()


@pytest.mark.parametrize("k", [1, 17, 64])
def test_weight_kind(gpu, k):
    rng = np.random.default_rng(70 + k)
    for B, n_shots in ((5, 1000), (2, 4099)):
        bits = rc.random_bits(rng, B, n_shots, k, high_bits=True)
        for expected in (np.zeros((B, k), dtype=np.uint8), np.ones((B, k), dtype=np.uint8), rng.integers(0, 2, size=(B, k))):
            got = agree(gpu, bits, None, expected, rc.WEIGHT)
            assert got.shape == (B, k + 1)
        exact = (bits & 1)[:, 0, :]                                     # the first shot as the pattern: bin 0 holds it
        assert (agree(gpu, bits, None, exact, rc.WEIGHT)[:, 0] >= 1).all()
        assert np.array_equal(agree(gpu, bits, None, None, rc.WEIGHT), agree(gpu, bits, None, np.zeros(k, dtype=np.uint8), rc.WEIGHT))
    bits = rc.random_bits(rng, 4, 1000, 8)                              # 8 columns: the table path
    agree(gpu, bits, rng.integers(0, 8, size=(4, k)), rng.integers(0, 2, size=(4, k)), rc.WEIGHT)


@pytest.mark.parametrize("n_cols", [8, 11])
def test_column_selections(gpu, n_cols):
    rng = np.random.default_rng(80 + n_cols)
    B, n_shots = 5, 1000
    bits = rc.random_bits(rng, B, n_shots, n_cols)
    for kind in (rc.JOINT, rc.WEIGHT):
        agree(gpu, bits, [1, 4, 6], None, kind)                         # not contiguous, shared
        agree(gpu, bits, [6, 0, 3, 1], None, kind)                      # permuted
        per_record = np.stack([rng.permutation(n_cols)[:4] for _ in range(B)])
        got = agree(gpu, bits, per_record, rng.integers(0, 2, size=(B, 4)), kind)
        for b in range(B):                                              # a record's row does not depend on its neighbours
            assert np.array_equal(host_hist(gpu, bits[b:b + 1], per_record[b], None, kind)[0],
                                  rc.histogram(bits[b:b + 1], per_record[b], None, kind)[0])
        assert got.shape[0] == B
    first = agree(gpu, bits[:, :, :8], None, None, rc.JOINT)            # cols = None: columns 0..k-1
    assert np.array_equal(first, agree(gpu, np.ascontiguousarray(bits[:, :, :8]), np.arange(8)))


def test_repeated_runs_agree_and_frequencies_are_one_division(gpu):
    rng = np.random.default_rng(9)
    from fbx import utils
    for n_shots in (1000, 4099, 3):
        bits = rc.random_bits(rng, 5, n_shots, 3)
        a, b = host_hist(gpu, bits), host_hist(gpu, bits)
        assert np.array_equal(a, b) and np.array_equal(a, dev_hist(gpu, bits))
        counts, freq = utils.bitstring_histogram_batch(bits, frequencies=True)
        assert np.array_equal(counts, a)
        assert freq.dtype == np.float64 and np.array_equal(freq, a / n_shots)
        assert np.array_equal(utils.counts_to_frequencies(a, 7), a / 7)
    wide = rc.random_bits(rng, 3, 500, 6)
    assert np.array_equal(utils.bitstring_histogram_batch(wide.astype(np.int64), cols=[5, 0], kind="weight"),
                          rc.histogram(wide, [5, 0], None, rc.WEIGHT))


def test_dev_form_marks_a_record_whose_selection_leaves_the_record(gpu):
    """the _dev form cannot check the selection on the host: such a record gets -1 in every bin and its neighbours are untouched"""
    rng = np.random.default_rng(10)
    for n_cols, n_shots in ((3, 1000), (11, 1000), (3, 20000)):
        bits = rc.random_bits(rng, 5, n_shots, n_cols)
        cols = np.tile(np.array([0, 2], dtype=np.uint8), (5, 1))
        cols[3, 1] = n_cols
        got = dev_hist(gpu, bits, cols)
        good = [0, 1, 2, 4]
        assert (got[3] == -1).all() and np.array_equal(got[good], rc.histogram(bits[good], [0, 2]))
