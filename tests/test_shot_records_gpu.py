"""fbx_qv_count_heavy[_dev] and fbx_rpe_from_shots[_dev] at the edges of their record walk (qv_count_record, rpe_count_record),
driven by tests/shot_record_cases.py: records with no run, a head only, one run and no tail, a run and a one-shot tail; every
run length; a workgroup per record and a wavefront per record; records of an odd number of bytes (every later record off the
16-byte grid); the record buffer 1 byte into its allocation; both sides of the wavefront / workgroup switch; more records than
the capped grid has wavefronts.  The expected values are direct numpy counts (qv_cases.count_heavy_direct,
rpe_cases.moments_from_shots) and every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

import qv_cases as qc
import rpe_cases as rc
import shot_record_cases as sr

pytestmark = pytest.mark.gpu
U8 = C.POINTER(C.c_uint8)
U64 = C.POINTER(C.c_uint64)
I64 = C.POINTER(C.c_int64)


def offset_buffer(gpu, arr, offset):
    """a device copy of arr that starts `offset` bytes into its allocation: (buffer, address)"""
    buf = gpu.DeviceBuffer(arr.nbytes + 16)
    gpu.check(gpu.lib().fbx_memcpy_h2d(buf.ptr.value + offset, arr.ctypes.data, arr.nbytes))
    return buf, buf.ptr.value + offset


# ---------------------------------------------------------------------------------------------------------------- quantum volume
def qv_host(gpu, bits, mask):
    B, shots, n = bits.shape
    out = np.full(B, -7, dtype=np.int64)
    gpu.check(gpu.lib().fbx_qv_count_heavy(n, B, shots, bits.ctypes.data_as(U8), mask.ctypes.data_as(U64), out.ctypes.data_as(I64)))
    return out


def qv_dev(gpu, bits, mask, offset):
    B, shots, n = bits.shape
    d_bits, at = offset_buffer(gpu, bits, offset)
    d_mask, d_out = gpu.DeviceBuffer.from_array(mask), gpu.DeviceBuffer(B * 8)
    gpu.check(gpu.lib().fbx_qv_count_heavy_dev(n, B, shots, at, d_mask.ptr, d_out.ptr))
    gpu.synchronize()
    out = d_out.to_array(np.int64, (B,))
    for buf in (d_bits, d_mask, d_out):
        buf.free()
    return out


def qv_agree(gpu, bits, heavy, offsets=(0, 1)):
    from fbx import quantum_volume as qv
    want = qc.count_heavy_direct(bits & 1, heavy)
    mask = qv.pack_heavy_mask(heavy)
    tag = bits.shape
    got = qv_host(gpu, bits, mask)
    assert np.array_equal(got, want), (tag, "host", np.flatnonzero(got != want)[:4])
    for offset in offsets:
        got = qv_dev(gpu, bits, mask, offset)
        assert np.array_equal(got, want), (tag, "dev", offset, np.flatnonzero(got != want)[:4])
    return want


@pytest.mark.parametrize("n", sr.QV_WIDTHS)
def test_qv_heads_runs_tails_and_teams(gpu, n):
    rng = np.random.default_rng(300 + n)
    for width, shots, B in sr.edge_cases((n,)):
        want = qv_agree(gpu, sr.random_bytes(rng, (B, shots, width)), sr.heavy_tables(rng, B, width))
        assert want[0] == 0
    ones = np.full((5, 33, n), 0xFF, dtype=np.uint8)                    # every shot is the last output, which record 1 holds
    assert list(qv_agree(gpu, ones, sr.heavy_tables(rng, 5, n))[:2]) == [0, 33]


def test_qv_both_sides_of_the_wavefront_workgroup_switch(gpu):
    rng = np.random.default_rng(31)
    width, (below, above), B = sr.QV_SWITCH
    assert below * width < sr.WAVE_BYTES <= above * width and B >= 4
    for shots in (below, above):
        qv_agree(gpu, sr.random_bytes(rng, (B, shots, width)), sr.heavy_tables(rng, B, width))


def test_qv_more_records_than_wavefronts(gpu):
    rng = np.random.default_rng(32)
    width, shots, B = sr.QV_SECOND_TRIP
    bits = sr.random_bytes(rng, (B, shots, width))
    bits[1::2] = 1                                                      # every other record: every shot is output 2^width - 1
    heavy = sr.heavy_tables(rng, B, width)
    want = qv_agree(gpu, bits, heavy, offsets=(0,))
    assert np.array_equal(want[1::2], shots * heavy[1::2, -1])


# ------------------------------------------------------------------------------------------------------ robust phase estimation
def rpe_host(gpu, xb, yb, col, zcol, ps):
    B, K, shots, n = xb.shape
    out = np.full((B, K, 4), -7.0)
    gpu.check(gpu.lib().fbx_rpe_from_shots(n, B, K, shots, xb.ctypes.data_as(U8), yb.ctypes.data_as(U8), col,
                                           -1 if zcol is None else zcol, ps, None, None, None, gpu.dptr(out)))
    return out


def rpe_dev(gpu, xb, yb, col, zcol, ps, offset):
    B, K, shots, n = xb.shape
    (d_x, at_x), (d_y, at_y) = offset_buffer(gpu, xb, offset), offset_buffer(gpu, yb, offset)
    d_out = gpu.DeviceBuffer(B * K * 4 * 8)
    gpu.check(gpu.lib().fbx_rpe_from_shots_dev(n, B, K, shots, at_x, at_y, col, -1 if zcol is None else zcol, ps, None, None, None,
                                               d_out.ptr))
    gpu.synchronize()
    out = d_out.to_array(np.float64, (B, K, 4))
    for buf in (d_x, d_y, d_out):
        buf.free()
    return out


def rpe_agree(gpu, xb, yb, col, zcol, ps, offsets=(0, 1)):
    want = rc.moments_from_shots(xb, yb, col, zcol, ps)
    tag = (xb.shape, col, zcol, ps)
    assert np.array_equal(rpe_host(gpu, xb, yb, col, zcol, ps), want), (tag, "host")
    for offset in offsets:
        assert np.array_equal(rpe_dev(gpu, xb, yb, col, zcol, ps, offset), want), (tag, "dev", offset)
    return want


def rpe_columns(n):
    """(col, zcol, post_select): no partner; a partner behind the column and one in front of it (both shift directions)"""
    return [(0, None, 0)] if n == 1 else [(n - 1, None, 0), (0, n - 1, 0), (n - 1, 0, 1)]


@pytest.mark.parametrize("n", sr.RPE_WIDTHS)
def test_rpe_heads_runs_tails_and_batches(gpu, n):
    rng = np.random.default_rng(400 + n)
    K = 2
    for width, shots, B in sr.edge_cases((n,)):
        for col, zcol, ps in rpe_columns(width):
            xb, yb = sr.random_bytes(rng, (B, K, shots, width)), sr.random_bytes(rng, (B, K, shots, width))
            rpe_agree(gpu, xb, yb, col, zcol, ps)
    xb = np.full((5, K, 33, n), 0xFF, dtype=np.uint8)                   # every bit set: <X> = <Y> = -1 exactly, no spread
    want = rpe_agree(gpu, xb, xb, n - 1, None, 0)
    assert np.array_equal(want, np.broadcast_to([-1.0, -1.0, 0.0, 0.0], want.shape))


def test_rpe_more_records_than_wavefronts(gpu):
    rng = np.random.default_rng(42)
    width, shots, B = sr.RPE_SECOND_TRIP
    xb, yb = sr.random_bytes(rng, (B, 1, shots, width)), sr.random_bytes(rng, (B, 1, shots, width))
    xb[1::2] = 1                                                        # every other item: <X> = -1 exactly
    want = rpe_agree(gpu, xb, yb, 0, None, 0, offsets=(0,))
    assert (want[1::2, 0, 0] == -1.0).all() and (want[1::2, 0, 2] == 0.0).all()
