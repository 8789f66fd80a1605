"""fbx_shots_to_moments[_dev] on every branch of its launcher (22 kernel instantiations, the per-record alignment fallbacks, the second
trip of every grid-stride loop, misaligned device buffers) against exact integer counts: the table and the reference of
tests/shots_cases.py, whose coverage tests/test_shots_cases_cpu.py proves.  The bytes carry random high bits (only bit 0 is the
outcome), the mask bytes are 0, 1, 2 or 255, and the bias per setting saturates the counts (m = +-1, n_minus = 0 and n_shots).

Tolerances, from the number of roundings between the integer count and the result, u = 2^-53 (the device compiler may fuse a
multiply-add, so bit equality is asked only where one operation separates the two):
  no prior  mean  bit for bit coef * ((shots - 2 n_minus) / shots) in numpy doubles
            var   4u coef^2 / shots + 8u |exact|        (m carries u; 1 - m^2 then at most 3u m^2 + u (1 - m^2); three more products)
  prior     mean  4u |coef| + 4u |exact|                (a / (a + b) carries u, doubled, minus one, times coef)
            var   16u |exact|                           (integers below 2^53 are exact: one division, two products)
  identity rows   exactly (coef, 0.0)
One miscounted shot moves the mean by 2 |coef| / shots, at least 1e-4 relative here."""
import ctypes as C

import numpy as np
import pytest

import shots_cases as sc

pytestmark = pytest.mark.gpu
U8 = C.POINTER(C.c_uint8)
U = 2.0 ** -53
MODES = [(with_coefs, prior) for with_coefs in (False, True) for prior in (0, 1)]


def host_moments(lib_mod, bits, masks, coefs, prior):
    S, shots, n = bits.shape
    mean, var = np.full(S, np.nan), np.full(S, np.nan)
    lib_mod.check(lib_mod.lib().fbx_shots_to_moments(n, S, shots, bits.ctypes.data_as(U8), masks.ctypes.data_as(U8), lib_mod.dptr(coefs),
                                                     prior, lib_mod.dptr(mean), lib_mod.dptr(var)))
    return mean, var


def dev_moments(lib_mod, bits, masks, coefs, prior, offset):
    """the _dev form on caller-owned buffers; the record buffer starts `offset` bytes into its allocation"""
    S, shots, n = bits.shape
    lib = lib_mod.lib()
    d_bits = lib_mod.DeviceBuffer(bits.nbytes + 16)
    assert d_bits.ptr.value % 16 == 0 and 0 <= offset <= 16
    lib_mod.check(lib.fbx_memcpy_h2d(d_bits.ptr.value + offset, bits.ctypes.data, bits.nbytes))
    d_masks = lib_mod.DeviceBuffer.from_array(masks)
    d_coefs = None if coefs is None else lib_mod.DeviceBuffer.from_array(coefs)
    d_mean, d_var = lib_mod.DeviceBuffer.from_array(np.full(S, np.nan)), lib_mod.DeviceBuffer.from_array(np.full(S, np.nan))
    lib_mod.check(lib.fbx_shots_to_moments_dev(n, S, shots, d_bits.ptr.value + offset, d_masks.ptr, None if d_coefs is None else d_coefs.ptr,
                                               prior, d_mean.ptr, d_var.ptr))
    lib_mod.synchronize()
    mean, var = d_mean.to_array(np.float64, (S,)), d_var.to_array(np.float64, (S,))
    for buf in (d_bits, d_masks, d_coefs, d_mean, d_var):
        if buf is not None:
            buf.free()
    return mean, var


def moments(lib_mod, case, bits, masks, coefs, prior):
    if case[3] == 0:
        return host_moments(lib_mod, bits, masks, coefs, prior)
    return dev_moments(lib_mod, bits, masks, coefs, prior, case[3])


def first_bad(ok):
    return np.flatnonzero(~ok)[:4]


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_every_dispatch_branch_on_exact_counts(gpu, case):
    n, S, shots, _ = case
    bits, masks, coefs = sc.make(case)
    n_minus = sc.count_minus(bits, masks)
    identity = ~masks.any(axis=1)
    live = ~identity
    for with_coefs, prior in MODES:
        cf = coefs if with_coefs else None
        c = coefs if with_coefs else np.ones(S)
        want_mean, want_var, _ = sc.exact(bits, masks, cf, prior, n_minus)
        mean, var = moments(gpu, case, bits, masks, cf, prior)
        tag = (sc.case_id(case), "coefs" if with_coefs else "unit", "prior" if prior else "plain")
        assert np.array_equal(mean[identity], c[identity]) and (var[identity] == 0.0).all(), tag
        if prior:
            mean_bound = 4 * U * np.abs(c) + 4 * U * np.abs(want_mean)
            var_bound = 16 * U * np.abs(want_var)
            ok = np.abs(mean - want_mean) <= mean_bound
        else:
            numpy_mean = c * ((shots - 2 * n_minus) / shots)
            var_bound = 4 * U * c * c / shots + 8 * U * np.abs(want_var)
            ok = mean == numpy_mean
        bad = first_bad(ok | identity)
        assert bad.size == 0, (tag, "mean", bad, mean[bad], want_mean[bad], n_minus[bad])
        bad = first_bad((np.abs(var - want_var) <= var_bound) | identity)
        assert bad.size == 0, (tag, "var", bad, var[bad], want_var[bad], n_minus[bad])
        assert np.isfinite(mean).all() and (var[live] >= 0.0).all(), tag


@pytest.mark.parametrize("case", [(2, sc.SECOND_TRIP_WAVE, 520, 0), (3, sc.SECOND_TRIP_WAVE, 1040, 0)], ids=sc.case_id)
def test_a_setting_does_not_depend_on_its_position(gpu, case):
    """the settings past the grid, run as a small batch of their own (first trips of the same kernel), give the same bits as in the
    large batch, and the large batch run twice is bit-identical"""
    assert case in sc.CASES and sc.route(*case).second_trip
    bits, masks, coefs = sc.make(case)
    back = sc.WAVES_PER_GROUP * sc.GRID_CAP
    small = (case[0], case[1] - back, case[2], 0)
    assert sc.route(*small).name == sc.route(*case).name and not sc.route(*small).second_trip
    for prior in (0, 1):
        mean, var = host_moments(gpu, bits, masks, coefs, prior)
        again_mean, again_var = host_moments(gpu, bits, masks, coefs, prior)
        assert np.array_equal(mean, again_mean) and np.array_equal(var, again_var)
        own_mean, own_var = host_moments(gpu, np.ascontiguousarray(bits[back:]), np.ascontiguousarray(masks[back:]),
                                         np.ascontiguousarray(coefs[back:]), prior)
        assert np.array_equal(own_mean, mean[back:]) and np.array_equal(own_var, var[back:])
        assert len(set(mean[back:])) > 1                               # five settings, not one answer five times


def test_calibrate_kernel_past_its_grid(gpu):
    """calibrate_kernel (csrc/fbx_shots.hip) is capped at 32 x 256 workgroups of 256 threads = 2^21 threads: 2^21 + 77 elements send 77
    threads round the grid-stride loop again.  The mean is one division; the error is a square root over two quotients and a sum."""
    from fbx.observable_estimation import calibrate_expectations_batch
    rng = np.random.default_rng(77)
    B, m, n_cal = 1, 32 * 256 * 256 + 77, 7                            # 2^21 + 77 is prime: one experiment of m settings
    expect = rng.uniform(-1.0, 1.0, size=(B, m))
    std_err = rng.uniform(0.0, 0.1, size=(B, m))
    cal_mean = rng.uniform(0.5, 1.0, size=n_cal) * np.where(np.arange(n_cal) % 2, -1.0, 1.0)
    cal_var = rng.uniform(0.0, 1e-3, size=n_cal)
    cal_index = rng.integers(0, n_cal, size=m)
    cal_index[-77:] = np.arange(77) % n_cal                            # the second trip sees every calibration
    mean, err = calibrate_expectations_batch(expect, std_err, cal_mean, cal_var, cal_index)
    b, vb = cal_mean[cal_index][None], cal_var[cal_index][None]
    assert np.array_equal(mean, expect / b)
    want = np.sqrt(std_err * std_err / (b * b) + (expect * expect * vb) / ((b * b) * (b * b)))
    bad = np.argwhere(~(np.abs(err - want) <= 16 * U * want))[:4]
    assert bad.size == 0, (bad, err[tuple(bad.T)], want[tuple(bad.T)])
