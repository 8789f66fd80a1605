"""fbx_sample_bitstrings_wide on the GPU (widths 14..26): bit for bit against the host restatement of its stream
(tests/sampling_wide_cases.py) wherever no summation rounds, shot by shot against exact prefix sums where it does, and the
independence properties of include/fbx.h.

The shapes are the smallest that cross every boundary of the implementation: width 14 (4 blocks of 4096 entries, segments of 4
entries under the coarse table), 15, 17 (the first width whose flips read Philox block t = 4) and 20 (256 blocks, 8 MiB per item,
flips up to block t = 5).  4099 shots leave the second record of a batch off a 16-byte boundary at every width used here, so the
byte-wise ends of the stores are exercised as well as the vectors.
"""
import ctypes as C

import numpy as np
import pytest

import sampling_cases as sc
import sampling_wide_cases as swc

pytestmark = pytest.mark.gpu
SHOTS = 4099
SEED = 0x5EED0000C0FFEE
BATCH = {14: 3, 15: 3, 17: 3, 20: 2}


@pytest.fixture(scope="module")
def dyadic():
    return {n: swc.dyadic_weights_wide(n, B, seed=40 + n) for n, B in BATCH.items()}


def _sample(*a, **k):
    from fbx import sampling
    return sampling.sample_bitstrings_wide_batch(*a, **k)


# ------------------------------------------------------------------------------------------------ 1 bit for bit
@pytest.mark.parametrize("flips", (False, True))
@pytest.mark.parametrize("lam", (0.0, 0.25))
@pytest.mark.parametrize("n", (14, 15, 17, 20))
def test_bit_for_bit_on_dyadic_weights(gpu, dyadic, n, lam, flips):
    p = dyadic[n]
    B = p.shape[0]
    flip = swc.asymmetric_flips(n, B, seed=9) if flips else None
    assert SHOTS * n % 16 != 0
    got, status = _sample(p, SHOTS, depolarizing=lam, readout_flip=flip, seed=SEED, first_item=3, return_status=True)
    want = swc.restate_batch(p, SHOTS, lam, flip, seed=SEED, first_item=3)
    assert got.shape == (B, SHOTS, n) and got.dtype == np.uint8 and not status.any()
    assert np.array_equal(got, want), f"{int((got != want).any(axis=2).sum())} of {B * SHOTS} shots differ"


# ------------------------------------------------------------------------------------------------ 2 one-hot rows
@pytest.mark.parametrize("n", (14, 20))
def test_one_hot_rows(gpu, n):
    where, p = swc.one_hot(n)
    for lam_free_scale in (1.0, 3.5):                                  # the weights need not be normalised
        got = _sample(p * lam_free_scale, 777, seed=SEED + n)
        assert np.array_equal(sc.from_bits(got), np.broadcast_to(where[:, None], (where.size, 777)))


# ------------------------------------------------------------------------------------------------ 3 rounding sums
@pytest.mark.parametrize("n", (14, 17, 20))
def test_every_shot_lies_in_its_interval_of_the_exact_prefix_sums(gpu, n):
    """Porter-Thomas weights, a random half of them exactly zero: shot s with the draw u_s produced outcome i only if
    C*_(i-1) - delta <= u_s T* <= C*_i + delta (C* exact, delta = N 2^-51 T* of sampling_cases.delta), and w_i > 0.
    Observed on the MI355X: no shot outside its exact interval at any of the three widths (largest excess 0, before delta)."""
    B = 2
    p = sc.porter_thomas(n, B, seed=7)
    got = _sample(p, SHOTS, seed=SEED + 3, first_item=11)
    worst = 0.0
    for b in range(B):
        idx = sc.from_bits(got[b])
        assert idx.shape == (SHOTS,)                                   # no shot left out
        assert np.all(p[b][idx] > 0.0), "an outcome of weight zero was drawn"
        Cx = sc.exact_prefix_sums(p[b])
        d = sc.delta(p[b])
        u = sc.uniforms(swc.words(SEED + 3, 11 + b, SHOTS, 0)).astype(np.longdouble)
        t = u * Cx[-1]
        below = np.where(idx > 0, Cx[np.maximum(idx - 1, 0)], np.longdouble(0.0))
        excess = np.maximum(below - t, t - Cx[idx])
        worst = max(worst, float(excess.max() / Cx[-1]))
        assert np.all(excess <= d), f"item {b}: {int((excess > d).sum())} shots outside their interval"
    print(f"width {n}: largest (u T* - interval) excess {worst:.3e} T* (<= 0: none), delta {float(2.0 ** -51 * p.shape[1]):.3e} T*")


# ------------------------------------------------------------------------------------------------ 4 independence
@pytest.fixture(scope="module")
def base(gpu):
    """19 Porter-Thomas items of width 14 with per-item depolarizing and flips, 1000 shots, items 5 .. 23 of the stream"""
    n, B = 14, 19
    p = sc.porter_thomas(n, B, seed=19)
    lam = np.linspace(0.0, 0.9, B)
    flip = swc.asymmetric_flips(n, B, seed=4) * 0.5
    bits = _sample(p, 1000, depolarizing=lam, readout_flip=flip, seed=SEED + 4, first_item=5)
    return p, lam, flip, bits


def test_independent_of_batch_shots_and_first_item(base):
    p, lam, flip, bits = base
    part = _sample(p[4:7], 1000, depolarizing=lam[4:7], readout_flip=flip[4:7], seed=SEED + 4, first_item=9)
    assert np.array_equal(part, bits[4:7])
    short = _sample(p, 300, depolarizing=lam, readout_flip=flip, seed=SEED + 4, first_item=5)
    assert np.array_equal(short, bits[:, :300])
    other = _sample(p[:2], 1000, depolarizing=lam[:2], readout_flip=flip[:2], seed=SEED + 4, first_item=6)
    assert not np.array_equal(other[0], bits[0])                       # another item of the stream: another record


def test_independent_of_the_workspace_option(base):
    p, lam, flip, bits = base
    from fbx import _lib
    with _lib.option("sample_wide_workspace_mib", 1.0):                # 7 items per chunk at width 14: chunks of 7, 7 and 5
        got, status = _sample(p, 1000, depolarizing=lam, readout_flip=flip, seed=SEED + 4, first_item=5, return_status=True)
    assert _lib.get_option("sample_wide_workspace_mib") == 128.0
    assert np.array_equal(got, bits) and not status.any()


def test_device_pointer_form_equals_the_host_form(base):
    p, lam, flip, bits = base
    from fbx import _lib
    B, shots, n = bits.shape
    DB = _lib.DeviceBuffer
    bufs = [DB.from_array(p), DB.from_array(lam), DB.from_array(flip), DB(bits.size), DB(4 * B)]
    try:
        _lib.check(_lib.lib().fbx_sample_bitstrings_wide_dev(n, B, shots, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, SEED + 4, 5,
                                                             bufs[3].ptr, bufs[4].ptr))
        _lib.synchronize()
        assert np.array_equal(bufs[3].to_array(np.uint8, bits.shape), bits)
        assert not bufs[4].to_array(np.int32, (B,)).any()
    finally:
        for b in bufs:
            b.free()


def test_independent_of_the_cut_into_shot_ranges(gpu, dyadic):
    """one record of 300 000 shots is drawn by 37 workgroups; the restatement knows nothing of ranges"""
    p = dyadic[14][:1]
    got = _sample(p, 300000, depolarizing=0.25, seed=SEED + 5, first_item=2)
    want = swc.restate_batch(p, 300000, 0.25, None, seed=SEED + 5, first_item=2)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ 5 poisoned items
def test_poisoned_items_between_good_ones(gpu):
    n, B = 14, 11
    N = 1 << n
    p = sc.porter_thomas(n, B, seed=23)
    p[:, 0] = 1.0                                                      # (a positive weight in the first block of every item)
    lam = np.full(B, 0.125)
    flip = np.full((B, n, 2), 0.03125)
    clean = _sample(p, 500, depolarizing=lam, readout_flip=flip, seed=SEED + 6)
    bad_p, bad_lam, bad_flip = p.copy(), lam.copy(), flip.copy()
    bad_p[1, N - 5] = -1e-300                                          # a negative weight in the last block only
    bad_p[3, 17] = np.nan                                              # a NaN in the first block
    bad_p[5] = 0.0                                                     # all weights zero
    bad_lam[7] = 1.5
    bad_flip[9, n - 1, 1] = -0.1
    got, status = _sample(bad_p, 500, depolarizing=bad_lam, readout_flip=bad_flip, seed=SEED + 6, return_status=True)
    assert status.tolist() == [0, 1] * 5 + [0]
    assert not got[1::2].any()
    assert np.array_equal(got[0::2], clean[0::2])
    with pytest.raises(ValueError, match=r"item 1 \(global id 41\)"):
        _sample(bad_p, 500, depolarizing=bad_lam, readout_flip=bad_flip, seed=SEED + 6, first_item=40)


# ------------------------------------------------------------------------------------------------ 6 consumers
def test_records_feed_the_consumers(gpu, dyadic):
    from fbx import observable_estimation as oe, quantum_volume as qv
    n = 14
    p = dyadic[n][:2]
    got = _sample(p, SHOTS, depolarizing=0.25, seed=SEED + 7)
    want = swc.restate_batch(p, SHOTS, 0.25, None, seed=SEED + 7)
    assert np.array_equal(got, want)
    heavy = np.random.default_rng(5).random((2, 1 << n)) < 0.5
    counts = qv.count_heavy_hitters_sampled_wide_batch(got, heavy)
    assert counts.tolist() == [int(heavy[b, sc.from_bits(want[b])].sum()) for b in range(2)]
    masks = np.zeros((2, n), dtype=np.uint8)
    masks[0, [0, 5, 13]] = 1
    masks[1, [2, 3, 7, 12]] = 1
    mean, var = oe.shots_to_obs_moments_batch(got, masks)
    for b in range(2):
        prod = np.prod(1 - 2 * want[b][:, masks[b] != 0].astype(np.int64), axis=1)
        m = prod.sum() / SHOTS
        # one division of exact integers, then 1 - m^2 and one more division: a few ulp at the most
        assert abs(mean[b] - m) <= 2.0 ** -52 and abs(var[b] - (1.0 - m * m) / SHOTS) <= 4.0 * 2.0 ** -52 / SHOTS


# ------------------------------------------------------------------------------------------------ 7 the resident chain
QV_SHOTS, QV_LAMBDA, QV_SEED = 2000, 0.2, 20261


def test_resident_quantum_volume_chain_at_width_14(gpu):
    """8 circuits of width 14 drawn as tests/test_quantum_volume_wide_gpu.py draws them, 2000 shots, lambda = 0.2.  The margins (5
    sigma on the total, 6 on every circuit) are those of the narrow chain's test: binomial tails, not measured numbers."""
    from fbx import quantum_volume as qv, sampling
    from test_quantum_volume_wide_gpu import _draw
    n = 14
    perms, gates, _ = _draw(n, 8, seed=2014, pairings=("reference",))
    counts, stats = qv.simulate_heavy_output_counts_wide_batch(perms, gates, QV_SHOTS, depolarizing=QV_LAMBDA, seed=QV_SEED)
    assert counts.shape == (8,) and counts.dtype == np.int64
    P = (1.0 - QV_LAMBDA) * stats["heavy_prob"] + QV_LAMBDA * stats["heavy_count"] / 2.0 ** n
    sigma = np.sqrt(QV_SHOTS * P * (1.0 - P))
    z = (counts - QV_SHOTS * P) / sigma
    total_z = (counts.sum() - QV_SHOTS * P.sum()) / np.sqrt((sigma ** 2).sum())
    print(f"resident wide QV chain: total {total_z:+.2f} sigma, worst circuit {np.abs(z).max():.2f} sigma")
    assert abs(total_z) <= 5.0 and np.all(np.abs(z) <= 6.0)
    # the composed host-pointer calls on the same seed
    B, L = 8, n * (n // 2)
    pairs, flat = qv.layer_pairs(perms, "reference").reshape(B, L, 2), gates.reshape(B, L, 4, 4)
    r = qv.heavy_outputs_flat_wide(n, pairs, flat)
    bits = sampling.sample_bitstrings_wide_batch(r["probabilities"], QV_SHOTS, depolarizing=QV_LAMBDA, seed=QV_SEED)
    assert np.array_equal(counts, qv.count_heavy_hitters_sampled_wide_batch(bits, r["mask"]))
    assert np.array_equal(stats["heavy_prob"], r["heavy_prob"]) and np.array_equal(stats["heavy_count"], r["heavy_count"])
    # one circuit per slice (a circuit holds 128 KiB of probabilities), and another tile
    for kwargs in ({"max_resident_mib": 0.01}, {"tile_bits": 12}, {"max_resident_mib": 0.5, "tile_bits": 10}):
        again, astats = qv.simulate_heavy_output_counts_wide_batch(perms, gates, QV_SHOTS, depolarizing=QV_LAMBDA, seed=QV_SEED,
                                                                   **kwargs)
        assert np.array_equal(again, counts), kwargs
        assert np.array_equal(astats["heavy_prob"], stats["heavy_prob"]) and np.array_equal(astats["heavy_count"], stats["heavy_count"])
    # flips that always fire complement every shot: exactly the shots whose complement is heavy are counted
    flipped, _ = qv.simulate_heavy_output_counts_wide_batch(perms, gates, QV_SHOTS, depolarizing=QV_LAMBDA,
                                                            readout_flip=np.ones((n, 2)), seed=QV_SEED, max_resident_mib=0.4)
    assert np.array_equal(flipped, qv.count_heavy_hitters_sampled_wide_batch(1 - bits, r["mask"]))


def test_wide_functions_are_the_narrow_ones_at_width_5(gpu):
    import qv_cases as qc
    from fbx import quantum_volume as qv, sampling
    perms, gates = qc.random_circuits(5, 6, seed=1811)
    narrow = qv.simulate_heavy_output_counts_batch(perms, gates, 500, depolarizing=0.1, readout_flip=np.full((5, 2), 0.02), seed=77)
    wide = qv.simulate_heavy_output_counts_wide_batch(perms, gates, 500, depolarizing=0.1, readout_flip=np.full((5, 2), 0.02), seed=77)
    assert np.array_equal(narrow[0], wide[0]) and np.array_equal(narrow[1]["heavy_prob"], wide[1]["heavy_prob"])
    p = sc.dyadic_weights(5, 3, seed=1)
    assert np.array_equal(sampling.sample_bitstrings_batch(p, 100, seed=3), sampling.sample_bitstrings_wide_batch(p, 100, seed=3))
