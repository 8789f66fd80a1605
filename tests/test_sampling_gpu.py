"""fbx_sample_bitstrings on the GPU against the host restatement of its stream (tests/sampling_cases.py).

Where no summation can round (dyadic weights) the device must reproduce the restatement bit for bit; for any other distribution
every shot is held against the exact prefix sums with the bound sampling_cases.delta; a record must not depend on the batch, the
shot count, the entry point or how the launch was cut; poisoned items are flagged and zeroed without touching their neighbours; and
the records feed the consumers they were made for."""
import functools

import numpy as np
import pytest

import qv_cases as qc
import sampling_cases as sc

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB            # both key words in use
B, SHOTS, FIRST = 5, 4099, 3         # a partial group of wavefronts; unaligned records and a tail; ids that do not start at 0
WIDTHS = (1, 2, 5, 8, 9, 13)         # both sides of the switch between the two kernels, and the largest table
LAMBDAS = (0.0, 0.25)


@functools.lru_cache(maxsize=None)
def case(n):
    p = sc.dyadic_weights(n, B, seed=2024)
    assert (p == 0.0).mean() > 0.2 or n == 1
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def device_record(n, lam, with_flips=False):
    """the [B, SHOTS, n] call that several tests share"""
    from fbx import sampling
    flips = sc.asymmetric_flips(n, B, seed=5) if with_flips else None
    out = sampling.sample_bitstrings_batch(case(n), SHOTS, depolarizing=lam if lam else None, readout_flip=flips, seed=SEED,
                                           first_item=FIRST)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def host_record(n, lam, with_flips=False):
    flips = sc.asymmetric_flips(n, B, seed=5) if with_flips else None
    out = sc.restate_batch(case(n), SHOTS, lam, flips, SEED, FIRST)
    out.setflags(write=False)
    return out


def mismatch(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return f"{len(bad)} bytes differ, first at (item, shot, column) {bad[0].tolist() if len(bad) else None}"


# ------------------------------------------------------------------------------------------------ exact against the restatement
@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("n", WIDTHS)
def test_dyadic_weights_bit_for_bit(gpu, n, lam):
    got, want = device_record(n, lam), host_record(n, lam)
    assert got.shape == (B, SHOTS, n) and got.dtype == np.uint8 and got.max() <= 1
    assert np.array_equal(got, want), mismatch(got, want)
    if lam == 0.0:                                       # an outcome of weight zero is never produced
        for b in range(B):
            assert np.all(case(n)[b][sc.from_bits(got[b])] > 0.0)


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("n", WIDTHS)
def test_readout_flips_bit_for_bit(gpu, n, lam):
    from fbx import sampling
    got, want = device_record(n, lam, True), host_record(n, lam, True)
    assert np.array_equal(got, want), mismatch(got, want)
    assert not np.array_equal(got, device_record(n, lam))
    if lam == LAMBDAS[0]:
        plain = device_record(n, lam)
        none = sampling.sample_bitstrings_batch(case(n), SHOTS, readout_flip=np.zeros((n, 2)), seed=SEED, first_item=FIRST)
        assert np.array_equal(none, plain), mismatch(none, plain)
        every = sampling.sample_bitstrings_batch(case(n), SHOTS, readout_flip=np.ones((B, n, 2)), seed=SEED, first_item=FIRST)
        assert np.array_equal(every, 1 - plain), mismatch(every, 1 - plain)


@pytest.mark.parametrize("n", range(1, 14))
def test_one_hot_distributions_spell_their_outcome(gpu, n):
    from fbx import sampling
    where, p = sc.one_hot(n)
    got = sampling.sample_bitstrings_batch(p, 257, seed=SEED)
    for k, i in enumerate(where):
        assert np.array_equal(got[k], np.broadcast_to(sc.to_bits([i], n), (257, n))), (n, i)
    # the caller does not normalise the weights
    assert np.array_equal(sampling.sample_bitstrings_batch(3.0 * p, 257, seed=SEED), got)


# ------------------------------------------------------------------------------------------------ any distribution
@pytest.mark.parametrize("n", (6, 10, 13))
def test_every_shot_lies_in_its_exact_interval(gpu, n):
    """C*_{i-1} - delta <= u T* <= C*_i + delta and p_i > 0 for every shot, C* and T* in numpy.longdouble, delta = N 2^-51 T*."""
    from fbx import sampling
    p = sc.porter_thomas(n, 3, seed=99)
    assert np.all((p == 0.0).sum(axis=1) == p.shape[1] // 2)
    shots = 4099
    got = sampling.sample_bitstrings_batch(p, shots, seed=SEED, first_item=FIRST)
    for b in range(p.shape[0]):
        i = sc.from_bits(got[b])
        assert np.all(p[b][i] > 0.0), (n, b)
        cs = sc.exact_prefix_sums(p[b])
        d = sc.delta(p[b])
        ut = sc.uniforms(sc.words(SEED, FIRST + b, shots)).astype(np.longdouble) * cs[-1]
        below = np.where(i > 0, cs[np.maximum(i - 1, 0)], np.longdouble(0.0))
        slack = np.maximum(below - ut, ut - cs[i])
        print(f"width {n} item {b}: worst excursion {float(slack.max() / cs[-1]):.3e} T (allowed {float(d / cs[-1]):.3e} T)")
        assert np.all(below - d <= ut) and np.all(ut <= cs[i] + d), (n, b)


# ------------------------------------------------------------------------------------------------ shape independence
@pytest.mark.parametrize("n", (5, 13))
def test_items_do_not_depend_on_the_batch(gpu, n):
    from fbx import sampling
    flips = sc.asymmetric_flips(n, B, seed=5)
    p8 = np.concatenate([sc.dyadic_weights(n, FIRST, seed=7), case(n)])
    f8 = np.concatenate([sc.asymmetric_flips(n, FIRST, seed=8), flips])
    lam8 = np.array([0.5, 0.0, 1.0] + [0.25] * B)
    got = sampling.sample_bitstrings_batch(p8, SHOTS, depolarizing=lam8, readout_flip=f8, seed=SEED, first_item=0)
    assert np.array_equal(got[FIRST:], device_record(n, 0.25, True)), mismatch(got[FIRST:], device_record(n, 0.25, True))


@pytest.mark.parametrize("n", (5, 13))
def test_shots_do_not_depend_on_the_shot_count(gpu, n):
    from fbx import sampling
    got = sampling.sample_bitstrings_batch(case(n), 1000, seed=SEED, first_item=FIRST)
    assert np.array_equal(got, device_record(n, 0.0)[:, :1000]), mismatch(got, device_record(n, 0.0)[:, :1000])


@pytest.mark.parametrize("n", (5, 13))
def test_device_pointer_form_equals_host_form(gpu, n):
    p, flips, lam = case(n), sc.asymmetric_flips(n, B, seed=5), np.full(B, 0.25)
    DB = gpu.DeviceBuffer
    bufs = [DB.from_array(p), DB.from_array(lam), DB.from_array(flips), DB(B * SHOTS * n), DB(4 * B)]
    try:
        gpu.check(gpu.lib().fbx_sample_bitstrings_dev(n, B, SHOTS, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, SEED, FIRST, bufs[3].ptr,
                                                      bufs[4].ptr))
        got, status = bufs[3].to_array(np.uint8, (B, SHOTS, n)), bufs[4].to_array(np.int32, (B,))
    finally:
        for b in bufs:
            b.free()
    assert not status.any()
    assert np.array_equal(got, device_record(n, 0.25, True)), mismatch(got, device_record(n, 0.25, True))


def test_a_long_record_is_split_and_still_the_same_stream(gpu):
    """one width-13 item of 300 000 shots is cut into shot ranges for many workgroups; its first shots are those of the short call,
    and the whole record is the restatement's"""
    from fbx import sampling
    n, shots = 13, 300_000
    got = sampling.sample_bitstrings_batch(case(n)[:1], shots, seed=SEED, first_item=FIRST)
    assert got.shape == (1, shots, n)
    assert np.array_equal(got[0, :SHOTS], device_record(n, 0.0)[0]), mismatch(got[:, :SHOTS], device_record(n, 0.0)[:1])
    want = sc.restate(case(n)[0], shots, 0.0, None, SEED, FIRST)[0]
    assert np.array_equal(got[0], want), mismatch(got, want[None])


def test_empty_calls_do_nothing(gpu):
    from fbx import sampling
    assert sampling.sample_bitstrings_batch(case(5), 0, seed=SEED).shape == (B, 0, 5)
    assert sampling.sample_bitstrings_batch(np.zeros((0, 32)), 10, seed=SEED).shape == (0, 10, 5)


# ------------------------------------------------------------------------------------------------ poisoned items
def _poisons(n):
    N = 1 << n
    good = sc.dyadic_weights(n, 1, seed=3)[0]
    nan = good.copy(); nan[N // 3] = np.nan
    neg = good.copy(); neg[N - 2] = -2.0 ** -20
    flip_bad = np.zeros((n, 2)); flip_bad[n - 1, 1] = -0.1
    return {"nan_weight": (nan, 0.0, None), "negative_weight": (neg, 0.0, None), "all_zero_row": (np.zeros(N), 0.0, None),
            "lambda_1.5": (good, 1.5, None), "flip_-0.1": (good, 0.0, flip_bad)}


@pytest.mark.parametrize("n", (5, 9))
@pytest.mark.parametrize("kind", ("nan_weight", "negative_weight", "all_zero_row", "lambda_1.5", "flip_-0.1"))
def test_poisoned_item_between_two_good_ones(gpu, kind, n):
    from fbx import sampling
    row, lam, flip = _poisons(n)[kind]
    shots = 531
    p = np.stack([case(n)[0], row, case(n)[2]])
    lams = np.array([0.25, lam, 0.25])
    flips = np.stack([sc.asymmetric_flips(n, 3, seed=5)[0], np.zeros((n, 2)) if flip is None else flip,
                      sc.asymmetric_flips(n, 3, seed=5)[2]])
    clean_p, clean_flips = p.copy(), flips.copy()
    clean_p[1], clean_flips[1] = case(n)[1], 0.0
    clean = sampling.sample_bitstrings_batch(clean_p, shots, depolarizing=[0.25, 0.0, 0.25], readout_flip=clean_flips, seed=SEED,
                                             first_item=FIRST)
    got, status = sampling.sample_bitstrings_batch(p, shots, depolarizing=lams, readout_flip=flips, seed=SEED, first_item=FIRST,
                                                   return_status=True)
    assert status.tolist() == [0, 1, 0]
    assert not got[1].any()
    assert np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2])
    assert clean[1].any()
    with pytest.raises(ValueError, match=r"item 1 \(global id 4\)"):
        sampling.sample_bitstrings_batch(p, shots, depolarizing=lams, readout_flip=flips, seed=SEED, first_item=FIRST)


# ------------------------------------------------------------------------------------------------ the consumers
def test_moments_of_one_hot_records(gpu):
    from fbx import sampling
    from fbx.observable_estimation import shots_to_obs_moments_batch
    n = 5
    where, p = sc.one_hot(n)
    bits = sampling.sample_bitstrings_batch(p, 257, seed=SEED)
    masks = np.array([[1] * n, [0] * (n - 1) + [1], [1] + [0] * (n - 1), [1] * n])
    mean, var = shots_to_obs_moments_batch(bits, masks)
    want = [(-1.0) ** bin(int(i) & int(sc.from_bits(m))).count("1") for i, m in zip(where, masks)]
    assert mean.tolist() == want and want == [1.0, -1.0, -1.0, -1.0]
    assert var.tolist() == [0.0] * 4


def test_joint_histogram_equals_bincount_of_the_restatement(gpu):
    from fbx import sampling
    from fbx.utils import bitstring_histogram_batch
    n = 6
    p = sc.dyadic_weights(n, B, seed=2024)
    bits = sampling.sample_bitstrings_batch(p, SHOTS, seed=SEED, first_item=FIRST)
    counts = bitstring_histogram_batch(bits, kind="joint")
    want = np.stack([np.bincount(sc.restate(p[b], SHOTS, seed=SEED, g=FIRST + b)[1], minlength=1 << n) for b in range(B)])
    assert np.array_equal(counts, want)
    assert np.all(counts[p == 0.0] == 0)


def test_readout_shots_batch_through_the_confusion_estimator(gpu):
    from fbx import readout, synthetic
    conf = np.array([[[3 / 4, 1 / 8, 1 / 16, 1 / 16], [1 / 8, 5 / 8, 1 / 8, 1 / 8], [0, 1 / 4, 3 / 4, 0], [1 / 32, 1 / 32, 1 / 16, 7 / 8]],
                     [[1, 0, 0, 0], [1 / 2, 1 / 2, 0, 0], [1 / 4, 1 / 4, 1 / 4, 1 / 4], [0, 0, 1 / 2, 1 / 2]]])
    shots, seed = 1000, 6000
    bits = synthetic.readout_shots_batch(conf, shots)
    assert bits.shape == (2, 4, shots, 2) and bits.dtype == np.uint8
    assert np.array_equal(synthetic.readout_shots_batch(conf[1], shots)[2], synthetic.readout_shots_batch(conf[1:], shots, seed)[0, 2])
    got = readout.joint_confusion_matrices_batch(bits)
    want = np.stack([[np.bincount(sc.restate(conf[g, r], shots, seed=seed, g=4 * g + r)[1], minlength=4) / shots for r in range(4)]
                     for g in range(2)])
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ the resident QV chain
QV_SEED, QV_CIRCUITS, QV_SHOTS, QV_LAMBDA = 20260, 64, 2000, 0.2


def test_resident_quantum_volume_chain(gpu):
    """64 circuits of width 5 (qv_cases.random_circuits(5, 64, seed=1811)), 2000 shots, lambda = 0.2, seed 20260.  Expected heavy
    probability per circuit P_b = (1 - lambda) heavy_prob_b + lambda heavy_count_b / 32.  The host restatement on the numpy
    simulation of these circuits, run before the seed was settled, gives a total of heavy shots 0.47 standard deviations below its
    expectation and a largest per-circuit deviation of 2.44 of its own (both within 3): the margins below (5 and 6) belong to the sampler."""
    from fbx import quantum_volume as qv, sampling
    perms, gates = qc.random_circuits(5, QV_CIRCUITS, seed=1811)
    counts, stats = qv.simulate_heavy_output_counts_batch(perms, gates, QV_SHOTS, depolarizing=QV_LAMBDA, seed=QV_SEED)
    assert counts.shape == (QV_CIRCUITS,) and counts.dtype == np.int64
    P = (1.0 - QV_LAMBDA) * stats["heavy_prob"] + QV_LAMBDA * stats["heavy_count"] / 32.0
    sigma = np.sqrt(QV_SHOTS * P * (1.0 - P))
    z = (counts - QV_SHOTS * P) / sigma
    total_z = (counts.sum() - QV_SHOTS * P.sum()) / np.sqrt((sigma ** 2).sum())
    print(f"resident QV chain: total {total_z:+.2f} sigma, worst circuit {np.abs(z).max():.2f} sigma")
    assert abs(counts.sum() - QV_SHOTS * P.sum()) <= 5.0 * np.sqrt((sigma ** 2).sum())
    assert np.all(np.abs(z) <= 6.0)
    # the composed host-pointer calls on the same seed
    heavy, probs, hstats = qv.collect_heavy_outputs_batch(perms, gates, return_probabilities=True, return_stats=True)
    bits = sampling.sample_bitstrings_batch(probs, QV_SHOTS, depolarizing=QV_LAMBDA, seed=QV_SEED)
    assert np.array_equal(counts, qv.count_heavy_hitters_sampled_batch(bits, heavy))
    assert np.array_equal(stats["heavy_prob"], hstats["heavy_prob"]) and np.array_equal(stats["heavy_count"], hstats["heavy_count"])
    # flips that always fire complement every shot: exactly the shots whose complement is heavy are counted
    flipped, _ = qv.simulate_heavy_output_counts_batch(perms, gates, QV_SHOTS, depolarizing=QV_LAMBDA, readout_flip=np.ones((5, 2)),
                                                       seed=QV_SEED)
    assert np.array_equal(flipped, qv.count_heavy_hitters_sampled_batch(1 - bits, heavy))
