"""fbx_rb_acquire / fbx_rb_depth_means on the GPU (include/fbx.h): the final vectors bit for bit against fbx_rb_sequences ->
fbx_rb_simulate on the same stream, the outcome distributions against an extended-precision restatement, histograms and moments
bit for bit against the host restatement of the shots, the exact-expectation mode, the depth means, exact and statistical
physics, the resident chains against the public calls chained by hand, poisoned experiments and the refusals.

The kernel gives a wavefront 64 consecutive sequences of one experiment and a workgroup four such units
(csrc/fbx_rb_acquire.hip): rb_acquire_cases.SHAPES holds S K = 15 (a partial wavefront), 64 (a full one), 70 (an experiment over
two units) and 300 (past a workgroup)."""

import numpy as np
import pytest

import rb_acquire_cases as cases
from fbx import _lib, synthetic
from fbx import randomized_benchmarking as rb
from fbx.analysis import fitting

pytestmark = pytest.mark.gpu

SEED = cases.SEED
MASK = 2 ** 64 - 1
# (name, unitarity, interleaved)
MODES = {"standard": (False, False), "interleaved": (False, True), "unitarity": (True, False)}


def acquire(n, mode, shape, shots=None, flips=None, first_item=0, E=slice(None), seed=SEED, ptms=None, **kw):
    """the public wrappers with every output: dict of e, s, vec, prob, (hist,) status"""
    unitarity, interleaved = MODES[mode]
    depths, K = cases.SHAPES[shape] if isinstance(shape, str) else shape
    ptms = cases.channels(n, interleaved)[E] if ptms is None else ptms
    if flips is not None and np.ndim(flips) == 3:
        flips = flips[E]
    want_hist = bool(shots)
    common = dict(shots=shots, flips=flips, seed=seed, first_item=first_item, return_vectors=True, return_probabilities=True,
                  return_histograms=want_hist, return_status=True, **kw)
    if unitarity:
        out = rb.simulate_unitarity_acquisition_batch(n, depths, K, ptms, **common)
    else:
        out = rb.simulate_rb_acquisition_batch(n, depths, K, ptms, interleaved_gate=cases.interleaved_gate(n) if interleaved else None,
                                               per_sequence=True, **common)
    names = ["e", "s", "vec", "prob"] + (["hist"] if want_hist else []) + ["status"]
    return dict(zip(names, out))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ 1. stream and arithmetic
@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("n", [1, 2])
def test_vectors_are_the_composition_bit_for_bit(gpu, n, mode, shape):
    """vec_out == fbx_rb_simulate on the sequences fbx_rb_sequences writes under the seed seed + gid"""
    unitarity, interleaved = MODES[mode]
    depths, K = cases.SHAPES[shape]
    ptms = cases.channels(n, interleaved)
    inter = cases.interleaved_gate(n) if interleaved else None
    got = acquire(n, mode, shape, first_item=5)
    assert got["vec"].shape == (3, len(depths) * K, 4 ** n) and not got["status"].any()
    for x in range(3):
        offsets, elems, ids = rb.generate_rb_sequences_batch(n, depths, K, inter, (SEED + 5 + x) & MASK, self_inverting=not unitarity)
        want = rb.simulate_rb_sequences_batch(n, offsets, elems, ptms[x], ids)
        assert same_bits(got["vec"][x], want), (x, np.abs(got["vec"][x] - want).max())


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("n", [1, 2])
def test_values_do_not_depend_on_the_batch(gpu, n, mode):
    """items 1..2 of a call are items 0..1 of a call with first_item = 1, and E = 3 is three calls of E = 1: every output"""
    flips = np.stack([cases.FLIPS[n], cases.FLIPS[n][::-1] * 0.5, cases.FLIPS[n] * 1.5])
    whole = acquire(n, mode, "two_units_70", shots=13, flips=flips)
    shifted = acquire(n, mode, "two_units_70", shots=13, flips=flips, first_item=1, E=slice(1, 3))
    for key in ("e", "s", "vec", "prob", "hist"):
        assert same_bits(whole[key][1:], shifted[key]), key
        assert not same_bits(whole[key][1], whole[key][2]), key            # (the experiments do differ)
    for x in range(3):
        one = acquire(n, mode, "two_units_70", shots=13, flips=flips, first_item=x, E=slice(x, x + 1))
        for key in ("e", "s", "vec", "prob", "hist"):
            assert same_bits(whole[key][x:x + 1], one[key]), (key, x)


def test_unitarity_sequences_are_those_of_the_generator(gpu):
    """generate_unitarity_experiment_sequences: S K arrays of `depth` words each, not self-inverting, and the ones the acquisition runs"""
    depths, K = (1, 3, 4), 6
    seqs = rb.generate_unitarity_experiment_sequences(None, [0, 1], depths, K, random_seed=SEED + 2)
    assert [len(s) for s in seqs] == list(np.repeat(depths, K))
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    ptm = cases.channels(2)[1]
    want = rb.simulate_rb_sequences_batch(2, offsets, np.concatenate(seqs), ptm)
    got = acquire(2, "unitarity", (depths, K), first_item=2, ptms=ptm[None])
    assert same_bits(got["vec"][0], want)
    from fbx import clifford
    total = clifford.identity(2)
    for w in seqs[-1]:
        total = clifford.compose(int(w), total, 2)
    assert total != clifford.identity(2)                                   # (one in 11520 would be; this one is not)


# ------------------------------------------------------------------------------------------------ 2. distributions
@pytest.mark.parametrize("mode", ["standard", "unitarity"])
@pytest.mark.parametrize("n", [1, 2])
def test_distributions_against_extended_precision(gpu, n, mode):
    """prob_out against rb_outcome_distributions evaluated in numpy.longdouble from vec_out and the flips.  The bound counts
    operations: a distribution entry is 2^n signed additions of components of the vector (the factor 2^-n is exact) followed by
    n confusion steps of at most four roundings each (1 - f, two products, one sum, some of them fused), every intermediate of
    magnitude at most A = sum_k |v_k|: (2^n + 4 n) 2^-53 A, absolute."""
    flips = np.stack([cases.FLIPS[n], cases.FLIPS[n][::-1] * 0.5, cases.FLIPS[n] * 1.5])
    got = acquire(n, mode, "two_units_70", flips=flips)
    want = synthetic.rb_outcome_distributions(got["vec"].astype(np.longdouble), n, mode, flips)
    bound = (2 ** n + 4 * n) * 2.0 ** -53 * np.abs(got["vec"]).sum(axis=-1)          # [E, Q]
    err = np.abs(got["prob"].astype(np.longdouble) - want).max(axis=(2, 3)).astype(np.float64)
    rows = np.abs(got["prob"].astype(np.longdouble).sum(axis=-1) - got["vec"][..., :1].astype(np.longdouble)).max(axis=2).astype(np.float64)
    print(f"rb_acquire distributions n={n} {mode}: worst excursion {float((err / bound).max()):.3f} of the bound, "
          f"row sums {float((rows / bound).max()):.3f}")
    assert got["prob"].shape == want.shape
    assert (err <= bound).all() and (rows <= bound).all()


# ------------------------------------------------------------------------------------------------ 3. shots
@pytest.mark.parametrize("shots", [1, 3, 4, 5, 1000])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("n", [1, 2])
def test_shots_are_the_documented_stream(gpu, n, mode, shots):
    """hist_out equals the host restatement of prob_out in integers (the tail rule for counts that are no multiple of 4
    included); expect_out and std_err_out equal the restated doubles bit for bit"""
    flips = np.stack([cases.FLIPS[n], cases.FLIPS[n][::-1] * 0.5, cases.FLIPS[n] * 1.5])
    got = acquire(n, mode, "two_units_70", shots=shots, flips=flips, first_item=(1 << 32) + 3)
    host_mode = "unitarity" if MODES[mode][0] else "standard"
    hist, expect, std_err = synthetic.restate_rb_counts(got["prob"], shots, host_mode, SEED, first_item=(1 << 32) + 3)
    np.testing.assert_array_equal(got["hist"].astype(np.int64), hist)
    assert same_bits(got["e"], expect) and same_bits(got["s"], std_err)
    assert (got["hist"].sum(axis=-1) == shots).all()
    h = got["hist"].astype(np.int64)
    if n == 2 and host_mode == "standard":                                 # IZ, ZI, ZZ from the same shots
        np.testing.assert_array_equal(shots * got["e"][..., 0], h[:, :, 0, 0] - h[:, :, 0, 1] + h[:, :, 0, 2] - h[:, :, 0, 3])
        np.testing.assert_array_equal(shots * got["e"][..., 1], h[:, :, 0, 0] + h[:, :, 0, 1] - h[:, :, 0, 2] - h[:, :, 0, 3])
        np.testing.assert_array_equal(shots * got["e"][..., 2], h[:, :, 0, 0] - h[:, :, 0, 1] - h[:, :, 0, 2] + h[:, :, 0, 3])
    if host_mode == "unitarity":                                           # every Pauli from the basis the rule assigns it
        for col, (pauli, basis, mask) in enumerate(synthetic.rb_pauli_assignment(n, "unitarity")):
            assert basis == rb.unitarity_basis_of_pauli(n, pauli)
            signs = np.array([-1 if bin(o & mask).count("1") & 1 else 1 for o in range(2 ** n)])
            np.testing.assert_array_equal(shots * got["e"][..., col], (h[:, :, basis, :] * signs).sum(axis=-1))


# ------------------------------------------------------------------------------------------------ 4. exact expectations
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("n", [1, 2])
def test_without_shots_the_expectations_are_the_vector(gpu, n, mode):
    got = acquire(n, mode, "two_units_70", shots=None, flips=cases.FLIPS[n])
    cols = np.arange(1, 4 ** n) if MODES[mode][0] else rb.z_product_indices(n)
    assert same_bits(got["e"], got["vec"][..., cols])
    assert same_bits(got["s"], np.zeros_like(got["e"]))
    with pytest.raises(ValueError, match="histograms need shots"):
        rb.simulate_rb_acquisition_batch(n, [2, 3], 2, cases.channels(n)[0], return_histograms=True)


# ------------------------------------------------------------------------------------------------ 5. depth means
@pytest.mark.parametrize("n", [1, 2])
def test_depth_means(gpu, n):
    depths, K = cases.SHAPES["two_units_70"]
    per_seq = acquire(n, "standard", "two_units_70", shots=50, flips=cases.FLIPS[n])
    mean, err = rb.simulate_rb_acquisition_batch(n, depths, K, cases.channels(n), shots=50, flips=cases.FLIPS[n], seed=SEED)
    v = per_seq["e"].reshape(3, len(depths), K, -1)
    np.testing.assert_allclose(mean, v.mean(axis=2), rtol=1e-13, atol=0)
    np.testing.assert_allclose(err, np.sqrt(v.var(axis=2, ddof=1) / K), rtol=1e-13, atol=0)
    m2, e2 = rb.depth_means_batch(v)
    assert same_bits(m2, mean) and same_bits(e2, err)
    for x in range(3):                                                     # E = 3 is three calls
        m1, e1 = rb.depth_means_batch(v[x:x + 1])
        assert same_bits(m1, mean[x:x + 1]) and same_bits(e1, err[x:x + 1])
    # K = 1: the sequence's own standard error passes through; without one, 0
    one = acquire(n, "standard", ((2, 3, 7), 1), shots=50)
    m1, e1 = rb.simulate_rb_acquisition_batch(n, (2, 3, 7), 1, cases.channels(n), shots=50, seed=SEED)
    assert same_bits(m1, one["e"]) and same_bits(e1, one["s"])
    m0, e0 = rb.depth_means_batch(one["e"][:, :, None, :])
    assert same_bits(m0, one["e"]) and not e0.any()
    # C = 1, as the purities go through it
    pm, pe = rb.depth_means_batch(v[..., :1])
    assert same_bits(pm, mean[..., :1]) and same_bits(pe, err[..., :1])


# ------------------------------------------------------------------------------------------------ 6. physics, exact
def test_depolarizing_survival_is_exact(gpu):
    p, depths, K = 0.96, (2, 3, 5, 9, 17), 4
    e, _ = rb.simulate_rb_acquisition_batch(1, depths, K, cases.depolarizing(1, p), seed=SEED, per_sequence=True)
    m = np.repeat(np.array(depths, dtype=np.float64), K)                   # noisy steps: depth - 1 Cliffords and the inverse
    np.testing.assert_allclose((1 + e[0, :, 0]) / 2, (1 + p ** m) / 2, rtol=1e-13)


@pytest.mark.parametrize("n", [1, 2])
def test_fits_recover_the_depolarizing_strength(gpu, n):
    """noise-free data: the tolerance of tests/test_curve_fit_gpu.py for noise-free curves (rtol 1e-8 on the parameters)"""
    p = np.array([0.99, 0.95, 0.9])
    ptms = np.array([cases.depolarizing(n, x) for x in p])[:, None]
    depths = (2, 3, 5, 8, 13, 21)
    fit = rb.simulate_and_fit_rb_batch(n, depths, 3, ptms, seed=SEED)
    assert fit.success.all()
    np.testing.assert_allclose(fit.value("decay"), p, rtol=1e-8)
    np.testing.assert_allclose(fit.value("decay"), rb.predicted_rb_decay(ptms[:, 0]), rtol=1e-8)
    ufit = rb.simulate_and_fit_unitarity_batch(n, depths, 3, ptms, seed=SEED)
    assert ufit.success.all()
    np.testing.assert_allclose(ufit.value("decay"), p * p, rtol=1e-8)
    np.testing.assert_allclose(ufit.value("decay"), rb.predicted_unitarity(ptms[:, 0]), rtol=1e-8)


@pytest.mark.parametrize("n", [1, 2])
def test_unitary_noise_keeps_the_purity(gpu, n):
    e, s = rb.simulate_unitarity_acquisition_batch(n, (1, 4, 16, 40), 8, cases.over_rotation(n, 0.11), seed=SEED)
    purity, _ = rb.purity_statistics_batch(e, s)
    assert np.abs(purity - 1.0).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ 7. physics, with shots
def test_mean_z_within_five_sigma_at_every_depth(gpu):
    """64 one-qubit experiments under depolarizing noise p, 32 sequences per depth, 200 shots, symmetric flips f: the mean Z over
    all E K N shots of a depth lies within five binomial standard deviations of (1 - 2 f) p^m, at every depth.  The seed is
    fixed; test_rb_acquire_cpu.py evaluates the same criterion on the host restatement."""
    s = cases.STAT
    ptms = np.tile(cases.depolarizing(1, s["p"]), (s["E"], 1, 1, 1))
    _, _, hist = rb.simulate_rb_acquisition_batch(1, s["depths"], s["K"], ptms, shots=s["shots"], flips=np.full((1, 2), s["flip"]),
                                                  seed=s["seed"], per_sequence=True, return_histograms=True)
    h = hist.astype(np.int64)[:, :, 0, :]
    z = (h[..., 0] - h[..., 1]).reshape(s["E"], len(s["depths"]), s["K"]).sum(axis=(0, 2)) / (s["E"] * s["K"] * s["shots"])
    mu, bound = cases.stat_bounds()
    print("rb_acquire mean Z per depth, in units of the five-sigma bound:", np.abs(z - mu) / bound)
    assert (np.abs(z - mu) <= bound).all()


# ------------------------------------------------------------------------------------------------ 8. the chains
def _same_fit(a, b):
    for f in ("params", "covar", "chisqr", "redchi", "grad_norm", "y"):
        assert same_bits(getattr(a, f), getattr(b, f)), f
    assert (a.status == b.status).all() and (a.iters == b.iters).all() and (a.has_weights == b.has_weights).all()


@pytest.mark.parametrize("points", ["depth", "sequence"])
@pytest.mark.parametrize("n,shots,interleaved", [(1, None, False), (1, 300, True), (2, 300, False)])
def test_rb_chain_is_the_composition(gpu, n, shots, interleaved, points):
    depths, K = (2, 4, 8, 16), 6
    kw = dict(interleaved_gate=cases.interleaved_gate(n) if interleaved else None, shots=shots, flips=cases.FLIPS[n], seed=SEED,
              first_item=2)
    ptms = cases.channels(n, interleaved)
    chain = rb.simulate_and_fit_rb_batch(n, depths, K, ptms, points=points, **kw)
    e, s = rb.simulate_rb_acquisition_batch(n, depths, K, ptms, per_sequence=points == "sequence", **kw)
    x = depths if points == "depth" else np.repeat(depths, K)
    _same_fit(chain, rb.fit_rb_results_batch(x, e, s, num_shots=shots))
    assert chain.params.shape == (3, 3)


@pytest.mark.parametrize("points", ["depth", "sequence"])
@pytest.mark.parametrize("n,shots", [(1, None), (1, 300), (2, 300)])
def test_unitarity_chain_is_the_composition(gpu, n, shots, points):
    depths, K = (1, 2, 4, 8), 6
    kw = dict(shots=shots, flips=cases.FLIPS[n], seed=SEED, first_item=2)
    ptms = cases.channels(n)
    chain = rb.simulate_and_fit_unitarity_batch(n, depths, K, ptms, points=points, **kw)
    e, s = rb.simulate_unitarity_acquisition_batch(n, depths, K, ptms, **kw)
    if points == "sequence":
        by_hand = rb.fit_unitarity_results_batch(np.repeat(depths, K), e, s)
    else:
        # purities -> depth means -> what fbx_fit_prepare_dev does (include/fbx.h) -> the fit
        purity, err = rb.purity_statistics_batch(e, s)
        y, y_err = (a[..., 0] for a in rb.depth_means_batch(purity.reshape(3, len(depths), K, 1), err.reshape(3, len(depths), K, 1)))
        weights = np.empty_like(y)
        for b in range(3):
            good = y_err[b] > 0
            weights[b] = 1.0 / np.where(good, y_err[b], y_err[b][good].min()) if good.any() else 1.0
        guess = np.stack([y[:, 0], np.full(3, 0.95), np.zeros(3)], axis=1)
        by_hand = fitting.curve_fit_batch(_lib.FIT_BASE_DECAY, np.array(depths, dtype=np.float64), y, weights, guess)
        by_hand.has_weights = (y_err > 0).any(axis=1)
    _same_fit(chain, by_hand)


# ------------------------------------------------------------------------------------------------ 9. poison and refusals
@pytest.mark.parametrize("mode", ["standard", "unitarity"])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("what", ["nan_ptm", "flip_1.5"])
def test_a_poisoned_experiment_stays_alone(gpu, n, mode, what):
    flips = np.stack([cases.FLIPS[n]] * 3)
    ptms = cases.channels(n).copy()
    clean = acquire(n, mode, "past_a_workgroup_300", shots=9, flips=flips, ptms=ptms)
    if what == "nan_ptm":
        ptms[1, 0, -1, -1] = np.nan
    else:
        flips[1, n - 1, 1] = 1.5
    got = acquire(n, mode, "past_a_workgroup_300", shots=9, flips=flips, ptms=ptms)
    assert list(got["status"]) == [0, 1, 0] and not clean["status"].any()
    for key in ("e", "s", "vec", "prob"):
        assert np.isnan(got[key][1]).all(), key
        assert same_bits(got[key][[0, 2]], clean[key][[0, 2]]), key
    assert not got["hist"][1].any() and same_bits(got["hist"][[0, 2]], clean["hist"][[0, 2]])
    with pytest.raises(ValueError, match="experiment 1 is poisoned"):
        rb.simulate_rb_acquisition_batch(n, (2, 3), 2, ptms, flips=flips, shots=9)


def test_a_distribution_without_a_sum_poisons_the_whole_experiment(gpu):
    """an all-zero noise matrix: finite inputs, but every distribution sums to 0 -- known to single lanes only, reported for all
    the sequences of the experiment"""
    ptms = cases.channels(1).copy()
    ptms[2] = 0.0
    got = acquire(1, "standard", "past_a_workgroup_300", shots=9, ptms=ptms)
    clean = acquire(1, "standard", "past_a_workgroup_300", shots=9)
    assert list(got["status"]) == [0, 0, 1]
    assert np.isnan(got["e"][2]).all() and np.isnan(got["prob"][2]).all() and np.isnan(got["vec"][2]).all() and not got["hist"][2].any()
    assert same_bits(got["e"][:2], clean["e"][:2]) and same_bits(got["hist"][:2], clean["hist"][:2])


CANARY = -7.25


def _raw(n=1, E=2, depths=(2, 3), K=2, mode=_lib.RB_STANDARD, inter=_lib.CLIFFORD_NONE, G=1, shots=4, first_item=0, outputs=True,
         hist=True, ptms=True):
    """the host-pointer C entry point on canary-filled outputs: (return code, outputs untouched?)"""
    D = 4 ** max(1, min(n, 2))
    cells = 4096                                                           # more than any call here that gets past its checks writes
    d = np.array(depths, dtype=np.int32)
    lam = np.tile(np.eye(D), (max(E, 1) * max(G, 1), 1, 1))
    outs = [np.full(cells, CANARY) for _ in range(4)]
    h = np.full(cells, 0xABCD1234, dtype=np.uint32)
    st = np.full(max(E, 1), -77, dtype=np.int32)
    vec, prob, expect, std_err = (_lib.dptr(o) if outputs else None for o in outs)
    rc = _lib.lib().fbx_rb_acquire(
        n, E, len(depths), d.ctypes.data_as(_lib._ip), K, mode, inter, G, _lib.dptr(lam) if ptms else None, None, None, shots, 5,
        first_item, vec, prob, h.ctypes.data_as(_lib._u32p) if outputs and hist else None, expect, std_err,
        st.ctypes.data_as(_lib._ip) if outputs else None)
    untouched = all((o == CANARY).all() for o in outs) and (h == 0xABCD1234).all() and (st == -77).all()
    return rc, untouched


def test_refusals_leave_the_outputs_alone(gpu):
    BAD, UNSUPPORTED = _lib.FBX_ERR_BAD_ARG, _lib.FBX_ERR_UNSUPPORTED
    assert _raw()[0] == _lib.FBX_OK and not _raw()[1]                       # the helper itself: a good call writes
    refused = {
        "n = 0": (dict(n=0), BAD), "n = 3": (dict(n=3), UNSUPPORTED), "E < 0": (dict(E=-1), BAD), "S < 1": (dict(depths=()), BAD),
        "K < 1": (dict(K=0), BAD), "depth 1, standard": (dict(depths=(2, 1)), BAD),
        "depth 0, unitarity": (dict(depths=(1, 0), mode=_lib.RB_UNITARITY), BAD),
        "invalid element": (dict(inter=0, G=2), BAD),
        "interleaved unitarity": (dict(inter=cases.interleaved_gate(1), G=2, mode=_lib.RB_UNITARITY), BAD),
        "G = 2 without an element": (dict(G=2), BAD), "G = 1 with an element": (dict(inter=cases.interleaved_gate(1), G=1), BAD),
        "first_item < 0": (dict(first_item=-1), BAD), "every output NULL": (dict(outputs=False), BAD),
        "hist without shots": (dict(shots=0), BAD), "n_shots < 0": (dict(shots=-1), BAD), "n_shots = 2^31": (dict(shots=2 ** 31), BAD),
        "S K NB = 2^32": (dict(depths=(1,) * 4, K=2 ** 30 // 9 * 9 + 9, mode=_lib.RB_UNITARITY, n=2), BAD),
        "unknown mode": (dict(mode=2), BAD), "257 depths": (dict(depths=(2,) * 257), UNSUPPORTED), "NULL noise_ptms": (dict(ptms=False), BAD),
    }
    for name, (kw, code) in refused.items():
        rc, untouched = _raw(**kw)
        assert rc == code and untouched, name
    try:
        _lib.check(_raw(depths=(2, 1))[0])
    except ValueError as err:
        assert str(err) == "Sequence depth must be at least 2 for rb sequences, or at least 1 for unitarity sequences."
    rc, untouched = _raw(E=0)
    assert rc == _lib.FBX_OK and untouched                                  # E == 0 does nothing
    # the depth means
    v = np.ones(8)
    out = np.full(8, CANARY)
    for args in ((-1, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        assert _lib.lib().fbx_rb_depth_means(*args, _lib.dptr(v), None, _lib.dptr(out), None) == BAD and (out == CANARY).all()
    assert _lib.lib().fbx_rb_depth_means(1, 1, 1, 1, _lib.dptr(v), None, None, None) == BAD
