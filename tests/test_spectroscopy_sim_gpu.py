"""fbx_spec_acquire and the simulators of fbx.qubit_spectroscopy on the device: the shots against the host restatement bit for bit,
the probabilities against 50-digit arithmetic, independence of the batch, the resident chains against the public calls chained by
hand, the physics, poison and refusals."""
import numpy as np
import pytest

import spectroscopy_cases as cases
from fbx import _lib, qubit_spectroscopy as qs, synthetic
from fbx.analysis import fitting
from fbx.utils import transform_pauli_moments_to_bit
from spectroscopy_cases import same_bits

pytestmark = pytest.mark.gpu

NAMES = ("prob", "exact", "expect", "std_err", "counts", "bit", "bit_err")
SENTINEL = -7.0


def acquire(x, params, flips=None, shots=0, seed=cases.SEED, first_item=0, dev=False):
    """every output of one call, by name, through the host form or (``dev``) the device-pointer form"""
    x, params = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(params, dtype=np.float64)
    flips = None if flips is None else np.ascontiguousarray(flips, dtype=np.float64)
    B, K = params.shape[0], x.shape[-1]
    stride = K if x.ndim == 2 else 0
    lib = _lib.lib()
    if dev:
        with _lib.DeviceScope() as scope:
            d = {name: scope.alloc(8 * B * K) for name in NAMES}
            d_status = scope.alloc(4 * B)
            d_x, d_p, d_f = scope.upload(x), scope.upload(params), scope.upload(flips)
            _lib.check(lib.fbx_spec_acquire_dev(B, K, d_x.ptr, stride, d_p.ptr, _lib.devptr(d_f), shots, seed, first_item,
                                                *[d[name].ptr for name in NAMES], d_status.ptr))
            _lib.synchronize()
            out = {name: d[name].to_array(np.float64, (B, K)) for name in NAMES}
            out["status"] = d_status.to_array(np.int32, (B,))
        return out
    out = {name: np.full((B, K), SENTINEL) for name in NAMES}
    out["status"] = np.full(B, -7, dtype=np.int32)
    _lib.check(lib.fbx_spec_acquire(B, K, _lib.dptr(x), stride, _lib.dptr(params), _lib.dptr(flips), shots, seed, first_item,
                                    *[_lib.dptr(out[name]) for name in NAMES], _lib.iptr(out["status"])))
    return out


def check_against_restatement(got, shots, first_item, rows=slice(None)):
    """expect / std_err / counts of the rows against the host restatement fed the device's own probabilities, and the bit form
    against _bit_data's operations on those outputs"""
    e, s, counts, _ = synthetic.restate_spectroscopy_counts(got["prob"][rows], shots, cases.SEED,
                                                            first_item + (rows.start or 0))
    assert same_bits(got["expect"][rows], e) and same_bits(got["std_err"][rows], s) and same_bits(got["counts"][rows], counts)
    assert same_bits(got["exact"][rows], 1 - 2 * got["prob"][rows])
    p1, var = transform_pauli_moments_to_bit(-1 * got["expect"][rows], got["std_err"][rows] ** 2)
    assert same_bits(got["bit"][rows], p1) and same_bits(got["bit_err"][rows], np.sqrt(var))
    p1_front, weights = qs._bit_data(got["expect"][rows], got["std_err"][rows])
    assert same_bits(got["bit"][rows], p1_front)
    err = got["bit_err"][rows]
    if weights is None:
        assert not (err > 0).any()
    else:
        pos = err > 0
        has = pos.any(axis=1, keepdims=True)
        smallest = np.where(has, np.where(pos, err, np.inf).min(axis=1, keepdims=True), 1.0)
        assert same_bits(weights, np.where(has, 1 / np.where(pos, err, smallest), 1.0))


# ------------------------------------------------------------------------------------------------ 1. counts bit for bit
@pytest.mark.parametrize("name", sorted(cases.shape_cases()))
def test_counts_equal_the_host_restatement(gpu, name):
    case = cases.shape_cases()[name]
    x, params, flips = cases.case_inputs(case)
    got = acquire(x, params, flips, case["shots"], first_item=case["first_item"])
    assert not got["status"].any()
    check_against_restatement(got, case["shots"], case["first_item"])
    if case["shots"]:
        assert (got["counts"] == case["shots"]).all()
        if case["shots"] >= 257:
            assert len(np.unique(got["expect"])) > 2             # (counts that vary: the comparison is not of constants)


@pytest.mark.parametrize("K", [32, 70])
def test_both_sides_of_the_lane_switch(gpu, K):
    """B K at FBX_TOMO_LANE_MIN_UNITS (K = 32: exactly; K = 70: the first B that reaches it, items straddling wavefronts) takes a
    lane per unit, one item fewer a wavefront per unit: the same bits on the shared items, and the restatement's at both ends"""
    units = cases.lane_min_units()
    B = -(-units // K)
    assert B * K >= units > (B - 1) * K and (K != 32 or B * K == units)
    x, params = cases.grid(B, K, per_item_x=False, seed=21)
    flips = np.broadcast_to(cases.FLIPS, (B, 2))
    first = cases.FIRST_ITEMS[1]
    lane = acquire(x, params, flips, 5, first_item=first)
    wave = acquire(x, params[:B - 1], flips[:B - 1], 5, first_item=first)
    assert not lane["status"].any()
    for name in NAMES:
        assert same_bits(lane[name][:B - 1], wave[name]), name
    check_against_restatement(lane, 5, first, slice(0, 40))
    check_against_restatement(lane, 5, first, slice(B - 40, B))
    assert len(np.unique(lane["expect"])) > 2


# ------------------------------------------------------------------------------------------------ 2. probabilities
@pytest.mark.parametrize("name", sorted(cases.PROBABILITY_GRIDS))
def test_probabilities_within_the_mirrors_own_error(gpu, name):
    """prob_out and exact_out against the contract's formula in 50 digits: within max(4 u, 8 x 2^-53), u the deviation of the
    numpy restatement from the same values (measured in tests/test_spectroscopy_sim_cpu.py: 1.3-1.6 x 2^-53 for prob, 3.0-3.6 x
    2^-53 for exact) -- a margin of 4 for a second libm, and a floor of four roundings around two functions of 1-2 ulp.
    Measured on one MI355X: 1.34-1.84 x 2^-53 for prob, 2.98-3.69 x 2^-53 for exact."""
    x, params, flips = cases.probability_grid(name)
    got = acquire(x, params, flips, 0)
    assert not got["status"].any()
    ps, mus = cases.mp_probabilities(name)
    u_p, u_mu = cases.mirror_deviation(name)
    d_p, d_mu = cases.deviation(got["prob"], ps), cases.deviation(got["exact"], mus)
    print(f"spectroscopy device deviation on {name}: prob {d_p / cases.U_ROUND:.2f} x 2^-53 (mirror {u_p / cases.U_ROUND:.2f}), "
          f"exact {d_mu / cases.U_ROUND:.2f} x 2^-53 (mirror {u_mu / cases.U_ROUND:.2f})")
    assert d_p <= max(4 * u_p, cases.FLOOR)
    assert d_mu <= max(4 * u_mu, cases.FLOOR)
    mirror = synthetic.spectroscopy_probabilities(x, params, flips)
    assert np.abs(got["prob"] - mirror).max() <= max(4 * u_p, cases.FLOOR) + u_p


def test_probabilities_are_exact_where_no_function_is_involved(gpu):
    x = np.array([0.0, 0.5, 3.0])
    params = [[0.25, np.inf, np.inf, 0.0, 0.0, 0.5],             # infinite times: env = 1; omega = offset = 0: cos = 1
              [0.25, 7.0, np.inf, 0.0, 0.0, 0.125],              # T1 at x = 0: baseline + amplitude
              [0.25, np.inf, np.inf, 1.3, 0.0, 0.5],             # x = 0: cos(0) = 1
              [0.25, np.inf, 4.0, 0.0, 0.0, 0.125]]              # a Gaussian envelope alone, at x = 0
    got = acquire(x, params)
    assert not got["status"].any()
    assert (got["prob"][0] == 0.75).all() and got["prob"][1, 0] == 0.375 and got["prob"][2, 0] == 0.75 and got["prob"][3, 0] == 0.375
    assert (got["exact"][0] == -0.5).all() and got["exact"][1, 0] == 0.25
    flipped = acquire(x, params[:1], flips=[cases.FLIPS])
    assert (flipped["prob"] == cases.FLIPS[0] * (1 - 0.75) + (1 - cases.FLIPS[1]) * 0.75).all()


# ------------------------------------------------------------------------------------------------ 3. batch independence
def test_an_item_does_not_depend_on_its_batch(gpu):
    """item 137 of a batch of 300, alone under first_item = 137, and as item 7 of the ten items from 130 on: the same bits"""
    x, params = cases.grid(300, 7, per_item_x=True, seed=31)
    flips = np.stack([cases.FLIPS * (1 + 0.001 * b) for b in range(300)])
    whole = acquire(x, params, flips, 257)
    alone = acquire(x[137:138], params[137:138], flips[137:138], 257, first_item=137)
    part = acquire(x[130:140], params[130:140], flips[130:140], 257, first_item=130)
    for name in NAMES:
        assert same_bits(whole[name][137:138], alone[name]) and same_bits(whole[name][130:140], part[name]), name
    assert not same_bits(whole["expect"][137], whole["expect"][138])


# ------------------------------------------------------------------------------------------------ 4. extremes
def test_probabilities_outside_the_unit_interval_are_clamped_for_the_threshold_only(gpu):
    x = np.array([0.0, 1.0])
    params = [[0.0, 1.0, 1.0, 0.0, 0.0, -0.25], [0.0, 1.0, 1.0, 0.0, 0.0, 0.0],            # p_read <= 0: every shot +1
              [0.0, 1.0, 1.0, 0.0, 0.0, 1.0], [0.0, 1.0, 1.0, 0.0, 0.0, 1.5]]              # p_read >= 1: every shot -1
    got = acquire(x, params, shots=1000)
    assert not got["status"].any()
    assert (got["expect"][:2] == 1.0).all() and (got["expect"][2:] == -1.0).all() and not got["std_err"].any()
    assert (got["counts"] == 1000).all()
    assert (got["prob"] == np.array([[-0.25], [0.0], [1.0], [1.5]])).all()
    assert (got["exact"] == np.array([[1.5], [1.0], [-1.0], [-2.0]])).all()                 # unclamped
    assert (got["bit"][:2] == 0.0).all() and (got["bit"][2:] == 1.0).all() and not got["bit_err"].any()


def test_without_shots_the_expectation_is_the_exact_one(gpu):
    x, params = cases.grid(9, 5, per_item_x=True, seed=41)
    got = acquire(x, params, flips=np.broadcast_to(cases.FLIPS, (9, 2)), shots=0)
    assert same_bits(got["expect"], got["exact"]) and not got["std_err"].any() and not got["counts"].any()
    assert not got["bit_err"].any() and same_bits(got["bit"], (-1 * got["exact"] + 1) / 2)


# ------------------------------------------------------------------------------------------------ 5. the resident chains
T2_TIMES = np.linspace(0.0, 20.0, 20)
CHAINS = {
    "t1": (lambda **kw: qs.simulate_and_fit_t1_batch(cases.TIMES, [14.0, 20.0, 26.0, 32.0, 38.0], **kw),
           lambda **kw: qs.simulate_t1_batch(cases.TIMES, [14.0, 20.0, 26.0, 32.0, 38.0], **kw),
           lambda e, s: qs.fit_t1_results_batch(cases.TIMES, e, s)),
    "t2_star": (lambda **kw: qs.simulate_and_fit_t2_batch(T2_TIMES, [9.0, 12.0, 15.0, 18.0, 21.0], detuning=2e5,
                                                          frequency_offset=[0.0, 1e4, -1e4, 2e4, 5e3], gauss_time=60.0, **kw),
                lambda **kw: qs.simulate_t2_star_batch(T2_TIMES, [9.0, 12.0, 15.0, 18.0, 21.0], detuning=2e5,
                                                       frequency_offset=[0.0, 1e4, -1e4, 2e4, 5e3], gauss_time=60.0, **kw),
                lambda e, s: qs.fit_t2_results_batch(T2_TIMES, e, s, detuning=2e5)),
    "t2_echo": (lambda **kw: qs.simulate_and_fit_t2_batch(T2_TIMES, [19.0, 22.0, 25.0, 28.0, 31.0], kind="echo", detuning=2e5,
                                                          contrast=0.9, **kw),
                lambda **kw: qs.simulate_t2_echo_batch(T2_TIMES, [19.0, 22.0, 25.0, 28.0, 31.0], detuning=2e5, contrast=0.9, **kw),
                lambda e, s: qs.fit_t2_results_batch(T2_TIMES, e, s, detuning=2e5)),
    "rabi": (lambda **kw: qs.simulate_and_fit_rabi_batch(cases.ANGLES, [1.0, 0.97, 1.03, 1.05, 0.95], offset=0.05, **kw),
             lambda **kw: qs.simulate_rabi_batch(cases.ANGLES, [1.0, 0.97, 1.03, 1.05, 0.95], offset=0.05, **kw),
             lambda e, s: qs.fit_rabi_results_batch(cases.ANGLES, e, s)),
    "cz_phase_ramsey": (lambda **kw: qs.simulate_and_fit_cz_phase_ramsey_batch(cases.ANGLES, [0.1, -0.4, 0.7, 1.0, -0.9], **kw),
                        lambda **kw: qs.simulate_cz_phase_ramsey_batch(cases.ANGLES, [0.1, -0.4, 0.7, 1.0, -0.9], **kw),
                        lambda e, s: qs.fit_cz_phase_ramsey_results_batch(cases.ANGLES, e, s)),
}


@pytest.mark.parametrize("shots", [None, 300])
@pytest.mark.parametrize("kind", sorted(CHAINS))
def test_chain_is_the_composition(gpu, kind, shots):
    """B = 5, K = 20: simulate_and_fit_* against simulate_* followed by fit_*_results_batch, every FitBatch field bit for bit"""
    chain_fn, simulate, fit = CHAINS[kind]
    kw = dict(shots=shots, flips=cases.FLIPS, seed=cases.SEED, first_item=2)
    chain = chain_fn(**kw)
    e, s = simulate(**kw)
    by_hand = fit(e, s)
    assert chain.params.shape[0] == 5 and chain.y.shape == (5, 20) and chain.model == by_hand.model
    for f in ("params", "covar", "chisqr", "redchi", "grad_norm", "y", "stderr", "best_fit", "init_values", "x"):
        assert same_bits(getattr(chain, f), getattr(by_hand, f)), f
    for f in ("status", "iters", "success", "singular"):
        assert (getattr(chain, f) == getattr(by_hand, f)).all(), f
    assert chain.vary == by_hand.vary and chain.param_names == by_hand.param_names
    if shots is None:
        # no error is above zero: the front end passes weights=None, the chain unit weights -- the same fit
        assert not (s > 0).any() and by_hand.weights is None and (chain.weights == 1.0).all() and not chain.has_weights.any()
    else:
        assert chain.has_weights.all() and same_bits(chain.weights, by_hand.weights)


def test_chain_raises_for_a_poisoned_qubit(gpu):
    with pytest.raises(ValueError, match="qubit 1 is poisoned"):
        qs.simulate_and_fit_t1_batch(cases.TIMES, [14.0, np.nan, 20.0])


# ------------------------------------------------------------------------------------------------ 6. physics
def _identifiable(kind, params):
    """the combinations of the fit parameters the data determine: decay_time_param_decay has amplitude and offset only through
    amplitude exp(offset / decay_time)"""
    if kind == "t1":
        return np.stack([params[:, 0] * np.exp(params[:, 2] / params[:, 1]), params[:, 1]], axis=1)
    return params


PHYSICS = {
    "t1": (dict(t1=[14.0, 20.0, 26.0, 32.0, 38.0]), cases.TIMES, np.array([0.0, 0.05]),
           lambda x, p, **kw: qs.simulate_and_fit_t1_batch(x, **p, **kw), lambda x, e: qs.fit_t1_results_batch(x, e)),
    "t2_star": (dict(t2=[9.0, 12.0, 15.0, 18.0, 21.0], detuning=2e5, frequency_offset=[0.0, 1e4, -1e4, 2e4, 5e3]), T2_TIMES, cases.FLIPS,
                lambda x, p, **kw: qs.simulate_and_fit_t2_batch(x, p["t2"], detuning=p["detuning"],
                                                                frequency_offset=p["frequency_offset"], **kw),
                lambda x, e: qs.fit_t2_results_batch(x, e, detuning=2e5)),
    "rabi": (dict(scale=[1.0, 0.97, 1.03, 1.05, 0.95], offset=0.05, contrast=0.9), cases.ANGLES, cases.FLIPS,
             lambda x, p, **kw: qs.simulate_and_fit_rabi_batch(x, **p, **kw), lambda x, e: qs.fit_rabi_results_batch(x, e)),
    "cz_phase_ramsey": (dict(cz_phase=[0.1, -0.4, 0.7, 1.0, -0.9], contrast=0.95), cases.ANGLES, cases.FLIPS,
                        lambda x, p, **kw: qs.simulate_and_fit_cz_phase_ramsey_batch(x, **p, **kw),
                        lambda x, e: qs.fit_cz_phase_ramsey_results_batch(x, e)),
}
HOST_MODELS = {"t1": fitting.decay_time_param_decay, "t2_star": fitting.decaying_cosine, "rabi": fitting.shifted_cosine,
               "cz_phase_ramsey": fitting.shifted_cosine}


@pytest.mark.parametrize("kind", sorted(PHYSICS))
def test_exact_chain_recovers_the_predicted_parameters(gpu, kind):
    """shots=None: the fitted parameters against predicted_fit_parameters, held to 4 x what fit_*_results_batch itself reaches on
    the host-evaluated model curve at the same points (measured here: ONE deviation per fit batch, the largest over the
    parameters, all of order one, and the five qubits -- both fits stop within a few 2^-53 of the prediction, where a single
    parameter of the reference fit can land on it exactly and 4 x 0 would bound nothing).  T1 without a readout floor (f0 = 0):
    the model has no baseline."""
    physical, x, flips, chain_fn, fit = PHYSICS[kind]
    predicted = qs.predicted_fit_parameters(kind, flips=flips, **physical)
    curve = np.stack([HOST_MODELS[kind](x, *row) for row in predicted])              # the probability of reading 1
    on_host_curve = fit(x, 1 - 2 * curve)
    chain = chain_fn(x, physical, flips=flips, seed=cases.SEED)
    assert on_host_curve.success.all() and chain.success.all()
    want = _identifiable(kind, predicted)
    d_host = np.abs(_identifiable(kind, on_host_curve.params) - want).max()
    d_chain = np.abs(_identifiable(kind, chain.params) - want).max()
    print(f"spectroscopy {kind}: largest |fitted - predicted|: chain {d_chain}, fit of the host curve {d_host}; per parameter: "
          f"chain {np.abs(_identifiable(kind, chain.params) - want).max(axis=0)}, "
          f"host curve {np.abs(_identifiable(kind, on_host_curve.params) - want).max(axis=0)}")
    assert d_chain <= 4 * d_host


def test_t1_with_shots_within_five_standard_errors(gpu):
    """64 qubits, 1000 shots, flips (0.02, 0.05): every fitted decay_time within 5 of its own fit standard errors of the true T1
    (amplitude and decay_time free, offset fixed: with all three free the covariance is singular).  The model has no baseline, so
    the readout floor f0 = 0.02 pulls every fitted T1 up; the delays stop at 12 us for T1 of 20-40 us, where a noise-free fit of
    the folded curve is off by 0.72-1.24 of the fit's standard error (tests/test_spectroscopy_sim_cpu.py), leaving 3.76: one item
    in 5900 by chance, 1 % over the 64.  Measured on one MI355X: largest 4.35, mean 1.16 -- the figures scipy gives on the host
    restatement of the same shots."""
    s = cases.T1_STAT
    truth = cases.t1_stat_truth()
    batch = qs.simulate_and_fit_t1_batch(cases.T1_STAT_TIMES, truth, shots=s["shots"], flips=s["flips"], seed=s["seed"],
                                         vary=(True, True, False))
    assert batch.success.all() and batch.has_weights.all()
    z = (batch.value("decay_time") - truth) / batch.error("decay_time")
    print("spectroscopy T1, (fitted - true) / stderr: largest", np.abs(z).max(), "mean", z.mean())
    assert (np.abs(z) <= 5).all()


def test_reference_shaped_results_give_the_batch_items(gpu):
    """simulate_spectroscopy_results -> get_stats_by_qubit -> fit_t1_results: the item of the batch call"""
    qubits, t1 = [3, 7, 11], [14.0, 22.0, 30.0]
    kw = dict(shots=200, flips=cases.FLIPS, seed=cases.SEED, first_item=4)
    results = qs.simulate_spectroscopy_results("t1", qubits, cases.TIMES, t1=t1, **kw)
    assert len(results) == len(cases.TIMES) and all(len(r) == 3 for r in results)
    assert str(results[0][1].setting) == "Z-_7→(1+0j)*Z7" and results[0][1].total_counts == 200
    e, s = qs.simulate_t1_batch(cases.TIMES, t1, **kw)
    batch = qs.fit_t1_results_batch(cases.TIMES, e, s)
    stats = qs.get_stats_by_qubit(results)
    assert sorted(stats) == qubits
    for b, q in enumerate(qubits):
        assert same_bits(stats[q]["expectation"], e[b]) and same_bits(stats[q]["std_err"], s[b])
        fit = qs.fit_t1_results(cases.TIMES, stats[q]["expectation"], stats[q]["std_err"])
        assert same_bits(list(fit.best_values.values()), batch.params[b]) and fit.chisqr == batch.chisqr[b]
    for kind, state, physical in (("t2_star", "Y-_5→(1+0j)*Y5", dict(t2=9.0)), ("t2_echo", "Y-_5→(1+0j)*Y5", dict(t2_echo=9.0)),
                                  ("rabi", "Z+_5→(1+0j)*Z5", {}), ("cz_phase_ramsey", "Y-_5→(1+0j)*Y5", dict(cz_phase=0.3))):
        assert str(qs.simulate_spectroscopy_results(kind, [5], [0.0, 1.0], **physical)[1][0].setting) == state


# ------------------------------------------------------------------------------------------------ 7. poison and refusals
POISON = {"nan_amplitude": (0, np.nan), "inf_omega": (3, np.inf), "nan_offset": (4, np.nan), "inf_baseline": (5, -np.inf),
          "zero_decay_time": (1, 0.0), "negative_decay_time": (1, -3.0), "nan_decay_time": (1, np.nan), "zero_gauss_time": (2, 0.0),
          "nan_gauss_time": (2, np.nan), "nan_x": ("x", np.nan), "inf_x": ("x", np.inf), "flip_1.5": ("flip", 1.5),
          "flip_negative": ("flip", -0.1), "flip_nan": ("flip", np.nan)}


@pytest.mark.parametrize("form", ["wavefront", "lane"])
@pytest.mark.parametrize("what", sorted(POISON))
def test_a_poisoned_item_stays_alone(gpu, what, form):
    """one poisoned item of each kind among clean ones: status 1, NaN in every double output, counts = n_shots; the neighbours
    bit-identical to the clean call.  Both forms: 3 items of 3 points, and FBX_TOMO_LANE_MIN_UNITS / 2048 items of 2048."""
    K = 3 if form == "wavefront" else 2048
    B = 3 if form == "wavefront" else cases.lane_min_units() // K
    x, params = cases.grid(B, K, per_item_x=True, seed=51)
    flips = np.broadcast_to(cases.FLIPS, (B, 2)).copy()
    clean = acquire(x, params, flips, 9)
    where, value = POISON[what]
    if where == "x":
        x[1, K - 1] = value
    elif where == "flip":
        flips[1, 1] = value
    else:
        params[1, where] = value
    got = acquire(x, params, flips, 9)
    others = [b for b in range(B) if b != 1]
    assert not clean["status"].any() and got["status"][1] == 1 and not got["status"][others].any()
    for name in NAMES:
        if name == "counts":
            assert (got[name][1] == 9).all()
        else:
            assert np.isnan(got[name][1]).all(), name
        assert same_bits(got[name][others], clean[name][others]), name


def test_infinite_times_are_not_poison_and_a_shared_bad_point_poisons_everyone(gpu):
    x = np.array([0.0, 1.0, np.nan])
    params = [[0.5, np.inf, np.inf, 1.0, 0.0, 0.5], [0.5, 3.0, np.inf, 1.0, 0.0, 0.5]]
    assert not acquire(x[:2], params, shots=3)["status"].any()
    got = acquire(x, params, shots=3)
    assert got["status"].all() and np.isnan(got["prob"]).all()


def test_front_ends_report_poison(gpu):
    with pytest.raises(ValueError, match="qubit 2 is poisoned"):
        qs.simulate_t1_batch(cases.TIMES, [10.0, 12.0, -1.0], shots=5)
    e, s, p, exact, status = qs.simulate_t1_batch(cases.TIMES, [10.0, 12.0, -1.0], shots=5, seed=1, return_probabilities=True,
                                                  return_exact=True, return_status=True)
    assert list(status) == [0, 0, 1] and np.isnan(e[2]).all() and np.isnan(p[2]).all() and np.isnan(exact[2]).all()
    assert np.isfinite(e[:2]).all() and np.isfinite(s[:2]).all() and same_bits(exact[:2], 1 - 2 * p[:2])


def test_refusals_touch_no_buffer(gpu):
    lib = _lib.lib()
    x, params = cases.grid(2, 4)
    out = np.full((2, 4), SENTINEL)
    status = np.full(2, -7, dtype=np.int32)
    for B, K, stride, shots, first in ((-1, 4, 0, 5, 0), (2, 0, 0, 5, 0), (2, 65537, 0, 5, 0), (2, 4, 3, 5, 0), (2, 4, 0, -1, 0),
                                       (2, 4, 0, 2 ** 32, 0), (2, 4, 0, 5, -1)):
        rc = lib.fbx_spec_acquire(B, K, _lib.dptr(x), stride, _lib.dptr(params), None, shots, 1, first, _lib.dptr(out), None,
                                  _lib.dptr(out), None, None, None, None, _lib.iptr(status))
        assert rc == _lib.FBX_ERR_BAD_ARG and (out == SENTINEL).all() and (status == -7).all(), (B, K, stride, shots, first)
    rc = lib.fbx_spec_acquire(2, 4, _lib.dptr(x), 0, _lib.dptr(params), None, 5, 1, 0, None, None, None, None, None, None, None, None)
    assert rc == _lib.FBX_ERR_BAD_ARG and b"every output is NULL" in lib.fbx_last_error()
    with pytest.raises(ValueError, match="every output is NULL"):
        _lib.check(rc)
    assert lib.fbx_spec_acquire(0, 4, None, 0, None, None, 5, 1, 0, _lib.dptr(out), None, None, None, None, None, None, None) == 0
    assert lib.fbx_spec_acquire_dev(0, 4, None, 0, None, None, 5, 1, 0, None, None, None, None, None, None, None,
                                    status.ctypes.data) == 0
    assert (out == SENTINEL).all() and (status == -7).all()
    # status alone is an output: the call runs
    assert lib.fbx_spec_acquire(2, 4, _lib.dptr(x), 0, _lib.dptr(params), None, 5, 1, 0, None, None, None, None, None, None, None,
                                _lib.iptr(status)) == 0 and not status.any()


@pytest.mark.parametrize("name", ["K70_shots257", "K3_shots5", "K1_shots0"])
def test_host_form_equals_device_form(gpu, name):
    case = cases.shape_cases()[name]
    x, params, flips = cases.case_inputs(case)
    host = acquire(x, params, flips, case["shots"], first_item=case["first_item"])
    dev = acquire(x, params, flips, case["shots"], first_item=case["first_item"], dev=True)
    for key in NAMES:
        assert same_bits(host[key], dev[key]), key
    assert (host["status"] == dev["status"]).all()
    # a call with some outputs only writes the same values
    some = np.full(host["bit"].shape, SENTINEL)
    K = x.shape[-1]
    _lib.check(_lib.lib().fbx_spec_acquire(params.shape[0], K, _lib.dptr(np.ascontiguousarray(x)), K if x.ndim == 2 else 0,
                                           _lib.dptr(params), _lib.dptr(flips), case["shots"], cases.SEED, case["first_item"], None,
                                           None, None, None, None, _lib.dptr(some), None, None))
    assert same_bits(some, host["bit"])
