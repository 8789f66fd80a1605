"""The host side of the qubit-spectroscopy acquisition (no GPU): the mirror of fbx_spec_acquire against 50-digit arithmetic and a
shot-by-shot count, the closed-form fit parameters, and the front ends' argument handling."""
import numpy as np
import pytest

import spectroscopy_cases as cases
from fbx import _lib, qubit_spectroscopy as qs, synthetic
from fbx.analysis import fitting


# ------------------------------------------------------------------------------------------------ the stream
@pytest.mark.parametrize("first_item", cases.FIRST_ITEMS)
@pytest.mark.parametrize("shots", [1, 3, 4, 5, 9])
def test_mirror_counts_equal_a_shot_by_shot_count(shots, first_item):
    """restate_spectroscopy_counts (vectorised over Philox blocks, the last block cut) against one block per shot"""
    p = np.array([[0.0, 0.3, 0.5], [0.77, 1.0, 1.3], [-0.2, 0.999, 1e-9]])
    e, s, counts, k_plus = synthetic.restate_spectroscopy_counts(p, shots, cases.SEED, first_item)
    want = cases.count_shot_by_shot(p, shots, cases.SEED, first_item)
    assert (k_plus == want).all()
    assert (k_plus[p <= 0.0] == shots).all() and (k_plus[p >= 1.0] == 0).all()       # clamped: all +1, all -1
    assert cases.same_bits(e, (2 * want - shots) / float(shots)) and (counts == shots).all()
    assert cases.same_bits(s, np.sqrt(4.0 * want * (shots - want) / shots) / shots)


def test_mirror_without_shots_is_exact():
    p = np.array([[0.25, 1.5]])
    e, s, counts, k_plus = synthetic.restate_spectroscopy_counts(p, None, 1)
    assert cases.same_bits(e, 1 - 2 * p) and not s.any() and not counts.any() and not k_plus.any()
    assert all(cases.same_bits(a, b) for a, b in zip(synthetic.restate_spectroscopy_counts(p, 0, 1)[:3], (e, s, counts)))


def test_streams_differ_by_tag_seed_item_and_point():
    p = np.full((2, 2), 0.5)
    base = synthetic.restate_spectroscopy_counts(p, 4096, 9)[3]
    assert len(set(base.ravel())) > 1                                                    # items and points draw apart
    assert (synthetic.restate_spectroscopy_counts(p, 4096, 10)[3] != base).any()
    assert (synthetic.restate_spectroscopy_counts(p, 4096, 9, first_item=1)[3][0] == base[1]).all()
    assert (synthetic.restate_tomography_counts(1 - 2 * p, 1.0, 4096, 9)[3] != base).any()     # another tag, same counters
    tags = [v for k, v in vars(synthetic).items() if k.endswith("KEY_TAG")]
    assert len(tags) == len(set(tags)) and synthetic.SPECTROSCOPY_KEY_TAG == int.from_bytes(b"QSPC", "big")


# ------------------------------------------------------------------------------------------------ the curve
@pytest.mark.parametrize("name", sorted(cases.PROBABILITY_GRIDS))
def test_mirror_probabilities_against_mpmath(name):
    """u: the largest deviation of the numpy restatement from the contract's formula in 50 digits.  Nothing bounds it from
    outside but the roundings it consists of: a division and a product in the exponent (|exponent| <= 20 + 16), exp, two
    products, cos, a sum, and with flips five more operations, all on values of magnitude <= 2 -- 40 unit roundoffs is generous."""
    u_p, u_mu = cases.mirror_deviation(name)
    print(f"spectroscopy mirror deviation on {name}: u(prob) = {u_p:.3e} = {u_p / cases.U_ROUND:.2f} x 2^-53, "
          f"u(exact) = {u_mu:.3e} = {u_mu / cases.U_ROUND:.2f} x 2^-53")
    assert 0 < u_p <= 40 * cases.U_ROUND and 0 < u_mu <= 80 * cases.U_ROUND


def test_mirror_is_exact_where_no_function_is_involved():
    x = np.array([0.0, 0.5, 3.0])
    p = synthetic.spectroscopy_probabilities(x, [[0.25, np.inf, np.inf, 0.0, 0.0, 0.5],        # env = 1, cos = 1
                                                 [0.25, 7.0, np.inf, 0.0, 0.0, 0.125],         # x = 0: exp(-0) = 1
                                                 [0.25, np.inf, np.inf, 1.3, 0.0, 0.5]])       # x = 0: cos(0) = 1
    assert (p[0] == 0.75).all() and p[1, 0] == 0.375 and p[2, 0] == 0.75
    flipped = synthetic.spectroscopy_probabilities(x, [[0.25, np.inf, np.inf, 0.0, 0.0, 0.5]], flips=(0.03, 0.08))
    assert (flipped == 0.03 * (1 - 0.75) + (1 - 0.08) * 0.75).all()


def test_mirror_argument_errors():
    with pytest.raises(ValueError):
        synthetic.spectroscopy_probabilities(np.zeros(3), np.zeros((2, 5)))
    with pytest.raises(ValueError):
        synthetic.spectroscopy_probabilities(np.zeros((3, 3)), np.zeros((2, 6)))


# ------------------------------------------------------------------------------------------------ closed forms
FIT_MODELS = {"t1": fitting.decay_time_param_decay, "t2_star": fitting.decaying_cosine, "t2_echo": fitting.decaying_cosine,
              "rabi": fitting.shifted_cosine, "cz_phase_ramsey": fitting.shifted_cosine}
PHYSICAL = {"t1": dict(t1=[17.0, 31.0, 8.5]),
            "t2_star": dict(t2=[9.0, 14.0, 22.0], detuning=2e6, frequency_offset=[0.0, 3e4, -5e4], contrast=[1.0, 0.9, 0.8]),
            "t2_echo": dict(t2_echo=[19.0, 24.0, 32.0], detuning=1.5e6, contrast=0.95),
            "rabi": dict(scale=[1.0, 0.97, 1.04], offset=[0.0, 0.1, -0.2], contrast=[1.0, 0.9, 0.8]),
            "cz_phase_ramsey": dict(cz_phase=[0.3, -1.1, 2.0], scale=1.0, contrast=[1.0, 0.9, 0.8])}
READOUT = np.array([[0.0, 0.05], [0.02, 0.05], [0.04, 0.0]])


@pytest.mark.parametrize("kind", sorted(FIT_MODELS))
def test_predicted_fit_parameters_describe_the_mirror_curve(kind):
    """the fit model at the predicted parameters equals the mirror's readout-folded curve at many points, to rounding (T1: the
    model has no baseline, so f0 = 0 and no thermal population)"""
    x = np.linspace(0.0, 50.0, 400)
    flips = READOUT if kind != "t1" else READOUT[[0, 0, 0]]
    predicted = qs.predicted_fit_parameters(kind, flips=flips, **PHYSICAL[kind])
    assert predicted.shape == (3, len(fitting.MODELS[qs._KINDS[kind][0]][2]))
    a = qs._Acquisition(x, qs._curve(kind, PHYSICAL[kind]), flips, None, 0, 0)
    curve = synthetic.spectroscopy_probabilities(a.x, a.params, a.flips)
    model = np.stack([FIT_MODELS[kind](x, *row) for row in predicted])
    assert np.abs(model - curve).max() <= 1e-13                    # arguments up to 2 pi 2.05 x 50 = 644: 644 x 2^-53 x 2 in the cosine


def test_predicted_fit_parameters_without_flips_and_bad_kinds():
    assert (qs.predicted_fit_parameters("rabi") == [[-0.5, 0.0, 0.5, 1.0]]).all()
    assert (qs.predicted_fit_parameters("t1", t1=12.0, thermal_population=0.1) == [[0.9, 12.0, 0.0]]).all()
    for bad in (lambda: qs.predicted_fit_parameters("t3"), lambda: qs.predicted_fit_parameters("t1"),
                lambda: qs.predicted_fit_parameters("rabi", t1=3.0), lambda: qs.predicted_fit_parameters("rabi", flips=[0.1])):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ the front ends' arguments
def test_curve_columns_and_units():
    """detuning and frequency_offset are in Hz, times in microseconds: omega = 2 pi (detuning + offset) / MHZ"""
    a = qs._Acquisition(np.arange(4.0), qs._curve("t2_star", dict(t2=[5.0, 6.0], detuning=2e6, frequency_offset=[0.0, 5e5],
                                                                  gauss_time=30.0, contrast=0.8)), None, 7, 3, 4)
    assert a.B == 2 and a.K == 4 and a.x.shape == (4,) and a.shots == 7 and a.seed == 3 and a.first_item == 4 and a.flips is None
    assert (a.params == [[0.4, 5.0, 30.0, 2 * np.pi * 2.0, 0.0, 0.5], [0.4, 6.0, 30.0, 2 * np.pi * 2.5, 0.0, 0.5]]).all()
    echo = qs._Acquisition(np.arange(4.0), qs._curve("t2_echo", dict(t2_echo=5.0)), None, None, 3, 0)
    assert (echo.params == [[0.5, 5.0, np.inf, 2 * np.pi, 0.0, 0.5]]).all() and echo.shots == 0
    t1 = qs._Acquisition(np.zeros((3, 2)), qs._curve("t1", dict(t1=9.0, thermal_population=0.25)), [0.1, 0.2], 1, 3, 0)
    assert t1.B == 3 and t1.x.shape == (3, 2) and (t1.params == [0.75, 9.0, np.inf, 0.0, 0.0, 0.25]).all()
    assert t1.flips.shape == (3, 2) and t1.flips.flags.c_contiguous and (t1.flips == [0.1, 0.2]).all()
    assert (qs._Acquisition([1.0], qs._curve("rabi", dict(scale=1.1, offset=0.2, contrast=0.9)), None, 1, 3, 0).params
            == [[-0.45, np.inf, np.inf, 1.1, 0.2, 0.5]]).all()
    assert (qs._Acquisition([1.0], qs._curve("cz_phase_ramsey", dict(cz_phase=0.7)), None, 1, 3, 0).params
            == [[0.5, np.inf, np.inf, 1.0, 0.7, 0.5]]).all()
    assert 0 <= qs._Acquisition([1.0], qs._curve("rabi", {}), None, 1, None, 0).seed < 2 ** 64           # seed=None: drawn


@pytest.mark.parametrize("call", [
    lambda: qs.simulate_t1_batch(np.zeros((2, 2, 2)), 5.0),                              # points of rank 3
    lambda: qs.simulate_t1_batch(np.arange(3.0), np.ones((2, 2))),                       # a per-qubit argument of rank 2
    lambda: qs.simulate_t1_batch(np.arange(3.0), [5.0, 6.0], thermal_population=[0.1, 0.2, 0.3]),      # B = 2 against B = 3
    lambda: qs.simulate_t1_batch(np.zeros((3, 4)), [5.0, 6.0]),                          # rows of the points against B
    lambda: qs.simulate_t1_batch(np.arange(3.0), 5.0, flips=[0.1, 0.2, 0.3]),
    lambda: qs.simulate_t1_batch(np.arange(3.0), [5.0, 6.0], flips=np.zeros((3, 2))),
    lambda: qs.simulate_t1_batch(np.arange(3.0), 5.0, shots=-1),
    lambda: qs.simulate_t1_batch(np.arange(3.0), 5.0, shots=2 ** 32),
    lambda: qs.simulate_t1_batch(np.arange(3.0), 5.0, first_item=-1),
    lambda: qs.simulate_t1_batch(np.zeros(0), 5.0),                                      # no points
    lambda: qs.simulate_t1_batch(np.zeros(_lib.SPEC_MAX_POINTS + 1), 5.0),
    lambda: qs.simulate_and_fit_t1_batch(np.zeros(1), 5.0),                              # a fit needs two points
    lambda: qs.simulate_and_fit_t1_batch(np.zeros(_lib.FIT_MAX_POINTS + 1), 5.0),
    lambda: qs.simulate_and_fit_t1_batch(np.zeros((2, 5)), [5.0, 6.0]),                  # the resident fit shares its points
    lambda: qs.simulate_and_fit_t1_batch(np.arange(5.0), 5.0, param_guesses=(1.0, 2.0)),
    lambda: qs.simulate_and_fit_t2_batch(np.arange(5.0), 5.0, kind="hahn"),
    lambda: qs.simulate_and_fit_t2_batch(np.arange(5.0), 5.0, kind="echo", frequency_offset=1e4),
    lambda: qs.simulate_spectroscopy_results("t1", [0, 1], np.zeros((2, 3)), t1=5.0),
    lambda: qs.simulate_spectroscopy_results("t1", [0, 1], np.arange(3.0), t1=[5.0, 6.0, 7.0]),
    lambda: qs.simulate_spectroscopy_results("ramsey", [0], np.arange(3.0)),
])
def test_front_ends_refuse_bad_arguments_before_the_device(call):
    with pytest.raises(ValueError):
        call()


def test_abi_refusals_need_no_device():
    """every FBX_ERR_BAD_ARG case of include/fbx.h returns before a buffer is touched: the pointers here are NULL or host
    memory handed to the _dev form, and no device is needed to be told so"""
    lib = _lib.lib()
    x, p, out = np.zeros(4), np.ones((2, 6)), np.zeros(8)
    outs = lambda first=None: [first, None, None, None, None, None, None, None]

    def call(fn, B, K, stride, n_shots, first_item, xs=x, params=p, first_out=out):
        cast = (lambda a: None if a is None else a.ctypes.data) if fn.__name__.endswith("_dev") else _lib.dptr
        return fn(B, K, cast(xs), stride, cast(params), None, n_shots, 1, first_item, *outs(cast(first_out)))

    for fn in (lib.fbx_spec_acquire, lib.fbx_spec_acquire_dev):
        for args, word in (((-1, 4, 0, 5, 0), "B >= 0"), ((2, 0, 0, 5, 0), "K must be"), ((2, 65537, 0, 5, 0), "K must be"),
                           ((2, 4, 3, 5, 0), "x_stride"), ((2, 4, 0, -1, 0), "n_shots >= 0"), ((2, 4, 0, 2 ** 32, 0), "below 2^32"),
                           ((2, 4, 0, 5, -1), "first_item >= 0")):
            assert call(fn, *args) == _lib.FBX_ERR_BAD_ARG, (fn.__name__, args)
            assert word in lib.fbx_last_error().decode(), (args, lib.fbx_last_error())
        assert call(fn, 2, 4, 0, 5, 0, xs=None) == _lib.FBX_ERR_BAD_ARG and "NULL x / params" in lib.fbx_last_error().decode()
        assert call(fn, 2, 4, 0, 5, 0, params=None) == _lib.FBX_ERR_BAD_ARG
        assert call(fn, 2, 4, 0, 5, 0, first_out=None) == _lib.FBX_ERR_BAD_ARG
        assert "every output is NULL" in lib.fbx_last_error().decode()
        assert call(fn, 0, 4, 0, 5, 0, xs=None, params=None) == _lib.FBX_OK                       # B = 0: nothing is done


# ------------------------------------------------------------------------------------------------ against the older generator
def test_t1_curve_equals_the_model_curve_of_spectroscopy_data():
    """synthetic.spectroscopy_data draws its binomials around the fit model's curve; the mirror's exact curve for the matching
    physical T1 experiment is the same curve (another stream: the counts are not compared)"""
    x = np.linspace(0.0, 80.0, 30)
    t1 = np.array([12.0, 25.0, 40.0])
    a = qs._Acquisition(x, qs._curve("t1", dict(t1=t1)), None, None, 0, 0)
    p = synthetic.spectroscopy_probabilities(a.x, a.params)
    model = np.stack([fitting.decay_time_param_decay(x, 1.0, t, 0.0) for t in t1])
    assert np.abs(p - model).max() <= 4 * cases.U_ROUND
    # ... and with many shots the two generators' means agree with it within five binomial standard deviations
    shots = 4000
    e_old, _ = synthetic.spectroscopy_data("t1", x, shots=shots, batch=3, amplitude=1.0, decay_time=t1, offset=0.0)
    e_new = synthetic.restate_spectroscopy_counts(p, shots, 5000)[0]
    bound = 5 * np.sqrt(np.clip(4 * p * (1 - p), 1e-12, None) / shots) + 1e-12
    assert (np.abs(e_old - (1 - 2 * p)) <= bound).all() and (np.abs(e_new - (1 - 2 * p)) <= bound).all()


# ------------------------------------------------------------------------------------------------ the T1 criterion of the GPU suite
def test_t1_five_sigma_criterion_on_the_host_restatement():
    """tests/test_spectroscopy_sim_gpu.py asks every fitted T1 of 64 qubits (1000 shots, flips (0.02, 0.05)) to lie within 5 fit
    standard errors of the truth.  decay_time_param_decay has no baseline, so the readout floor f0 = 0.02 biases the fit upward:
    here the design of that test is held to a noise-free bias below 1.5 standard errors (scipy's fit of the folded curve under
    the exact binomial errors), and the same criterion is evaluated on the host restatement of the very shots, under its seed."""
    from scipy.optimize import curve_fit
    s, times, truth = cases.T1_STAT, cases.T1_STAT_TIMES, cases.t1_stat_truth()
    a = qs._Acquisition(times, qs._curve("t1", dict(t1=truth)), s["flips"], s["shots"], s["seed"], 0)
    p = synthetic.spectroscopy_probabilities(a.x, a.params, a.flips)
    model = lambda x, amplitude, decay_time: amplitude * np.exp(-x / decay_time)
    bias = []
    for b in range(s["B"]):
        popt, pcov = curve_fit(model, times, p[b], p0=(1.0, 15.0), sigma=np.sqrt(p[b] * (1 - p[b]) / s["shots"]), absolute_sigma=True)
        bias.append((popt[1] - truth[b]) / np.sqrt(pcov[1, 1]))
    e, err, _, _ = synthetic.restate_spectroscopy_counts(p, s["shots"], s["seed"])
    p1, weights = qs._bit_data(e, err)
    z = []
    for b in range(s["B"]):
        popt, pcov = curve_fit(model, times, p1[b], p0=(1.0, 15.0), sigma=1 / weights[b])
        z.append((popt[1] - truth[b]) / np.sqrt(pcov[1, 1]))
    print(f"spectroscopy T1 design: noise-free bias / stderr {min(bias):.2f} .. {max(bias):.2f}; host restatement, "
          f"(fitted - true) / stderr: largest {np.abs(z).max():.2f}, mean {np.mean(z):.2f}")
    assert 0 < min(bias) and max(bias) < 1.5
    assert np.abs(z).max() <= 5
