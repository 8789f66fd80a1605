"""Host side of the curve fits: result objects, JSON, argument errors, the no-device code, and the stored scipy partners."""
import json

import numpy as np
import pytest

import fit_cases as fc


def _batch():
    """A FitBatch assembled by hand (no device): two fits of base_param_decay, the second without a covariance."""
    from fbx import _lib
    from fbx.analysis import fitting
    x = np.array([1.0, 2.0, 4.0, 8.0])
    params = np.array([[0.5, 0.9, 0.25], [0.4, 0.8, 0.3]])
    y = np.stack([fitting.base_param_decay(x, *p) for p in params]) + 0.01
    covar = np.stack([np.diag([4e-4, 1e-4, 9e-4]), np.full((3, 3), np.nan)])
    status = np.array([_lib.FIT_CONVERGED_FTOL, _lib.FIT_CONVERGED_XTOL | _lib.FIT_SINGULAR_COVAR], dtype=np.int32)
    return fitting.FitBatch(_lib.FIT_BASE_DECAY, x, y, None, np.tile([1.0, 0.95, 0.0], (2, 1)), 0b011, params, covar,
                            np.array([4e-4, 4e-4]), np.array([2e-4, 2e-4]), np.array([5, 7], dtype=np.int32), status,
                            np.array([1e-9, 2e-9]))


def test_fit_result_fields():
    from fbx.analysis import fitting
    batch = _batch()
    one = batch[0]
    assert list(one.params) == ["amplitude", "decay", "baseline"]
    assert one.params["decay"].value == 0.9 and one.params["decay"].stderr == pytest.approx(1e-2)
    assert one.params["baseline"].vary is False and one.params["baseline"].stderr == 0.0
    assert one.best_values == {"amplitude": 0.5, "decay": 0.9, "baseline": 0.25}
    assert one.init_values == {"amplitude": 1.0, "decay": 0.95, "baseline": 0.0}
    assert np.array_equal(one.best_fit, fitting.base_param_decay(batch.x, 0.5, 0.9, 0.25))
    assert one.covar.shape == (3, 3) and one.chisqr == 4e-4 and one.redchi == 2e-4 and one.success
    assert one.nvarys == 2 and one.nfree == 2 and one.var_names == ["amplitude", "decay"]
    two = batch[1]
    assert two.covar is None and two.params["decay"].stderr is None and two.success
    assert batch.success.tolist() == [True, True] and batch.singular.tolist() == [False, True]
    assert np.array_equal(batch.value("decay"), [0.9, 0.8]) and batch.error("decay")[0] == pytest.approx(1e-2)


def test_fit_result_to_json_round_trip():
    from fbx.analysis import fitting
    batch = _batch()
    for one in (batch[0], batch[1]):
        d = json.loads(json.dumps(fitting.fit_result_to_json(one)))
        assert set(d) == {"chisqr", "redchi", "best_fit", "best_values", "covar", "params"}
        assert d["chisqr"] == one.chisqr and d["redchi"] == one.redchi and d["best_values"] == one.best_values
        assert d["best_fit"] == one.best_fit.tolist()
        assert (d["covar"] is None) == (one.covar is None)
        back = fitting.Parameters.loads(d["params"])
        assert back.valuesdict() == one.best_values
        assert [p.stderr for p in back.values()] == [p.stderr for p in one.params.values()]


def test_model_functions():
    from fbx.analysis import fitting
    x = np.linspace(0.0, 5.0, 11)
    for m, (name, fn, names) in fitting.MODELS.items():
        theta = np.linspace(0.3, 1.1, len(names))
        assert np.allclose(fn(x, *theta), fc.model(m, theta, x), rtol=0, atol=0) and names == fc.PARAM_NAMES[m]


def test_argument_errors_come_before_any_device_work():
    from fbx import _lib
    from fbx.analysis import fitting
    from fbx import randomized_benchmarking as rb
    x = np.arange(4.0)
    with pytest.raises(ValueError, match="Lengths of x and y arrays must be equal"):
        fitting.fit_base_param_decay(x, np.zeros(5))
    with pytest.raises(ValueError, match="Lengths of x and weights arrays must be equal"):
        fitting.fit_shifted_cosine(x, np.zeros(4), weights=np.ones(3))
    with pytest.raises(ValueError, match="param_guesses"):
        fitting.fit_decaying_cosine(x, np.zeros(4), param_guesses=(1.0, 2.0))
    with pytest.raises(ValueError, match="number of shots is necessary"):
        rb.z_obs_stats_to_survival_statistics([0.9, 0.8, 0.7], [0.01] * 3)
    with pytest.raises(ValueError, match="number of shots is necessary"):
        rb.fit_rb_results([2, 4], [[0.9, 0.8, 0.7]] * 2, [[0.01] * 3] * 2)
    lib = _lib.lib()
    a = np.zeros(257 * 5)
    tail = (_lib.dptr(a), 0b111, 1e-12, 1e-12, 10, None, None, None, None, None, None, None)
    assert lib.fbx_curve_fit(_lib.FIT_BASE_DECAY, 1, 257, _lib.dptr(a), 0, _lib.dptr(a), None, *tail) == _lib.FBX_ERR_UNSUPPORTED
    assert b"256" in lib.fbx_last_error()
    assert lib.fbx_curve_fit(9, 1, 8, _lib.dptr(a), 0, _lib.dptr(a), None, *tail) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_curve_fit(_lib.FIT_BASE_DECAY, 1, 8, _lib.dptr(a), 3, _lib.dptr(a), None, *tail) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_rb_survival(3, 1, _lib.dptr(a), _lib.dptr(a), 1, _lib.dptr(a), _lib.dptr(a)) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_rb_purity(16, 1, _lib.dptr(a), _lib.dptr(a), 1, _lib.dptr(a), _lib.dptr(a)) == _lib.FBX_ERR_UNSUPPORTED
    assert lib.fbx_fit_prepare_dev(5, 1, 4, None, None, 0, None, None, None) == _lib.FBX_ERR_BAD_ARG


def test_without_a_device_the_fit_fails_loudly():
    """No GPU: FBX_ERR_NO_DEVICE, never a host fit.  With a GPU the same call simply works."""
    import fbx
    from fbx import _lib
    from fbx.analysis import fitting
    x = np.arange(1.0, 9.0)
    y = fitting.base_param_decay(x, 0.5, 0.9, 0.25)
    if fbx.device_count() == 0:
        with pytest.raises(fbx.FbxError) as ei:
            fitting.fit_base_param_decay(x, y)
        assert ei.value.code == _lib.FBX_ERR_NO_DEVICE
    else:
        assert fitting.fit_base_param_decay(x, y).success


def test_stored_partners_agree_with_a_fresh_scipy_run():
    """golden/fit_cases.npz: the data are regenerated bit for bit from their seeds; the first cases of every set are refitted --
    theta_tight to 1e-6 of its standard errors, theta_minpack within the set's stored MINPACK deviation of the stored one (its
    stopping point is a discrete decision, so it is not asked to the last bit)."""
    stored = fc.load()
    raw = fc.raw_sets()
    assert sorted(stored) == sorted(raw)
    for name, s in raw.items():
        g = stored[name]
        assert g["model"] == s["model"] and g["vary"] == s["vary"]
        assert np.array_equal(g["y"], s["y"]) and np.array_equal(g["x"], s["x"]) and np.array_equal(g["guess"], s["guess"])
        assert (g["w"] is None) == (s["w"] is None) and (s["w"] is None or np.array_equal(g["w"], s["w"]))
        assert len(g["y"]) == fc.N_CASES
        p = fc.partners(s, cases=4)
        sl = slice(0, 4)
        assert fc.deviation_in_sigma(p["theta_tight"], g["theta_tight"][sl], g["cov_tight"][sl], s["vary"]) < 1e-6
        ref = fc.deviation_in_sigma(g["theta_minpack"], g["theta_tight"], g["cov_tight"], s["vary"])
        assert fc.deviation_in_sigma(p["theta_minpack"], g["theta_minpack"][sl], g["cov_tight"][sl], s["vary"]) <= ref
        assert 1e-7 < ref < 1e-2                       # MINPACK's stop is near the minimiser, and visibly not at it
