"""fbx_curve_fit on the device against the scipy partners of tests/fit_cases.py (golden/fit_cases.npz) and against itself."""
import ctypes

import numpy as np
import pytest

import fit_cases as fc

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture(scope="module")
def sets():
    return fc.load()


def _fit(s, **kw):
    from fbx.analysis import fitting
    return fitting.curve_fit_batch(s["model"], s["x"], s["y"], s["w"], s["guess"], vary=s["vary"], **kw)


@pytest.mark.parametrize("name", ["rb_w", "rb_u", "t1_w", "t1_u", "t2_w", "t2_u", "rabi_w", "rabi_u"])
def test_no_further_from_the_minimiser_than_minpack(gpu, sets, name):
    """The acceptance rule: in units of the tight standard error, the device's largest deviation from theta_tight over the set
    does not exceed that of scipy.optimize.leastsq (MINPACK at lmfit's default tolerances); the same for the standard errors,
    relatively.  Phase offsets enter absolutely either way (the deviation is a difference over a standard error).  No case is
    left out.  Figures measured on an MI355X are in DESIGN.md 4.9."""
    s = sets[name]
    fit = _fit(s)
    assert fit.success.all(), (name, fit.status[~fit.success])
    assert not fit.singular.any()
    dev = fc.deviation_in_sigma(fit.params, s["theta_tight"], s["cov_tight"], s["vary"])
    ref = fc.deviation_in_sigma(s["theta_minpack"], s["theta_tight"], s["cov_tight"], s["vary"])
    sdev = fc.stderr_deviation(fit.stderr, s["cov_tight"], s["vary"])
    sref = fc.stderr_deviation(s["stderr_minpack"], s["cov_tight"], s["vary"])
    print(f"FITDEV {name}: theta device {dev:.3g} sigma, minpack {ref:.3g} sigma; stderr device {sdev:.3g}, minpack {sref:.3g}; "
          f"iterations mean {fit.iters.mean():.1f} max {fit.iters.max()}")
    assert dev <= ref
    assert sdev <= sref
    np.testing.assert_allclose(fit.chisqr, s["chisqr_tight"], rtol=1e-9)


def test_degenerate_t1_model_reports_a_singular_covariance(gpu, sets):
    """All three parameters of FBX_FIT_TIME_DECAY free, as the reference fits T1: amplitude and offset enter only through
    amplitude * exp(offset / decay_time).  decay_time and that product are compared with the fit that holds the offset at 0, under
    the rule of every set: no further from the tight minimiser than MINPACK is, in tight standard errors (ref).  best_fit is the
    function A exp(-x / tau) of exactly those two quantities, so the same rule bounds it point by point, to first order:
    |d best_fit_i| <= ref (|df_i/dA| sigma_A + |df_i/dtau| sigma_tau), times (1 + ref) for the second-order term, plus 8u |f_i| for
    the two numpy evaluations.  chisqr is second order in the deviation: 1e-9 relative.  The status has FBX_FIT_SINGULAR_COVAR,
    covar is NaN and stderr is None.  Nothing is claimed about lmfit's covariance here."""
    from fbx import _lib
    from fbx.analysis import fitting
    s = sets["t1_w"]
    fit = fitting.curve_fit_batch(s["model"], s["x"], s["y"], s["w"], s["guess"], vary=0b111)
    assert fit.success.all()
    assert ((fit.status & _lib.FIT_SINGULAR_COVAR) != 0).all()
    assert np.isnan(fit.covar).all()
    one = fit[0]
    assert one.covar is None and one.params["decay_time"].stderr is None and one.success
    sig = np.sqrt(np.einsum("bii->bi", s["cov_tight"]))
    ref = fc.deviation_in_sigma(s["theta_minpack"], s["theta_tight"], s["cov_tight"], s["vary"])
    tau = fit.value("decay_time")
    product = fit.value("amplitude") * np.exp(fit.value("offset") / tau)
    dev = max(np.max(np.abs(tau - s["theta_tight"][:, 1]) / sig[:, 1]), np.max(np.abs(product - s["theta_tight"][:, 0]) / sig[:, 0]))
    print(f"FITDEV t1 all free: {dev:.3g} sigma (minpack with the offset fixed {ref:.3g})")
    assert dev <= ref
    np.testing.assert_allclose(fit.chisqr, s["chisqr_tight"], rtol=1e-9)
    want = np.stack([fc.model(s["model"], t, s["x"]) for t in s["theta_tight"]])
    J = np.stack([fc.jacobian(s["model"], t, s["x"]) for t in s["theta_tight"]])            # [B, K, P]
    allowed = ref * (1 + ref) * (np.abs(J[:, :, 0]) * sig[:, None, 0] + np.abs(J[:, :, 1]) * sig[:, None, 1]) + 8 * U * np.abs(want)
    worst = np.max(np.abs(fit.best_fit - want) / allowed)
    print(f"FITDEV t1 all free: best_fit at most {worst:.3g} of its bound")
    assert worst <= 1.0


TRUTH = {fc.BASE_DECAY: (0.7, 0.96, 0.25), fc.TIME_DECAY: (0.9, 17.0, 0.0), fc.DECAYING_COSINE: (0.45, 9.0, 0.1, 0.5, 1.02),
         fc.SHIFTED_COSINE: (-0.45, 0.2, 0.5, 1.03)}
SET_OF = {fc.BASE_DECAY: "rb_u", fc.TIME_DECAY: "t1_u", fc.DECAYING_COSINE: "t2_u", fc.SHIFTED_COSINE: "rabi_u"}


@pytest.mark.parametrize("model", sorted(TRUTH))
def test_noise_free_data_returns_the_parameters(gpu, sets, model):
    """y generated from known parameters.  At the returned point J^T r = g is what is left of the gradient; to first order (the
    residual is at rounding level, so the Gauss-Newton model is exact to that order) the scaled error D (theta - truth) is
    A^-1 gs with A the unit-diagonal scaling of J^T J and |gs_j| <= grad_norm, so
        |theta_j - truth_j| <= 2 * ||A^-1||_2 * sqrt(n) * grad_norm / ||J_j||
    (the factor 2 covers the second-order term).  grad_norm is the gradient of the residual the DEVICE evaluates; the true one
    differs by J^T eps with eps the rounding of the data (y is the model rounded to fp64: u |y_i|) and of the device's own model
    values (pow / exp / cos and two or three operations, each within an ulp or two of terms that together are at most twice
    |y_i| for these curves: 8u * 2 |y_i| is generous), so 16 u ||y||_2 is added to 2 grad_norm."""
    from fbx.analysis import fitting
    s = sets[SET_OF[model]]
    truth = np.asarray(TRUTH[model])
    x = s["x"]
    y = fc.model(model, truth, x)[None, :]
    vary = s["vary"]
    fit = fitting.curve_fit_batch(model, x, y, None, s["guess"][:1], vary=vary)
    assert fit.success[0], fit.status
    idx = fc.free_indices(model, vary)
    J = fc.jacobian(model, truth, x)[:, idx]
    cn = np.linalg.norm(J, axis=0)
    A = (J.T @ J) / np.outer(cn, cn)
    ainv = np.linalg.norm(np.linalg.inv(A), 2)
    bound = ainv * np.sqrt(len(idx)) * (2 * fit.grad_norm[0] + 16 * U * np.linalg.norm(y)) / cn
    err = np.abs(fit.params[0] - truth)[idx]
    print(f"FITDEV noise-free model {model}: error {err}, bound {bound}, grad_norm {fit.grad_norm[0]:.3g}, iters {fit.iters[0]}")
    assert (err <= bound).all()
    assert (bound < 1e-9 * np.maximum(1.0, np.abs(truth[idx]))).all()        # the bound itself says something


@pytest.mark.parametrize("name", ["rb_w", "t1_u", "t2_w", "rabi_w"])
def test_chisqr_grad_norm_and_fixed_parameters(gpu, sets, name):
    """chisqr equals a numpy evaluation at the returned parameters within the summation bound
    K u chisqr + sum 2 |r_i| w_i 8u |model_i|; grad_norm of every converged item is below the bound include/fbx.h documents and
    equals max_j |J_j^T r| / ||J_j|| recomputed in numpy; a parameter that does not vary is its guess bit for bit."""
    from fbx import _lib
    from fbx.analysis import fitting
    s = sets[name]
    fit = _fit(s)
    K = len(s["x"])
    idx = fc.free_indices(s["model"], s["vary"])
    for b in range(len(fit)):
        w = np.ones(K) if s["w"] is None else s["w"][b]
        f = fc.model(s["model"], fit.params[b], s["x"])
        r = (f - s["y"][b]) * w
        chi = float(r @ r)
        assert abs(fit.chisqr[b] - chi) <= K * U * chi + np.sum(2 * np.abs(r) * w * 8 * U * np.abs(f)), (name, b)
        assert fit.redchi[b] == pytest.approx(chi / (K - len(idx)), rel=1e-12)
        J = (fc.jacobian(s["model"], fit.params[b], s["x"]) * w[:, None])[:, idx]
        gn = np.max(np.abs(J.T @ r) / np.linalg.norm(J, axis=0))
        limit = np.sqrt((len(idx) + 1) * 1e-12 * chi) + _lib.FIT_GRAD_FLOOR * np.linalg.norm(w * s["y"][b])
        assert fit.grad_norm[b] <= limit, (name, b, fit.grad_norm[b], limit)
        assert gn <= 2 * limit
    fixed = [j for j in range(fit.params.shape[1]) if j not in idx]
    for j in fixed:
        assert (fit.params[:, j].view(np.int64) == s["guess"][:, j].view(np.int64)).all()
        assert (fit.covar[:, j, :] == 0).all() and (fit.covar[:, :, j] == 0).all()
    # hold another one: the decay / decay_time / frequency at a rounded value
    hold = {fc.BASE_DECAY: 1, fc.TIME_DECAY: 1, fc.DECAYING_COSINE: 4, fc.SHIFTED_COSINE: 3}[s["model"]]
    g = s["guess"].copy()
    g[:, hold] = s["theta_tight"][:, hold] * (1 + 1e-3)
    held = fitting.curve_fit_batch(s["model"], s["x"], s["y"], s["w"], g, vary=s["vary"] & ~(1 << hold))
    assert (held.params[:, hold].view(np.int64) == g[:, hold].view(np.int64)).all()
    assert held.success.all() and (held.chisqr >= fit.chisqr * (1 - 1e-12)).all()


def test_a_nan_item_poisons_itself_only(gpu, sets):
    from fbx import _lib
    s = sets["t2_w"]
    clean = _fit(s)
    for where in ("y", "w", "guess"):
        d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
        d[where][5, 1] = np.nan
        d["y"][70, 0] = np.inf if where == "y" else d["y"][70, 0]
        got = _fit(d)
        bad = [5, 70] if where == "y" else [5]
        keep = np.setdiff1d(np.arange(len(clean)), bad)
        for b in bad:
            assert got.status[b] == _lib.FIT_BAD_START and np.isnan(got.params[b]).all() and np.isnan(got.chisqr[b])
            assert not got.success[b] and got[b].covar is None
        for f in ("params", "covar", "chisqr", "redchi", "grad_norm"):
            assert (getattr(got, f)[keep].view(np.int64) == getattr(clean, f)[keep].view(np.int64)).all(), (where, f)
        assert (got.iters[keep] == clean.iters[keep]).all() and (got.status[keep] == clean.status[keep]).all()


def _same(a, b, rows=None):
    for f in ("params", "covar", "chisqr", "redchi", "grad_norm"):
        x, y = getattr(a, f), getattr(b, f)
        if rows is not None:
            x = x[rows]
        assert (np.ascontiguousarray(x).view(np.int64) == np.ascontiguousarray(y).view(np.int64)).all(), f
    ai, asx = (a.iters, a.status) if rows is None else (a.iters[rows], a.status[rows])
    assert (ai == b.iters).all() and (asx == b.status).all()


@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_batch_geometry_and_items_alone(gpu, sets, B):
    """Any batch size, shared and per-item x: every item -- every lane position -- equals the same item fitted alone, with
    shared and with its own x, bit for bit."""
    from fbx.analysis import fitting
    s = sets["rb_w"]
    reps = -(-B // len(s["y"]))
    y, w, g = (np.tile(s[k], (reps, 1))[:B] for k in ("y", "w", "guess"))
    shared = fitting.curve_fit_batch(s["model"], s["x"], y, w, g)
    per_item = fitting.curve_fit_batch(s["model"], np.tile(s["x"], (B, 1)), y, w, g)
    _same(shared, per_item)
    for b in range(B):
        alone = fitting.curve_fit_batch(s["model"], s["x"], y[b:b + 1], w[b:b + 1], g[b:b + 1])
        _same(shared, alone, rows=slice(b, b + 1))
        alone_x = fitting.curve_fit_batch(s["model"], s["x"][None, :].copy(), y[b:b + 1], w[b:b + 1], g[b:b + 1])
        _same(shared, alone_x, rows=slice(b, b + 1))


@pytest.mark.parametrize("name", ["t1_u", "t2_w", "rabi_u"])
def test_other_models_items_alone(gpu, sets, name):
    """The same for the other three kernels: a batch of 65 (a full wavefront and one lane of the next), every item alone."""
    s = sets[name]
    B = 65
    d = {k: (v[:B] if isinstance(v, np.ndarray) and v.ndim >= 1 and len(v) == len(s["y"]) and k != "x" else v) for k, v in s.items()}
    whole = _fit(d)
    for b in range(B):
        one = {k: (v[b:b + 1] if isinstance(v, np.ndarray) and k in ("y", "w", "guess") else v) for k, v in d.items()}
        _same(whole, _fit(one), rows=slice(b, b + 1))


def test_large_batch_and_extreme_point_counts(gpu, sets):
    """B = 10^5 (items repeat with the period of the case set, and so must the results); K = 2 and K = 256."""
    from fbx.analysis import fitting
    s = sets["rb_u"]
    n = len(s["y"])
    B = 100_000
    reps = -(-B // n)
    y, g = np.tile(s["y"], (reps, 1))[:B], np.tile(s["guess"], (reps, 1))[:B]
    big = fitting.curve_fit_batch(s["model"], s["x"], y, None, g)
    small = fitting.curve_fit_batch(s["model"], s["x"], s["y"], None, s["guess"])
    rows = np.arange(B) % n
    for f in ("params", "covar", "chisqr", "grad_norm"):
        assert (getattr(big, f).view(np.int64) == getattr(small, f)[rows].view(np.int64)).all(), f
    assert (big.iters == small.iters[rows]).all() and (big.status == small.status[rows]).all()
    # K = 256: a T1 curve on a fine grid, noise-free; K = 2: fewer points than parameters runs, stays finite and reports a
    # singular covariance
    x = np.linspace(0.0, 60.0, 256)
    truth = np.array([0.9, 20.0, 0.0])
    f256 = fitting.curve_fit_batch(fc.TIME_DECAY, x, np.tile(fc.model(fc.TIME_DECAY, truth, x), (3, 1)), None, (1.0, 15.0, 0.0), vary=0b011)
    assert f256.success.all() and np.allclose(f256.params, truth, rtol=1e-9, atol=1e-12)
    f2 = fitting.curve_fit_batch(fc.BASE_DECAY, np.array([2.0, 64.0]), np.array([[0.9, 0.6], [0.8, 0.5]]), None, (0.5, 0.95, 0.4))
    assert np.isfinite(f2.params).all() and f2.singular.all()
    alone = fitting.curve_fit_batch(fc.BASE_DECAY, np.array([2.0, 64.0]), np.array([[0.8, 0.5]]), None, (0.5, 0.95, 0.4))
    _same(f2, alone, rows=slice(1, 2))


def test_rejected_steps_keep_the_fit_finite(gpu):
    """Starts far from the minimum, where an undamped step can leave the model's domain (a negative decay under non-integer
    depths is NaN; a decay_time of 0.05 underflows most of the curve and the next step can cross 0): such trial points are
    rejected, the damping rises, and the results stay finite."""
    from fbx.analysis import fitting
    x = np.linspace(0.5, 40.5, 41)
    y = fc.model(fc.BASE_DECAY, (0.7, 0.8, 0.25), x)[None, :]
    fit = fitting.curve_fit_batch(fc.BASE_DECAY, x, y, None, (0.2, 0.05, 0.0))
    assert fit.success[0] and np.allclose(fit.params[0], (0.7, 0.8, 0.25), rtol=1e-8)
    t = np.linspace(0.0, 60.0, 31)
    y = fc.model(fc.TIME_DECAY, (0.9, 3.0, 0.0), t)[None, :]
    fit = fitting.curve_fit_batch(fc.TIME_DECAY, t, y, None, (1.0, 0.05, 0.0), vary=0b011)
    assert np.isfinite(fit.params).all() and np.isfinite(fit.chisqr).all()


def test_unsupported_and_bad_arguments_are_refused_before_device_work(gpu):
    from fbx import _lib
    lib = _lib.lib()
    a = np.zeros(257 * 5)
    args = (_lib.dptr(a), 0, _lib.dptr(a), None, _lib.dptr(a), 0b111, 1e-12, 1e-12, 10, None, None, None, None, None, None, None)
    assert lib.fbx_curve_fit(_lib.FIT_BASE_DECAY, 1, 257, *args) == _lib.FBX_ERR_UNSUPPORTED
    assert b"256" in lib.fbx_last_error()
    assert lib.fbx_curve_fit(7, 1, 10, *args) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_curve_fit(_lib.FIT_BASE_DECAY, 1, 1, *args) == _lib.FBX_ERR_BAD_ARG
    bad_vary = list(args)
    bad_vary[5] = 0b1111
    assert lib.fbx_curve_fit(_lib.FIT_BASE_DECAY, 1, 10, *bad_vary) == _lib.FBX_ERR_BAD_ARG
    with pytest.raises(_lib.FbxError):
        from fbx.analysis import fitting
        fitting.curve_fit_batch(_lib.FIT_BASE_DECAY, np.arange(257.0), np.zeros((1, 257)), None, (1.0, 0.9, 0.0))
