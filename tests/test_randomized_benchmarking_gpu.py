"""fbx_rb_survival / fbx_rb_purity against the reference's recorded results (golden/rb_cases.npz), the front ends against a
numpy-and-scipy restatement of the reference's weights-and-guess logic, and the device-resident chain against the host calls."""
import os

import numpy as np
import pytest

import fit_cases as fc

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rb_cases.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("dim", [2, 4, 8, 16, 32])
def test_survival_statistics_match_the_reference(gpu, gold, dim):
    """Plain summation: 4 dim^2 u relative to the sum of the absolute terms of each result."""
    from fbx import randomized_benchmarking as rb
    e, se, shots = gold[f"surv{dim}_e"], gold[f"surv{dim}_se"], int(gold["shots"])
    surv, var = rb.survival_statistics_batch(e, se, shots)
    _, var_ind = rb.survival_statistics_batch(e, se, None, obs_are_independent=True)
    tol = 4 * dim * dim * U
    assert (np.abs(surv - gold[f"surv{dim}_p"]) <= tol * (np.abs(e).sum(-1) + 1) / dim).all()
    ind_terms = (se ** 2).sum(-1) / dim ** 2
    assert (np.abs(var_ind - gold[f"surv{dim}_var_ind"]) <= tol * ind_terms).all()
    a = np.abs(e)
    cov_terms = (2 * a.sum(-1) + (a.sum(-1) ** 2 - (a * a).sum(-1))) / shots / dim ** 2 if dim > 2 else 0.0
    assert (np.abs(var - gold[f"surv{dim}_var"]) <= tol * (ind_terms + cov_terms)).all()
    one = rb.z_obs_stats_to_survival_statistics(list(e[3]), list(se[3]), shots)
    assert one == (surv[3], var[3])


@pytest.mark.parametrize("dim", [2, 4, 8])
def test_purity_and_its_error_match_the_reference(gpu, gold, dim):
    from fbx import randomized_benchmarking as rb
    e, se = gold[f"pur{dim}_e"], gold[f"pur{dim}_se"]
    tol = 4 * dim * dim * U
    scale = dim / (dim - 1.0)
    for renorm, kp, ke in ((True, "p", "err"), (False, "p_raw", "err_raw")):
        pur, err = rb.purity_statistics_batch(e, se, renorm=renorm)
        terms = ((e * e).sum(-1) + 1) / dim
        terms = scale * (terms + 1.0 / dim) if renorm else terms
        assert (np.abs(pur - gold[f"pur{dim}_{kp}"]) <= tol * terms).all()
        # the error is the square root of a sum of non-negative terms: relative
        want = gold[f"pur{dim}_{ke}"]
        assert (np.abs(err - want) <= tol * want).all()


def _restated_fit(depths, y, err, guess):
    """What the reference does after its statistics: zero errors replaced, no weights when all are zero, then the decay fit --
    here by scipy at the machine floor."""
    w = fc.weights_from_errors(err)
    theta, status = fc.tight(fc.BASE_DECAY, depths, y, w, guess, 0b111)
    assert status > 0
    cov, chi = fc.covariance(fc.BASE_DECAY, theta, depths, y, w, 0b111)
    return theta, cov, chi, w


def test_fit_rb_results_reproduces_the_restated_front_end(gpu):
    from fbx import randomized_benchmarking as rb, synthetic
    depths = np.repeat([2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0], 5)
    shots = 500
    e, se = synthetic.rb_data(2, depths, [0.97, 0.95, 0.99], shots, 3, seed=77)
    e[1, 0] = 1.0                                      # a sequence that always returned 00: zero variance, replaced
    se[1, 0] = 0.0
    e[2], se[2] = np.round(e[2], 1), 0.0               # every standard error zero ...
    batch = rb.fit_rb_results_batch(depths, e, se, shots)
    assert batch.has_weights.tolist() == [True, True, True]      # ... but the covariance term remains (where it is negative the
                                                                 # error is NaN and is replaced like a zero, as in the reference)
    for b in range(3):
        y, var = fc.survival_numpy(e[b], se[b], shots)
        guess = (y[0] - y[-1], 0.95, y[-1])
        with np.errstate(invalid="ignore"):
            theta, cov, chi, w = _restated_fit(depths, y, np.sqrt(var), guess)
        assert np.allclose(batch.y[b], y, rtol=0, atol=1e-15)
        assert np.allclose(batch.weights[b], w, rtol=1e-13)
        assert np.allclose(batch.init_values[b], guess, rtol=0, atol=1e-15)
        sig = np.sqrt(np.diag(cov))
        assert (np.abs(batch.params[b] - theta) <= 1e-4 * sig).all()
        assert np.allclose(batch.stderr[b], sig, rtol=1e-4)
        single = rb.fit_rb_results(depths, e[b], se[b], shots)
        assert single.params["decay"].value == batch.params[b, 1] and single.params["decay"].stderr == batch.stderr[b, 1]
        assert single.chisqr == batch.chisqr[b] and single.success
    # one qubit: no covariance term, so all-zero errors mean no weights; a zero among non-zero errors is replaced
    e1, se1 = synthetic.rb_data(1, depths, 0.96, shots, 2, seed=78)
    se1[0] = 0.0
    se1[1, :5] = 0.0
    b1 = rb.fit_rb_results_batch(depths, e1, se1)
    assert b1.has_weights.tolist() == [False, True]
    assert (b1.weights[0] == 1.0).all()
    for b in range(2):
        y, var = fc.survival_numpy(e1[b], se1[b], shots)
        theta, cov, chi, w = _restated_fit(depths, y, np.sqrt(var), (y[0] - y[-1], 0.95, y[-1]))
        assert (np.abs(b1.params[b] - theta) <= 1e-4 * np.sqrt(np.diag(cov))).all()
        if w is not None:
            assert np.allclose(b1.weights[b], w, rtol=1e-13)
    with pytest.raises(ValueError, match="number of shots is necessary"):
        rb.fit_rb_results(depths, e[0], se[0])
    custom = rb.fit_rb_results(depths, e[0], se[0], shots, param_guesses=(0.7, 0.9, 0.25))
    assert custom.init_values == {"amplitude": 0.7, "decay": 0.9, "baseline": 0.25}
    assert abs(custom.params["decay"].value - batch.params[0, 1]) <= 1e-4 * batch.stderr[0, 1]


def test_fit_unitarity_results_reproduces_the_restated_front_end(gpu):
    from fbx import randomized_benchmarking as rb
    rng = np.random.default_rng(5)
    depths = np.repeat([2.0, 4.0, 8.0, 16.0, 32.0], 4)
    shots, dim = 2000, 2
    B = 3
    r = 0.95 * 0.97 ** depths                                   # Bloch-vector length after a sequence
    dirs = rng.normal(size=(B, len(depths), 3))
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    exact = r[None, :, None] * dirs
    e = 2 * rng.binomial(shots, (1 + exact) / 2) / shots - 1
    se = np.sqrt((1 - e * e) / shots)
    se[1, 3] = 0.0
    se[2] = 0.0
    batch = rb.fit_unitarity_results_batch(depths, e, se)
    assert batch.has_weights.tolist() == [True, True, False]
    for b in range(B):
        ex = np.concatenate([e[b], np.ones((len(depths), 1))], axis=1)
        va = np.concatenate([se[b], np.zeros((len(depths), 1))], axis=1) ** 2
        pur, err = rb.estimate_purity(dim, ex), rb.estimate_purity_err(dim, ex, va)
        theta, cov, chi, w = _restated_fit(depths, pur, err, (pur[0], 0.95, 0.0))
        assert np.allclose(batch.y[b], pur, rtol=0, atol=1e-14)
        assert np.allclose(batch.init_values[b], (pur[0], 0.95, 0.0), rtol=0, atol=1e-14)
        assert (np.abs(batch.params[b] - theta) <= 1e-4 * np.sqrt(np.diag(cov))).all()
        single = rb.fit_unitarity_results(depths, e[b], se[b])
        assert single.params["decay"].value == batch.params[b, 1]
    u = batch.value("decay")
    assert np.all((u > 0.85) & (u < 1.02))


def test_resident_chain_equals_host_pointer_calls(gpu):
    """fbx_rb_survival_dev -> fbx_fit_prepare_dev -> fbx_curve_fit_dev without leaving the device, against fbx_rb_survival and
    fbx_curve_fit through host pointers (weights and guess in between through the same prepare kernel): bit for bit."""
    from fbx import _lib, randomized_benchmarking as rb, synthetic
    from fbx.analysis import fitting
    depths = np.repeat([2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0], 5)
    B, K, shots = 130, len(depths), 500
    e, se = synthetic.rb_data(2, depths, np.linspace(0.9, 0.99, B), shots, B, seed=91)
    chain = rb.fit_rb_results_batch(depths, e, se, shots)
    surv, var = rb.survival_statistics_batch(e, se, shots)
    DB = _lib.DeviceBuffer
    d_v, d_e, d_w, d_g = DB.from_array(surv), DB.from_array(var), DB(8 * B * K), DB(8 * B * 3)
    _lib.check(_lib.lib().fbx_fit_prepare_dev(_lib.FIT_PREPARE_RB, B, K, d_v.ptr, d_e.ptr, 1, d_w.ptr, d_g.ptr, None))
    _lib.synchronize()
    w, g = d_w.to_array(np.float64, (B, K)), d_g.to_array(np.float64, (B, 3))
    assert (w.view(np.int64) == (1.0 / np.sqrt(var)).view(np.int64)).all()
    host = fitting.curve_fit_batch(_lib.FIT_BASE_DECAY, depths, surv, w, g)
    for f in ("params", "covar", "chisqr", "redchi", "grad_norm", "y", "weights", "init_values"):
        assert (getattr(chain, f).view(np.int64) == getattr(host, f).view(np.int64)).all(), f
    assert (chain.iters == host.iters).all() and (chain.status == host.status).all()
    gate_error = rb.rb_decay_to_gate_error(chain.value("decay"), 4)
    assert np.all((gate_error > 0) & (gate_error < 0.1))


def test_dimension_limits(gpu):
    from fbx import _lib
    lib = _lib.lib()
    a = np.zeros(4096)
    assert lib.fbx_rb_survival(64, 1, _lib.dptr(a), _lib.dptr(a), 10, _lib.dptr(a), _lib.dptr(a)) == _lib.FBX_ERR_UNSUPPORTED
    assert lib.fbx_rb_survival(3, 1, _lib.dptr(a), _lib.dptr(a), 10, _lib.dptr(a), _lib.dptr(a)) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_rb_purity(16, 1, _lib.dptr(a), _lib.dptr(a), 1, _lib.dptr(a), _lib.dptr(a)) == _lib.FBX_ERR_UNSUPPORTED
