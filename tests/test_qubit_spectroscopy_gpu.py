"""The T1 / T2 / Rabi / CZ-Ramsey front ends against a numpy-and-scipy restatement of what the reference does before its fit."""
import numpy as np
import pytest

import fit_cases as fc

pytestmark = pytest.mark.gpu


def _restated(model, xs, e, se, guess, vary):
    p1 = (-e + 1) / 2
    w = None if se is None else fc.weights_from_errors(np.sqrt(se ** 2 / 4))
    theta, status = fc.tight(model, xs, p1, w, guess, vary)
    assert status > 0
    cov, chi = fc.covariance(model, theta, xs, p1, w, vary)
    return p1, w, theta, cov, chi


CASES = {
    "t2": (fc.DECAYING_COSINE, np.linspace(0.0, 13.0, 53), dict(amplitude=0.45, decay_time=9.0, offset=0.0, baseline=0.5, frequency=1.02),
           (.5, 10, 0.0, 0.5, 1.0)),
    "rabi": (fc.SHIFTED_COSINE, np.linspace(0.0, 2 * np.pi, 21), dict(amplitude=-0.47, offset=0.0, baseline=0.5, frequency=0.98),
             (-.5, 0, .5, 1.)),
    "cz_ramsey": (fc.SHIFTED_COSINE, np.linspace(0.0, 2 * np.pi, 21), dict(amplitude=0.46, offset=0.3, baseline=0.5, frequency=1.0),
                  (.5, 0, .5, 1.)),
}


@pytest.mark.parametrize("kind", sorted(CASES))
@pytest.mark.parametrize("weighted", [True, False])
def test_front_ends_reproduce_the_restated_reference(gpu, kind, weighted):
    from fbx import qubit_spectroscopy as qs, synthetic
    model, xs, truth, guess = CASES[kind]
    B = 6
    e, se = synthetic.spectroscopy_data(kind, xs, 500, B, seed=300, **truth)
    if weighted:
        se[0, 2] = 0.0                                           # replaced by the row's smallest non-zero error
    fit_batch = {"t2": qs.fit_t2_results_batch, "rabi": qs.fit_rabi_results_batch, "cz_ramsey": qs.fit_cz_phase_ramsey_results_batch}[kind]
    fit_one = {"t2": qs.fit_t2_results, "rabi": qs.fit_rabi_results, "cz_ramsey": qs.fit_cz_phase_ramsey_results}[kind]
    batch = fit_batch(xs, e, se if weighted else None)
    assert batch.success.all()
    for b in range(B):
        p1, w, theta, cov, chi = _restated(model, xs, e[b], se[b] if weighted else None, guess, (1 << len(guess)) - 1)
        sig = np.sqrt(np.diag(cov))
        assert (batch.y[b] == p1).all()
        if weighted:
            assert np.allclose(batch.weights[b], w, rtol=1e-15)
        assert (np.abs(batch.params[b] - theta) <= 1e-4 * sig).all()
        assert np.allclose(batch.stderr[b], sig, rtol=1e-4) and batch.chisqr[b] == pytest.approx(chi, rel=1e-9)
        one = fit_one(xs, e[b], se[b] if weighted else None)
        assert [one.params[n].value for n in batch.param_names] == batch.params[b].tolist()
        assert one.init_values == dict(zip(batch.param_names, map(float, guess)))


def test_t1_front_end(gpu):
    """All three parameters free, as the reference has it: decay_time and amplitude * exp(offset / decay_time) are those of the
    restated fit with the offset held (1e-4 of their standard errors), and there is no covariance; with the offset held through
    ``vary`` the covariance is the restated one."""
    from fbx import qubit_spectroscopy as qs, synthetic
    times = np.linspace(0.0, 60.0, 31)
    e, se = synthetic.spectroscopy_data("t1", times, 500, 4, seed=301, amplitude=0.95, decay_time=18.0, offset=0.0)
    free = qs.fit_t1_results_batch(times, e, se)
    held = qs.fit_t1_results_batch(times, e, se, vary=(True, True, False))
    assert free.success.all() and free.singular.all() and not held.singular.any()
    for b in range(4):
        p1, w, theta, cov, chi = _restated(fc.TIME_DECAY, times, e[b], se[b], (1.0, 15, 0.0), 0b011)
        sig = np.sqrt(np.diag(cov))[:2]
        assert (np.abs(held.params[b, :2] - theta[:2]) <= 1e-4 * sig).all() and held.params[b, 2] == 0.0
        assert np.allclose(held.stderr[b, :2], sig, rtol=1e-4)
        tau = free.params[b, 1]
        prod = free.params[b, 0] * np.exp(free.params[b, 2] / tau)
        assert abs(tau - theta[1]) <= 1e-4 * sig[1] and abs(prod - theta[0]) <= 1e-4 * sig[0]
    one = qs.fit_t1_results(times, e[0], se[0])
    assert one.covar is None and one.params["decay_time"].stderr is None
    assert one.params["decay_time"].value == free.params[0, 1]
    unweighted = qs.fit_t1_results(times, e[0])
    assert unweighted.weights is None and unweighted.success
