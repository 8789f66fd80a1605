"""Case sets and partners for the curve-fit tests (tests/test_curve_fit_*.py).

The weighted least-squares minimiser is a mathematical object, so the partner is scipy, twice per case:

* ``theta_tight`` -- ``scipy.optimize.least_squares(method="lm")`` with the analytic Jacobian and ftol = xtol = gtol at the machine
  floor, from the same guess: the minimiser as well as fp64 gives it.  Its covariance inv(J^T J) * redchi is stored with it.
* ``theta_minpack`` -- ``scipy.optimize.leastsq``, the MINPACK routine behind lmfit's default method, with a finite-difference
  Jacobian, ftol = xtol = 1.5e-8 and maxfev = 2000 (P + 1): lmfit's defaults as far as they can be known without the package (it is
  not installed where these fixtures are made, and the reference's own fit functions cannot run there).  This is what a user of
  the reference gets.

Acceptance rule: measured against ``theta_tight`` in units of the tight standard error of each parameter, the device's largest
deviation over a case set must not exceed that of ``theta_minpack`` over the same set (``deviation_in_sigma``); the same for the
standard errors, relatively (``stderr_deviation``).

Data: binomially sampled at 500 shots through ``fbx.synthetic``, fitted from the reference's default guesses.  RB: depths 2..128,
five sequences per depth (35 points), one and two qubits; T1: 31 times; T2: 53 times at one cycle per unit; Rabi: 21 angles over
one period.  One set per model with weights and one without.  Nothing is excluded: every case of every set converges in both
partners (``make`` asserts it).

``python tests/fit_cases.py`` writes tests/golden/fit_cases.npz.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fit_cases.npz")
N_CASES = 96
SHOTS = 500

BASE_DECAY, TIME_DECAY, DECAYING_COSINE, SHIFTED_COSINE = range(4)
PARAM_NAMES = {BASE_DECAY: ("amplitude", "decay", "baseline"), TIME_DECAY: ("amplitude", "decay_time", "offset"),
               DECAYING_COSINE: ("amplitude", "decay_time", "offset", "baseline", "frequency"),
               SHIFTED_COSINE: ("amplitude", "offset", "baseline", "frequency")}
# the parameters that are phase offsets: compared absolutely (they sit at 0)
PHASES = {BASE_DECAY: (), TIME_DECAY: (), DECAYING_COSINE: (2,), SHIFTED_COSINE: (1,)}


def model(m, t, x):
    if m == BASE_DECAY:
        return t[2] + t[0] * t[1] ** x
    if m == TIME_DECAY:
        return t[0] * np.exp(-(x - t[2]) / t[1])
    if m == DECAYING_COSINE:
        return t[0] * np.exp(-x / t[1]) * np.cos(2 * np.pi * t[4] * x + t[2]) + t[3]
    return t[0] * np.cos(t[3] * x + t[1]) + t[2]


def jacobian(m, t, x):
    """[K, P] derivatives of the model."""
    one = np.ones_like(x)
    if m == BASE_DECAY:
        p = t[1] ** x
        return np.stack([p, t[0] * x * t[1] ** (x - 1), one], axis=1)
    if m == TIME_DECAY:
        u = (x - t[2]) / t[1]
        f = t[0] * np.exp(-u)
        return np.stack([np.exp(-u), f * u / t[1], f / t[1]], axis=1)
    if m == DECAYING_COSINE:
        e = np.exp(-x / t[1])
        ph = 2 * np.pi * t[4] * x + t[2]
        c, s = np.cos(ph), np.sin(ph)
        return np.stack([e * c, t[0] * e * c * x / t[1] ** 2, -t[0] * e * s, one, -t[0] * e * s * 2 * np.pi * x], axis=1)
    ph = t[3] * x + t[1]
    return np.stack([np.cos(ph), -t[0] * np.sin(ph), one, -t[0] * np.sin(ph) * x], axis=1)


def free_indices(m, vary):
    return [j for j in range(len(PARAM_NAMES[m])) if (vary >> j) & 1]


def _embed(m, vary, guess):
    idx = free_indices(m, vary)

    def full(free):
        t = np.array(guess, dtype=np.float64)
        t[idx] = free
        return t
    return idx, full


def covariance(m, theta, x, y, w, vary):
    """inv(J^T J) * redchi over the free parameters, embedded in [P, P] with zero rows / columns for the fixed ones
    (lmfit's scale_covar=True); chisqr with it."""
    idx = free_indices(m, vary)
    ww = 1.0 if w is None else w
    J = (jacobian(m, theta, x) * np.reshape(ww, (-1, 1)))[:, idx]
    r = (model(m, theta, x) - y) * ww
    chisqr = float(r @ r)
    redchi = chisqr / max(1, len(x) - len(idx))
    P = len(theta)
    cov = np.zeros((P, P))
    cov[np.ix_(idx, idx)] = np.linalg.inv(J.T @ J) * redchi
    return cov, chisqr


def tight(m, x, y, w, guess, vary):
    from scipy.optimize import least_squares
    idx, full = _embed(m, vary, guess)
    ww = 1.0 if w is None else w
    eps = np.finfo(np.float64).eps
    res = least_squares(lambda f: (model(m, full(f), x) - y) * ww, np.asarray(guess, dtype=np.float64)[idx],
                        jac=lambda f: (jacobian(m, full(f), x) * np.reshape(ww, (-1, 1)))[:, idx], method="lm",
                        ftol=eps, xtol=eps, gtol=eps, max_nfev=20000)
    return full(res.x), res.status


def minpack(m, x, y, w, guess, vary):
    from scipy.optimize import leastsq
    idx, full = _embed(m, vary, guess)
    ww = 1.0 if w is None else w
    P = len(guess)
    f, cov_x, info, msg, ier = leastsq(lambda f: (model(m, full(f), x) - y) * ww, np.asarray(guess, dtype=np.float64)[idx],
                                       ftol=1.5e-8, xtol=1.5e-8, maxfev=2000 * (P + 1), full_output=True)
    theta = full(f)
    r = (model(m, theta, x) - y) * ww
    redchi = float(r @ r) / max(1, len(x) - len(idx))
    stderr = np.zeros(P)
    stderr[idx] = np.sqrt(np.diag(cov_x) * redchi) if cov_x is not None else np.nan
    return theta, stderr, ier


def weights_from_errors(err):
    """The reference's rule: 1 / err with zeros replaced by the smallest non-zero error; None when all are zero."""
    err = np.asarray(err, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        pos = err > 0                                    # False for the NaN of a negative variance, as in the reference
    if not pos.any():
        return None
    return 1.0 / np.where(pos, err, err[pos].min())


def survival_numpy(e, se, shots):
    """z_obs_stats_to_survival_statistics restated in numpy for [.., dim - 1] rows."""
    e, se = np.asarray(e, dtype=np.float64), np.asarray(se, dtype=np.float64)
    dim = e.shape[-1] + 1
    surv = (e.sum(-1) + 1) / dim
    var = (se ** 2).sum(-1) / dim ** 2
    if dim > 2:
        tot = e.sum(-1)
        cross = (e * (tot[..., None] - e)).sum(-1)
        var = var + (2 * tot - cross) / shots / dim ** 2
    return surv, var


def raw_sets():
    """name -> dict(model, x [K], y [B, K], w [B, K] or None, guess [B, P], vary): the data, without the partners."""
    import fbx.synthetic as syn
    rng = np.random.default_rng(20240)
    sets = {}
    depths = np.repeat([2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0], 5)
    half = N_CASES // 2
    ys, vs = [], []
    for nq, first in ((1, 0), (2, half)):
        e, se = syn.rb_data(nq, depths, rng.uniform(0.9, 0.99, half), SHOTS, half, seed=4100 + nq)
        s, v = survival_numpy(e, se, SHOTS)
        ys.append(s); vs.append(v)
    y, err = np.concatenate(ys), np.sqrt(np.concatenate(vs))
    guess = np.stack([y[:, 0] - y[:, -1], np.full(len(y), 0.95), y[:, -1]], axis=1)
    w = np.stack([weights_from_errors(r) for r in err])
    sets["rb_w"] = dict(model=BASE_DECAY, x=depths, y=y, w=w, guess=guess, vary=0b111)
    sets["rb_u"] = dict(model=BASE_DECAY, x=depths, y=y, w=None, guess=guess, vary=0b111)

    def spectro(kind, xs, seed, **par):
        e, se = syn.spectroscopy_data(kind, xs, SHOTS, N_CASES, seed=seed, **par)
        p1, er = (1 - e) / 2, np.sqrt(se ** 2 / 4)
        return p1, np.stack([weights_from_errors(r) for r in er])

    times = np.linspace(0.0, 60.0, 31)
    p1, w = spectro("t1", times, 5100, amplitude=rng.uniform(0.85, 1.0, N_CASES), decay_time=rng.uniform(10.0, 30.0, N_CASES), offset=0.0)
    g = np.tile([1.0, 15.0, 0.0], (N_CASES, 1))
    sets["t1_w"] = dict(model=TIME_DECAY, x=times, y=p1, w=w, guess=g, vary=0b011)
    sets["t1_u"] = dict(model=TIME_DECAY, x=times, y=p1, w=None, guess=g, vary=0b011)
    t2 = np.linspace(0.0, 13.0, 53)
    p1, w = spectro("t2", t2, 5200, amplitude=rng.uniform(0.4, 0.5, N_CASES), decay_time=rng.uniform(6.0, 16.0, N_CASES), offset=0.0,
                    baseline=0.5, frequency=rng.uniform(0.97, 1.03, N_CASES))
    g = np.tile([0.5, 10.0, 0.0, 0.5, 1.0], (N_CASES, 1))
    sets["t2_w"] = dict(model=DECAYING_COSINE, x=t2, y=p1, w=w, guess=g, vary=0b11111)
    sets["t2_u"] = dict(model=DECAYING_COSINE, x=t2, y=p1, w=None, guess=g, vary=0b11111)
    ang = np.linspace(0.0, 2 * np.pi, 21)
    p1, w = spectro("rabi", ang, 5300, amplitude=-rng.uniform(0.4, 0.5, N_CASES), offset=0.0, baseline=0.5,
                    frequency=rng.uniform(0.95, 1.05, N_CASES))
    g = np.tile([-0.5, 0.0, 0.5, 1.0], (N_CASES, 1))
    sets["rabi_w"] = dict(model=SHIFTED_COSINE, x=ang, y=p1, w=w, guess=g, vary=0b1111)
    sets["rabi_u"] = dict(model=SHIFTED_COSINE, x=ang, y=p1, w=None, guess=g, vary=0b1111)
    return sets


def partners(s, cases=None):
    """theta_tight [B, P], cov_tight [B, P, P], chisqr_tight [B], theta_minpack [B, P], stderr_minpack [B, P] of a raw set."""
    B = len(s["y"]) if cases is None else cases
    out = {k: [] for k in ("theta_tight", "cov_tight", "chisqr_tight", "theta_minpack", "stderr_minpack")}
    for b in range(B):
        w = None if s["w"] is None else s["w"][b]
        tt, st = tight(s["model"], s["x"], s["y"][b], w, s["guess"][b], s["vary"])
        assert st > 0, ("tight fit did not converge", b, st)
        cov, chi = covariance(s["model"], tt, s["x"], s["y"][b], w, s["vary"])
        tm, sm, ier = minpack(s["model"], s["x"], s["y"][b], w, s["guess"][b], s["vary"])
        assert ier in (1, 2, 3, 4), ("leastsq did not converge", b, ier)
        for k, v in zip(out, (tt, cov, chi, tm, sm)):
            out[k].append(v)
    return {k: np.asarray(v) for k, v in out.items()}


def deviation_in_sigma(theta, theta_tight, cov_tight, vary):
    """max over items and free parameters of |theta - theta_tight| / tight standard error."""
    sig = np.sqrt(np.einsum("bii->bi", cov_tight))
    free = [j for j in range(theta.shape[1]) if (vary >> j) & 1]
    return float(np.max(np.abs(theta - theta_tight)[:, free] / sig[:, free]))


def stderr_deviation(stderr, cov_tight, vary):
    """max over items and free parameters of |stderr - tight stderr| / tight stderr."""
    sig = np.sqrt(np.einsum("bii->bi", cov_tight))
    free = [j for j in range(stderr.shape[1]) if (vary >> j) & 1]
    return float(np.max(np.abs(stderr - sig)[:, free] / sig[:, free]))


def load():
    """name -> the raw set plus its stored partners."""
    z = np.load(GOLDEN)
    names = sorted({k.split("/")[0] for k in z.files})
    out = {}
    for n in names:
        d = {k.split("/")[1]: z[k] for k in z.files if k.startswith(n + "/")}
        d["model"], d["vary"] = int(d["model"]), int(d["vary"])
        d["w"] = d["w"] if d["w"].ndim == 2 else None
        out[n] = d
    return out


def make():
    out = {}
    for name, s in raw_sets().items():
        p = partners(s)
        for k, v in {**s, **p}.items():
            out[f"{name}/{k}"] = np.asarray(np.nan if v is None else v)
        print(name, "minpack: max deviation %.3g sigma, stderr %.3g relative" % (
            deviation_in_sigma(p["theta_minpack"], p["theta_tight"], p["cov_tight"], s["vary"]),
            stderr_deviation(p["stderr_minpack"], p["cov_tight"], s["vary"])), flush=True)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "forest-benchmarking_amd"))
    make()
