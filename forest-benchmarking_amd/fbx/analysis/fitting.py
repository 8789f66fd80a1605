"""The reference's curve fits (forest/benchmarking/analysis/fitting.py) on the device.

Same names and signatures: the four model functions, ``fit_base_param_decay``, ``fit_decay_time_param_decay``,
``fit_decaying_cosine``, ``fit_shifted_cosine`` and ``fit_result_to_json``; each fit also has a ``*_batch`` form that takes
``y[B, K]`` (and ``weights[B, K]``, ``param_guesses[B, P]`` or one tuple) and runs the B fits in one launch of
``fbx_curve_fit`` -- a Levenberg-Marquardt iteration per GPU lane (include/fbx.h).  The reference fits through lmfit, which is
not a dependency here: the single-item forms return a small ``FitResult`` with the fields users of lmfit's ``ModelResult``
read (``params[name].value`` / ``.stderr``, ``best_values``, ``best_fit``, ``init_values``, ``covar``, ``chisqr``, ``redchi``,
``success``).  Plotting (``plot_figure_for_fit``) needs lmfit's own result object and is not restated.

The tolerances default to 1e-12, tighter than lmfit's 1.5e-8: an iteration costs little here, and the fit then sits closer to
the minimiser than MINPACK's default stop does.
"""
import json

import numpy as np
from numpy import pi

from .. import _lib

DEFAULT_FTOL = 1e-12
DEFAULT_XTOL = 1e-12
DEFAULT_MAX_ITERS = 200


def _check_data(x, y, weights):
    if not len(x) == len(y):
        raise ValueError("Lengths of x and y arrays must be equal.")
    if weights is not None and not len(x) == len(weights):
        raise ValueError("Lengths of x and weights arrays must be equal if weights is not None.")


def base_param_decay(x, amplitude: float, decay: float, baseline: float):
    """``baseline + amplitude * decay**x`` (fitting.py:16-27)."""
    return np.asarray(baseline + amplitude * decay ** x)


def decay_time_param_decay(x, amplitude: float, decay_time: float, offset: float = 0.0):
    """``amplitude * exp(-(x - offset) / decay_time)`` (fitting.py:48-59)."""
    return np.asarray(amplitude * np.exp(-1 * (x - offset) / decay_time))


def decaying_cosine(x, amplitude: float, decay_time: float, offset: float, baseline: float, frequency: float):
    """``amplitude * exp(-x / decay_time) * cos(2 pi frequency x + offset) + baseline`` (fitting.py:81-96)."""
    return amplitude * np.exp(-1 * x / decay_time) * np.cos(2 * pi * frequency * x + offset) + baseline


def shifted_cosine(x, amplitude: float, offset: float, baseline: float, frequency: float):
    """``amplitude * cos(frequency x + offset) + baseline`` (fitting.py:118-130)."""
    return amplitude * np.cos(frequency * x + offset) + baseline


# model id (include/fbx.h) -> (name, function, parameter names in the reference's order)
MODELS = {
    _lib.FIT_BASE_DECAY: ("base_param_decay", base_param_decay, ("amplitude", "decay", "baseline")),
    _lib.FIT_TIME_DECAY: ("decay_time_param_decay", decay_time_param_decay, ("amplitude", "decay_time", "offset")),
    _lib.FIT_DECAYING_COSINE: ("decaying_cosine", decaying_cosine,
                               ("amplitude", "decay_time", "offset", "baseline", "frequency")),
    _lib.FIT_SHIFTED_COSINE: ("shifted_cosine", shifted_cosine, ("amplitude", "offset", "baseline", "frequency")),
}


class Parameter:
    """One fitted parameter: ``value``, ``stderr`` (None when the fit has no covariance), ``vary``, ``init_value``."""

    def __init__(self, name, value, stderr=None, vary=True, init_value=None):
        self.name, self.value, self.stderr, self.vary, self.init_value = name, value, stderr, vary, init_value

    def __repr__(self):
        return f"<Parameter '{self.name}', value={self.value} +/- {self.stderr}, vary={self.vary}>"


class Parameters(dict):
    """name -> Parameter, in the model's order; ``dumps`` / ``loads`` round-trip through a JSON string."""

    def dumps(self):
        return json.dumps([{"name": p.name, "value": p.value, "stderr": p.stderr, "vary": p.vary, "init_value": p.init_value}
                           for p in self.values()])

    @classmethod
    def loads(cls, text):
        out = cls()
        for d in json.loads(text):
            out[d["name"]] = Parameter(d["name"], d["value"], d["stderr"], d["vary"], d["init_value"])
        return out

    def valuesdict(self):
        return {k: p.value for k, p in self.items()}


class FitResult:
    """What a user of the reference reads from lmfit's ModelResult, for one fit."""

    def __init__(self, model, params, best_fit, covar, chisqr, redchi, success, status, iters, grad_norm, data, x, weights):
        self.model_name = MODELS[model][0]
        self.model_id = model
        self.params = params
        self.best_values = params.valuesdict()
        self.init_values = {k: p.init_value for k, p in params.items()}
        self.best_fit = best_fit
        self.covar = covar
        self.chisqr, self.redchi = chisqr, redchi
        self.success = success
        self.status, self.iters, self.grad_norm = status, iters, grad_norm
        self.data, self.x, self.weights = data, x, weights
        self.ndata = len(data)
        self.nvarys = sum(1 for p in params.values() if p.vary)
        self.nfree = self.ndata - self.nvarys
        self.var_names = [k for k, p in params.items() if p.vary]

    def eval(self, x=None):
        return MODELS[self.model_id][1](self.x if x is None else np.asarray(x), **self.best_values)


class FitBatch:
    """B fits of one model: ``params[B, P]``, ``stderr[B, P]`` (NaN without a covariance), ``covar[B, P, P]``, ``chisqr[B]``,
    ``redchi[B]``, ``iters[B]``, ``status[B]`` (FBX_FIT_* of include/fbx.h), ``grad_norm[B]``, ``success[B]``,
    ``best_fit[B, K]``, ``init_values[B, P]``, ``param_names``; ``batch[b]`` is item b as a FitResult and ``batch.value(name)``
    the column of one parameter."""

    def __init__(self, model, x, y, weights, guesses, vary, params, covar, chisqr, redchi, iters, status, grad_norm):
        self.model = model
        self.param_names = MODELS[model][2]
        self.x, self.y, self.weights, self.init_values, self.vary = x, y, weights, guesses, vary
        self.params, self.covar, self.chisqr, self.redchi = params, covar, chisqr, redchi
        self.iters, self.status, self.grad_norm = iters, status, grad_norm
        self.singular = (status & _lib.FIT_SINGULAR_COVAR) != 0
        reason = status & 0xF
        self.success = (reason == _lib.FIT_CONVERGED_FTOL) | (reason == _lib.FIT_CONVERGED_XTOL)
        with np.errstate(invalid="ignore"):
            self.stderr = np.sqrt(np.einsum("bii->bi", covar))
        xs = x if x.ndim == 2 else x[None, :]
        with np.errstate(all="ignore"):
            self.best_fit = np.asarray(MODELS[model][1](xs, *[params[:, j:j + 1] for j in range(params.shape[1])]))

    def __len__(self):
        return len(self.chisqr)

    def value(self, name):
        return self.params[:, self.param_names.index(name)]

    def error(self, name):
        return self.stderr[:, self.param_names.index(name)]

    def __getitem__(self, b):
        has_cov = not self.singular[b] and (self.status[b] & 0xF) != _lib.FIT_BAD_START
        pars = Parameters()
        for j, name in enumerate(self.param_names):
            free = bool((self.vary >> j) & 1)
            pars[name] = Parameter(name, float(self.params[b, j]), (float(self.stderr[b, j]) if free else 0.0) if has_cov else None,
                                   free, float(self.init_values[b, j]))
        return FitResult(self.model, pars, self.best_fit[b], self.covar[b].copy() if has_cov else None, float(self.chisqr[b]),
                         float(self.redchi[b]), bool(self.success[b]), int(self.status[b]), int(self.iters[b]),
                         float(self.grad_norm[b]), self.y[b], self.x[b] if self.x.ndim == 2 else self.x,
                         None if self.weights is None else self.weights[b])


def _vary_mask(model, vary):
    P = len(MODELS[model][2])
    if vary is None:
        return (1 << P) - 1
    if isinstance(vary, (int, np.integer)):
        return int(vary)
    names = MODELS[model][2]
    if isinstance(vary, dict):
        vary = [vary.get(n, True) for n in names]
    if len(vary) != P:
        raise ValueError(f"vary needs one entry per parameter {names}")
    return sum(1 << j for j, v in enumerate(vary) if v)


def _guess_array(model, param_guesses, B):
    P = len(MODELS[model][2])
    g = np.asarray(param_guesses, dtype=np.float64)
    if g.shape == (P,):
        g = np.broadcast_to(g, (B, P))
    if g.shape != (B, P):
        raise ValueError(f"param_guesses must have {P} entries (or shape [{B}, {P}]) for {MODELS[model][0]}")
    return np.ascontiguousarray(g)


def curve_fit_batch(model: int, x, y, weights=None, param_guesses=None, vary=None, ftol: float = DEFAULT_FTOL,
                    xtol: float = DEFAULT_XTOL, max_iters: int = DEFAULT_MAX_ITERS) -> FitBatch:
    """B fits of ``model`` (an FBX_FIT_* id) in one call of fbx_curve_fit: ``x`` [K] (shared) or [B, K], ``y`` [B, K],
    ``weights`` None or [B, K], ``param_guesses`` one tuple or [B, P]; ``vary`` None (all), a bit mask, a sequence of bools or a
    ``{name: bool}`` dict -- a parameter that does not vary keeps its guess."""
    if model not in MODELS:
        raise ValueError(f"unknown model id {model}")
    y = np.ascontiguousarray(y, dtype=np.float64)
    if y.ndim != 2:
        raise ValueError("y must be [B, K]")
    B, K = y.shape
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.shape not in ((K,), (B, K)):
        raise ValueError("Lengths of x and y arrays must be equal.")
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.shape != (B, K):
            raise ValueError("Lengths of x and weights arrays must be equal if weights is not None.")
    guesses = _guess_array(model, param_guesses, B)
    mask = _vary_mask(model, vary)
    P = guesses.shape[1]
    params, covar = np.empty((B, P)), np.empty((B, P, P))
    chisqr, redchi, gnorm = np.empty(B), np.empty(B), np.empty(B)
    iters, status = np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
    _lib.check(_lib.lib().fbx_curve_fit(
        model, B, K, _lib.dptr(x), K if x.ndim == 2 else 0, _lib.dptr(y), _lib.dptr(weights), _lib.dptr(guesses), mask,
        float(ftol), float(xtol), int(max_iters), _lib.dptr(params), _lib.dptr(covar), _lib.dptr(chisqr), _lib.dptr(redchi),
        _lib.iptr(iters), _lib.iptr(status), _lib.dptr(gnorm)))
    return FitBatch(model, x, y, weights, guesses, mask, params, covar, chisqr, redchi, iters, status, gnorm)


def curve_fit_resident(model: int, x, d_y, d_weights, d_guess, B: int, K: int, vary=None, ftol: float = DEFAULT_FTOL,
                       xtol: float = DEFAULT_XTOL, max_iters: int = DEFAULT_MAX_ITERS) -> FitBatch:
    """The same for data that already sit in device memory (``_lib.DeviceBuffer`` of y[B, K], weights[B, K] or None and
    guess[B, P], which stay the caller's; ``x`` [K] on the host): fbx_curve_fit_dev, then one copy of every result back."""
    mask = _vary_mask(model, vary)
    P = len(MODELS[model][2])
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.shape != (K,):
        raise ValueError("Lengths of x and y arrays must be equal.")
    with _lib.DeviceScope() as dev:
        d_x = dev.upload(x)
        outs = [dev.alloc(n) for n in (8 * B * P, 8 * B * P * P, 8 * B, 8 * B, 4 * B, 4 * B, 8 * B)]
        _lib.check(_lib.lib().fbx_curve_fit_dev(
            model, B, K, d_x.ptr, 0, d_y.ptr, _lib.devptr(d_weights), d_guess.ptr, mask, float(ftol),
            float(xtol), int(max_iters), *[o.ptr for o in outs]))
        _lib.synchronize()
        params, covar = outs[0].to_array(np.float64, (B, P)), outs[1].to_array(np.float64, (B, P, P))
        chisqr, redchi = outs[2].to_array(np.float64, (B,)), outs[3].to_array(np.float64, (B,))
        iters, status = outs[4].to_array(np.int32, (B,)), outs[5].to_array(np.int32, (B,))
        gnorm = outs[6].to_array(np.float64, (B,))
        y = d_y.to_array(np.float64, (B, K))
        w = None if d_weights is None else d_weights.to_array(np.float64, (B, K))
        g = d_guess.to_array(np.float64, (B, P))
    return FitBatch(model, x, y, w, g, mask, params, covar, chisqr, redchi, iters, status, gnorm)


def _single(model, x, y, weights, param_guesses, **kw):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    _check_data(x, y, weights)
    w = None if weights is None else np.asarray(weights, dtype=np.float64)[None, :]
    return curve_fit_batch(model, x, y[None, :], w, param_guesses, **kw)[0]


def fit_base_param_decay(x, y, weights=None, param_guesses: tuple = (1., .9, 0.), **kw) -> FitResult:
    """Fit ``base_param_decay`` (fitting.py:30-45); ``kw``: vary, ftol, xtol, max_iters."""
    return _single(_lib.FIT_BASE_DECAY, x, y, weights, param_guesses, **kw)


def fit_base_param_decay_batch(x, y, weights=None, param_guesses=(1., .9, 0.), **kw) -> FitBatch:
    return curve_fit_batch(_lib.FIT_BASE_DECAY, x, y, weights, param_guesses, **kw)


def fit_decay_time_param_decay(x, y, weights=None, param_guesses: tuple = (1., 10, 0), **kw) -> FitResult:
    """Fit ``decay_time_param_decay`` (fitting.py:62-78).  ``amplitude`` and ``offset`` enter only through
    amplitude * exp(offset / decay_time): with all three free, as the reference has it, the fit reports a singular covariance
    (``covar is None``, ``stderr is None``); pass ``vary=(True, True, False)`` for error bars."""
    return _single(_lib.FIT_TIME_DECAY, x, y, weights, param_guesses, **kw)


def fit_decay_time_param_decay_batch(x, y, weights=None, param_guesses=(1., 10, 0), **kw) -> FitBatch:
    return curve_fit_batch(_lib.FIT_TIME_DECAY, x, y, weights, param_guesses, **kw)


def fit_decaying_cosine(x, y, weights=None, param_guesses: tuple = (.5, 10, 0.0, 0.5, 5), **kw) -> FitResult:
    """Fit ``decaying_cosine`` (fitting.py:99-115)."""
    return _single(_lib.FIT_DECAYING_COSINE, x, y, weights, param_guesses, **kw)


def fit_decaying_cosine_batch(x, y, weights=None, param_guesses=(.5, 10, 0.0, 0.5, 5), **kw) -> FitBatch:
    return curve_fit_batch(_lib.FIT_DECAYING_COSINE, x, y, weights, param_guesses, **kw)


def fit_shifted_cosine(x, y, weights=None, param_guesses: tuple = (.5, 0, .5, 1.), **kw) -> FitResult:
    """Fit ``shifted_cosine`` (fitting.py:133-149)."""
    return _single(_lib.FIT_SHIFTED_COSINE, x, y, weights, param_guesses, **kw)


def fit_shifted_cosine_batch(x, y, weights=None, param_guesses=(.5, 0, .5, 1.), **kw) -> FitBatch:
    return curve_fit_batch(_lib.FIT_SHIFTED_COSINE, x, y, weights, param_guesses, **kw)


def fit_result_to_json(fit_result):
    """A JSON-serialisable dict of a fit (fitting.py:152-179): chisqr, redchi, best_fit, best_values, covar (or None) and the
    parameters as the string ``Parameters.dumps`` makes -- a string, so that an infinite value never becomes a bare token."""
    return {
        "chisqr": fit_result.chisqr,
        "redchi": fit_result.redchi,
        "best_fit": np.asarray(fit_result.best_fit).tolist(),
        "best_values": fit_result.best_values,
        "covar": fit_result.covar.tolist() if fit_result.covar is not None else None,
        "params": fit_result.params.dumps(),
    }
