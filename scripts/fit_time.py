"""Fits per second of fbx_curve_fit on one GPU, against scipy.optimize.leastsq (MINPACK, the routine under lmfit) on one host core
in the same run.

    python scripts/fit_time.py [--batch 100000] [--reps 7] [--baseline-fits 200]

Three configurations: B RB decays of 35 points (weighted), B T2 curves of 53 points (weighted), and the resident RB chain.
What each figure includes:

* ``abi_fits_per_s``: one call of the host-pointer entry point fbx_curve_fit through ctypes with preallocated numpy outputs --
  the copies of x, y, weights and guess in, the transposes, the kernel, the copies of all seven outputs back, one synchronise.
  Nothing of the Python layer (no FitBatch, no best_fit evaluation).
* ``kernel_fits_per_s``: fbx_curve_fit_dev with everything resident, the library's device timer around one launch (the transposes
  and the fit kernel).
* ``rb_resident_chain``: the ABI calls of ``fit_rb_results_batch`` without its Python post-processing: copies of expectations and
  standard errors in, fbx_rb_survival_dev, fbx_fit_prepare_dev, fbx_curve_fit_dev, copies of params, covar, chisqr, redchi, iters,
  status and grad_norm out.  Device buffers are allocated before the timed region.
* ``leastsq_one_core_fits_per_s``: scipy.optimize.leastsq with a finite-difference Jacobian at ftol = xtol = 1.5e-8 from the same
  guesses, one fit after the other.

The data are 512 distinct binomially sampled curves, tiled to B (generation is not what is measured).  Every configuration runs once
as warm-up and then `reps` times; the rate is that of the median time, `spread` is (slowest - fastest) / median.

Idle lanes: the items of a wavefront stop at different iterations and a finished lane waits for the slowest of its 64.  From
iters[] (the wavefronts are the consecutive groups of 64 items), idle_share = 1 - sum(iters) / sum over wavefronts of 64 * max(iters).
One JSON line per configuration."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "forest-benchmarking_amd"))

from fbx import _lib, randomized_benchmarking as rb, synthetic  # noqa: E402
from fbx.analysis import fitting  # noqa: E402

DISTINCT = 512


def summary(times):
    t = np.asarray(times)
    med = float(np.median(t))
    return med, round(float((t.max() - t.min()) / med), 3)


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return out


def idle_share(iters):
    it = np.asarray(iters, dtype=np.int64)
    pad = (-len(it)) % 64
    waves = np.concatenate([it, np.zeros(pad, dtype=np.int64)]).reshape(-1, 64)
    busy = 64 * waves.max(axis=1).sum()                       # the lanes of a partly filled last wavefront idle too
    return round(float(1.0 - it.sum() / max(1, busy)), 4)


def tile(a, B):
    return np.ascontiguousarray(np.tile(a, (-(-B // len(a)),) + (1,) * (a.ndim - 1))[:B])


def rb_inputs(B):
    depths = np.repeat([2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0], 5)
    rng = np.random.default_rng(1)
    e, se = synthetic.rb_data(2, depths, rng.uniform(0.9, 0.99, DISTINCT), 500, DISTINCT, seed=6000)
    return depths, tile(e, B), tile(se, B)


def weights_from_errors(err):
    """1 / err, errors not above zero replaced by the row's smallest positive one (the reference's rule)"""
    with np.errstate(invalid="ignore"):
        pos = err > 0
    small = np.where(pos, err, np.inf).min(axis=1, keepdims=True)
    return 1.0 / np.where(pos, err, small)


def leastsq_seconds_per_fit(model, x, y, w, guess, n):
    from scipy.optimize import leastsq
    fn = fitting.MODELS[model][1]
    t = time.perf_counter()
    for b in range(n):
        leastsq(lambda th: (fn(x, *th) - y[b]) * w[b], guess[b], ftol=1.5e-8, xtol=1.5e-8, maxfev=2000 * (len(guess[b]) + 1))
    return (time.perf_counter() - t) / n


def device_outputs(B, P):
    DB = _lib.DeviceBuffer
    return [DB(8 * B * P), DB(8 * B * P * P), DB(8 * B), DB(8 * B), DB(4 * B), DB(4 * B), DB(8 * B)]


def host_outputs(B, P):
    return [np.empty((B, P)), np.empty((B, P, P)), np.empty(B), np.empty(B), np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32),
            np.empty(B)]


def fit_config(name, model, x, y, w, guess, reps, baseline_fits):
    B, K = y.shape
    P = guess.shape[1]
    lib = _lib.lib()
    tol = (fitting.DEFAULT_FTOL, fitting.DEFAULT_XTOL, fitting.DEFAULT_MAX_ITERS)
    outs = host_outputs(B, P)
    ptrs = [_lib.iptr(o) if o.dtype == np.int32 else _lib.dptr(o) for o in outs]

    def abi():
        _lib.check(lib.fbx_curve_fit(model, B, K, _lib.dptr(x), 0, _lib.dptr(y), _lib.dptr(w), _lib.dptr(guess), (1 << P) - 1, *tol, *ptrs))
    host = timed(abi, reps)
    iters, status = outs[4].copy(), outs[5].copy()
    DB = _lib.DeviceBuffer
    bufs = [DB.from_array(a) for a in (x, y, w, guess)] + device_outputs(B, P)

    def launch():
        _lib.check(lib.fbx_curve_fit_dev(model, B, K, bufs[0].ptr, 0, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, (1 << P) - 1, *tol,
                                         *[b.ptr for b in bufs[4:]]))
    launch(); _lib.synchronize()
    dev = []
    ms = C.c_double(0.0)
    for _ in range(reps):
        _lib.check(lib.fbx_timer_begin())
        launch()
        _lib.check(lib.fbx_timer_end(C.byref(ms)))
        dev.append(ms.value * 1e-3)
    for b in bufs:
        b.free()
    cpu = leastsq_seconds_per_fit(model, x, y, w, guess, min(baseline_fits, B))
    hm, hs = summary(host)
    dm, ds = summary(dev)
    reason = status & 0xF
    print(json.dumps({"config": name, "B": B, "K": K, "abi_fits_per_s": round(B / hm), "abi_spread": hs,
                      "kernel_fits_per_s": round(B / dm), "kernel_spread": ds, "kernel_ms": round(dm * 1e3, 3),
                      "leastsq_one_core_fits_per_s": round(1 / cpu), "iters_mean": round(float(iters.mean()), 2),
                      "iters_max": int(iters.max()), "idle_lane_share": idle_share(iters),
                      "converged": int(((reason == 1) | (reason == 2)).sum())}), flush=True)


def chain_config(depths, e, se, shots, reps):
    B, K, n = e.shape
    dim = n + 1
    lib = _lib.lib()
    DB = _lib.DeviceBuffer
    d_x = DB.from_array(np.ascontiguousarray(depths, dtype=np.float64))
    d_e, d_s, d_surv, d_var, d_w, d_g = DB(e.nbytes), DB(se.nbytes), DB(8 * B * K), DB(8 * B * K), DB(8 * B * K), DB(8 * B * 3)
    d_out, outs = device_outputs(B, 3), host_outputs(B, 3)
    vp = C.c_void_p

    def chain():
        _lib.check(lib.fbx_memcpy_h2d(d_e.ptr, e.ctypes.data_as(vp), e.nbytes))
        _lib.check(lib.fbx_memcpy_h2d(d_s.ptr, se.ctypes.data_as(vp), se.nbytes))
        _lib.check(lib.fbx_rb_survival_dev(dim, B * K, d_e.ptr, d_s.ptr, shots, d_surv.ptr, d_var.ptr))
        _lib.check(lib.fbx_fit_prepare_dev(_lib.FIT_PREPARE_RB, B, K, d_surv.ptr, d_var.ptr, 1, d_w.ptr, d_g.ptr, None))
        _lib.check(lib.fbx_curve_fit_dev(_lib.FIT_BASE_DECAY, B, K, d_x.ptr, 0, d_surv.ptr, d_w.ptr, d_g.ptr, 0b111, fitting.DEFAULT_FTOL,
                                         fitting.DEFAULT_XTOL, fitting.DEFAULT_MAX_ITERS, *[b.ptr for b in d_out]))
        for o, b in zip(outs, d_out):
            _lib.check(lib.fbx_memcpy_d2h(o.ctypes.data_as(vp), b.ptr, o.nbytes))
        _lib.synchronize()
    cm, cs = summary(timed(chain, reps))
    reason = outs[5] & 0xF
    print(json.dumps({"config": "rb_resident_chain", "B": B, "K": K, "fits_per_s": round(B / cm), "spread": cs,
                      "bytes_in": int(e.nbytes + se.nbytes), "bytes_out": int(sum(o.nbytes for o in outs)),
                      "converged": int(((reason == 1) | (reason == 2)).sum())}), flush=True)
    for b in [d_x, d_e, d_s, d_surv, d_var, d_w, d_g] + d_out:
        b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline-fits", type=int, default=200)
    a = ap.parse_args()
    _lib.set_device(0)
    B = a.batch
    depths, e, se = rb_inputs(B)
    surv, var = rb.survival_statistics_batch(e[:DISTINCT], se[:DISTINCT], 500)
    with np.errstate(invalid="ignore"):
        w = weights_from_errors(np.sqrt(var))
    guess = np.stack([surv[:, 0] - surv[:, -1], np.full(DISTINCT, 0.95), surv[:, -1]], axis=1)
    fit_config("rb_decay", _lib.FIT_BASE_DECAY, depths, tile(surv, B), tile(w, B), tile(guess, B), a.reps, a.baseline_fits)
    t2 = np.linspace(0.0, 13.0, 53)
    rng = np.random.default_rng(2)
    ex, sx = synthetic.spectroscopy_data("t2", t2, 500, DISTINCT, seed=6100, amplitude=rng.uniform(0.4, 0.5, DISTINCT),
                                         decay_time=rng.uniform(6.0, 16.0, DISTINCT), offset=0.0, baseline=0.5,
                                         frequency=rng.uniform(0.97, 1.03, DISTINCT))
    p1 = (1 - ex) / 2
    w2 = weights_from_errors(sx / 2)
    g2 = np.tile([0.5, 10.0, 0.0, 0.5, 1.0], (DISTINCT, 1))
    fit_config("t2_decaying_cosine", _lib.FIT_DECAYING_COSINE, t2, tile(p1, B), tile(w2, B), tile(g2, B), a.reps, a.baseline_fits)
    chain_config(depths, e, se, 500, a.reps)


if __name__ == "__main__":
    main()
