"""Generate tests/golden/rb_cases.npz from the reference's randomized_benchmarking.py and utils.py (build machine only; needs the
reference checkout).

The reference's own non-fit functions are called on seeded inputs and their results recorded: the survival statistics with the
covariance sum (:308-383), the purity and its error (:490-533), every conversion and bound formula (:595-800) and
``transform_pauli_moments_to_bit`` / ``transform_bit_moments_to_pauli`` (utils.py:431-458).  ``lmfit`` and ``pyquil`` are not
installed here and are stubbed for the import only -- so the reference's FIT functions cannot run, and nothing recorded here comes
from a fit (the partner of the fits is scipy, tests/fit_cases.py).  Only arrays are stored.
Usage: python tests/golden/make_rb_goldens.py
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import _ref_harness as rh  # noqa: E402


def load_reference_rb():
    rh._install_stubs()
    inert = rh._Inert

    def mod(name, **attrs):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
        sys.modules[name].__dict__.update(attrs)

    try:
        import tqdm  # noqa: F401
    except ImportError:
        mod("tqdm", tqdm=lambda it, **k: it)
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        mod("matplotlib")
        mod("matplotlib.pyplot", figure=inert)
        mod("matplotlib.ticker")
    mod("lmfit", Model=inert)
    mod("lmfit.model", ModelResult=inert)
    mod("rpcq")
    mod("rpcq.messages", TargetDevice=inert)
    mod("rpcq._utils", RPCErrorError=type("RPCErrorError", (Exception,), {}))
    mod("pyquil.external")
    mod("pyquil.external.rpcq", CompilerISA=inert)
    mod("pyquil.quil", DefGate=inert, Pragma=inert, merge_programs=inert())
    if rh.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, rh.REFERENCE_ROOT)
    return (importlib.import_module("forest.benchmarking.randomized_benchmarking"),
            importlib.import_module("forest.benchmarking.utils"))


def main():
    rb, utils = load_reference_rb()
    rng = np.random.default_rng(11)
    out = {}
    shots = 500
    for dim in (2, 4, 8, 16, 32):
        S = 24
        e = rng.uniform(-1, 1, (S, dim - 1))
        e[0] = 1.0                                                   # the ideal all-zeros outcome
        e[1] = 0.0
        se = np.sqrt((1 - e * e) / shots)
        surv, var, var_ind, cov = [], [], [], []
        for s in range(S):
            a, b = rb.z_obs_stats_to_survival_statistics(list(e[s]), list(se[s]), shots)
            c, d = rb.z_obs_stats_to_survival_statistics(list(e[s]), list(se[s]), None, obs_are_independent=True)
            assert a == c
            surv.append(a); var.append(b); var_ind.append(d)
            cov.append(rb.covariances_of_all_iz_obs(list(e[s]), shots))
        out[f"surv{dim}_e"], out[f"surv{dim}_se"] = e, se
        out[f"surv{dim}_p"], out[f"surv{dim}_var"], out[f"surv{dim}_var_ind"] = np.asarray(surv), np.asarray(var), np.asarray(var_ind)
        out[f"surv{dim}_cov"] = np.asarray(cov)
    out["shots"] = np.asarray(shots)
    for dim in (2, 4, 8):
        S = 24
        n = dim * dim - 1
        e = rng.uniform(-1, 1, (S, n))
        e[0] = 0.0
        e[1, ::2] = rng.uniform(-1e-3, 1e-3, len(e[1, ::2]))          # small expectations: the second-order branch
        e[2] = rng.uniform(-2e-2, 2e-2, n)
        se = np.sqrt((1 - e * e) / shots)
        se[3] = 0.0
        pur, pur_raw, err, err_raw = [], [], [], []
        for s in range(S):
            ex = np.asarray(list(e[s]) + [1.])
            va = np.asarray(list(se[s]) + [0.]) ** 2
            pur.append(rb.estimate_purity(dim, ex)); pur_raw.append(rb.estimate_purity(dim, ex, renorm=False))
            err.append(rb.estimate_purity_err(dim, ex, va.copy())); err_raw.append(rb.estimate_purity_err(dim, ex, va.copy(), renorm=False))
        out[f"pur{dim}_e"], out[f"pur{dim}_se"] = e, se
        out[f"pur{dim}_p"], out[f"pur{dim}_p_raw"] = np.asarray(pur), np.asarray(pur_raw)
        out[f"pur{dim}_err"], out[f"pur{dim}_err_raw"] = np.asarray(err), np.asarray(err_raw)
    # conversion and bound formulas: columns (irb_decay, rb_decay, unitarity, dim, gate_error)
    N = 40
    dims = rng.choice([2, 4, 8], N)
    rbd = rng.uniform(0.9, 0.999, N)
    irb = rbd * rng.uniform(0.95, 0.9999, N)
    uni = np.minimum(1.0, (rbd * rng.uniform(1.0, 1.02, N)) ** 2)
    err = rng.uniform(1e-4, 5e-2, N)
    out["f_dim"], out["f_rb"], out["f_irb"], out["f_unitarity"], out["f_error"] = dims, rbd, irb, uni, err
    res = {k: [] for k in ("unitarity_to_rb_decay", "coherence_angle", "gamma", "bounds", "bounds_unitarity", "gate_error_to_irb_decay",
                           "irb_decay_to_gate_error", "average_gate_error_to_rb_decay", "rb_decay_to_gate_error")}
    for i in range(N):
        d = int(dims[i])
        res["unitarity_to_rb_decay"].append(rb.unitarity_to_rb_decay(uni[i], d))
        res["coherence_angle"].append(rb.coherence_angle(rbd[i], uni[i]))
        res["gamma"].append(rb.gamma(irb[i], uni[i]))
        res["bounds"].append(rb.interleaved_gate_fidelity_bounds(irb[i], rbd[i], d))
        res["bounds_unitarity"].append(rb.interleaved_gate_fidelity_bounds(irb[i], rbd[i], d, uni[i]))
        res["gate_error_to_irb_decay"].append(rb.gate_error_to_irb_decay(err[i], rbd[i], d))
        res["irb_decay_to_gate_error"].append(rb.irb_decay_to_gate_error(irb[i], rbd[i], d))
        res["average_gate_error_to_rb_decay"].append(rb.average_gate_error_to_rb_decay(err[i], d))
        res["rb_decay_to_gate_error"].append(rb.rb_decay_to_gate_error(rbd[i], d))
    for k, v in res.items():
        out["f_" + k] = np.asarray(v, dtype=np.float64)
    m, v = rng.uniform(-1, 1, 16), rng.uniform(0, 1, 16)
    out["moments_in"] = np.stack([m, v])
    out["moments_to_bit"] = np.stack(utils.transform_pauli_moments_to_bit(m, v))
    out["moments_to_pauli"] = np.stack(utils.transform_bit_moments_to_pauli(m, v))
    path = os.path.join(HERE, "rb_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
