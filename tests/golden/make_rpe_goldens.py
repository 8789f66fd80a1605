"""Generate tests/golden/rpe_cases.npz from the reference's robust_phase_estimation.py (build machine only; needs the reference
checkout).  The reference's own ``estimate_phase_from_moments`` supplies phase, bloch data and the depth at which an item stopped,
its ``robust_phase_estimate`` the phases of the two-qubit ``results`` structures, its ``num_trials`` / ``get_variance_upper_bound``
the tables.  Only arrays are stored.

The estimator is discontinuous where an offset meets an end of its window and where r meets r_std: a last-bit difference in atan2
would legitimately move the answer by a whole window there.  Every stored set therefore keeps every offset at least 1e-9 of the
window's width away from both ends and |r - r_std| >= 1e-9 r (tests/rpe_cases.py::estimate reports the margins); a draw that does
not is drawn again, never dropped later.  Usage: python tests/golden/make_rpe_goldens.py
"""
import importlib
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
import _ref_harness as rh  # noqa: E402
import rpe_cases as rc  # noqa: E402

SETS_PER_DEPTH = 50
SHOTS = 500


def load_rpe():
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
        import matplotlib.pyplot  # noqa: F401
    except ImportError:
        mod("matplotlib")
        mod("matplotlib.pyplot", Axes=inert)
    mod("pyquil.quil", Program=inert, merge_programs=inert(), DefGate=inert, Pragma=inert)
    mod("pyquil.quilbase", Gate=inert)
    if rh.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, rh.REFERENCE_ROOT)
    return importlib.import_module("forest.benchmarking.robust_phase_estimation")


def reference_estimate(rpe, x, y, xe, ye):
    bloch = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        phase = rpe.estimate_phase_from_moments(list(x), list(y), list(xe), list(ye), bloch)
    rows = np.full((len(x), 2), np.nan)
    if bloch:
        rows[:len(bloch)] = bloch
    return float(phase), len(bloch), rows


def two_qubit_structure(rng, kind, n_depths):
    """(qubits, observables [S, 2] codes, in_states [S, 2, 2] (label, index), expectations [D, S], std_errs [D, S])"""
    qubits = [0, 1]
    depth = 2.0 ** np.arange(n_depths)
    vis = np.exp(-depth / (2.0 ** n_depths * 1.5))
    phi_a, phi_b = rng.uniform(0, rc.TWO_PI, size=2)             # the phase with the partner in |0> / in |1>
    if kind == "all_eigvecs":                                    # both qubits in |+>; X / Y on either, alone or with a Z on the other
        obs = [(1, 0), (1, 3), (2, 0), (2, 3), (0, 1), (3, 1), (0, 2), (3, 2)]
        states = [[(0, 0), (0, 0)]] * 8
        weights = (0.5, 0.5)
    else:                                                        # qubit 0 fixed in |1> or |0>, qubit 1 rotates
        obs = [(0, 1), (0, 2), (3, 1), (3, 2)]
        fixed = 1 if kind == "fixed_one" else 0
        states = [[(2, fixed), (0, 0)]] * 4
        weights = (0.0, 1.0) if fixed else (1.0, 0.0)
    exps = np.empty((n_depths, len(obs)))
    for s, (p0, p1) in enumerate(obs):
        xy = p0 if p0 in (1, 2) else p1
        fn = np.cos if xy == 1 else np.sin
        with_z = 3 in (p0, p1)
        ideal = weights[0] * fn(depth * phi_a) + (-1 if with_z else 1) * weights[1] * fn(depth * phi_b)
        exps[:, s] = 2 * rng.binomial(SHOTS, (1 + vis * ideal) / 2) / SHOTS - 1
    errs = np.sqrt((1 - exps * exps) / SHOTS)
    return qubits, np.asarray(obs, dtype=np.int8), np.asarray(states, dtype=np.int8), exps, errs


def main():
    rpe = load_rpe()
    ref = rh.load_reference()
    oe = ref.observable_estimation
    rng = np.random.default_rng(20240607)
    out = {}
    for K in rc.GOLDEN_DEPTHS:
        x, y, xe, ye, phi = rc.moment_sets(rng, SETS_PER_DEPTH, K, shots=SHOTS)
        got = [reference_estimate(rpe, *row) for row in zip(x, y, xe, ye)]
        out[f"k{K}_x"], out[f"k{K}_y"], out[f"k{K}_x_err"], out[f"k{K}_y_err"], out[f"k{K}_true_phase"] = x, y, xe, ye, phi
        out[f"k{K}_phase"] = np.array([g[0] for g in got])
        out[f"k{K}_depth_reached"] = np.array([g[1] for g in got], dtype=np.int32)
        out[f"k{K}_bloch"] = np.stack([g[2] for g in got])
        print(f"K = {K}: {SETS_PER_DEPTH} sets, {(out[f'k{K}_depth_reached'] < K).sum()} cut short")
    # two-qubit `results` structures, run through the reference's robust_phase_estimate
    seen = []
    original = rpe.estimate_phase_from_moments
    rpe.estimate_phase_from_moments = lambda *a, **k: (seen.append(a[:4]), original(*a, **k))[1]
    for name in rc.RESULT_STRUCTURES:
        while True:
            qubits, obs, states, exps, errs = two_qubit_structure(rng, name, 6)
            trial = {f"{name}_qubits": np.asarray(qubits), f"{name}_observables": obs, f"{name}_in_states": states,
                     f"{name}_expectations": exps, f"{name}_std_errs": errs, f"{name}_shots": np.asarray(SHOTS)}
            results, _ = rc.build_results(
                trial, name, lambda label, index, q: oe.TensorProductState([oe._OneQState(label, index, q)]),
                lambda ops: rh.PauliTerm.from_list([(op, q) for q, op in ops.items()]), oe.ExperimentSetting,
                lambda setting, e, s, n: oe.ExperimentResult(setting=setting, expectation=e, total_counts=n, std_err=s))
            del seen[:]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                phases = rpe.robust_phase_estimate(results, qubits)
            if all(rc.safe(rc.estimate(*args)[3]) for args in seen):
                break
        trial[f"{name}_phases"] = np.asarray(phases, dtype=np.float64)
        out.update(trial)
        print(f"{name}: {len(phases)} phases")
    rpe.estimate_phase_from_moments = original
    # host tables
    args = [(d, m, f, a) for m in (1, 8, 64, 2048) for d in (1, 2, 8, 64, 2048) if d <= m
            for f, a in ((1.0, 0.0), (2.5, 0.0), (1.0, 0.05), (3.0, 0.2))]
    out["num_trials_args"] = np.asarray(args, dtype=np.float64)
    out["num_trials_out"] = np.asarray([rpe.num_trials(int(d), int(m), f, a if a else None) for d, m, f, a in args], dtype=np.int64)
    vargs = [(n, f, a) for n in (1, 2, 3, 6, 10, 12) for f, a in ((1.0, 0.0), (2.0, 0.0), (1.0, 0.1), (4.0, 0.25))]
    out["variance_args"] = np.asarray(vargs, dtype=np.float64)
    out["variance_out"] = np.asarray([rpe.get_variance_upper_bound(int(n), f, a if a else None) for n, f, a in vargs])
    fargs = [(m, a) for m in (0.5, 3.0, 25.5) for a in (0.0, 0.01, 0.2, 0.35)]
    out["factor_args"] = np.asarray(fargs)
    out["factor_out"] = np.asarray([rpe.get_additive_error_factor(m, a) for m, a in fargs])
    out["p_max_args"] = np.arange(1, 40)
    out["p_max_out"] = np.asarray([rpe._p_max(int(m)) for m in out["p_max_args"]])
    out["xci_out"] = np.asarray([rpe._xci(int(h)) for h in range(0, 20)])
    angles = [(0.0, 0.0), (np.pi / 2, 0.0), (np.pi / 2, np.pi / 2), (0.3, 1.1), (2.2, 4.0)]
    out["eigvec_angles"] = np.asarray(angles)
    out["eigvecs"] = np.asarray([np.hstack(rpe.bloch_rotation_to_eigenvectors(t, p)) for t, p in angles])
    out["change_of_basis"] = np.asarray([rpe.get_change_of_basis_from_eigvecs(rpe.bloch_rotation_to_eigenvectors(t, p))
                                         for t, p in angles])
    rng4 = np.random.default_rng(4)
    q, _ = np.linalg.qr(rng4.normal(size=(4, 4)) + 1j * rng4.normal(size=(4, 4)))
    out["eigvecs_4"] = q
    out["change_of_basis_4"] = rpe.get_change_of_basis_from_eigvecs([q[:, i] for i in range(4)])
    path = os.path.join(HERE, "rpe_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
