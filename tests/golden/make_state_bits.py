"""Writes tests/golden/state_bits.npz: the exact bits the state-tomography kernels (csrc/fbx_state.hip, csrc/fbx_state_measures.hip)
produce, from the build it is run with on a GPU (tests/test_state_bits_gpu.py compares later builds against them).

    python tests/golden/make_state_bits.py [OUT.npz]         (FBX_LIBRARY selects the build; default: the in-tree libfbx.so)

Designs and data are those of tests/state_cases.py (case, device_design, mode_kwargs) and the 4200-setting one-qubit list of
tests/golden/repeated.npz; each case is the smallest that reaches one kernel instantiation or one path through it.

MLE_CASES (fbx_mle_state: rho, iteration counts, hit_max):
    packed<n>_unit / _signed     mle_state_packed_kernel<1 | 2>   standard, to convergence, B = 17 / 5: a full wavefront and a partly
                                                                  filled one, groups that stop at different iterations
    packedD<n>                   ...                              with_identity (m = D), plain, B = 2
    tab<n>                       mle_state_kernel<1 | 2>          d_plus_1, signed, plain: a setting per lane
    staged<n>                    ...                              sixty_five, plain: settings walked, weights staged in LDS
    streamed_plain / _hedged     mle_state_kernel<1>              4200 settings, 12 iterations: weights added with LDS atomics
    three_hedged / _maxent       mle_state_kernel<3>              standard, B = 2
    three_staged                 ...                              twice (m = 126), plain, B = 1
    plain3_<kind>_<mode>         mle_state_plain3_kernel          standard / with_identity, plain / converge, B = 2
    big4_plain / _hedged / _maxent   mle_state_big_kernel<4>      standard, signed, 10 / 6 / 6 iterations, B = 2
    big5_plain / _hedged / _maxent   mle_state_big_kernel<5>      the 1023-setting design, 3 / 2 / 2 iterations, B = 1
OTHER_CASES (fbx_r_operator, fbx_state_log_likelihood, fbx_linv_state; 2 items): standard for 1-5 qubits, sixty_five at 2 qubits, the
4200-setting list; with_identity and twice for 1-3 qubits (linear inversion only).
proj<n> (fbx_proj_state_physical, 1-5 qubits): a state times 1.7 (physical once divided by its trace: comes back as divided), a
Hermitian matrix with negative eigenvalues (rebuilt), a state with a NaN in it.
measures<n> (fbx_state_measures, 1-5 qubits, all four outputs): two full-rank pairs and a pair with a NaN.
pauli<n> (fbx_pauli_vector, 1, 3 and 5 qubits): two states.

Matrices of up to 3 qubits are stored as raw float64 [items, d, d, 2]; those of 4 and 5 qubits as one sha256 digest per item.

Where several wavefronts add to the R operator's weights with LDS atomics (4 and 5 qubits) every design here measures each Pauli
operator once, so no sum depends on an order; inside one wavefront (the repeated designs at 1-3 qubits) the hardware fixes it.

Run it from the commit whose results are the contract -- a change that only moves or folds code must not need it."""
import functools
import hashlib
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (os.path.join(ROOT, "forest-benchmarking_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import state_cases as sc                  # noqa: E402
import state_measure_cases as smc         # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
RAW_QUBITS = 3                            # matrices of more qubits are stored as digests
# name -> (qubits, design, signed, items, mode, maxiter or None for the mode's own)
MLE_CASES = {
    "packed1_unit": (1, "standard", False, 17, "converge", None), "packed1_signed": (1, "standard", True, 17, "converge", None),
    "packed2_unit": (2, "standard", False, 5, "converge", None), "packed2_signed": (2, "standard", True, 5, "converge", None),
    "packedD1": (1, "with_identity", False, 2, "plain", None), "packedD2": (2, "with_identity", False, 2, "plain", None),
    "tab1": (1, "d_plus_1", True, 2, "plain", None), "tab2": (2, "d_plus_1", True, 2, "plain", None),
    "staged1": (1, "sixty_five", False, 2, "plain", None), "staged2": (2, "sixty_five", False, 2, "plain", None),
    "streamed_plain": (1, "s1", False, 2, "plain", 12), "streamed_hedged": (1, "s1", False, 2, "hedged", 12),
    "three_hedged": (3, "standard", False, 2, "hedged", None), "three_maxent": (3, "standard", False, 2, "maxent", None),
    "three_staged": (3, "twice", False, 1, "plain", None),
    "plain3_standard_plain": (3, "standard", False, 2, "plain", None), "plain3_standard_converge": (3, "standard", False, 2, "converge", None),
    "plain3_with_identity_plain": (3, "with_identity", False, 2, "plain", None),
    "plain3_with_identity_converge": (3, "with_identity", False, 2, "converge", None),
    "big4_plain": (4, "standard", True, 2, "plain", 10), "big4_hedged": (4, "standard", True, 2, "hedged", 6),
    "big4_maxent": (4, "standard", True, 2, "maxent", 6),
    "big5_plain": (5, "standard", False, 1, "plain", 3), "big5_hedged": (5, "standard", False, 1, "hedged", 2),
    "big5_maxent": (5, "standard", False, 1, "maxent", 2),
}
# name -> (qubits, design, linear inversion only)
OTHER_CASES = {f"other{n}_standard": (n, "standard", False) for n in (1, 2, 3, 4, 5)}
OTHER_CASES.update({"other2_sixty_five": (2, "sixty_five", False), "other1_s1": (1, "s1", False)})
OTHER_CASES.update({f"other{n}_{kind}": (n, kind, True) for n in (1, 2, 3) for kind in ("with_identity", "twice")})
OTHER_ITEMS = 2
POST_QUBITS = (1, 2, 3, 4, 5)
PAULI_QUBITS = (1, 3, 5)
MEASURES = ("purity", "fidelity", "trace_distance", "hs_ip")


def keys():
    """every key of the fixture"""
    out = {f"{n}/{k}" for n in MLE_CASES for k in ("rho", "iterations", "hit_max")}
    out |= {f"{n}/{k}" for n, (_, _, linv_only) in OTHER_CASES.items() for k in (("linv",) if linv_only else ("r", "ll", "linv"))}
    out |= {f"proj{n}/out" for n in POST_QUBITS} | {f"measures{n}/{k}" for n in POST_QUBITS for k in MEASURES}
    return out | {f"pauli{n}/out" for n in PAULI_QUBITS}


@functools.lru_cache(maxsize=None)
def case(n, kind, signed, B):
    """(paulis, coefs, expectations, counts): state_cases.case, the 4200-setting list of repeated.npz ('s1'), and at 5 qubits -- for
    which state_cases has no row -- the standard design with the data of state_cases.data"""
    if kind == "s1":
        with np.load(os.path.join(GOLDEN, "repeated.npz")) as g:
            p = np.ascontiguousarray(g["s1_paulis"])
            return p, np.ones(len(p)), g["s1_e"][:B], g["s1_c"][:B]
    if n == 5:
        assert kind == "standard" and not signed
        from fbx_oracle import design as od
        p = np.ascontiguousarray(od.traceless_pauli_codes(5), dtype=np.uint8)
        return (p, np.ones(len(p))) + sc.data(5, p, np.ones(len(p)), B, sc.DEFAULT_SEED)
    return sc.case(n, kind, signed, B)


def mle_kwargs(name):
    n, kind, _, _, mode, maxiter = MLE_CASES[name]
    if kind == "s1" and mode == "hedged":            # the step of tests/test_repeated_datasets.py for this list
        return dict(beta=0.5, epsilon=1e-4, maxiter=maxiter)
    return sc.mode_kwargs(mode, n, len(case(*MLE_CASES[name][:4])[0]), maxiter)


def stored(x, n):
    """complex [B, d, d] (or real [B, k]) as the fixture holds it: raw float64 up to RAW_QUBITS qubits, else a sha256 digest per item"""
    x = np.ascontiguousarray(x)
    if n <= RAW_QUBITS:
        return x.view(np.float64).reshape(x.shape + (2,)).copy() if np.iscomplexobj(x) else x.astype(np.float64)
    return np.array([np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8) for a in x])


def run_mle(name):
    from fbx import tomography
    n, kind, signed, B = MLE_CASES[name][:4]
    p, cf, e, c = case(n, kind, signed, B)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")              # 'Maximum number of iterations reached'
        rho, st = tomography.iterative_mle_state_estimate_batch(sc.device_design(n, p, cf), e, c, return_stats=True, **mle_kwargs(name))
    return {"rho": stored(rho, n), "iterations": np.array(st["iterations"], dtype=np.int32), "hit_max": np.array(st["hit_max"], dtype=np.uint8)}


def run_other(name):
    from fbx import tomography
    n, kind, linv_only = OTHER_CASES[name]
    p, cf, e, c = case(n, kind, False, OTHER_ITEMS)
    des = sc.device_design(n, p, cf)
    out = {"linv": stored(tomography.linear_inv_state_estimate_batch(des, e), n)}
    if not linv_only:
        states = smc.full_rank_pairs(n, OTHER_ITEMS, 97)[0]
        out["r"] = stored(tomography._R_batch(states, des, e), n)
        out["ll"] = np.array(tomography.state_log_likelihood_batch(states, des, e, c), dtype=np.float64)
    return out


def proj_inputs(n):
    """[3, d, d]: physical once divided by its trace, indefinite, with a NaN"""
    rho = smc.full_rank_pairs(n, 2, 211)[0]
    x = np.stack([1.7 * rho[0], smc.indefinite(n, 1, 215)[0], rho[1]])
    x[2, 1, 0] = np.nan
    assert np.linalg.eigvalsh(x[0]).min() > 0 and np.linalg.eigvalsh(x[1]).min() < 0
    return x


def run_proj(n):
    from fbx.operator_tools import project_state_matrix as psm
    return {"out": stored(psm.project_state_matrix_to_physical_batch(proj_inputs(n)), n)}


def measure_inputs(n):
    """rho, sigma [3, d, d]: two full-rank pairs and a pair with a NaN in sigma"""
    rho, sig = (np.array(x) for x in smc.full_rank_pairs(n, 3, 213))
    sig[2, 0, 1] = np.nan
    return rho, sig


def run_measures(n):
    from fbx import distance_measures as dm
    out = dm.state_measures_batch(*measure_inputs(n), which=MEASURES)
    return {k: np.array(out[k], dtype=np.float64) for k in MEASURES}


def run_pauli(n):
    from fbx import plotting
    vec, _ = plotting.state_pauli_rep_plot_inputs(smc.full_rank_pairs(n, 2, 214)[0])
    return {"out": stored(vec[:, :, 0], n)}


def run_all():
    arrays = {}

    def add(name, got):
        for k, v in got.items():
            arrays[f"{name}/{k}"] = v
    for name in MLE_CASES:
        add(name, run_mle(name))
        print(name, "iterations", arrays[name + "/iterations"], "hit_max", arrays[name + "/hit_max"], flush=True)
    for name in OTHER_CASES:
        add(name, run_other(name))
    for n in POST_QUBITS:
        add(f"proj{n}", run_proj(n))
        add(f"measures{n}", run_measures(n))
        print(n, "qubits: fidelity", arrays[f"measures{n}/fidelity"], flush=True)
    for n in PAULI_QUBITS:
        add(f"pauli{n}", run_pauli(n))
    return arrays


if __name__ == "__main__":
    from fbx import _lib
    _lib.set_device(0)
    arrays = run_all()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLDEN, "state_bits.npz")
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")
