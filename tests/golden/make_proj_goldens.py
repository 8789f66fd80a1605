"""Generate proj_cases.npz: high-precision answers for the structured Choi-projection inputs of tests/proj_cases.py, for
tests/test_proj_structured_gpu.py and tests/test_proj_cases_cpu.py.  CPU only (numpy, scipy, mpmath at 50 digits), about a
minute on eight cores:

    python tests/golden/make_proj_goldens.py

The inputs are rebuilt from their seeds by the tests; this file holds
  sha256                  of every input's bytes
  cp_<key>                sum_{w > 0} w v v^H from mpmath.eighe of the Hermitised input, rounded to float64: every case at D = 4,
                          9, 16 and the subset proj_cases.CP64_STORED at D = 64 (64 KB each: the fixture stays under 1 MB)
  normh_<..> (by key)     ||(x + x^H) / 2||_F
  tnihi_<key>, tnilo_<..> the d x d correction C = P - V min(w, 1) V^H, P = tr_out x, (w, V) from the Hermitised P, as a float64
                          pair hi + lo; the expected output x - kron(C / d, I_d) is formed in long double by the tests
  normp (by key)          ||P||_F
  dyk_<kind>_<key>        the final iterate of Dykstra's iteration (project_superoperators.py:87-144 restated in mpmath) for both
                          kinds on the channel family at d = 2, 3, 4, with its iteration count and the whole sequence of
                          stopping-functional values (dykseq_<kind>_<key>)
and the yardsticks, measured here on the float64 oracle (oracle/fbx_oracle/superops.py) against the unrounded mpmath answers:
  c_p = max(1, 4 x the largest ||oracle - mp||_F / (D eps ||H||_F))   over every single projection (TNI: d and ||P||_F)
  c_d = max(1, 4 x the largest ||oracle - mp||_F / (iters D eps s))   over the Dykstra cases, s = ||x||_F + d
Data only.  Deterministic: the same file on every run.
"""
import os
import sys
from multiprocessing import Pool

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
sys.dont_write_bytecode = True

import proj_cases as pc  # noqa: E402
from make_linalg_goldens import _save  # noqa: E402

DPS = 50
OUT = os.path.join(HERE, "proj_cases.npz")


def to_mp(a):
    n, m = a.shape
    out = mp.matrix(n, m)
    for r in range(n):
        for c in range(m):
            out[r, c] = mp.mpc(float(a[r, c].real), float(a[r, c].imag))
    return out


def to_np(m):
    return np.array([[complex(m[r, c]) for c in range(m.cols)] for r in range(m.rows)], dtype=np.complex128)


def norm2(m):
    return sum((z.real ** 2 + z.imag ** 2 for z in m), mp.mpf(0))


def clamp_rebuild(h, keep):
    """sum_k keep(w_k) v_k v_k^H over the eigenpairs of the Hermitian h"""
    n = h.rows
    if norm2(h) == 0:
        return mp.zeros(n, n)
    w, v = mp.eighe(h)
    out = mp.zeros(n, n)
    cols = [k for k in range(n) if keep(w[k]) != 0]
    if not cols:
        return out
    vs = mp.matrix(n, len(cols))
    vw = mp.matrix(n, len(cols))
    for j, k in enumerate(cols):
        for r in range(n):
            vs[r, j] = v[r, k]
            vw[r, j] = v[r, k] * keep(w[k])
    return vw * vs.H


def cp_mp(x):
    return clamp_rebuild((x + x.H) / 2, lambda w: w if w > 0 else mp.mpf(0))


def tr_out_mp(x, d):
    p = mp.zeros(d, d)
    for i in range(d):
        for j in range(d):
            p[i, j] = sum((x[i * d + o, j * d + o] for o in range(d)), mp.mpc(0))
    return p


def sub_kron(x, c, d):
    out = x.copy()
    for i in range(d):
        for j in range(d):
            for o in range(d):
                out[i * d + o, j * d + o] -= c[i, j] / d
    return out


def tni_corr_mp(x, d):
    p = tr_out_mp(x, d)
    return p - clamp_rebuild((p + p.H) / 2, lambda w: w if w < 1 else mp.mpf(1)), p


def tp_mp(x, d):
    return sub_kron(x, tr_out_mp(x, d) - mp.eye(d), d)


def vdot(a, b):
    return sum((mp.conj(p) * q for p, q in zip(a, b)), mp.mpc(0))


def dykstra_mp(x, d, tp):
    """project_superoperators.py:87-144"""
    D = d * d
    old_cp, old_tp, last_cp, last_state = mp.zeros(D, D), mp.zeros(D, D), mp.zeros(D, D), x
    seq = []
    while True:
        pre_cp = last_state - old_cp
        cp = cp_mp(pre_cp)
        new_cp = cp - pre_cp
        pre_tp = cp - old_tp
        new_state = tp_mp(pre_tp, d) if tp else sub_kron(pre_tp, tni_corr_mp(pre_tp, d)[0], d)
        new_tp = new_state - pre_tp
        crit = norm2(new_cp - old_cp) + norm2(new_tp - old_tp) + 2 * abs(vdot(old_tp, new_state - last_state)) \
            + 2 * abs(vdot(old_cp, cp - last_cp))
        seq.append(crit)
        if crit < mp.mpf(pc.DYKSTRA_THRESHOLD) or len(seq) > pc.DYKSTRA_MAX_ITERS:
            return new_state, seq
        old_cp, old_tp, last_cp, last_state = new_cp, new_tp, cp, new_state


def err_f(a_np, m):
    return mp.sqrt(norm2(to_mp(a_np) - m))


def solve(job):
    what, key = job
    x_np = np.array(pc.all_cases()[key])
    D = x_np.shape[0]
    d = pc.dim_of(D)
    with mp.workdps(DPS):
        x = to_mp(x_np)
        if what == "cp":
            ref = cp_mp(x)
            nh = mp.sqrt(norm2((x + x.H) / 2))
            err = err_f(pc.oracle_single("cp", x_np), ref)
            ratio = float(err / (D * pc.EPS * nh)) if nh > 0 else 0.0
            assert nh > 0 or err == 0
            return dict(what=what, key=key, ref=to_np(ref), norm=float(nh), ratio=ratio)
        if what == "tni":
            c, p = tni_corr_mp(x, d)
            npn = mp.sqrt(norm2(p))
            err = err_f(pc.oracle_single("tni", x_np), sub_kron(x, c, d))
            ratio = float(err / (d * pc.EPS * npn)) if npn > 0 else 0.0
            assert npn > 0 or err == 0
            hi = to_np(c)
            lo = to_np(c - to_mp(hi))
            return dict(what=what, key=key, hi=hi, lo=lo, norm=float(npn), ratio=ratio)
        tp = what == "ptp"
        ref, seq = dykstra_mp(x, d, tp)
        o_ref, o_iters, _ = pc.oracle_dykstra(key, tp)
        assert len(seq) == o_iters, (what, key, len(seq), o_iters)
        s = mp.sqrt(norm2(x)) + d
        ratio = float(err_f(o_ref, ref) / (len(seq) * D * pc.EPS * s))
        return dict(what=what, key=key, ref=to_np(ref), seq=np.array([float(v) for v in seq]), ratio=ratio)


def jobs():
    out = []
    for D in pc.CP_SIZES:
        for key in pc.cp_inputs(D):
            if D < 64 or key in pc.CP64_STORED:
                out.append(("cp", key))
    for d in pc.DIMS:
        out += [("tni", key) for key in pc.tni_inputs(d)]
        if d < 8:
            out += [(kind, key) for kind in ("ptp", "ptni") for key in pc.channel_cases(d)]
    return out


def cost(job):
    what, key = job
    D = pc.all_cases()[key].shape[0]
    return D ** 3 * (pc.oracle_dykstra(key, what == "ptp")[1] if what in ("ptp", "ptni") else 1)


def main():
    todo = jobs()
    order = sorted(range(len(todo)), key=lambda k: -cost(todo[k]))           # the slow ones first
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        done = pool.map(solve, [todo[k] for k in order], chunksize=1)
    results = [None] * len(todo)
    for k, r in zip(order, done):
        results[k] = r
    arrays, norms = {}, {}
    worst = {"single": (0.0, ""), "dykstra": (0.0, "")}
    for r in results:
        what, key = r["what"], r["key"]
        tag = f"{what} {key}"
        if what == "cp":
            arrays["cp_" + key] = r["ref"]
            norms["normh_" + key] = r["norm"]
            print(f"{tag:32s} ||H||_F={r['norm']:.6e} oracle err / (D eps ||H||_F) = {r['ratio']:.3f}")
        elif what == "tni":
            arrays["tnihi_" + key], arrays["tnilo_" + key] = r["hi"], r["lo"]
            norms["normp_" + key] = r["norm"]
            print(f"{tag:32s} ||P||_F={r['norm']:.6e} oracle err / (d eps ||P||_F) = {r['ratio']:.3f}")
        else:
            arrays[f"dyk_{what}_{key}"], arrays[f"dykseq_{what}_{key}"] = r["ref"], r["seq"]
            near = float(np.abs(r["seq"] / pc.DYKSTRA_THRESHOLD - 1.0).min())
            print(f"{tag:32s} iterations={len(r['seq']):3d} closest |crit / 1e-4 - 1| = {near:.3e} "
                  f"oracle err / (iters D eps s) = {r['ratio']:.3f}")
            assert pc.sequence_is_clear(r["seq"]) and len(r["seq"]) <= pc.DYKSTRA_MAX_ITERS, tag
        slot = "dykstra" if what in ("ptp", "ptni") else "single"
        if r["ratio"] > worst[slot][0]:
            worst[slot] = (r["ratio"], tag)
    c_p, c_d = max(1.0, 4.0 * worst["single"][0]), max(1.0, 4.0 * worst["dykstra"][0])
    print(f"largest single-projection ratio {worst['single'][0]:.3f} ({worst['single'][1]}); c_p = {c_p:.17g}")
    print(f"largest Dykstra ratio {worst['dykstra'][0]:.3f} ({worst['dykstra'][1]}); c_d = {c_d:.17g}")
    cases = pc.all_cases()
    arrays["keys"] = np.array(list(cases))
    arrays["sha256"] = np.array([pc.sha256(a) for a in cases.values()])
    arrays["norm_keys"] = np.array(list(norms))
    arrays["norms"] = np.array(list(norms.values()))
    arrays["c_p"], arrays["c_d"] = np.array(c_p), np.array(c_d)
    _save(OUT, arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; proj_cases.FIXTURE_DIGEST =", pc.fixture_digest({k: np.asarray(v) for k, v in arrays.items()}))


if __name__ == "__main__":
    main()
