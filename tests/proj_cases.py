"""Structured inputs for the Choi projections (fbx_proj_choi: CP, TP, TNI and Dykstra to the physical TP / TNI sets), for
tests/test_proj_structured_gpu.py, tests/test_proj_cases_cpu.py and tests/golden/make_proj_goldens.py.

The inputs tomography produces are not generic: a noise-free unitary channel has a rank-1 Choi matrix (D - 1 eigenvalues on
the CP clamp), the depolarising channel is fully degenerate, and a TP map has a partial trace that is exactly I (an
eigenvalue of multiplicity d on the TNI clamp).  Four families, every case rebuilt from a seed with the BLAS-free builders
of tests/linalg_cases.py and checked against a SHA-256 in the fixture (tests/golden/proj_cases.npz):

  cp       linalg_cases.build(name, D) as the Hermitian part, plus an anti-Hermitian part of Frobenius norm 0.25 ||H||_F that
           the projection has to remove (`diagonal` and `zero` get none: their answers are exact; `scale_up` / `scale_down` are
           the whole gaussian case times 2^±200), plus -(I + small PSD);
           D = 4, 16, 64 (the fused kernels) and D = 9 (the qutrit, through eigh + matmul)
  channel  Choi matrices around a seeded Haar unitary, d = 2, 4, 8 and 3: the inputs of the Dykstra tests
  tni      x = kron(P, I_d) / d + R - kron(tr_out R, I_d) / d with a prescribed partial trace P; R lies on the grid 2^-20, so
           that for d a power of two its traceless part is exact and P = I gives a partial trace that is exactly I
  tpx      integer real and imaginary parts below 2^20: the TP projection is exact in float64

Conventions of the oracle: un-normalised Choi matrix on H_in (x) H_out, index (i, o) -> i d + o; tr_out sums over o.
"""
import functools
import hashlib
import os

import numpy as np

import linalg_cases as lc

EPS = lc.EPS
SEED = 20261020
CP_SIZES = (4, 9, 16, 64)
DIMS = (2, 3, 4, 8)                              # d of the channel / tni / tpx families; D = d^2
CP_FAMILIES = ("gaussian", "repeated", "cluster9", "cluster13", "rank1", "rankhalf", "graded", "diagonal", "realsym",
               "imagoff", "oplus0", "zero", "scale_up", "scale_down", "negdef")
CP_FAMILIES_9 = lc.PADDED_FAMILIES + ("negdef",)
NO_ANTI = ("diagonal", "zero")
CHANNEL_FAMILIES = ("unitary", "identity", "depol", "mix", "noisy_e1", "noisy_e3", "noisy_e6", "noisy_e9", "cp17", "tpnotcp",
                    "negdef", "zero")
ONE_ITERATION = ("identity", "depol", "mix")     # CPTP inputs: Dykstra leaves after one iteration
TNI_FAMILIES = ("below", "above", "straddle", "eye", "eye17", "cluster9", "cluster13", "one1", "nonherm")
CP64_STORED = ("cp_D64_rank1", "cp_D64_repeated", "cp_D64_cluster13", "cp_D64_graded", "ch_d8_unitary", "ch_d8_noisy_e6")
DYKSTRA_THRESHOLD = 1e-4
DYKSTRA_MARGIN = 1e-6                            # no stopping-functional value within this relative distance of the threshold
DYKSTRA_MAX_ITERS = 300
KINDS = ("cp", "tp", "tni", "ptp", "ptni")


def _rs(tag, d, k):
    return np.random.RandomState([SEED, tag, d, k])


def _norm_f(a):
    """Frobenius norm with a sequential sum"""
    return float(np.sqrt(lc._sum0((a.real * a.real + a.imag * a.imag).reshape(-1))))


def _anti(D, rs):
    gr, gi = rs.standard_normal((D, D)), rs.standard_normal((D, D))
    return lc._cplx(gr - gr.T, gi + gi.T)


def _negdef(D, rs):
    """-(I + small PSD), smallest |eigenvalue| >= 1"""
    psd = lc.from_spectrum(lc.haar(D, rs), rs.uniform(0.0, 0.05, D))
    return lc._cplx(-(np.eye(D) + psd.real), -psd.imag)


def _eye_c(D):
    return lc._cplx(np.eye(D), np.zeros((D, D)))


# ------------------------------------------------------------------------------------------------ cp
def build_cp(name, D):
    fam = CP_FAMILIES if D in lc.DIRECT_SIZES else CP_FAMILIES_9
    if name in ("scale_up", "scale_down"):                    # the whole gaussian case, anti-Hermitian part included, times 2^±200
        g = build_cp("gaussian", D)
        e = 200 if name == "scale_up" else -200
        return lc._cplx(np.ldexp(g.real, e), np.ldexp(g.imag, e))
    rs = _rs(1, D, fam.index(name))
    h = _negdef(D, rs) if name == "negdef" else lc.build(name, D)
    if h is None:
        return None
    if name in NO_ANTI:
        return h
    a = _anti(D, rs)
    s = 0.25 * _norm_f(h) / _norm_f(a)
    return lc._cplx(h.real + s * a.real, h.imag + s * a.imag)


# ------------------------------------------------------------------------------------------------ partial trace, kron
def tr_out(x, d):
    """sum_o x[(i, o), (i', o)], strictly in the order of o"""
    t = x.reshape(d, d, d, d)
    re, im = np.zeros((d, d)), np.zeros((d, d))
    for o in range(d):
        re, im = re + t[:, o, :, o].real, im + t[:, o, :, o].imag
    return lc._cplx(re, im)


def kron_eye(c, d):
    """kron(c, I_d): no arithmetic, placement only"""
    out = np.zeros((d, d, d, d), dtype=np.complex128)
    for o in range(d):
        out[:, o, :, o] = c
    return out.reshape(d * d, d * d)


def tp_projection(x, d):
    """x - kron((tr_out x - I) / d, I_d), one rounding per step"""
    c = tr_out(x, d)
    c = lc._cplx((c.real - np.eye(d)) / d, c.imag / d)
    k = kron_eye(c, d)
    return lc._cplx(x.real - k.real, x.imag - k.imag)


# ------------------------------------------------------------------------------------------------ channel
def _unitary_choi(d, rs):
    ur, ui = lc.haar(d, rs)
    vr, vi = ur.T.reshape(-1).copy(), ui.T.reshape(-1).copy()              # column-stacking vec
    return lc._cplx(np.multiply.outer(vr, vr) + np.multiply.outer(vi, vi), np.multiply.outer(vi, vr) - np.multiply.outer(vr, vi))


def build_channel(name, d):
    D = d * d
    u = _unitary_choi(d, _rs(2, d, 0))                                      # the same unitary in every case of one d
    rs = _rs(3, d, CHANNEL_FAMILIES.index(name))
    if name == "unitary":
        return u
    if name == "identity":
        v = np.eye(d).reshape(-1)
        return lc._cplx(np.multiply.outer(v, v), np.zeros((D, D)))
    if name == "depol":
        return lc._cplx(np.eye(D) / d, np.zeros((D, D)))
    if name == "mix":
        return lc._cplx(0.5 * u.real + 0.5 * (np.eye(D) / d), 0.5 * u.imag)
    if name.startswith("noisy_e"):
        eps = {"1": 1e-1, "3": 1e-3, "6": 1e-6, "9": 1e-9}[name[-1]]
        g = lc._gaussian(D, rs)
        return lc._cplx(u.real + eps * g.real, u.imag + eps * g.imag)
    if name == "cp17":
        return lc._cplx(1.7 * u.real, 1.7 * u.imag)
    if name == "tpnotcp":
        g = lc._gaussian(D, rs)
        return tp_projection(lc._cplx(u.real + 0.3 * g.real, u.imag + 0.3 * g.imag), d)
    if name == "negdef":
        return _negdef(D, rs)
    if name == "zero":
        return np.zeros((D, D), dtype=np.complex128)
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ tni
def _tni_p(name, d, rs):
    if name == "eye":
        return _eye_c(d)
    if name == "eye17":
        return lc._cplx(1.7 * np.eye(d), np.zeros((d, d)))
    if name == "below":
        spec = rs.uniform(0.1, 0.9, d)
    elif name == "above":
        spec = rs.uniform(1.1, 2.0, d)
    elif name in ("straddle", "nonherm"):
        spec = np.where(np.arange(d) % 2 == 0, rs.uniform(0.2, 0.8, d), rs.uniform(1.2, 1.8, d))
    elif name in ("cluster9", "cluster13"):
        if d < 3:
            return None
        spec = np.where(np.arange(d) % 2 == 0, rs.uniform(0.2, 0.8, d), rs.uniform(1.2, 1.8, d))
        gap = 1e-9 if name == "cluster9" else 1e-13
        spec[:3] = [1.0 * (1.0 + j * gap) for j in range(3)]
    elif name == "one1":
        spec = np.where(np.arange(d) % 2 == 0, rs.uniform(1.2, 1.8, d), rs.uniform(0.2, 0.8, d))
        spec[d // 2] = 1.0
    else:
        raise KeyError(name)
    p = lc.from_spectrum(lc.haar(d, rs), spec[rs.permutation(d)])
    if name == "nonherm":
        p = lc._cplx(p.real + 1e-3 * rs.standard_normal((d, d)), p.imag + 1e-3 * rs.standard_normal((d, d)))
    return p


def build_tni(name, d):
    rs = _rs(4, d, TNI_FAMILIES.index(name))
    p = _tni_p(name, d, rs)
    if p is None:
        return None
    D = d * d
    r = lc._cplx(np.rint(rs.standard_normal((D, D)) * 2.0 ** 20) * 2.0 ** -20, np.rint(rs.standard_normal((D, D)) * 2.0 ** 20) * 2.0 ** -20)
    t = tr_out(r, d)
    k = kron_eye(lc._cplx(p.real / d - t.real / d, p.imag / d - t.imag / d), d)
    return lc._cplx(r.real + k.real, r.imag + k.imag)


# ------------------------------------------------------------------------------------------------ tpx
def build_tpx(d):
    """[3][D][D] with integer parts below 2^20; for d = 3 the entries (i d, i' d) are shifted so that tr_out x - I is divisible
    by 3: then x - kron((tr_out x - I) / d, I_d) is exact in float64 at every d"""
    D = d * d
    rs = _rs(5, d, 0)
    re = rs.randint(-2 ** 20 + 4, 2 ** 20 - 4, (3, D, D)).astype(np.float64)
    im = rs.randint(-2 ** 20 + 4, 2 ** 20 - 4, (3, D, D)).astype(np.float64)
    if d == 3:
        for b in range(3):
            t = tr_out(lc._cplx(re[b], im[b]), d)
            re[b, ::d, ::d] -= np.mod(t.real - np.eye(d), 3.0)
            im[b, ::d, ::d] -= np.mod(t.imag, 3.0)
    return lc._cplx(re, im)


# ------------------------------------------------------------------------------------------------ the case tables
def _freeze(out):
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cp_cases(D):
    fam = CP_FAMILIES if D in lc.DIRECT_SIZES else CP_FAMILIES_9
    built = ((name, build_cp(name, D)) for name in fam)
    return _freeze({f"cp_D{D}_{name}": a for name, a in built if a is not None})


@functools.lru_cache(maxsize=None)
def channel_cases(d):
    return _freeze({f"ch_d{d}_{name}": build_channel(name, d) for name in CHANNEL_FAMILIES})


@functools.lru_cache(maxsize=None)
def tni_cases(d):
    built = ((name, build_tni(name, d)) for name in TNI_FAMILIES)
    return _freeze({f"tni_d{d}_{name}": a for name, a in built if a is not None})


@functools.lru_cache(maxsize=None)
def tpx_cases(d):
    return _freeze({f"tpx_d{d}": build_tpx(d)})


def dim_of(D):
    d = int(round(np.sqrt(D)))
    assert d * d == D
    return d


def cp_inputs(D):
    """everything the CP projection is run on at one size: the cp family and the channel family"""
    return {**cp_cases(D), **channel_cases(dim_of(D))}


def tni_inputs(d):
    return {**tni_cases(d), **channel_cases(d)}


def all_cases():
    out = {}
    for D in CP_SIZES:
        out.update(cp_cases(D))
    for d in DIMS:
        out.update(channel_cases(d))
        out.update(tni_cases(d))
        out.update(tpx_cases(d))
    return out


def family_of(key):
    return key.split("_", 2)[2] if key.count("_") >= 2 else ""


sha256 = lc.sha256


# ------------------------------------------------------------------------------------------------ long-double helpers
def hermitise_ld(x):
    xl = x.astype(np.clongdouble)
    return (xl + xl.conj().T) / 2


def norm_ld(a):
    a = np.asarray(a, dtype=np.clongdouble)
    return float(np.sqrt((a.real ** 2 + a.imag ** 2).sum()))


def tr_out_ld(x, d):
    return np.einsum("iojo->ij", np.asarray(x, dtype=np.clongdouble).reshape(d, d, d, d))


def kron_eye_ld(c, d):
    return np.einsum("ij,ol->iojl", np.asarray(c, dtype=np.clongdouble), np.eye(d, dtype=np.longdouble)).reshape(d * d, d * d)


def tp_reference_ld(x, d):
    """(x - kron((tr_out x - I) / d, I_d), entrywise magnitude bound |x| + kron((tr_out |x| + I) / d, I_d)) in long double"""
    want = x.astype(np.clongdouble) - kron_eye_ld((tr_out_ld(x, d) - np.eye(d)) / d, d)
    mag = np.abs(x).astype(np.longdouble) + kron_eye_ld((tr_out_ld(np.abs(x), d) + np.eye(d)) / d, d).real
    return want, mag


def tni_expected_ld(x, corr, d):
    """x - kron(C / d, I_d) for the stored d x d correction C"""
    return x.astype(np.clongdouble) - kron_eye_ld(np.asarray(corr, dtype=np.clongdouble) / d, d)


# ------------------------------------------------------------------------------------------------ the bounds of the tests
# The eigensolver stops at off-norm <= sqrt(FBX_JACOBI_TOL2) ||H||_F = 1e-13 ||H||_F: the computed decomposition is exact for a
# matrix within that distance of H (a backward error), and the projection onto a convex set is non-expansive, so the stopping rule
# costs at most 1e-13 ||H||_F.  The rest is rounding, measured on the float64 oracle (LAPACK) against mpmath with a factor 4 of
# margin: c_p for one projection, c_d per Dykstra iteration (tests/golden/make_proj_goldens.py).
def cp_tol(D, norm_h, c_p):
    return (1e-13 + c_p * D * EPS) * norm_h


def tni_tol(d, norm_p, c_p):
    return (1e-13 + c_p * d * EPS) * norm_p


def dykstra_scale(x, d):
    return norm_ld(x) + d


def dykstra_tol(iters, D, scale, c_d):
    return iters * (1e-13 + c_d * D * EPS) * scale


def dykstra_tol_vs_oracle(iters, D, scale, c_d):
    """against the float64 oracle instead of mpmath: the oracle's own budget, iters c_d D eps s, is added"""
    return iters * (1e-13 + 2.0 * c_d * D * EPS) * scale


def sequence_is_clear(seq):
    """no stopping-functional value within a relative DYKSTRA_MARGIN of the threshold: the iteration count is then defined by the
    mathematics and not by rounding"""
    seq = np.asarray(seq, dtype=np.float64)
    return bool((np.abs(seq - DYKSTRA_THRESHOLD) > DYKSTRA_MARGIN * DYKSTRA_THRESHOLD).all())


# ------------------------------------------------------------------------------------------------ the float64 oracle
def oracle_single(kind, x):
    from fbx_oracle import superops as so
    if kind == "cp":
        return so.proj_choi_to_completely_positive(np.array(x))
    if kind == "tp":
        return so.proj_choi_to_trace_preserving(np.array(x))
    return so.proj_choi_to_trace_non_increasing(np.array(x))


@functools.lru_cache(maxsize=None)
def _oracle_dykstra(key, tp):
    from fbx_oracle import superops as so
    x = np.array(all_cases()[key])
    old_cp, old_tp, last_cp, last_state = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x), x
    seq = []
    while True:
        pre_cp = last_state - old_cp
        cp = so.proj_choi_to_completely_positive(pre_cp)
        new_cp = cp - pre_cp
        pre_tp = cp - old_tp
        new_state = so.proj_choi_to_trace_preserving(pre_tp) if tp else so.proj_choi_to_trace_non_increasing(pre_tp)
        new_tp = new_state - pre_tp
        crit = np.linalg.norm(new_cp - old_cp) ** 2 + np.linalg.norm(new_tp - old_tp) ** 2 \
            + 2 * abs(np.dot(so.vec(old_tp).conj().T, so.vec(new_state - last_state))) \
            + 2 * abs(np.dot(so.vec(old_cp).conj().T, so.vec(cp - last_cp)))
        seq.append(float(np.asarray(crit).reshape(-1)[0]))
        if crit < DYKSTRA_THRESHOLD:
            break
        old_cp, old_tp, last_cp, last_state = new_cp, new_tp, cp, new_state
    new_state.setflags(write=False)
    return new_state, len(seq), np.array(seq)


def oracle_dykstra(key, tp):
    """(final iterate, iterations, stopping-functional values) of the oracle's Dykstra (proj_choi_to_physical, with the functional
    recorded); computed once per process and shared"""
    return _oracle_dykstra(key, bool(tp))


# ------------------------------------------------------------------------------------------------ the fixture
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proj_cases.npz")
# SHA-256 over the fixture's array names, shapes and bytes (fixture_digest): an altered array is reported as that
FIXTURE_DIGEST = "1a7f8574ca6930099acfcbc9514faaba1e16407a4a575bec042ff36092d91a52"


def fixture_digest(arrays):
    h = hashlib.sha256()
    for k in sorted(arrays):
        a = np.ascontiguousarray(arrays[k])
        h.update(k.encode() + str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def gold():
    with np.load(GOLD) as z:
        arrays = {k: z[k] for k in z.files}
    for a in arrays.values():
        a.setflags(write=False)
    return {"arrays": arrays, "c_p": float(arrays["c_p"]), "c_d": float(arrays["c_d"]),
            "sha": dict(zip((str(k) for k in arrays["keys"]), (str(s) for s in arrays["sha256"]))),
            "norm": dict(zip((str(k) for k in arrays["norm_keys"]), (float(v) for v in arrays["norms"])))}


def check_hashes(cases, g):
    for key, a in cases.items():
        assert sha256(a) == g["sha"][key], f"{key}: the generator no longer builds the fixture's input"


def shuffled(cases, seed):
    """(keys, stacked inputs) in a seeded order"""
    keys = list(cases)
    keys = [keys[k] for k in np.random.RandomState([9, seed]).permutation(len(keys))]
    return keys, np.stack([cases[k] for k in keys])


# ------------------------------------------------------------------------------------------------ the checks
# Shared by the GPU test (got = the device's output) and the CPU test (got = the float64 oracle's: the bounds are attainable
# without the code under test).  Each prints the ratio of what it saw to what it allows and returns the largest.
def extreme_eig_ld(a, top=False):
    """The Rayleigh quotient, in long double, of LAPACK's float64 lowest (highest) eigenvector of the Hermitian part.  A Rayleigh
    quotient lies inside the spectrum: it is an upper bound on the smallest eigenvalue (a lower bound on the largest), off by
    the eigenvector's error squared times the spectrum's width, and inside a cluster -- the zeros of a rank-1 result -- by up to
    the cluster's width, about D eps ||H||_F.  A violation of that size, a small fraction of the bound, can hide here."""
    h = hermitise_ld(a)
    _, v = np.linalg.eigh(h.astype(np.complex128))
    vl = v[:, -1 if top else 0].astype(np.clongdouble)
    return float((vl.conj() @ h @ vl).real / (vl.conj() @ vl).real)


def _ratio(err, tol):
    return err / tol if tol > 0 else (0.0 if err == 0 else np.inf)


def check_cp(label, keys, xs, got, g):
    """||got - ref||_F <= (1e-13 + c_p D eps) ||H||_F against the fixture (where it holds no reference: against the float64 oracle,
    with the oracle's budget c_p D eps ||H||_F added); the exact answers; smallest eigenvalue >= -(1e-13 + c_p D eps) ||H||_F
    in every case"""
    D, worst = xs.shape[-1], 0.0
    for key, x, y in zip(keys, xs, got):
        name, stored = family_of(key), "cp_" + key in g["arrays"]
        norm_h = norm_ld(hermitise_ld(x))
        ref = g["arrays"]["cp_" + key] if stored else oracle_single("cp", x)
        tol = cp_tol(D, norm_h, g["c_p"] if stored else 2.0 * g["c_p"])
        eig_tol = cp_tol(D, norm_h, g["c_p"])                      # no reference enters: never the oracle's budget
        assert np.isfinite(y).all(), (label, key)
        err = norm_ld(y.astype(np.clongdouble) - ref)
        low = extreme_eig_ld(y)
        r_err, r_low = _ratio(err, tol), _ratio(max(-low, 0.0), eig_tol)
        print(f"ratio {label:8s} cp   {key:22s} {'mp    ' if stored else 'oracle'} err {r_err:.3f} -min eig {r_low:.3f}")
        assert err <= tol, (label, key, err, tol)
        assert low >= -eig_tol, (label, key, low, eig_tol)
        if name in ("zero", "negdef"):
            assert not y.any(), (label, key, "no positive eigenvalue: exactly zero")
        if name == "diagonal":
            assert np.array_equal(y, np.diag(np.maximum(np.diag(x).real, 0.0))), (label, key)
        worst = max(worst, r_err, r_low)
    return worst


def check_tni(label, keys, xs, got, g):
    """||got - (x - kron(C / d, I))||_F <= (1e-13 + c_p d eps) ||P||_F; the partial trace's eigenvalues are <= 1 + that bound"""
    d, worst = dim_of(xs.shape[-1]), 0.0
    for key, x, y in zip(keys, xs, got):
        corr = g["arrays"]["tnihi_" + key].astype(np.clongdouble) + g["arrays"]["tnilo_" + key]
        tol = tni_tol(d, norm_ld(tr_out_ld(x, d)), g["c_p"])
        assert np.isfinite(y).all(), (label, key)
        err = norm_ld(y.astype(np.clongdouble) - tni_expected_ld(x, corr, d))
        top = extreme_eig_ld(tr_out_ld(y, d), top=True)
        r_err, r_top = _ratio(err, tol), _ratio(max(top - 1.0, 0.0), tol)
        print(f"ratio {label:8s} tni  {key:22s} err {r_err:.3f} max eig - 1 {r_top:.3f} unchanged {np.array_equal(x, y)}")
        assert err <= tol, (label, key, err, tol)
        assert top <= 1.0 + tol, (label, key, top, tol)
        worst = max(worst, r_err, r_top)
    return worst


def check_tp(label, keys, xs, got):
    """|got - ref| <= (D + 2) eps (|x| + kron((tr_out |x| + I) / d, I)) entrywise against long double, and
    ||tr_out got - I||_F <= D eps (||x||_F + d)"""
    D = xs.shape[-1]
    d, worst = dim_of(D), 0.0
    for key, x, y in zip(keys, xs, got):
        want, mag = tp_reference_ld(x, d)
        err = np.abs(y.astype(np.clongdouble) - want)
        bound = (D + 2) * EPS * mag
        r_err = float(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0)).max())
        tr_err, tr_tol = norm_ld(tr_out_ld(y, d) - np.eye(d)), D * EPS * dykstra_scale(x, d)
        print(f"ratio {label:8s} tp   {key:22s} err {r_err:.3f} tr_out - I {tr_err / tr_tol:.3f}")
        assert (err <= bound).all(), (label, key, r_err)
        assert tr_err <= tr_tol, (label, key, tr_err, tr_tol)
        worst = max(worst, r_err, tr_err / tr_tol)
    return worst


def check_dykstra(label, kind, keys, xs, got, iters, g):
    """The iteration count equals the reference's and ||got - ref||_F <= iters (1e-13 + c_d D eps) s, s = ||x||_F + d: against the
    mpmath iteration where the fixture holds it (d = 2, 3, 4), else against the float64 oracle with its own budget added (only on
    cases whose oracle sequence stays clear of the threshold); CPTP inputs leave after one iteration; physical-TP outputs have
    ||tr_out - I||_F <= D eps s"""
    D = xs.shape[-1]
    d, worst = dim_of(D), 0.0
    for key, x, y, it in zip(keys, xs, got, iters):
        s = dykstra_scale(x, d)
        if f"dyk_{kind}_{key}" in g["arrays"]:
            ref, n_ref, src = g["arrays"][f"dyk_{kind}_{key}"], len(g["arrays"][f"dykseq_{kind}_{key}"]), "mp    "
            tol = dykstra_tol(n_ref, D, s, g["c_d"])
        else:
            ref, n_ref, seq = oracle_dykstra(key, kind == "ptp")
            assert sequence_is_clear(seq), (label, key, "replace this case: its iteration count is defined by rounding")
            tol, src = dykstra_tol_vs_oracle(n_ref, D, s, g["c_d"]), "oracle"
        assert np.isfinite(y).all(), (label, key)
        err = norm_ld(y.astype(np.clongdouble) - ref)
        line = f"ratio {label:8s} {kind:4s} {key:22s} {src} iterations {int(it):3d} / {n_ref:3d} err {_ratio(err, tol):.3f}"
        worst = max(worst, _ratio(err, tol))
        if kind == "ptp":
            tr_err, tr_tol = norm_ld(tr_out_ld(y, d) - np.eye(d)), D * EPS * s
            line += f" tr_out - I {tr_err / tr_tol:.3f}"
            worst = max(worst, tr_err / tr_tol)
        print(line)
        assert int(it) == n_ref, (label, kind, key, int(it), n_ref)
        assert err <= tol, (label, kind, key, err, tol)
        if kind == "ptp":
            assert tr_err <= tr_tol, (label, key, tr_err, tr_tol)
        if family_of(key) in ONE_ITERATION:
            assert int(it) == 1, (label, kind, key, int(it))
    return worst


def check_twice(label, kind, keys, xs, got, again, g):
    """a second application of CP, TNI or TP moves the result by no more than the bound of the first (Frobenius norm; for TP the
    Frobenius norm of its entrywise bound)"""
    D = xs.shape[-1]
    d, worst = dim_of(D), 0.0
    for key, x, y, z in zip(keys, xs, got, again):
        if kind == "cp":
            tol = cp_tol(D, norm_ld(hermitise_ld(x)), g["c_p"])
        elif kind == "tni":
            tol = tni_tol(d, norm_ld(tr_out_ld(x, d)), g["c_p"])
        else:
            tol = (D + 2) * EPS * norm_ld(tp_reference_ld(x, d)[1])
        move = norm_ld(np.asarray(z).astype(np.clongdouble) - y)
        print(f"ratio {label:8s} {kind:4s} {key:22s} applied twice {_ratio(move, tol):.3f}")
        assert move <= tol, (label, kind, key, move, tol)
        worst = max(worst, _ratio(move, tol))
    return worst
