"""Generate diamond_exact.npz: pairs of channels (Choi matrices) with a high-precision bracket [L, U] on their diamond-norm
distance, for tests/test_diamond_exact_gpu.py and tests/test_diamond_exact_cpu.py.  CPU only (numpy, scipy, mpmath):

    python tests/golden/make_diamond_goldens.py

The quantity is the one every solver of the project computes (fbx.distance_measures):
    2 max over density matrices rho of g(rho),   g(rho) = tr[(S J S)_+],   S = 1 (x) rho^1/2,
J the Hermitian part of choi0 - choi1.  For each pair:
  1. g is maximised in float64 (L-BFGS over a Hermitian T with rho = T^2 / tr T^2, several starts) -> T_h.
  2. L = 2 g(rho_h) in mpmath at DPS digits, with S built from T_h exactly: any input state gives a lower bound.
  3. U = min over an eps list of 2 lambda_max(Tr_1 Z), Z = S_eps^-1 (S_eps J S_eps)_+ S_eps^-1, S_eps = 1 (x) rho_eps^1/2,
     rho_eps = (1 - eps) rho_h + eps 1/d, all in mpmath.  Z >= J and Z >= 0 hold in exact arithmetic (Watrous' dual); at the
     chosen eps both are checked at DPS digits and any deficit s added as Z + s 1 (U grows by 2 d s).
Only pairs with (U - L) / U <= MAX_WIDTH are kept; the relative width is stored.  Data only: inputs, L, U, width, the closed form
where the pair has one (NaN otherwise), the family name and the optimal T_h.  Deterministic: the same file on every run.
"""
import io
import os
import sys
import zipfile
from multiprocessing import Pool

import mpmath as mp
import numpy as np
from scipy.optimize import minimize

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import diamond_cases as dc  # noqa: E402

DPS = 30
MAX_WIDTH = 1e-10
OUT = os.path.join(HERE, "diamond_exact.npz")
EPS = {1: [10.0 ** -k for k in range(0, 19)], 2: [10.0 ** -k for k in range(0, 19)], 3: [1.0, 1e-8, 1e-11, 1e-14]}


# ------------------------------------------------------------------------------------------------ float64 maximisation
def _unpack(x, d):
    t = np.zeros((d, d), dtype=complex)
    iu = np.triu_indices(d, 1)
    nd = len(iu[0])
    t[np.diag_indices(d)] = x[:d]
    t[iu] = x[d:d + nd] + 1j * x[d + nd:]
    return t + np.triu(t, 1).conj().T


def _pack(g, d):
    iu = np.triu_indices(d, 1)
    return np.concatenate([np.real(np.diag(g)), np.real(g[iu]), np.imag(g[iu])])


def _neg_quotient(x, J, d):
    t = _unpack(x, d)
    n2 = float(np.real(np.trace(t @ t)))
    s = np.kron(np.eye(d), t)
    m = s @ J @ s
    lam, v = np.linalg.eigh((m + m.conj().T) / 2)
    pos = lam > 0
    g = float(lam[pos].sum())
    a = v[:, pos] @ v[:, pos].conj().T @ s @ J
    a = a + a.conj().T
    grad = np.einsum("iaib->ab", a.reshape(d, d, d, d))
    q = g / n2
    gp = _pack(grad - 2 * q * t, d)
    gp[d:] *= 2
    return -q, -gp / n2


def maximise(J, d, seed, starts=6):
    """T_h (normalised, tr T^2 = 1) of the best of several L-BFGS runs on g(T) / tr(T^2)."""
    rs = np.random.RandomState(seed)
    best, best_t = -np.inf, None
    inits = [np.eye(d, dtype=complex)] + [dc.random_hermitian(d, rs) for _ in range(starts - 1)]
    for t0 in inits:
        t0 = t0 / np.sqrt(np.real(np.trace(t0 @ t0)))
        x = _pack(t0, d)
        for _ in range(3):                                   # restarts from the last point sharpen the optimum
            res = minimize(_neg_quotient, x, args=(J, d), jac=True, method="L-BFGS-B",
                           options={"maxiter": 3000, "maxcor": 30, "ftol": 1e-16, "gtol": 1e-14})
            x = res.x / np.sqrt(np.real(np.trace(_unpack(res.x, d) @ _unpack(res.x, d))))
        if -res.fun > best:
            best, best_t = -res.fun, _unpack(x, d)
    return best_t


# ------------------------------------------------------------------------------------------------ mpmath evaluation
def _mp(a):
    return mp.matrix([[mp.mpc(complex(z)) for z in row] for row in np.asarray(a)])


def _kron_eye(d, s):
    out = mp.zeros(d * s.rows, d * s.cols)
    n = s.rows
    for i in range(d):
        for a in range(n):
            for b in range(n):
                out[i * n + a, i * n + b] = s[a, b]
    return out


def _herm(a):
    return (a + a.H) / 2


def _tr1(z, d):
    out = mp.zeros(d, d)
    for a in range(d):
        for b in range(d):
            out[a, b] = mp.fsum(z[i * d + a, i * d + b] for i in range(d))
    return out


def bracket(choi0, choi1, T):
    """(L, U, eps of U, shift at that eps) at DPS digits."""
    d = T.shape[0]
    J = _mp((np.asarray(choi0) - np.asarray(choi1) + (np.asarray(choi0) - np.asarray(choi1)).conj().T) / 2)
    Tm = _mp(T)
    n2 = mp.re(sum(((Tm * Tm)[k, k] for k in range(d)), mp.mpf(0)))
    Sh = _kron_eye(d, Tm / mp.sqrt(n2))
    lam = mp.eighe(_herm(Sh * J * Sh), eigvals_only=True)
    L = 2 * mp.fsum(x for x in lam if x > 0)
    mu, W = mp.eighe(_herm(Tm * Tm / n2))
    best = None
    for eps in EPS[d.bit_length() - 1]:
        e = mp.mpf(eps)
        r = [(1 - e) * max(mu[k], mp.mpf(0)) + e / d for k in range(d)]
        s = W * mp.diag([mp.sqrt(x) for x in r]) * W.H
        si = W * mp.diag([1 / mp.sqrt(x) for x in r]) * W.H
        S, Si = _kron_eye(d, s), _kron_eye(d, si)
        lamM, V = mp.eighe(_herm(S * J * S))
        Mp = V * mp.diag([max(x, mp.mpf(0)) for x in lamM]) * V.H
        Z = _herm(Si * Mp * Si)
        u0 = max(mp.eighe(_herm(_tr1(Z, d)), eigvals_only=True))
        if best is None or u0 < best[0]:
            best = (u0, eps, Z)
    u0, eps, Z = best
    m1 = min(mp.eighe(_herm(Z - J), eigvals_only=True))
    m2 = min(mp.eighe(Z, eigvals_only=True))
    shift = max(mp.mpf(0), -m1, -m2)
    U = 2 * (u0 + d * shift)
    return L, U, eps, shift


# ------------------------------------------------------------------------------------------------ the pairs
def random_channel(d, rank, rs):
    g = rs.randn(d * rank, d) + 1j * rs.randn(d * rank, d)
    q, _ = np.linalg.qr(g)
    return dc.kraus2choi([q[j * d:(j + 1) * d] for j in range(rank)])


def non_tp_channel(d, rank, rs):
    """A trace-non-increasing CP map (the kind PGDB returns with trace_preserving=False): Kraus operators of a random channel
    followed by a random contraction, sum K^H K = C^H C <= 1."""
    g = rs.randn(d * rank, d) + 1j * rs.randn(d * rank, d)
    q, _ = np.linalg.qr(g)
    w, v = np.linalg.eigh(dc.random_hermitian(d, rs))
    c = v @ np.diag(0.6 + 0.4 * rs.rand(d)) @ v.conj().T
    return dc.kraus2choi([q[j * d:(j + 1) * d] @ c for j in range(rank)])


def amplitude_damping(nq, gamma):
    k0 = np.array([[1, 0], [0, np.sqrt(1 - gamma)]], dtype=complex)
    k1 = np.array([[0, np.sqrt(gamma)], [0, 0]], dtype=complex)
    ks = [np.eye(1, dtype=complex)]
    for _ in range(nq):
        ks = [np.kron(a, k) for a in ks for k in (k0, k1)]
    return dc.kraus2choi(ks)


def candidates(nq):
    """(family, choi0, choi1, exact or NaN) in a fixed order."""
    d = 2 ** nq
    rs = np.random.RandomState(7000 + nq)
    nan = float("nan")
    out = []
    n_random = {1: 6, 2: 8, 3: 2}[nq]
    for i in range(n_random):
        out.append(("random_cptp", random_channel(d, 1 + i % 4, rs), random_channel(d, 1 + (i + 1) % 4, rs), nan))
    out.append(("amplitude_damping", amplitude_damping(nq, 0.1), dc.kraus2choi(np.eye(d)), nan))
    if nq < 3:
        out.append(("amplitude_damping", amplitude_damping(nq, 0.7), dc.kraus2choi(np.eye(d)), nan))
    for i in range(2 if nq < 3 else 1):
        out.append(("non_tp", non_tp_channel(d, 1 + i, rs), non_tp_channel(d, 2, rs), nan))
    base = random_channel(d, 2, rs)
    other = random_channel(d, 3, rs)
    out.append(("near_identical", base + 2.0 ** -20 * (other - base), base, nan))
    fam = dc.families(nq, seed=1)
    picks = ["unitary", "pauli", "depolarizing", "replacement", "mixture"] if nq < 3 else ["unitary", "pauli", "replacement"]
    for name in picks:
        c0, c1, ex = fam[name][2 if name == "unitary" else 0]
        out.append((name, c0, c1, ex))
    if nq < 3:
        c0, c1, ex = fam["unitary"][6]                       # diag(e^{i 1e-3}, 1, ...) against 1: rank-2 optimum
        out.append(("unitary", c0, c1, ex))
    return out


def solve(job):
    nq, k, (name, c0, c1, exact) = job
    d = 2 ** nq
    J = (c0 - c1 + (c0 - c1).conj().T) / 2
    T = maximise(J, d, seed=100 * nq + k)
    with mp.workdps(DPS):
        L, U, eps, shift = bracket(c0, c1, T)
        width = (U - L) / U if U > 0 else mp.mpf(0)
        return dict(nq=nq, name=name, c0=c0, c1=c1, exact=exact, T=T, L=float(L), U=float(U), width=float(width),
                    eps=eps, shift=float(shift))


def _save(path, arrays):
    """np.savez with fixed timestamps, so that the same arrays give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            arr = io.BytesIO()
            np.lib.format.write_array(arr, np.asarray(arrays[key]), allow_pickle=False)
            zf.writestr(info, arr.getvalue())
    with open(path, "wb") as f:
        f.write(buf.getvalue())


def main():
    jobs = [(nq, k, c) for nq in (1, 2, 3) for k, c in enumerate(candidates(nq))]
    jobs.sort(key=lambda j: -j[0])                           # the slow 3-qubit pairs first
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        results = pool.map(solve, jobs, chunksize=1)
    arrays = {}
    for nq in (1, 2, 3):
        rows = [r for r in results if r["nq"] == nq]
        keep = [r for r in rows if r["width"] <= MAX_WIDTH]
        for r in rows:
            print(f"{nq}q {r['name']:18s} L={r['L']:.17g} U={r['U']:.17g} width={r['width']:.2e} eps={r['eps']:.0e} "
                  f"shift={r['shift']:.1e} exact={r['exact']:.17g}{'' if r['width'] <= MAX_WIDTH else '  DROPPED'}")
        p = f"q{nq}_"
        arrays[p + "choi0"] = np.array([r["c0"] for r in keep])
        arrays[p + "choi1"] = np.array([r["c1"] for r in keep])
        arrays[p + "T"] = np.array([r["T"] for r in keep])
        arrays[p + "lower"] = np.array([r["L"] for r in keep])
        arrays[p + "upper"] = np.array([r["U"] for r in keep])
        arrays[p + "width"] = np.array([r["width"] for r in keep])
        arrays[p + "exact"] = np.array([r["exact"] for r in keep])
        arrays[p + "family"] = np.array([r["name"] for r in keep])
    _save(OUT, arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
