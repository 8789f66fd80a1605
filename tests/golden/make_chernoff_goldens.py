"""Generate chernoff_exact.npz: pairs of states with a high-precision bracket [lo, hi] on their quantum Chernoff bound, for
tests/test_chernoff_gpu.py and tests/test_chernoff_cpu.py.  CPU only (numpy, mpmath):

    python tests/golden/make_chernoff_goldens.py

The quantity is the one fbx_chernoff_bound computes (tests/chernoff_cases.py): lower triangles read, eigenvalues
<= 1e-12 lambda_max of their matrix counted as zero, min over s in [0, 1] of Q(s) = sum_ij O_ij a_i^s b_j^(1-s).  For each
float64 pair the eigendecompositions come from mp.eighe and the minimum from bisection on Q' to the working precision, both at
DPS digits; [lo, hi] are the float64 neighbours below and above that value.  Families: random full-rank, random low-rank
(overlapping supports) and nearly commuting pairs at 1-5 qubits.  Data only: inputs, lo, hi, the argmin and the family name.
Deterministic: the same file on every run.
"""
import io
import os
import sys
import zipfile
from multiprocessing import Pool

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import chernoff_cases as cc  # noqa: E402

DPS = 40
OUT = os.path.join(HERE, "chernoff_exact.npz")
KINDS = ("full", "lowrank", "near")
COUNT = {1: 6, 2: 5, 3: 4, 4: 2, 5: 1}        # pairs per family


def candidates(nq):
    rng = np.random.default_rng([20261016, nq])
    d = 2 ** nq
    return [(kind,) + cc.golden_pair(kind, d, rng) for kind in KINDS for _ in range(COUNT[nq])]


def solve(job):
    nq, kind, rho, sigma = job
    with mp.workdps(DPS):
        value, s = cc.mp_chernoff(rho, sigma, zero_tol=1e-12, dps=DPS)
        v = float(value)
        lo, hi = np.nextafter(v, -np.inf), np.nextafter(v, np.inf)
        assert mp.mpf(lo) <= value <= mp.mpf(hi)
        return dict(nq=nq, kind=kind, rho=rho, sigma=sigma, lo=lo, hi=hi, s=float(s))


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
    jobs = [(nq,) + c for nq in (1, 2, 3, 4, 5) for c in candidates(nq)]
    order = sorted(range(len(jobs)), key=lambda k: -jobs[k][0])         # the slow 5-qubit pairs first
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        done = pool.map(solve, [jobs[k] for k in order], chunksize=1)
    results = [None] * len(jobs)
    for k, r in zip(order, done):
        results[k] = r
    arrays = {}
    for nq in (1, 2, 3, 4, 5):
        rows = [r for r in results if r["nq"] == nq]
        for r in rows:
            print(f"{nq}q {r['kind']:8s} value={r['lo']:.17g}..{r['hi']:.17g} s={r['s']:.10f}")
        p = f"q{nq}_"
        arrays[p + "rho"] = np.array([r["rho"] for r in rows])
        arrays[p + "sigma"] = np.array([r["sigma"] for r in rows])
        arrays[p + "lo"] = np.array([r["lo"] for r in rows])
        arrays[p + "hi"] = np.array([r["hi"] for r in rows])
        arrays[p + "s"] = np.array([r["s"] for r in rows])
        arrays[p + "family"] = np.array([r["kind"] for r in rows])
    _save(OUT, arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
