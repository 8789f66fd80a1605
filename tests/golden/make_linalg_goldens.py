"""Generate linalg_cases.npz: high-precision eigenvalues of the structured Hermitian matrices of tests/linalg_cases.py, for
tests/test_linalg_gpu.py and tests/test_linalg_cpu.py.  CPU only (numpy, mpmath), a few minutes on eight cores:

    python tests/golden/make_linalg_goldens.py

The matrices themselves are rebuilt from their seeds by the tests; this file holds, per case, the eigenvalues from
mpmath.eighe(..., eigvals_only=True) at DPS digits on the exact float64 matrix (lower triangle mirrored) rounded to float64,
the SHA-256 of the matrix's bytes, ||A||_2 (the largest |eigenvalue|) and ||A||_F.  It also measures numpy.linalg.eigvalsh
against mpmath on every case and stores c_w = max(1, 4 x the largest err / (N eps ||A||_2)): the yardstick of the eigenvalue
and residual bounds (the factor 4: Jacobi applies several sweeps of N - 1 rotation rounds where LAPACK reduces the matrix
once).  Data only.  Deterministic: the same file on every run.
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

import linalg_cases as lc  # noqa: E402

DPS = 34
OUT = os.path.join(HERE, "linalg_cases.npz")


def solve(job):
    name, N = job
    a = lc.hermitian(lc.cases(N)[name])
    with mp.workdps(DPS):
        m = mp.matrix(N, N)
        f2 = mp.mpf(0)
        for r in range(N):
            for c in range(N):
                z = mp.mpc(float(a[r, c].real), float(a[r, c].imag))
                m[r, c] = z
                f2 += z.real ** 2 + z.imag ** 2
        w = sorted(mp.eighe(m, eigvals_only=True)) if f2 > 0 else [mp.mpf(0)] * N
        norm2 = max(abs(x) for x in w)
        w_np = np.linalg.eigvalsh(a)
        err = max(abs(mp.mpf(float(x)) - y) for x, y in zip(w_np, w))
        ratio = float(err / (N * lc.EPS * norm2)) if norm2 > 0 else 0.0
        assert norm2 > 0 or err == 0
        return dict(key=lc.key(name, N), w=np.array([float(x) for x in w]), norm2=float(norm2), normF=float(mp.sqrt(f2)),
                    sha=lc.sha256(lc.cases(N)[name]), ratio=ratio)


def _save(path, arrays):
    """np.savez with fixed timestamps, so that the same arrays give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            arr = io.BytesIO()
            np.lib.format.write_array(arr, np.asarray(arrays[k]), allow_pickle=False)
            zf.writestr(info, arr.getvalue())
    with open(path, "wb") as f:
        f.write(buf.getvalue())


def main():
    jobs = [(name, N) for N in lc.DIRECT_SIZES + lc.PADDED_SIZES for name in lc.cases(N)]
    order = sorted(range(len(jobs)), key=lambda k: -jobs[k][1])              # the slow large matrices first
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        done = pool.map(solve, [jobs[k] for k in order], chunksize=1)
    results = [None] * len(jobs)
    for k, r in zip(order, done):
        results[k] = r
    for r in results:
        print(f"{r['key']:24s} norm2={r['norm2']:.6e} normF={r['normF']:.6e} lapack err / (N eps norm2) = {r['ratio']:.3f}")
    worst = max(results, key=lambda r: r["ratio"])
    c_w = max(1.0, 4.0 * worst["ratio"])
    print(f"largest LAPACK ratio {worst['ratio']:.3f} ({worst['key']}); c_w = {c_w:.17g}")
    arrays = {"w_" + r["key"]: r["w"] for r in results}
    arrays["keys"] = np.array([r["key"] for r in results])
    arrays["sha256"] = np.array([r["sha"] for r in results])
    arrays["norm2"] = np.array([r["norm2"] for r in results])
    arrays["normF"] = np.array([r["normF"] for r in results])
    arrays["c_w"] = np.array(c_w)
    _save(OUT, arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
