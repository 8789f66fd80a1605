"""Time of fbx_rpe_simulate on one GPU next to fbx_tomo_simulate in the same run -- the sibling that does the same Philox counting --
both in device-pointer form on resident buffers.

    python scripts/rpe_sim_time.py [--reps 9] [--configs 1:100000:8:500 2:100000:8:500]

A config is n_qubits:batch:depths:shots.  The RPE call simulates `batch` experiments of `depths` depths with `shots` shots at every
depth (one qubit: a noisy rotation, X and Y; two qubits: a noisy controlled phase with a Z partner) and writes the eight moment
planes.  The tomography call runs the one-qubit Pauli process design (18 settings) with as many items as give the same number
of (item, setting) units as the RPE call has (item, depth, basis) units -- rounded up -- at the same shots per unit, and writes
(expectations, counts).  A third call asks fbx_rpe_simulate for the distributions only (the matrix powers without the shots).  Each
call is timed with device events around each of `reps` separate launches after one warm-up; the two
calls alternate, so that a drift of the clock meets both; the time is the median, `spread` is (slowest - fastest) / median.  The
ratio compares seconds per drawn shot.  One JSON line per configuration."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "forest-benchmarking_amd")]

from fbx import _lib, synthetic  # noqa: E402
from fbx.design import process_design  # noqa: E402
from fbx.operator_tools.superoperator_transformations import convert_batch  # noqa: E402


def summary(times):
    t = np.asarray(times)
    med = float(np.median(t))
    return round(med, 6), round(float((t.max() - t.min()) / med), 3)


def timed_alternating(launches, reps):
    """seconds per launch of every entry of `launches`, from the library's device timer around each of `reps` launches (after one
    warm-up each); the entries take turns"""
    lib = _lib.lib()
    for launch in launches:
        launch()
    _lib.synchronize()
    out = [[] for _ in launches]
    ms = C.c_double(0.0)
    for _ in range(reps):
        for times, launch in zip(out, launches):
            _lib.check(lib.fbx_timer_begin())
            launch()
            _lib.check(lib.fbx_timer_end(C.byref(ms)))
            times.append(ms.value * 1e-3)
    return out


def noisy_gates(n, B):
    """[B, D, D]: 16 distinct noisy gates, repeated -- a rotation about z (one qubit) or diag(1, 1, 1, e^{i phi}) (two), then
    depolarizing of 1 %"""
    rng = np.random.default_rng(n)
    if n == 1:
        us = np.array([np.diag([np.exp(-0.5j * a), np.exp(0.5j * a)]) for a in rng.uniform(0, 2 * np.pi, 16)])
    else:
        us = np.array([np.diag([1, 1, 1, np.exp(1j * a)]) for a in rng.uniform(0, 2 * np.pi, 16)])
    ptm = np.array([synthetic.pauli_transfer_matrix(u) for u in us])
    ptm[:, 1:, :] *= 0.99
    return np.ascontiguousarray(ptm[np.arange(B) % 16])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--configs", nargs="+", default=["1:100000:8:500", "2:100000:8:500"])
    args = ap.parse_args()
    _lib.set_device(0)
    lib, DB = _lib.lib(), _lib.DeviceBuffer
    design = process_design(1, "pauli")
    m = design.m
    for cfg in args.configs:
        n, B, K, shots = (int(x) for x in cfg.split(":"))
        units = B * K * 2
        Bt = (units + m - 1) // m
        flips = np.random.default_rng(7).uniform(0.0, 0.05, size=(n, 2))
        d_g = DB.from_array(noisy_gates(n, B))
        d_f = DB.from_array(np.ascontiguousarray(np.broadcast_to(flips, (B, n, 2))))
        d_m, d_st = DB(8 * B * K * 8), DB(B * 4)
        schedule = np.full(K, shots, dtype=np.int32)
        us = np.array([synthetic.haar_unitary(2, np.random.RandomState(1000 + b)) for b in range(16)])
        ptm = np.ascontiguousarray(convert_batch("kraus", "pauli_liouville", us[:, None]).real[np.arange(Bt) % 16])
        d_t = DB.from_array(ptm)
        d_tf = DB.from_array(np.ascontiguousarray(np.broadcast_to(flips[:1], (Bt, 1, 2))))
        d_e, d_c, d_st2 = DB(Bt * m * 8), DB(Bt * m * 8), DB(Bt * 4)

        def rpe_sim():
            _lib.check(lib.fbx_rpe_simulate_dev(n, B, K, d_g.ptr, None, None, 0, None, 0, 1 if n == 2 else -1, d_f.ptr,
                                                _lib.iptr(schedule), 1234, 0, None, None, d_m.ptr, None, None, d_st.ptr))

        def tomo_sim():
            _lib.check(lib.fbx_tomo_simulate_dev(design.handle, Bt, d_t.ptr, shots, d_tf.ptr, 1234, 0, d_e.ptr, d_c.ptr, None, None,
                                                 d_st2.ptr))
        d_p = DB(units * (4 if n == 2 else 2) * 8)

        def distributions_only():
            _lib.check(lib.fbx_rpe_simulate_dev(n, B, K, d_g.ptr, None, None, 0, None, 0, 1 if n == 2 else -1, d_f.ptr,
                                                _lib.iptr(schedule), 1234, 0, d_p.ptr, None, None, None, None, d_st.ptr))
        tr, tt, td = timed_alternating((rpe_sim, tomo_sim, distributions_only), args.reps)
        assert not d_st.to_array(np.int32, (B,)).any() and not d_st2.to_array(np.int32, (Bt,)).any()
        (rm, rs), (tm, ts) = summary(tr), summary(tt)
        per_shot = (np.asarray(tr) / (units * shots)) / (np.asarray(tt) / (Bt * m * shots))
        print(json.dumps({
            "what": "rpe_simulate", "n_qubits": n, "batch": B, "depths": K, "shots": shots, "units": units, "reps": args.reps,
            "split": "lane" if units >= _lib.RPE_SIM_LANE_MIN_UNITS else "wavefront",
            "rpe_simulate_dev": {"seconds": rm, "spread": rs, "experiments_per_s": round(B / rm, 1),
                                 "shots_per_s": round(units * shots / rm, 1),
                                 "distributions_only_seconds": summary(td)[0]},
            "tomo_simulate_dev": {"batch": Bt, "settings": m, "seconds": tm, "spread": ts,
                                  "shots_per_s": round(Bt * m * shots / tm, 1),
                                  "split": "lane" if Bt * m >= 131072 else "wavefront"},
            "rpe_over_tomo_per_shot": round(float(np.median(per_shot)), 4),
            "ratio_per_repetition": {"min": round(float(per_shot.min()), 4), "max": round(float(per_shot.max()), 4)}}), flush=True)
        for buf in (d_g, d_f, d_m, d_st, d_t, d_tf, d_e, d_c, d_st2, d_p):
            buf.free()


if __name__ == "__main__":
    main()
