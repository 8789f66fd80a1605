"""Time of fbx_tomo_simulate_symmetrized and fbx_tomo_simulate_calibration on one GPU next to fbx_tomo_simulate_grouped at the
same total shots in the same run: the same design, grouping and truths, all in device-pointer form on resident buffers.

    python scripts/tomo_sim_symm_time.py [--reps 7] [--configs 2:1024:1000 2:65536:1000]

A config is n_qubits:batch:shots on the Pauli design of n qubits with its greedy grouping (two qubits: 540 settings in 324
groups, 15 calibrations).  Truths are Haar unitaries; the readout error of the symmetrized call is an asymmetric correlated
confusion matrix under exhaustive symmetrization (symm_type = -1: up to 2^n patterns of floor(shots / patterns) shots per
group), that of the grouped call independent flips; both write (expectations, counts).  Each call is timed with device events
around each of `reps` separate launches after two warm-ups of every call; the calls alternate, so that a drift of the clock meets
all of them; the time is the median, `spread` is (slowest - fastest) / median, and the ratio to the grouped call is reported
with its range over the repetitions.  No threshold is asserted.  One JSON line per configuration."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "forest-benchmarking_amd")]

from fbx import _lib, synthetic  # noqa: E402
from fbx.design import group_design, process_design  # noqa: E402
from fbx.operator_tools.superoperator_transformations import convert_batch  # noqa: E402
from fbx.readout import confusion_from_flips  # noqa: E402
from fbx.tomography import calibration_list  # noqa: E402


def summary(times):
    t = np.asarray(times)
    med = float(np.median(t))
    return round(med, 6), round(float((t.max() - t.min()) / med), 3)


def timed_alternating(launches, reps, warmups=2):
    """seconds per launch of every entry of `launches`, from the library's device timer around each of `reps` launches (after
    `warmups` untimed rounds); the entries take turns"""
    lib = _lib.lib()
    for _ in range(warmups):
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


def correlated_confusion(n, rng, weight=0.125):
    """(1 - weight) x a tensor product of asymmetric flips (about 3 % / 8 %) + weight x a random row-stochastic matrix"""
    d = 1 << n
    flips = np.stack([rng.uniform(0.02, 0.04, n), rng.uniform(0.06, 0.10, n)], axis=1)
    r = rng.random((d, d)) ** 3
    return (1.0 - weight) * confusion_from_flips(flips) + weight * r / r.sum(axis=1, keepdims=True), flips


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--configs", nargs="+", default=["2:1024:1000", "2:65536:1000"])
    args = ap.parse_args()
    _lib.set_device(0)
    lib, DB = _lib.lib(), _lib.DeviceBuffer
    for cfg in args.configs:
        n, B, shots = (int(x) for x in cfg.split(":"))
        design = process_design(n, "pauli")
        grouping = group_design(design)
        m, G, d = design.m, grouping.n_groups, 1 << n
        n_cal = calibration_list(design)[0].shape[0]
        us = np.array([synthetic.haar_unitary(d, np.random.RandomState(1000 + b)) for b in range(min(B, 16))])
        ptm = np.ascontiguousarray(convert_batch("kraus", "pauli_liouville", us[:, None]).real[np.arange(B) % len(us)])
        conf, flips = correlated_confusion(n, np.random.default_rng(n))
        d_t = DB.from_array(ptm)
        d_f = DB.from_array(np.ascontiguousarray(np.broadcast_to(flips, (B, n, 2))))
        d_cf = DB.from_array(np.ascontiguousarray(np.broadcast_to(conf, (B, d, d))))
        d_e, d_c, d_st = DB(B * m * 8), DB(B * m * 8), DB(B * 4)
        d_e2, d_c2, d_st2 = DB(B * m * 8), DB(B * m * 8), DB(B * 4)
        d_cm, d_cv, d_st3 = DB(B * n_cal * 8), DB(B * n_cal * 8), DB(B * 4)

        def symmetrized():
            _lib.check(lib.fbx_tomo_simulate_symmetrized_dev(design.handle, grouping.handle, B, d_t.ptr, d_cf.ptr, -1, shots, 1234, 0,
                                                             d_e.ptr, d_c.ptr, None, None, None, None, d_st.ptr))

        def grouped():
            _lib.check(lib.fbx_tomo_simulate_grouped_dev(design.handle, grouping.handle, B, d_t.ptr, shots, d_f.ptr, 1234, 0,
                                                         d_e2.ptr, d_c2.ptr, None, None, None, None, d_st2.ptr))

        def calibration():
            _lib.check(lib.fbx_tomo_simulate_calibration_dev(design.handle, B, d_cf.ptr, -1, shots, 1234, 0, d_cm.ptr, d_cv.ptr, None,
                                                             None, d_st3.ptr))
        ts, tg, tc = timed_alternating((symmetrized, grouped, calibration), args.reps)
        assert not any(buf.to_array(np.int32, (B,)).any() for buf in (d_st, d_st2, d_st3))
        (sm, ss), (gm, gs), (cm, cs) = summary(ts), summary(tg), summary(tc)
        ratios = np.asarray(ts) / np.asarray(tg)
        print(json.dumps({
            "what": "tomo_simulate_symmetrized", "n_qubits": n, "batch": B, "settings": m, "groups": G, "calibrations": n_cal,
            "shots": shots, "symm_type": -1, "reps": args.reps,
            "symmetrized_dev": {"seconds": sm, "spread": ss, "items_per_s": round(B / sm, 1)},
            "grouped_dev": {"seconds": gm, "spread": gs, "items_per_s": round(B / gm, 1),
                            "split": "lane" if n <= 3 and B * G >= 131072 else "wavefront"},
            "calibration_dev": {"seconds": cm, "spread": cs, "items_per_s": round(B / cm, 1)},
            "symmetrized_over_grouped": round(sm / gm, 4),
            "ratio_per_repetition": {"min": round(float(ratios.min()), 4), "max": round(float(ratios.max()), 4)}}), flush=True)
        for buf in (d_t, d_f, d_cf, d_e, d_c, d_st, d_e2, d_c2, d_st2, d_cm, d_cv, d_st3):
            buf.free()


if __name__ == "__main__":
    main()
