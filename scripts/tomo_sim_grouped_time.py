"""Time of fbx_tomo_simulate_grouped on one GPU next to fbx_tomo_simulate in the same run: the same design, truths, flips and
shots, both in device-pointer form on resident buffers.

    python scripts/tomo_sim_grouped_time.py [--reps 7] [--configs 2:1024:1000 2:65536:1000]

A config is n_qubits:batch:shots on the Pauli design of n qubits with its greedy grouping (two qubits: 540 settings in 324
groups).  Truths are Haar unitaries; both simulations run with readout flips and write (expectations, counts).  Each call is
timed with device events around each of `reps` separate launches after one warm-up; the two calls alternate, so that a drift of
the clock meets both; the time is the median, `spread` is (slowest - fastest) / median.  One JSON line per configuration."""
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
        m, G = design.m, grouping.n_groups
        us = np.array([synthetic.haar_unitary(2 ** n, np.random.RandomState(1000 + b)) for b in range(min(B, 16))])
        ptm = np.ascontiguousarray(convert_batch("kraus", "pauli_liouville", us[:, None]).real[np.arange(B) % len(us)])
        flips = np.ascontiguousarray(np.broadcast_to(np.random.default_rng(n).uniform(0.0, 0.05, size=(n, 2)), (B, n, 2)))
        d_t, d_f = DB.from_array(ptm), DB.from_array(flips)
        d_e, d_c, d_st = DB(B * m * 8), DB(B * m * 8), DB(B * 4)
        d_e2, d_c2, d_st2 = DB(B * m * 8), DB(B * m * 8), DB(B * 4)

        def grouped():
            _lib.check(lib.fbx_tomo_simulate_grouped_dev(design.handle, grouping.handle, B, d_t.ptr, shots, d_f.ptr, 1234, 0,
                                                         d_e.ptr, d_c.ptr, None, None, None, None, d_st.ptr))

        def ungrouped():
            _lib.check(lib.fbx_tomo_simulate_dev(design.handle, B, d_t.ptr, shots, d_f.ptr, 1234, 0, d_e2.ptr, d_c2.ptr, None, None,
                                                 d_st2.ptr))
        tg, tu = timed_alternating((grouped, ungrouped), args.reps)
        assert not d_st.to_array(np.int32, (B,)).any() and not d_st2.to_array(np.int32, (B,)).any()
        (gm, gs), (um, us_) = summary(tg), summary(tu)
        ratios = np.asarray(tg) / np.asarray(tu)
        print(json.dumps({
            "what": "tomo_simulate_grouped", "n_qubits": n, "batch": B, "settings": m, "groups": G, "shots": shots, "reps": args.reps,
            "grouped_dev": {"seconds": gm, "spread": gs, "items_per_s": round(B / gm, 1), "words_per_s": round(B * G * shots / gm, 1)},
            "ungrouped_dev": {"seconds": um, "spread": us_, "items_per_s": round(B / um, 1), "words_per_s": round(B * m * shots / um, 1),
                              "split": "lane" if B * m >= 131072 else "wavefront"},
            "grouped_over_ungrouped": round(gm / um, 4),
            "ratio_per_repetition": {"min": round(float(ratios.min()), 4), "max": round(float(ratios.max()), 4)}}), flush=True)
        for buf in (d_t, d_f, d_e, d_c, d_st, d_e2, d_c2, d_st2):
            buf.free()


if __name__ == "__main__":
    main()
