"""Time of fbx_tomo_simulate on one GPU, next to the PGDB reconstruction it feeds (fbx_pgdb_process on the very batch it wrote,
same run) and to synthetic.process_batch on one host core (the einsum plus one binomial call per item that the examples and timing
scripts drew their tomography data with).

    python scripts/tomo_sim_time.py [--reps 7] [--configs 2:1024:1000 2:65536:1000 1:64:1000000 3:256:1000] [--no-pgdb]

A config is n_qubits:batch:shots on the Pauli design of n qubits (540 settings for two qubits).  Truths are Haar unitaries; the
simulation runs with readout flips.  The _dev form is timed with device events around each of `reps` separate launches after one
warm-up, buffers resident; the rate is that of the median, `spread` is (slowest - fastest) / median.  The host baseline is timed
on at most 8 items and scaled per item.  One JSON line per configuration."""
import argparse
import ctypes as C
import json
import os
import sys
import time

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


def timed_dev(launch, reps):
    """seconds per launch from the library's device timer around each of `reps` launches (after one warm-up)"""
    lib = _lib.lib()
    launch(); _lib.synchronize()
    out = []
    ms = C.c_double(0.0)
    for _ in range(reps):
        _lib.check(lib.fbx_timer_begin())
        launch()
        _lib.check(lib.fbx_timer_end(C.byref(ms)))
        out.append(ms.value * 1e-3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--configs", nargs="+", default=["2:1024:1000", "2:65536:1000", "1:64:1000000", "3:256:1000"])
    ap.add_argument("--no-pgdb", action="store_true")
    args = ap.parse_args()
    _lib.set_device(0)
    lib, DB = _lib.lib(), _lib.DeviceBuffer
    for cfg in args.configs:
        n, B, shots = (int(x) for x in cfg.split(":"))
        design = process_design(n, "pauli")
        m, D = design.m, 4 ** n
        us = np.array([synthetic.haar_unitary(2 ** n, np.random.RandomState(1000 + b)) for b in range(min(B, 16))])
        ptm = np.ascontiguousarray(convert_batch("kraus", "pauli_liouville", us[:, None]).real[np.arange(B) % len(us)])
        flips = np.ascontiguousarray(np.broadcast_to(np.random.default_rng(n).uniform(0.0, 0.05, size=(n, 2)), (B, n, 2)))
        nb = min(B, 8)
        t = time.perf_counter()
        synthetic.process_batch(n, "pauli", nb, shots)
        host_per_item = (time.perf_counter() - t) / nb
        d_t, d_f = DB.from_array(ptm), DB.from_array(flips)
        d_e, d_c, d_st = DB(B * m * 8), DB(B * m * 8), DB(B * 4)
        sm, ss = summary(timed_dev(lambda: _lib.check(lib.fbx_tomo_simulate_dev(
            design.handle, B, d_t.ptr, shots, d_f.ptr, 1234, 0, d_e.ptr, d_c.ptr, None, None, d_st.ptr)), args.reps))
        assert not d_st.to_array(np.int32, (B,)).any()
        rec = {"what": "tomo_simulate", "n_qubits": n, "batch": B, "settings": m, "shots": shots, "reps": args.reps,
               "units": B * m, "split": "lane" if B * m >= 131072 else "wavefront",
               "simulate_dev": {"seconds": sm, "spread": ss, "items_per_s": round(B / sm, 1), "shots_per_s": round(B * m * shots / sm, 1)},
               "host_process_batch_items_per_s": round(1.0 / host_per_item, 2), "ratio_to_host": round(host_per_item * B / sm, 1)}
        if not args.no_pgdb:
            d_choi = DB(B * D * D * 16)
            pm, ps = summary(timed_dev(lambda: _lib.check(lib.fbx_pgdb_process_dev(
                design.handle, B, d_e.ptr, d_c.ptr, 1, _lib.MODE_CONVERGE, 0, d_choi.ptr, None, None, None, None, None)),
                min(args.reps, 3)))
            rec["pgdb_on_the_same_batch"] = {"seconds": pm, "spread": ps, "items_per_s": round(B / pm, 1)}
            rec["simulate_over_pgdb"] = round(sm / pm, 4)
            d_choi.free()
        print(json.dumps(rec), flush=True)
        for buf in (d_t, d_f, d_e, d_c, d_st):
            buf.free()


if __name__ == "__main__":
    main()
