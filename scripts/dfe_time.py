"""Time of the DFE kernels on one GPU, next to the host mirror (fbx/clifford_circuit.py, synthetic.restate_dfe_counts) on one core.

    python scripts/dfe_time.py [--reps 7] [--n 64] [--gates 1000] [--settings 1000000] [--simulate 1000:256:1000 1000:16:1000]

Part 1, the walks: `--settings` Monte Carlo process settings of a random circuit of `--gates` gates on `--n` qubits are written by
fbx_dfe_settings_dev (Philox draw and forward conjugation) and walked backwards by fbx_dfe_propagate_dev (two noise classes: one-
and two-qubit gates); the mirror is timed on at most 20 000 of the settings and scaled per setting.  Part 2, the simulation: a config
is settings:batch:shots on the first `settings` of them, with class errors and readout flips; the host is restate_dfe_counts on at
most 2000 units, scaled per unit.  The _dev forms are timed with device events around each of `reps` separate launches after one
warm-up, buffers resident; the rate is that of the median, `spread` is (slowest - fastest) / median.  One JSON line per result."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "forest-benchmarking_amd")]

from fbx import _lib, clifford_circuit as cc, synthetic  # noqa: E402

ONE_QUBIT, TWO_QUBIT = cc.GATE_NAMES[:12], cc.GATE_NAMES[12:]


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


def random_circuit(rng, n, n_gates):
    gates = []
    for _ in range(n_gates):
        if n >= 2 and rng.random() < 0.4:
            a, b = rng.choice(n, size=2, replace=False)
            gates.append((TWO_QUBIT[rng.integers(3)], (int(a), int(b))))
        else:
            gates.append((ONE_QUBIT[rng.integers(12)], (int(rng.integers(n)),)))
    return gates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--gates", type=int, default=1000)
    ap.add_argument("--settings", type=int, default=1000000)
    ap.add_argument("--simulate", nargs="*", default=["1000:256:1000", "1000:16:1000"])
    args = ap.parse_args()
    _lib.set_device(0)
    lib, DB = _lib.lib(), _lib.DeviceBuffer
    n, G, m, K, seed = args.n, args.gates, args.settings, 2, 2024
    gates = random_circuit(np.random.default_rng(1), n, G)
    words = cc.encode_gates(gates, n)                                    # validated here: the _dev forms take the words as they are
    classes = np.array([0 if len(q) == 1 else 1 for _, q in gates], dtype=np.uint8)
    d_gates, d_classes = DB.from_array(words), DB.from_array(classes)
    names = ("in_x", "in_z", "in_minus", "obs_x", "obs_z")
    d = {k: DB(m * 8) for k in names}
    d_sign, d_sigma, d_touches = DB(m), DB(m), DB(m * K * 4)
    ptrs = [d[k].ptr for k in names]

    # ---- part 1: settings and propagation
    sm, ss = summary(timed_dev(lambda: _lib.check(lib.fbx_dfe_settings_dev(
        n, _lib.KIND_PROCESS, m, seed, G, d_gates.ptr, m, *ptrs, d_sign.ptr)), args.reps))
    pm, ps = summary(timed_dev(lambda: _lib.check(lib.fbx_dfe_propagate_dev(
        n, G, d_gates.ptr, d_classes.ptr, K, m, *ptrs, d_sign.ptr, d_sigma.ptr, d_touches.ptr)), args.reps))
    mh = min(m, 20000)
    t = time.perf_counter()
    s = cc.restate_dfe_settings(n, "process", mh, seed, words)
    host_settings = (time.perf_counter() - t) / mh
    t = time.perf_counter()
    sigma, touches = cc.propagate_settings(words, n, s["in_x"], s["in_z"], s["in_minus"], s["obs_x"], s["obs_z"], classes, K)
    host_propagate = (time.perf_counter() - t) / mh
    assert np.array_equal(d_sigma.to_array(np.int8, (m,))[:mh], sigma)
    assert np.array_equal(d_touches.to_array(np.uint32, (m, K))[:mh], touches)
    assert np.array_equal(d["obs_x"].to_array(np.uint64, (m,))[:mh], s["obs_x"])
    for what, med, spread, host in (("dfe_settings", sm, ss, host_settings), ("dfe_propagate", pm, ps, host_propagate)):
        print(json.dumps({"what": what, "n_qubits": n, "gates": G, "settings": m, "classes": K, "reps": args.reps,
                          "dev": {"seconds": med, "spread": spread, "settings_per_s": round(m / med, 1),
                                  "gate_steps_per_s": round(m * G / med, 1)},
                          "host_mirror_settings_per_s": round(1.0 / host, 1), "ratio_to_host": round(host * m / med, 1)}), flush=True)

    # ---- part 2: the simulation
    rng = np.random.default_rng(2)
    for cfg in args.simulate:
        ms_, B, shots = (int(v) for v in cfg.split(":"))
        ms_ = min(ms_, m)
        p, f = rng.uniform(0.0, 0.002, size=(B, K)), rng.uniform(0.0, 0.03, size=(B, n))
        d_p, d_f = DB.from_array(p), DB.from_array(f)
        d_e, d_c, d_se, d_x, d_st = DB(B * ms_ * 8), DB(B * ms_ * 8), DB(B * ms_ * 8), DB(B * ms_ * 8), DB(B * 4)

        def simulate(exact=None):
            _lib.check(lib.fbx_dfe_simulate_dev(n, ms_, K, d_sigma.ptr, d_touches.ptr, d["obs_x"].ptr, d["obs_z"].ptr, d_sign.ptr, B,
                                                d_p.ptr, d_f.ptr, 0, shots, seed, 0, d_e.ptr, d_c.ptr, d_se.ptr, exact, d_st.ptr))
        med, spread = summary(timed_dev(simulate, args.reps))
        simulate(d_x.ptr); _lib.synchronize()
        assert not d_st.to_array(np.int32, (B,)).any()
        exact, e = d_x.to_array(np.float64, (B, ms_)), d_e.to_array(np.float64, (B, ms_))
        coefs = 1.0 - 2.0 * d_sign.to_array(np.uint8, (m,))[:ms_].astype(np.float64)
        mh = min(ms_, 2000)
        t = time.perf_counter()
        want = synthetic.restate_dfe_counts(exact[:1, :mh], coefs[:mh], shots, seed)[0]
        host = (time.perf_counter() - t) / mh
        assert np.array_equal(e[:1, :mh], want)
        print(json.dumps({"what": "dfe_simulate", "n_qubits": n, "gates": G, "settings": ms_, "batch": B, "shots": shots,
                          "units": B * ms_, "split": "lane" if B * ms_ >= 131072 else "wavefront", "reps": args.reps,
                          "dev": {"seconds": med, "spread": spread, "units_per_s": round(B * ms_ / med, 1),
                                  "shots_per_s": round(B * ms_ * shots / med, 1)},
                          "host_restate_units_per_s": round(1.0 / host, 1), "ratio_to_host": round(host * B * ms_ / med, 1)}), flush=True)
        for buf in (d_p, d_f, d_e, d_c, d_se, d_x, d_st):
            buf.free()
    for buf in list(d.values()) + [d_gates, d_classes, d_sign, d_sigma, d_touches]:
        buf.free()


if __name__ == "__main__":
    main()
