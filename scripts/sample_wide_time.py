"""Shots per second of fbx_sample_bitstrings_wide (widths 14..26) on one GPU, its table passes as bytes moved per second, numpy's
Generator.choice on one host core for the same distribution, and the sampler's share of a resident quantum-volume run.

    python scripts/sample_wide_time.py [--widths 14 16 18 20 24] [--reps 7] [--prob-mib 512] [--out FILE]

Per width, two shot regimes, each with and without readout flips, the _dev form on resident buffers, device events around each of
`reps` launches after one warm-up (median; `spread` is (slowest - fastest) / median):
  * "many": 10^3 shots per item, as many items as make `--prob-mib` MiB of probabilities per call;
  * "one":  10^6 shots of one item.
The table passes (1-5 of csrc/fbx_sample_wide.hip) and the draw are reported separately: `table` is the time of the same call with
ONE shot per item (passes 1-5 and a draw launch that loads the coarse tables and draws one shot each), `draw` the difference to the
full call.  Bytes moved by the table passes, counted from the code: p read twice (totals, scan), the table written (scan), read and
written (apply) = 40 B x 2^n per item, plus 40 B per 4096 entries of block sums and offsets; the yardstick is the 6.29 TB/s copy
rate of DESIGN.md.  Distributions are Porter-Thomas-like (squared moduli of complex normals) with depolarizing 0.1.
For the "many" shape the ideal distributions of as many model circuits are also computed on the device
(fbx_qv_heavy_outputs_wide_dev, reference pairing) and sampled, and the sampler's share of the two together is reported.
One JSON line per configuration; with --out they are appended to that file too."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "forest-benchmarking_amd")]

from fbx import _lib, quantum_volume as qv  # noqa: E402

COPY_RATE = 6.29e12    # bytes / s, the measured copy rate DESIGN.md uses as its yardstick


def summary(times):
    t = np.asarray(times)
    med = float(np.median(t))
    return med, round(float((t.max() - t.min()) / med), 3)


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


def table_bytes(n, B):
    return B * (40 * (1 << n) + 40 * ((1 << n) // 4096))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", type=int, nargs="+", default=[14, 16, 18, 20, 24])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--prob-mib", type=int, default=512)
    ap.add_argument("--no-circuits", action="store_true", help="skip the share of the resident quantum-volume run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.set_device(0)
    lib = _lib.lib()
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n"); sink.flush()

    emit({"what": "setup", "device": _lib.device_name()[0], "workspace_mib": _lib.get_option("sample_wide_workspace_mib"),
          "reps": args.reps, "prob_mib": args.prob_mib})
    for n in args.widths:
        N = 1 << n
        rng = np.random.default_rng([n, 4343])
        many = max(1, (args.prob_mib << 20) // (8 * N))
        rows = min(many, 4)
        z = rng.standard_normal((rows, N)) + 1j * rng.standard_normal((rows, N))
        base = np.abs(z) ** 2
        del z
        # the host baseline: one Generator.choice per record on one core, on the distribution the device samples
        w = 0.9 * base[0] + 0.1 * base[0].sum() / N
        w /= w.sum()
        host = {}
        for shots in (1000, 1000000):
            t = time.perf_counter()
            np.random.default_rng(1).choice(N, size=shots, p=w)
            host[shots] = shots / (time.perf_counter() - t)
        for kind, B, shots in (("many", many, 1000), ("one", 1, 1000000)):
            p = np.ascontiguousarray(base[np.arange(B) % rows])
            lam = np.full(B, 0.1)
            flips = np.ascontiguousarray(np.broadcast_to(rng.uniform(0.0, 0.05, size=(n, 2)), (B, n, 2)))
            nbytes = B * shots * n
            DB = _lib.DeviceBuffer
            d_p, d_lam, d_flips = DB.from_array(p), DB.from_array(lam), DB.from_array(flips)
            del p
            d_bits, d_status = DB(nbytes), DB(4 * B)

            def call(s, f):
                _lib.check(lib.fbx_sample_bitstrings_wide_dev(n, B, s, d_p.ptr, d_lam.ptr, d_flips.ptr if f else None, 1234, 0,
                                                              d_bits.ptr, d_status.ptr))
            tm, ts = summary(timed_dev(lambda: call(1, False), args.reps))
            for with_flips in (False, True):
                fm, fs = summary(timed_dev(lambda: call(shots, with_flips), args.reps))
                emit({"what": "sample_bitstrings_wide", "n_qubits": n, "shape": kind, "batch": B, "shots": shots, "flips": with_flips,
                      "seconds": round(fm, 6), "spread": fs, "shots_per_s": round(B * shots / fm, 1),
                      "output_bytes_per_s": round(nbytes / fm, 1),
                      "table_seconds": round(tm, 6), "table_spread": ts, "table_bytes": table_bytes(n, B),
                      "table_bytes_per_s": round(table_bytes(n, B) / tm, 1),
                      "table_fraction_of_copy_rate": round(table_bytes(n, B) / tm / COPY_RATE, 4),
                      "draw_seconds": round(fm - tm, 6), "draw_shots_per_s": round(B * shots / max(fm - tm, 1e-9), 1),
                      "numpy_choice_shots_per_s_one_core": round(host[shots], 1), "ratio_to_numpy_choice": round(B * shots / fm / host[shots], 1)})
            assert not d_status.to_array(np.int32, (B,)).any()
            for buf in (d_p, d_lam, d_flips, d_bits, d_status):
                buf.free()
        if args.no_circuits:
            continue
        # the sampler's share of a resident run: ideal distributions of `many` model circuits, then 10^3 noisy shots of each
        B, shots = many, 1000
        perms, gates = qv.generate_abstract_qv_circuits_batch(n, min(B, 16), seed=5)
        L = n * (n // 2)
        pairs = np.ascontiguousarray(qv.layer_pairs(perms, "reference").reshape(-1, L, 2)[np.arange(B) % len(perms)])
        flat = np.ascontiguousarray(gates.reshape(-1, L, 4, 4)[np.arange(B) % len(perms)])
        DB = _lib.DeviceBuffer
        d_pairs, d_gates, d_lam = DB.from_array(pairs), DB.from_array(flat), DB.from_array(np.full(B, 0.1))
        d_probs, d_mask, d_hp, d_hc = DB(8 * B * N), DB(8 * B * (N // 64)), DB(8 * B), DB(4 * B)
        d_bits, d_status, d_counts = DB(B * shots * n), DB(4 * B), DB(8 * B)
        hm, hs = summary(timed_dev(lambda: _lib.check(lib.fbx_qv_heavy_outputs_wide_dev(
            n, B, L, d_pairs.ptr, d_gates.ptr, 0, d_probs.ptr, None, d_mask.ptr, d_hp.ptr, d_hc.ptr)), args.reps))
        sm, ss = summary(timed_dev(lambda: _lib.check(lib.fbx_sample_bitstrings_wide_dev(
            n, B, shots, d_probs.ptr, d_lam.ptr, None, 1234, 0, d_bits.ptr, d_status.ptr)), args.reps))
        cm, cs = summary(timed_dev(lambda: _lib.check(lib.fbx_qv_count_heavy_wide_dev(
            n, B, shots, d_bits.ptr, d_mask.ptr, d_counts.ptr)), args.reps))
        assert not d_status.to_array(np.int32, (B,)).any()
        emit({"what": "resident_qv_run", "n_qubits": n, "circuits": B, "shots": shots,
              "heavy_outputs_seconds": round(hm, 6), "heavy_outputs_spread": hs, "sample_seconds": round(sm, 6), "sample_spread": ss,
              "count_seconds": round(cm, 6), "count_spread": cs,
              "sampler_over_heavy_outputs": round(sm / hm, 4), "sampler_share_of_run": round(sm / (hm + sm + cm), 4)})
        for buf in (d_pairs, d_gates, d_lam, d_probs, d_mask, d_hp, d_hc, d_bits, d_status, d_counts):
            buf.free()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
