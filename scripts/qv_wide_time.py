"""Circuits per second of fbx_qv_heavy_outputs_wide_dev (widths 14..26: the state in HBM, a tile at a time in LDS) on one GPU,
against the numpy restatement of collect_heavy_outputs (tests/qv_cases.py) on one host core in the same run.

    python scripts/qv_wide_time.py [--widths 14 16 18 20 22 24] [--tile-bits 12 13] [--reps 5] [--baseline-max-width 20]
                                   [--log2-amplitudes 25] [--workspace-mib 128 ...]

Per (width, tile_bits, with / without probs_out): the _dev form, buffers resident, timed with device events around `reps`
separate calls after one warm-up; the rate is that of the median time, `spread` is (slowest - fastest) / median.  The batch is
max(1, 2^(log2_amplitudes - width)) circuits (2^25 amplitudes = 512 MiB of state by default), built from 4 distinct ones, reference
pairing; every --workspace-mib value is set as the option "qv_wide_workspace_mib" in turn (default: the library's), which decides
into how many chunks the batch is cut.  `passes_per_circuit` comes from
plan_wide_passes (the numpy mirror of the device planner).  `effective_bytes` counts what the kernels move per circuit: passes x
32 B x 2^n (a tile is read and written once per pass), 24 B x 2^n for the probabilities, 8 B x 2^n for each radix-select round the
circuit's distribution needs (from the first bit in which its smallest and largest pattern differ, 8 bits a round) and 8 B x 2^n
each for the rank-N/2 pass and the mask pass; `fraction_of_copy_rate` relates it to the 6.29 TB/s a plain copy reaches on this
part.  Above --baseline-max-width the restatement is timed on the first two layers and scaled by the gate count (its cost per
gate does not depend on the gate).  One JSON line per configuration."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "forest-benchmarking_amd"), os.path.join(ROOT, "tests")]

import qv_cases as qc  # noqa: E402
from fbx import _lib, quantum_volume as qv  # noqa: E402

COPY_RATE = 6.29e12     # bytes / s: measured rate of a plain device copy on the MI355X


def summary(times):
    t = np.asarray(times)
    med = float(np.median(t))
    return med, round(float((t.max() - t.min()) / med), 3)


def timed_dev(launch, reps):
    """seconds per call from the library's device timer around each of `reps` calls (after one warm-up)"""
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


def draw(n, count, seed):
    rng = np.random.default_rng(seed)
    perms = np.stack([np.stack([rng.permutation(n) for _ in range(n)]) for _ in range(count)])
    z = rng.standard_normal((count, n, n // 2, 4, 4)) + 1j * rng.standard_normal((count, n, n // 2, 4, 4))
    q, r = np.linalg.qr(z)
    d = np.diagonal(r, axis1=-2, axis2=-1)
    return perms, q * (d / np.abs(d))[..., None, :]


def baseline(n, perms, gates, full):
    """(seconds per circuit of the numpy restatement on this host, one core; whether it was scaled from two layers)"""
    pairs, flat = qc.pairs_of(perms[0]), gates[0].reshape(-1, 4, 4)
    L = len(pairs)
    k = L if full else 2 * (n // 2)
    t = time.perf_counter()
    p = qc.simulate(n, pairs[:k], flat[:k])
    t_gates = (time.perf_counter() - t) * L / k
    t = time.perf_counter()
    med = 0.5 * np.sum(np.partition(p, [len(p) // 2 - 1, len(p) // 2])[len(p) // 2 - 1:len(p) // 2 + 1])
    np.flatnonzero(p > med)
    return t_gates + (time.perf_counter() - t), not full


def select_rounds(probs):
    """radix-select rounds per circuit: from the highest bit in which the smallest and the largest pattern differ, 8 bits a round"""
    x = np.ascontiguousarray(probs).view(np.uint64)
    diff = x.min(axis=1) ^ x.max(axis=1)
    return np.asarray([0 if d == 0 else -(-int(d).bit_length() // 8) for d in diff])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", type=int, nargs="+", default=[14, 16, 18, 20, 22, 24])
    ap.add_argument("--tile-bits", type=int, nargs="+", default=[12, 13])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-max-width", type=int, default=20)
    ap.add_argument("--log2-amplitudes", type=int, default=25)
    ap.add_argument("--workspace-mib", type=float, nargs="+", default=None)
    args = ap.parse_args()
    _lib.set_device(0)
    lib = _lib.lib()
    for n in args.widths:
        L, N, W = n * (n // 2), 1 << n, (1 << n) // 64
        B = 1 << max(0, args.log2_amplitudes - n)
        perms, gates = draw(n, min(B, 4), seed=n)
        base_s, scaled = baseline(n, perms, gates, n <= args.baseline_max_width)
        sel = np.arange(B) % len(perms)
        pairs = np.ascontiguousarray(qv.layer_pairs(perms[sel]).reshape(B, L, 2))
        flat = np.ascontiguousarray(gates[sel].reshape(B, L, 4, 4))
        d_pairs, d_gates = _lib.DeviceBuffer.from_array(pairs), _lib.DeviceBuffer.from_array(flat)
        d_p, d_m, d_k = _lib.DeviceBuffer(B * N * 8), _lib.DeviceBuffer(B * 8), _lib.DeviceBuffer(B * W * 8)
        d_hp, d_hc = _lib.DeviceBuffer(B * 8), _lib.DeviceBuffer(B * 4)
        rounds = None
        caps = args.workspace_mib or [_lib.get_option("qv_wide_workspace_mib")]
        for cap, tile_bits in ((c, t) for c in caps for t in args.tile_bits):
            _lib.set_option("qv_wide_workspace_mib", cap)
            passes = qv.plan_wide_passes(n, pairs[:len(perms)], tile_bits)[0][sel]
            for with_probs in (True, False):
                dev = timed_dev(lambda: _lib.check(lib.fbx_qv_heavy_outputs_wide_dev(
                    n, B, L, d_pairs.ptr, d_gates.ptr, tile_bits, d_p.ptr if with_probs else None, d_m.ptr, d_k.ptr, d_hp.ptr,
                    d_hc.ptr)), args.reps)
                if with_probs and rounds is None:
                    rounds = select_rounds(d_p.to_array(np.float64, (B, N)))
                dm, ds = summary(dev)
                line = {"what": "heavy_outputs_wide", "n_qubits": n, "gates": L, "batch": B, "tile_bits": tile_bits,
                        "workspace_mib": cap, "probs_out": with_probs, "reps": args.reps, "passes_per_circuit": round(float(passes.mean()), 2),
                        "dev_form": {"circuits_per_s": round(B / dm, 2), "seconds": round(dm, 6), "spread": ds},
                        "baseline_numpy_circuits_per_s": round(1.0 / base_s, 3), "baseline_scaled_from_two_layers": scaled,
                        "ratio_dev_form": round(base_s * B / dm, 1)}
                if rounds is not None:
                    moved = float((passes * 32.0 + 24.0 + 8.0 * rounds + 16.0).sum()) * N
                    line.update({"select_rounds_per_circuit": round(float(rounds.mean()), 2), "effective_bytes": moved,
                                 "effective_bytes_per_s": round(moved / dm, 1), "fraction_of_copy_rate": round(moved / dm / COPY_RATE, 4)})
                print(json.dumps(line), flush=True)
        for buf in (d_pairs, d_gates, d_p, d_m, d_k, d_hp, d_hc):
            buf.free()
        _lib.release_workspace()


if __name__ == "__main__":
    main()
