"""A/B of two builds of the library on the four readers of shot records (fbx_shots, fbx_histogram, fbx_rpe, fbx_qvolume), on ONE box:
the builds alternate, a fresh process per build and round, the same inputs in every process.

    python scripts/ab_shot_records.py libA.so libB.so [--rounds 5] [--reps 7] [--out raw.jsonl] [--summary summary.txt] [--no-bench]

(names inside forest-benchmarking_amd/; libA is the parent.)  A process times, with the sizes of the scripts it is named after and
their method (buffers resident, one warm-up, device events around each of `reps` launches, the median):
    shots_time      fbx_shots_to_moments_dev, the nine shapes of scripts/shots_time.py
    histogram_time  fbx_bit_histogram_dev, the twelve configurations of scripts/histogram_time.py
    qv_time         fbx_qv_count_heavy_dev, widths 2..13 x (4096 circuits x 1000 shots, 100 x 100000): the counting part of scripts/qv_time.py
    rpe_time        fbx_rpe_from_shots_dev, scripts/rpe_time.py's default without and with --zcol
and, unless --no-bench, `bench.py --gpus 1 --steps 10 --warmup 2 --workload shots` runs once per build and round (ms_per_step of
shots_2q).  Values are milliseconds.  Summary, one line per metric: the parent's min..max over the rounds, that range widened on
both sides by the parent's own spread (max - min), and where the other build's median lies.  A process that fails ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import ctypes as C, json, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "forest-benchmarking_amd"))
import numpy as np
from fbx import _lib
REPS = int(sys.argv[2])
_lib.set_device(0)
lib, DB = _lib.lib(), _lib.DeviceBuffer
def bits01(rng, shape):
    return (np.frombuffer(rng.bytes(int(np.prod(shape))), dtype=np.uint8) & 1).reshape(shape)
def timed(launch):
    launch(); _lib.synchronize()
    ms, out = C.c_double(0.0), []
    for _ in range(REPS):
        _lib.check(lib.fbx_timer_begin())
        launch()
        _lib.check(lib.fbx_timer_end(C.byref(ms)))
        out.append(ms.value)
    return float(np.median(out))
def report(metric, value, bufs):
    print(json.dumps({"metric": metric, "ms": value}), flush=True)
    for b in bufs:
        if b is not None:
            b.free()
rng = np.random.default_rng(1)
for n, S, shots in ((2, 540 * 256, 1000), (2, 540 * 64, 10000), (3, 4032 * 16, 1000), (3, 4032 * 16, 1003), (8, 65536, 1000),
                    (5, 65536, 1000), (6, 65536, 1000), (7, 32768, 1001), (9, 32768, 1000)):
    mask = rng.integers(0, 2, size=(S, n), dtype=np.uint8); mask[:, 0] |= (mask.sum(1) == 0)
    d_bits, d_mask, d_mean, d_var = DB.from_array(bits01(rng, (S, shots, n))), DB.from_array(mask), DB(S * 8), DB(S * 8)
    t = timed(lambda: _lib.check(lib.fbx_shots_to_moments_dev(n, S, shots, d_bits.ptr, d_mask.ptr, None, 0, d_mean.ptr, d_var.ptr)))
    report(f"shots_time n={n} settings={S} shots={shots}", t, (d_bits, d_mask, d_mean, d_var))
for kind, k in ((0, 1), (0, 2), (0, 3), (0, 10), (1, 5), (1, 17)):
    for shots, B in ((1000, 4096), (10 ** 6, 64)):
        r = np.random.default_rng([kind, k, shots])
        bits = r.integers(0, 2, size=(B, shots, k), dtype=np.uint8)
        bins = (1 << k) if kind == 0 else k + 1
        d_bits, d_counts = DB.from_array(bits), DB(B * bins * 8)
        d_exp = DB.from_array(r.integers(0, 2, size=(B, k), dtype=np.uint8)) if kind == 1 else None
        t = timed(lambda: _lib.check(lib.fbx_bit_histogram_dev(k, B, shots, d_bits.ptr, k, None, 1, d_exp.ptr if d_exp else None, kind,
                                                               d_counts.ptr)))
        assert (d_counts.to_array(np.int64, (B, bins)).sum(axis=1) == shots).all()
        report(f"histogram_time {'joint' if kind == 0 else 'weight'} k={k} shots={shots} batch={B}", t, (d_bits, d_counts, d_exp))
for n in range(2, 14):
    W = max(1, (1 << n) // 64)
    for shots in (1000, 100000):
        B = 100 if shots >= 100000 else 4096
        r = np.random.default_rng([n, shots])
        mask = r.integers(0, 2 ** 63, size=(B, W), dtype=np.uint64)
        d_bits, d_mask, d_c = DB.from_array(bits01(r, (B, shots, n))), DB.from_array(mask), DB(B * 8)
        t = timed(lambda: _lib.check(lib.fbx_qv_count_heavy_dev(n, B, shots, d_bits.ptr, d_mask.ptr, d_c.ptr)))
        report(f"qv_time count_heavy n={n} shots={shots} batch={B}", t, (d_bits, d_mask, d_c))
B, K, shots, n = 100000, 10, 500, 2
r = np.random.default_rng(0)
depth, phases, bits = 2.0 ** np.arange(K), r.uniform(0, 2 * np.pi, 64), []
for fn in (np.cos, np.sin):
    b = r.integers(0, 2, size=(64, K, shots, n), dtype=np.uint8)
    b[..., 0] = r.random((64, K, shots)) < (1 - 0.9 * fn(depth[None, :, None] * phases[:, None, None])) / 2
    bits.append(np.ascontiguousarray(b[np.arange(B) % 64]))
d_x, d_y, d_phase, d_depth = DB.from_array(bits[0]), DB.from_array(bits[1]), DB(B * 8), DB(B * 4)
for zcol in (-1, 1):
    t = timed(lambda: _lib.check(lib.fbx_rpe_from_shots_dev(n, B, K, shots, d_x.ptr, d_y.ptr, 0, zcol, 0, d_phase.ptr, d_depth.ptr, None,
                                                            None)))
    report(f"rpe_time from_shots batch={B} depths={K} shots={shots} n={n} zcol={zcol}", t, ())
'''


def run(cmd, lib, timeout):
    env = dict(os.environ, FBX_LIBRARY=os.path.join(ROOT, "forest-benchmarking_amd", lib))
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    if r.returncode != 0:                          # a build that failed is not followed by another run on the same device
        sys.exit(f"{lib}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--summary", default=None)
    ap.add_argument("--no-bench", action="store_true")
    args = ap.parse_args()
    values = {lib: {} for lib in args.libs}        # lib -> metric -> one value per round
    for rnd in range(args.rounds):
        for lib in args.libs:
            for line in run([sys.executable, "-c", CHILD, ROOT, str(args.reps)], lib, 600).splitlines():
                if line.startswith("{"):
                    rec = json.loads(line)
                    values[lib].setdefault(rec["metric"], []).append(rec["ms"])
            if not args.no_bench:
                out = run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "2", "--workload",
                           "shots"], lib, 600)
                rec = json.loads([x for x in out.splitlines() if x.startswith("{")][-1])     # the headline: shots_2q as the primary line
                assert rec["metric"].startswith("shots -> observable moments"), rec["metric"]
                values[lib].setdefault("bench shots_2q ms_per_step", []).append(rec["ms_per_step"])
            print(f"round {rnd + 1} {lib}: {len(values[lib])} metrics", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for lib in args.libs:
                for metric, v in values[lib].items():
                    f.write(json.dumps({"lib": lib, "metric": metric, "ms": v}) + "\n")
    a, b = args.libs
    text = [f"{'metric (ms)':62s} {a + ' min..max':>22s} {'margin':>22s} {b + ' median':>14s}  verdict"]
    outside = 0
    for metric, pa in values[a].items():
        pb = sorted(values[b][metric])
        med = pb[len(pb) // 2] if len(pb) % 2 else 0.5 * (pb[len(pb) // 2 - 1] + pb[len(pb) // 2])
        lo, hi = min(pa), max(pa)
        spread = hi - lo
        verdict = "inside" if lo - spread <= med <= hi + spread else "faster" if med < lo - spread else "SLOWER"
        outside += verdict == "SLOWER"
        text.append(f"{metric:62s} {lo:10.4f}..{hi:<10.4f} {lo - spread:10.4f}..{hi + spread:<10.4f} {med:14.4f}  {verdict}")
    text.append(f"{outside} metric(s) slower than the margin allows")
    print("\n".join(text))
    if args.summary:
        with open(args.summary, "w") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
