"""A simulated quantum-volume run that never leaves the device: model circuits -> ideal output distributions -> noisy measured
bitstrings -> heavy counts (``quantum_volume.simulate_heavy_output_counts_batch``), then the reference's statistics
(``get_prob_sample_heavy_by_depth``, ``extract_quantum_volume_from_results``), for widths 2..10, and two wide rungs (widths 14 and
16, a few circuits each) through ``simulate_heavy_output_counts_wide_batch``, whose table of prefix sums lives in device memory.

The simulated device depolarises its state by a fixed amount per layer of a model circuit and misreads every qubit with a small,
asymmetric probability.  Under depolarizing alone a shot of circuit b is heavy with probability
``(1 - lambda) heavy_prob_b + lambda heavy_count_b / 2^n`` -- printed next to the measured frequency, so the closed form and the
sampler can be compared by eye.  The counterpart with shots drawn on the host: examples/quantum_volume_from_shots.py.

    python examples/quantum_volume_simulated.py [--circuits 200] [--shots 1000] [--wide-circuits 8]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "forest-benchmarking_amd"))

from fbx import quantum_volume as qv  # noqa: E402


def measure(depths, num_circuits, num_shots, depolarizing_per_layer, readout_flip, seed, simulate=None):
    """({depth: (heavy-output frequency, 2-sigma lower bound)}, {depth: expected frequency under the depolarizing alone})"""
    simulate = simulate or qv.simulate_heavy_output_counts_batch
    all_depths, all_heavy, all_shots = [], [], []
    expected = {}
    for depth in depths:
        permutations, gates = qv.generate_abstract_qv_circuits_batch(depth, num_circuits, seed=seed + depth)
        noise = 1.0 - (1.0 - depolarizing_per_layer) ** depth
        flips = None if readout_flip is None else np.broadcast_to(np.asarray(readout_flip, dtype=float), (depth, 2))
        counts, stats = simulate(permutations, gates, num_shots, depolarizing=noise, readout_flip=flips, seed=seed + 100 * depth)
        expected[depth] = float(((1.0 - noise) * stats["heavy_prob"] + noise * stats["heavy_count"] / 2.0 ** depth).mean())
        all_depths += [depth] * num_circuits
        all_heavy += [int(c) for c in counts]
        all_shots += [num_shots] * num_circuits
    return qv.get_prob_sample_heavy_by_depth(all_depths, all_heavy, all_shots), expected


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--circuits", type=int, default=200)
    ap.add_argument("--shots", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--wide-circuits", type=int, default=8)
    args = ap.parse_args()
    depths = list(range(2, 11))
    for label, noise, flips in (("noiseless", 0.0, None), ("2 % depolarizing per layer", 0.02, None),
                                ("2 % depolarizing per layer, readout errors 1 % (0 -> 1) and 3 % (1 -> 0)", 0.02, (0.01, 0.03)),
                                ("6 % depolarizing per layer", 0.06, None)):
        results, expected = measure(depths, args.circuits, args.shots, noise, flips, args.seed)
        print(f"--- {label}: {args.circuits} circuits x {args.shots} shots per depth")
        for depth in depths:
            est, lower = results[depth]
            print(f"  depth {depth}: heavy-output frequency {est:.4f} (depolarizing alone: {expected[depth]:.4f}), 2-sigma lower bound "
                  f"{lower:.4f} {'> 2/3' if lower > 2 / 3 else '<= 2/3'}")
        print(f"  quantum volume = {qv.extract_quantum_volume_from_results(results)}")
    # the same run above width 13 (one function for widths 2..26): few circuits, so the bounds are loose
    wide = [14, 16]
    results, expected = measure(wide, args.wide_circuits, args.shots, 0.005, (0.01, 0.03), args.seed,
                                simulate=qv.simulate_heavy_output_counts_wide_batch)
    print(f"--- wide rungs, 0.5 % depolarizing per layer, readout errors 1 % and 3 %: {args.wide_circuits} circuits x {args.shots} shots")
    for depth in wide:
        est, lower = results[depth]
        print(f"  depth {depth}: heavy-output frequency {est:.4f} (depolarizing alone: {expected[depth]:.4f}), 2-sigma lower bound "
              f"{lower:.4f} {'> 2/3' if lower > 2 / 3 else '<= 2/3'}")


if __name__ == "__main__":
    main()
