"""Quantum volume from measured bitstrings, with the reference's names (forest/benchmarking/quantum_volume.py).

circuits -> ideal heavy sets (GPU) -> bitstrings (here: synthetic shots from the ideal distribution mixed with the uniform one; on
a device: ``qc.run`` of the compiled model circuits) -> heavy counts (GPU) -> ``get_prob_sample_heavy_by_depth`` ->
``extract_quantum_volume_from_results``, for widths 2..8.

    python examples/quantum_volume_from_shots.py [--circuits 200] [--shots 1000]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "forest-benchmarking_amd"))

from fbx import quantum_volume as qv, synthetic  # noqa: E402


def measure(depths, num_circuits, num_shots, depolarizing_per_layer, seed):
    """{depth: (heavy-output frequency, 2-sigma lower bound)} for a simulated device whose state is depolarised by
    ``depolarizing_per_layer`` per layer of a model circuit"""
    all_depths, all_heavy, all_shots = [], [], []
    ideal = {}
    for depth in depths:
        permutations, gates = qv.generate_abstract_qv_circuits_batch(depth, num_circuits, seed=seed + depth)
        heavy, probabilities, stats = qv.collect_heavy_outputs_batch(permutations, gates, return_probabilities=True, return_stats=True)
        ideal[depth] = float(stats["heavy_prob"].mean())
        noise = 1.0 - (1.0 - depolarizing_per_layer) ** depth
        bitarrays = synthetic.qv_shots(probabilities, num_shots, depolarizing=noise, seed=seed + 100 * depth)
        counts = qv.count_heavy_hitters_sampled_batch(bitarrays, heavy)
        # (the reference's generator form, one circuit at a time, gives the same numbers:
        #  qv.count_heavy_hitters_sampled(iter(bitarrays), (np.flatnonzero(h) for h in heavy)))
        all_depths += [depth] * num_circuits
        all_heavy += [int(c) for c in counts]
        all_shots += [num_shots] * num_circuits
    return qv.get_prob_sample_heavy_by_depth(all_depths, all_heavy, all_shots), ideal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--circuits", type=int, default=200)
    ap.add_argument("--shots", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=11)
    args = ap.parse_args()
    depths = list(range(2, 9))
    for label, noise in (("noiseless", 0.0), ("2 % depolarizing per layer", 0.02), ("6 % depolarizing per layer", 0.06)):
        results, ideal = measure(depths, args.circuits, args.shots, noise, args.seed)
        print(f"--- {label}: {args.circuits} circuits x {args.shots} shots per depth")
        for depth in depths:
            est, lower = results[depth]
            print(f"  depth {depth}: heavy-output frequency {est:.4f} (ideal {ideal[depth]:.4f}), 2-sigma lower bound {lower:.4f} "
                  f"{'> 2/3' if lower > 2 / 3 else '<= 2/3'}")
        print(f"  quantum volume = {qv.extract_quantum_volume_from_results(results)}")


if __name__ == "__main__":
    main()
