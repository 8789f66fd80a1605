"""Which quantum volume does a two-qubit gate error predict?  Widths 2..8 at ONE gate error: every gate of every model circuit is
followed, with that probability, by one of the 15 two-qubit Paulis on its pair (``fbx_qv_noisy_trajectories``: stochastic
Pauli-error trajectories, the Pauli folded into the gate's own pass over the state).

Per width the example prints
  * the ideal heavy-output probability of the circuits (``ideal_heavy_output_probability_batch``),
  * the NOISY heavy-output probability -- the mean over the trajectories of the weight on the ideal heavy set -- with its standard
    error (``noisy_heavy_output_probability_batch``), next to the crude estimate "all-or-nothing": a circuit with no error keeps
    its ideal probability, one with any error drops to 1/2, i.e. ``f h + (1 - f) / 2`` with ``f = (1 - p)^L``,
  * the heavy-output frequency of a simulated run (``simulate_noisy_heavy_output_counts_batch``: shots drawn on the device from
    the trajectory-mean distributions, optionally with readout flips) and its 2-sigma lower bound,
and then the quantum volume the run achieves (``extract_quantum_volume_from_results``) beside the largest width whose noisy
heavy-output probability is still above 2/3: the two agree up to the statistics of the run.

    python examples/quantum_volume_gate_noise.py [--gate-error 0.01] [--circuits 200] [--trajectories 200] [--shots 1000]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "forest-benchmarking_amd"))

from fbx import quantum_volume as qv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gate-error", type=float, default=0.01)
    ap.add_argument("--circuits", type=int, default=200)
    ap.add_argument("--trajectories", type=int, default=200)
    ap.add_argument("--shots", type=int, default=1000)
    ap.add_argument("--readout-flip", type=float, nargs=2, default=None, metavar=("P01", "P10"))
    ap.add_argument("--seed", type=int, default=11)
    args = ap.parse_args()
    p, depths = args.gate_error, list(range(2, 9))
    all_depths, all_heavy, all_shots = [], [], []
    predicted = 1
    still_above = True
    print(f"two-qubit gate error {p}: {args.circuits} circuits x {args.trajectories} trajectories x {args.shots} shots per width")
    for depth in depths:
        permutations, gates = qv.generate_abstract_qv_circuits_batch(depth, args.circuits, seed=args.seed + depth)
        L = depth * (depth // 2)
        ideal = qv.ideal_heavy_output_probability_batch(permutations, gates)
        noisy, err = qv.noisy_heavy_output_probability_batch(permutations, gates, p, args.trajectories, seed=args.seed + 100 * depth)
        flips = None if args.readout_flip is None else [list(args.readout_flip)] * depth
        counts, stats = qv.simulate_noisy_heavy_output_counts_batch(permutations, gates, args.shots, p, args.trajectories,
                                                                    readout_flip=flips, seed=args.seed + 100 * depth)
        f = (1.0 - p) ** L
        crude = f * ideal.mean() + (1.0 - f) / 2.0
        # standard error of the batch mean: the trajectories' own error and the spread between circuits
        batch_err = float(((err ** 2).mean() / args.circuits + noisy.var(ddof=1) / args.circuits) ** 0.5)
        print(f"  width {depth} ({L:2d} gates): ideal {ideal.mean():.4f}, noisy {noisy.mean():.4f} +- {batch_err:.4f} "
              f"(all-or-nothing estimate {crude:.4f}), simulated run {counts.sum() / (args.circuits * args.shots):.4f}")
        still_above = still_above and noisy.mean() > 2 / 3
        if still_above:
            predicted = depth
        all_depths += [depth] * args.circuits
        all_heavy += [int(c) for c in counts]
        all_shots += [args.shots] * args.circuits
    results = qv.get_prob_sample_heavy_by_depth(all_depths, all_heavy, all_shots)
    for depth in depths:
        est, lower = results[depth]
        print(f"  width {depth}: heavy-output frequency {est:.4f}, 2-sigma lower bound {lower:.4f} {'> 2/3' if lower > 2 / 3 else '<= 2/3'}")
    print(f"quantum volume achieved by the simulated run = {qv.extract_quantum_volume_from_results(results)}; "
          f"noisy heavy-output probability above 2/3 up to width {predicted}: 2^{predicted} = {2 ** predicted}")


if __name__ == "__main__":
    main()
