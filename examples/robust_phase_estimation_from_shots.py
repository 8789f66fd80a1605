"""Robust phase estimation from measured bitstrings, with the reference's names (forest/benchmarking/robust_phase_estimation.py).

A known RZ(angle) on every qubit of a (simulated) chip: bitstrings of the X and the Y basis after 2^j applications (here: synthetic
shots with a visibility that decays with depth; on a device: the results of ``generate_rpe_experiments``) -> phases (GPU, one
wavefront per qubit) -> bootstrap error bars (GPU, resident) -> compared with ``get_variance_upper_bound``.

    python examples/robust_phase_estimation_from_shots.py [--qubits 1000] [--depths 8] [--shots 500]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "forest-benchmarking_amd"))

from fbx import robust_phase_estimation as rpe  # noqa: E402


def synthetic_shots(angles, num_depths, num_shots, t2_in_gates, seed):
    """x_bits, y_bits [B, K, shots, 1]: outcome 1 (eigenvalue -1) with probability (1 - v cos(2^j angle)) / 2 in the X basis and
    (1 - v sin(2^j angle)) / 2 in the Y basis, v = exp(-2^j / t2_in_gates)"""
    rng = np.random.default_rng(seed)
    depth = 2.0 ** np.arange(num_depths)
    vis = np.exp(-depth / t2_in_gates)[None, :, None]
    arg = depth[None, :, None] * np.asarray(angles)[:, None, None]
    shape = (len(angles), num_depths, num_shots)
    x_bits = (rng.random(shape) < (1 - vis * np.cos(arg)) / 2).astype(np.uint8)[..., None]
    y_bits = (rng.random(shape) < (1 - vis * np.sin(arg)) / 2).astype(np.uint8)[..., None]
    return x_bits, y_bits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, default=1000)
    ap.add_argument("--depths", type=int, default=8)
    ap.add_argument("--shots", type=int, default=500)
    ap.add_argument("--resamples", type=int, default=200)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    angles = rng.uniform(0, 2 * np.pi, args.qubits)
    x_bits, y_bits = synthetic_shots(angles, args.depths, args.shots, t2_in_gates=4.0 * 2 ** args.depths, seed=2)

    phases, stats = rpe.robust_phase_estimate_from_shots_batch(x_bits, y_bits, col=0, return_stats=True)
    error = np.abs((phases - angles + np.pi) % (2 * np.pi) - np.pi)
    moments = stats["moments"]
    _, variance, _ = rpe.phase_variance_batch(moments[..., 0], moments[..., 1], moments[..., 2], moments[..., 3], args.shots,
                                              n_resamples=args.resamples, seed=3)
    bound = rpe.get_variance_upper_bound(args.depths)
    print(f"{args.qubits} qubits, {args.depths} depths (up to {2 ** (args.depths - 1)} gates), {args.shots} shots per setting")
    print(f"  estimates cut short by decoherence: {(stats['depth_reached'] < args.depths).sum()}")
    print(f"  rms error against the true angles:  {np.sqrt((error ** 2).mean()):.3e} rad")
    print(f"  median bootstrap standard error:    {np.sqrt(np.median(variance)):.3e} rad")
    print(f"  sqrt(get_variance_upper_bound({args.depths})):   {np.sqrt(bound):.3e} rad  (Eq. V.9 of arXiv:1502.02677, with the optimal")
    print(f"     shot schedule of num_trials: {[rpe.num_trials(2 ** j, 2 ** (args.depths - 1)) for j in range(args.depths)]}; "
          f"{args.shots} shots at every depth are more)")
    # the reference's one-at-a-time form gives the same number for any one qubit
    b = 0
    one = rpe.estimate_phase_from_moments(list(moments[b, :, 0]), list(moments[b, :, 1]), list(moments[b, :, 2]), list(moments[b, :, 3]))
    assert one == phases[b]


if __name__ == "__main__":
    main()
