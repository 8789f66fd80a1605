"""Robust phase estimation, simulated end to end on the GPU (forest/benchmarking/robust_phase_estimation.py and its test_noisy_rpe).

Part 1: a rotation by an unknown angle about a tilted axis on every qubit of a (simulated) chip, with amplitude damping after
dephasing behind every gate (T1 = 25 us, T2 = 20 us, 200 ns gates) and asymmetric readout (p00 = 0.92, p11 = 0.87): gate ->
Pauli transfer matrix -> shots at depths 1, 2, 4, ... (``fbx_rpe_simulate``) -> phases (``fbx_rpe_phase``), never leaving the
device; the rms error is compared with ``get_variance_upper_bound``.

Part 2: the phase of a controlled-phase gate, three ways: the partner in plusX and post-selected on 1 or on 0 (X and X Z are read
off the same shots), and the partner fixed in |1> with no post-selection.

    python examples/robust_phase_estimation_simulated.py [--qubits 10000] [--depths 7]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "forest-benchmarking_amd"))

from fbx import robust_phase_estimation as rpe  # noqa: E402
from fbx.operator_tools.superoperator_transformations import convert_batch  # noqa: E402


def damping_after_dephasing(t1, t2, gate_time):
    """Kraus operators of amplitude damping (T1) after pure dephasing (what T2 leaves beyond T1) over one gate"""
    p_damp = 1 - np.exp(-gate_time / t1)
    gamma_phi = gate_time / t2 - gate_time / (2 * t1)
    p_deph = 0.5 * (1 - np.exp(-2 * gamma_phi))
    damping = [np.array([[1, 0], [0, np.sqrt(1 - p_damp)]]), np.array([[0, np.sqrt(p_damp)], [0, 0]])]
    dephasing = [np.sqrt(1 - p_deph) * np.eye(2), np.sqrt(p_deph) * np.diag([1.0, -1.0])]
    return np.array([a @ b for a in damping for b in dephasing], dtype=complex)


def ptm(kraus):
    """[B, K, d, d] Kraus operators -> real Pauli transfer matrices [B, D, D], on the device"""
    return np.ascontiguousarray(convert_batch("kraus", "pauli_liouville", np.asarray(kraus, dtype=complex)).real)


def rms(err):
    return float(np.sqrt(np.mean(err ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, default=10000)
    ap.add_argument("--depths", type=int, default=7)
    args = ap.parse_args()
    B, K = args.qubits, args.depths
    rng = np.random.default_rng(1)
    noise = damping_after_dephasing(25e-6, 20e-6, 200e-9)
    noise_ptm = ptm(noise[None])[0]
    flips = [[0.08, 0.13]]                                     # p00 = 0.92, p11 = 0.87

    # ---- part 1: rotations about the axis tilted by pi / 4 from z, as RY(pi/4) RZ(angle) RY(-pi/4)
    angles = rng.uniform(0, 2 * np.pi, B)
    cob = rpe.get_change_of_basis_from_eigvecs(rpe.bloch_rotation_to_eigenvectors(np.pi / 4, 0.0))
    rz = np.zeros((B, 2, 2), dtype=complex)
    rz[:, 0, 0], rz[:, 1, 1] = np.exp(-0.5j * angles), np.exp(0.5j * angles)
    rotations = cob @ rz @ cob.conj().T
    gates = noise_ptm @ ptm(rotations[:, None])                # the noise follows the gate
    prep = noise_ptm @ ptm(cob[None, None])[0]
    pre_meas = noise_ptm @ ptm(cob.conj().T[None, None])[0]
    mult, add = 5.0, 0.15
    phases, depth, err = rpe.simulate_and_estimate_rpe_batch(gates, prep=prep, pre_meas=pre_meas, num_depths=K,
                                                             multiplicative_factor=mult, additive_error=add, flips=flips,
                                                             seed=5, true_phases=angles)
    print(f"{B} qubits, {K} depths (up to {2 ** (K - 1)} gates), shots per depth {rpe.rpe_shot_schedule(K, mult, add).tolist()}")
    print(f"  estimates cut short by decoherence: {int((depth < K).sum())}")
    print(f"  rms error against the true angles:  {rms(err):.3e} rad   (largest {err.max():.3e})")
    print(f"  sqrt(get_variance_upper_bound({K}, {mult}, {add})): {np.sqrt(rpe.get_variance_upper_bound(K, mult, add)):.3e} rad")

    # ---- part 2: the phase of diag(1, 1, 1, e^{i phi}), noise on both qubits behind the gate
    phis = rng.uniform(0, 2 * np.pi, B)
    cz = np.zeros((B, 4, 4), dtype=complex)
    cz[:, [0, 1, 2], [0, 1, 2]] = 1.0
    cz[:, 3, 3] = np.exp(1j * phis)
    noise2 = np.array([np.kron(a, b) for a in noise for b in noise])
    gates2 = ptm(noise2[None])[0] @ ptm(cz[:, None])
    flips2 = [[0.08, 0.13], [0.08, 0.13]]
    common = dict(num_depths=K, multiplicative_factor=mult, additive_error=add, flips=flips2, xy_qubit=0, n_qubits=2)
    _, _, on_one = rpe.simulate_and_estimate_rpe_batch(gates2, z_qubit=1, post_select=1, seed=6, true_phases=phis, **common)
    _, _, on_zero = rpe.simulate_and_estimate_rpe_batch(gates2, z_qubit=1, post_select=0, seed=6, true_phases=np.zeros(B), **common)
    plus_one = np.kron([1, 1, 0, 0], [1, 0, 0, -1]).astype(float)          # Pauli vector of |+>|1>
    _, _, fixed = rpe.simulate_and_estimate_rpe_batch(gates2, init=plus_one, seed=7, true_phases=phis, **common)
    print(f"controlled phase on {B} pairs:")
    print(f"  partner in plusX, post-selected on 1 (phase phi): rms error {rms(on_one):.3e} rad")
    print(f"  partner in plusX, post-selected on 0 (phase 0):   rms error {rms(on_zero):.3e} rad")
    print(f"  partner fixed in |1>, no post-selection:          rms error {rms(fixed):.3e} rad")
    print("  (post-selection reads both relative phases off one experiment, each from about half of its shots)")

    # ---- the same experiment in the reference's structure, for one qubit
    results = rpe.simulate_rpe_results(gates[0], cob, [0], num_depths=K, multiplicative_factor=mult, additive_error=add, flips=flips, seed=5)
    one = rpe.robust_phase_estimate(results, [0])
    print(f"reference structure, qubit 0: {len(results)} depths x {len(results[0])} results, phase {one:.4f} (true {angles[0]:.4f})")


if __name__ == "__main__":
    main()
