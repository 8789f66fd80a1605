"""Randomized benchmarking from expectations to a gate error, with the reference's function names.

    python examples/randomized_benchmarking_from_expectations.py

Synthetic data stand in for the QuantumComputer: 64 two-qubit groups, 35 sequences each, for standard RB, for RB with a gate
interleaved, and for a unitarity experiment on one qubit.  Everything from the expectations on runs on the GPU:
expectations -> survival probabilities -> weights and default guess -> decay fits, all groups in one chain of device calls."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "forest-benchmarking_amd"))

from fbx import randomized_benchmarking as rb, synthetic  # noqa: E402

depths = np.repeat([2, 4, 8, 16, 32, 64, 128], 5)
shots, groups, dim = 500, 64, 4
rng = np.random.default_rng(0)
true_decay = rng.uniform(0.95, 0.99, groups)
gate_decay = 0.985                                             # the interleaved gate alone

# standard and interleaved RB: [groups, sequences, dim - 1] expectations of the I/Z observables
z, z_err = synthetic.rb_data(2, depths, true_decay, shots, groups, seed=1)
zi, zi_err = synthetic.rb_data(2, depths, true_decay * gate_decay, shots, groups, seed=2)
fit = rb.fit_rb_results_batch(depths, z, z_err, shots)
fit_i = rb.fit_rb_results_batch(depths, zi, zi_err, shots)
decay, decay_i = fit.value("decay"), fit_i.value("decay")
print("converged: %d / %d standard, %d / %d interleaved" % (fit.success.sum(), groups, fit_i.success.sum(), groups))
print("group 0: rb decay %.4f +/- %.4f (true %.4f), gate error %.4f" %
      (decay[0], fit.error("decay")[0], true_decay[0], rb.rb_decay_to_gate_error(decay[0], dim)))
one = rb.fit_rb_results(depths, z[0], z_err[0], shots)         # the reference's single-experiment call: the same numbers
assert one.params["decay"].value == decay[0]

# interleaved gate: point estimate and the bounds of the reference
err_gate = rb.irb_decay_to_gate_error(decay_i, decay, dim)
lo, hi = rb.interleaved_gate_fidelity_bounds(decay_i, decay, dim)
print("group 0: interleaved gate error %.4f (true %.4f), fidelity in [%.4f, %.4f]" %
      (err_gate[0], rb.irb_decay_to_gate_error(gate_decay, 1.0, dim), lo[0], hi[0]))

# unitarity on one qubit: Bloch vectors shrinking by sqrt(u) per Clifford, measured along X, Y, Z
u_true = 0.97
r = 0.98 * np.sqrt(u_true) ** depths
dirs = rng.normal(size=(8, len(depths), 3))
dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
e = 2 * rng.binomial(4000, (1 + r[None, :, None] * dirs) / 2) / 4000 - 1
ufit = rb.fit_unitarity_results_batch(depths, e, np.sqrt((1 - e * e) / 4000))
u = ufit.value("decay")
print("unitarity %.4f +/- %.4f (true %.4f); rb decay it allows %.4f" %
      (u[0], ufit.error("decay")[0], u_true, rb.unitarity_to_rb_decay(u[0], 2)))
rb1, _ = synthetic.rb_data(1, depths, 0.975, shots, 1, seed=3)
d1 = rb.fit_rb_results(depths, rb1[0], np.sqrt((1 - rb1[0] ** 2) / shots)).params["decay"].value
print("coherence angle of a decay of %.4f under that unitarity: %.4f rad" % (d1, rb.coherence_angle(min(d1, np.sqrt(u[0])), u[0])))
