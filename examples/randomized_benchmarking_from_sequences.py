"""Randomized benchmarking from a noise channel: noise PTM -> Clifford sequences -> simulation -> fit, with the reference's names.

    python examples/randomized_benchmarking_from_sequences.py

No decay is assumed anywhere: a random CPTP map close to the identity follows every Clifford, the sequences are drawn, composed
and inverted on the GPU (no quilc), simulated in the Pauli basis, and the fitted decay is compared with the one the channel
predicts, p = (tr L - 1) / (d^2 - 1) -- for a plain run and for a run with a noisy CZ interleaved."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "forest-benchmarking_amd"))

from fbx import clifford, randomized_benchmarking as rb  # noqa: E402
from fbx.operator_tools import random_operators as ro, superoperator_transformations as st  # noqa: E402

n, dim = 2, 4
D = dim * dim


def noisy_identity(strength, seed):
    """PTM of (1 - strength) identity + strength (a random CPTP map): completely positive, trace preserving, not unital"""
    kraus = ro.random_kraus_batch(dim, 4, 1, seed=seed)[0]
    return (1 - strength) * np.eye(D) + strength * np.real(st.kraus2pauli_liouville(list(kraus)))


def predicted_decay(ptm):
    return (np.trace(ptm) - 1) / (D - 1)


lam, lam_cz = noisy_identity(0.02, seed=1), noisy_identity(0.05, seed=2)
depths = [2, 3, 5, 9, 17, 33, 65, 129]
cz = clifford.gate_word("CZ", (0, 1))
print("CZ as native gates:", clifford.to_gates(cz), "- a random Clifford:", clifford.to_gates(int(clifford.from_index(2, 4711))))

# one sequence with the reference's call, then whole experiments: 64 sequences per depth, no shot noise
seq = rb.generate_rb_sequence(None, [0, 1], 5, random_seed=7)
print("a depth-5 sequence:", [hex(int(e)) for e in seq])
z, z_err = rb.simulate_rb_experiment_batch(n, depths, 64, lam, seed=10)
zi, zi_err = rb.simulate_rb_experiment_batch(n, depths, 64, np.array([lam, lam_cz]), interleaved_gate=cz, seed=11)
# two qubits: the fit adds the covariance of IZ, ZI, ZZ over num_shots; exact expectations are the limit of many shots
exact = 10 ** 12
fit, fit_i = rb.fit_rb_results_batch(depths, z, z_err, exact), rb.fit_rb_results_batch(depths, zi, zi_err, exact)
decay, decay_i = fit.value("decay")[0], fit_i.value("decay")[0]
print("rb decay          %.5f +/- %.5f, predicted %.5f" % (decay, fit.error("decay")[0], predicted_decay(lam)))
# an interleaved step is a random Clifford with its noise, then the CZ with its own: to first order the decays multiply
print("interleaved decay %.5f +/- %.5f, predicted %.5f (first order)" %
      (decay_i, fit_i.error("decay")[0], predicted_decay(lam) * predicted_decay(lam_cz)))
print("gate error of the Cliffords %.5f (from the PTM: %.5f)" %
      (rb.rb_decay_to_gate_error(decay, dim), 1 - (dim * np.trace(lam) / D + 1) / (dim + 1)))
lo, hi = rb.interleaved_gate_fidelity_bounds(decay_i, decay, dim)
print("interleaved CZ: error %.5f (from its PTM: %.5f), fidelity in [%.5f, %.5f]" %
      (rb.irb_decay_to_gate_error(decay_i, decay, dim), 1 - (dim * np.trace(lam_cz) / D + 1) / (dim + 1), lo, hi))

# the same with 500 shots per sequence
zs, zs_err = rb.simulate_rb_experiment_batch(n, depths, 64, lam, seed=10, shots=500)
fit_s = rb.fit_rb_results_batch(depths, zs, zs_err, 500)
print("with 500 shots    %.5f +/- %.5f" % (fit_s.value("decay")[0], fit_s.error("decay")[0]))
