"""Randomized benchmarking of a whole chip in three device calls: 4096 qubits, each with its own noise and readout error, through
standard RB, interleaved RB and unitarity RB -- sequences, simulation, shots and fits on the GPU.

    python examples/randomized_benchmarking_chip_wide.py

Every "qubit" gets a gate noise of its own: relaxation (T1, T2 drawn per qubit) over the gate time followed by a small coherent
over-rotation about x, and an asymmetric readout error.  Each experiment draws 32 sequences at seven depths and measures every
sequence with 500 shots (per basis, for unitarity); the fitted decays are printed against what the channels predict:
p = (tr L - 1) / (d^2 - 1) for RB, the product of the two decays for the interleaved run (first order), and the squared norm of
the unital block / (d^2 - 1) for the unitarity."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "forest-benchmarking_amd"))

from fbx import clifford, randomized_benchmarking as rb  # noqa: E402

E, K, SHOTS = 4096, 32, 500
DEPTHS = (2, 16, 64, 128, 256, 512, 1024)              # error rates of 10^-3: the decay shows only over hundreds of Cliffords
rng = np.random.default_rng(2026)


def relaxation(t, T1, T2):
    """PTM of amplitude and phase damping over a time t: not unital"""
    e1, e2 = np.exp(-t / T1), np.exp(-t / T2)
    out = np.zeros(T1.shape + (4, 4))
    out[..., 0, 0], out[..., 1, 1], out[..., 2, 2], out[..., 3, 3], out[..., 3, 0] = 1.0, e2, e2, e1, 1.0 - e1
    return out


def rx(theta):
    c, s = np.cos(theta), np.sin(theta)
    out = np.zeros(theta.shape + (4, 4))
    out[..., 0, 0], out[..., 1, 1] = 1.0, 1.0
    out[..., 2, 2], out[..., 2, 3], out[..., 3, 2], out[..., 3, 3] = c, -s, s, c
    return out


T1 = rng.uniform(20e-6, 60e-6, E)
T2 = np.minimum(rng.uniform(15e-6, 50e-6, E), 2 * T1)
gate_noise = rx(rng.normal(0.0, 0.02, E)) @ relaxation(40e-9, T1, T2)            # after every Clifford
slow_gate_noise = rx(rng.normal(0.0, 0.05, E)) @ relaxation(120e-9, T1, T2)      # after the interleaved gate: longer, less exact
flips = np.stack([rng.uniform(0.005, 0.03, E), rng.uniform(0.02, 0.08, E)], axis=1)[:, None, :]     # P(1 | 0) < P(0 | 1)
gate = clifford.from_index(1, 13)
common = dict(shots=SHOTS, flips=flips, seed=7)

fit = rb.simulate_and_fit_rb_batch(1, DEPTHS, K, gate_noise[:, None], **common)
fit_i = rb.simulate_and_fit_rb_batch(1, DEPTHS, K, np.stack([gate_noise, slow_gate_noise], axis=1), interleaved_gate=gate, **common)
fit_u = rb.simulate_and_fit_unitarity_batch(1, DEPTHS, K, gate_noise[:, None], **common)

decay, decay_i, unitarity = fit.value("decay"), fit_i.value("decay"), fit_u.value("decay")
want, want_i, want_u = (rb.predicted_rb_decay(gate_noise), rb.predicted_rb_decay(gate_noise) * rb.predicted_rb_decay(slow_gate_noise),
                        rb.predicted_unitarity(gate_noise))
print(f"{E} qubits x {len(DEPTHS)} depths x {K} sequences x {SHOTS} shots; fits converged: "
      f"rb {int(fit.success.sum())}, interleaved {int(fit_i.success.sum())}, unitarity {int(fit_u.success.sum())}")
print("qubit   rb decay  predicted | interleaved  predicted | unitarity  predicted | gate error  interleaved gate error")
for q in range(6):
    print("%5d   %.5f   %.5f   |   %.5f    %.5f   |  %.5f    %.5f   |  %.2e    %.2e" %
          (q, decay[q], want[q], decay_i[q], want_i[q], unitarity[q], want_u[q], rb.rb_decay_to_gate_error(decay[q], 2),
           rb.irb_decay_to_gate_error(decay_i[q], decay[q], 2)))
for name, got, ref, err in (("rb decay", decay, want, fit.error("decay")), ("interleaved decay", decay_i, want_i, fit_i.error("decay")),
                            ("unitarity", unitarity, want_u, fit_u.error("decay"))):
    dev = got - ref
    print("%-18s fitted - predicted over the chip: median %+.2e, rms %.2e; median fit error %.2e" %
          (name, np.median(dev), np.sqrt(np.mean(dev ** 2)), np.nanmedian(err)))
