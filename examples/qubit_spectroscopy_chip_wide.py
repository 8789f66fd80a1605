"""T1 and T2* of a whole chip in two device calls each: 10^4 qubits with their own relaxation times, thermal populations and readout
errors -- curves, shots and fits on the GPU -- and what the fit reports against what was put in.

    python examples/qubit_spectroscopy_chip_wide.py

Two questions the simulator answers in one call each:
  * Which T1 does the fit report for a qubit with this relaxation time, thermal population and readout error at 500 shots?  The
    fit model has no baseline, so the floor f0 + (1 - f0 - f1) p_eq of the measured curve pulls the fitted T1 up.
  * How far is the fitted T2* off when the dephasing envelope is Gaussian?  exp(-t / T2 - (t / T_g)^2) is fitted with
    exp(-t / T2'): the run is repeated with an infinite Gaussian time, same seed, and the two fitted T2 are compared."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "forest-benchmarking_amd"))

from fbx import qubit_spectroscopy as qs  # noqa: E402

B, SHOTS = 10000, 500
rng = np.random.default_rng(2026)
T1 = rng.uniform(20.0, 60.0, B)                                         # microseconds
T2 = np.minimum(rng.uniform(10.0, 30.0, B), 2 * T1)
p_eq = rng.uniform(0.0, 0.02, B)
flips = np.stack([rng.uniform(0.005, 0.03, B), rng.uniform(0.02, 0.08, B)], axis=1)        # P(1 | 0) < P(0 | 1)
t1_times, t2_times = np.linspace(0.0, 100.0, 26), np.linspace(0.0, 40.0, 41)
DETUNING = 2e5                                                          # Hz: a fringe of 5 us, sampled every microsecond

fit_t1 = qs.simulate_and_fit_t1_batch(t1_times, T1, thermal_population=p_eq, shots=SHOTS, flips=flips, seed=7,
                                      vary=(True, True, False))
exact_t1 = qs.simulate_and_fit_t1_batch(t1_times, T1, thermal_population=p_eq, flips=flips, vary=(True, True, False))
got, err = fit_t1.value("decay_time"), fit_t1.error("decay_time")
print(f"T1: {B} qubits x {len(t1_times)} delays x {SHOTS} shots; fits converged: {int(fit_t1.success.sum())}")
print("qubit   true T1   fitted    +-     without shot noise   floor f0 + s p_eq")
floor = flips[:, 0] + (1 - flips[:, 0] - flips[:, 1]) * p_eq
for q in range(6):
    print("%5d   %6.2f   %6.2f   %5.2f        %6.2f             %.4f" % (q, T1[q], got[q], err[q], exact_t1.value("decay_time")[q], floor[q]))
print("fitted - true over the chip: median %+.2f us, rms %.2f us; median fit error %.2f us; the bias of the model alone "
      "(no shot noise): median %+.2f us" % (np.median(got - T1), np.sqrt(np.mean((got - T1) ** 2)), np.nanmedian(err),
                                            np.median(exact_t1.value("decay_time") - T1)))

common = dict(detuning=DETUNING, shots=SHOTS, flips=flips, seed=8)
lorentzian = qs.simulate_and_fit_t2_batch(t2_times, T2, **common)
gaussian = qs.simulate_and_fit_t2_batch(t2_times, T2, gauss_time=40.0, **common)
a, g = lorentzian.value("decay_time"), gaussian.value("decay_time")
print(f"T2*: {B} qubits x {len(t2_times)} delays x {SHOTS} shots; fits converged: {int(lorentzian.success.sum())} / "
      f"{int(gaussian.success.sum())} with a Gaussian envelope of 40 us")
print("fitted - true T2 over the chip: exponential envelope median %+.2f us (rms %.2f), with the Gaussian envelope median %+.2f us "
      "(rms %.2f): quasi-static dephasing reads as a shorter T2" %
      (np.median(a - T2), np.sqrt(np.mean((a - T2) ** 2)), np.median(g - T2), np.sqrt(np.mean((g - T2) ** 2))))
predicted = qs.predicted_fit_parameters("t2_star", flips=flips, t2=T2, detuning=DETUNING)
print("fitted fringe amplitude - predicted (1 - f0 - f1) / 2: median %+.4f; fitted frequency - detuning: median %+.2e MHz" %
      (np.median(lorentzian.value("amplitude") - predicted[:, 0]), np.median(lorentzian.value("frequency") - predicted[:, 4])))
