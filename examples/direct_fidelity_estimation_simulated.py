"""Direct fidelity estimation of Clifford circuits with simulated data: the experiment generators, the noisy acquisition and the
estimate all run on the device (``fbx.direct_fidelity_estimation``), for circuits far wider than tomography reaches.

1. A GHZ state on 5 qubits, all 31 settings, against the fidelity of a dense density-matrix simulation of the same noise.
2. A GHZ state on 50 qubits by Monte Carlo (200 settings), under a sweep of the two-qubit gate error.
3. A 2-qubit process (H, CNOT) by the exhaustive and the Monte Carlo generator.

The noise is a depolarizing channel after every gate (one error rate for one-qubit gates, one for two-qubit gates) and a
symmetric readout flip per qubit, which the calibration runs divide out again.

    python examples/direct_fidelity_estimation_simulated.py [--shots 2000] [--terms 200]
"""
import argparse
import functools
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "forest-benchmarking_amd"))

from fbx import direct_fidelity_estimation as dfe  # noqa: E402


def ghz(n):
    return [("H", (0,))] + [("CNOT", (q, q + 1)) for q in range(n - 1)]


def by_arity(gates):
    """noise class 0 for one-qubit gates, 1 for two-qubit gates"""
    return np.array([len(q) - 1 for _, q in gates], dtype=np.uint8)


def dense_ghz_fidelity(n, p1, p2):
    """<GHZ| rho |GHZ> after H and the CNOT chain, each followed by a depolarizing channel on its qubits (dense, for small n)."""
    paulis = [np.eye(2), np.array([[0, 1], [1, 0]]), np.array([[0, -1j], [1j, 0]]), np.diag([1.0, -1.0])]

    def embed(ops):                                        # {qubit: 2 x 2 matrix}, qubit 0 leftmost
        return functools.reduce(np.kron, [ops.get(q, np.eye(2)) for q in range(n)])

    def depolarize(rho, qubits, p):
        mixed = sum(embed(dict(zip(qubits, ps))) @ rho @ embed(dict(zip(qubits, ps))).conj().T
                    for ps in itertools.product(paulis, repeat=len(qubits)))
        return (1 - p) * rho + p * mixed / 4 ** len(qubits)

    rho = np.zeros((2 ** n, 2 ** n), dtype=complex)
    rho[0, 0] = 1.0
    h = embed({0: np.array([[1, 1], [1, -1]]) / np.sqrt(2)})
    rho = depolarize(h @ rho @ h.T, (0,), p1)
    for q in range(n - 1):
        cnot = embed({q: np.diag([1.0, 0.0])}) + embed({q: np.diag([0.0, 1.0]), q + 1: paulis[1]})
        rho = depolarize(cnot @ rho @ cnot.T, (q, q + 1), p2)
    psi = np.zeros(2 ** n)
    psi[0] = psi[-1] = np.sqrt(0.5)
    return float((psi @ rho @ psi).real)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=2000)
    ap.add_argument("--terms", type=int, default=200)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()

    # 1. five qubits, exhaustive
    n, p1, p2 = 5, 0.002, 0.02
    gates = ghz(n)
    expt = dfe.generate_exhaustive_state_dfe_experiment(None, gates, list(range(n)))
    noise = dict(noise_class=by_arity(gates), readout_flip=np.full(n, 0.03), seed=args.seed)
    print(f"GHZ on {n} qubits, {expt.m} settings, e.g. {expt.settings()[-1]}")
    results = dfe.simulate_dfe_results(expt, [p1, p2], args.shots, calibrate=True, **noise)
    fidelity, err = dfe.estimate_dfe(results, "state")
    print(f"  DFE estimate {fidelity:.4f} +- {err:.4f} from {args.shots} shots per setting, readout calibrated; "
          f"dense simulation {dense_ghz_fidelity(n, p1, p2):.4f}")

    # 2. fifty qubits, Monte Carlo, a sweep of the two-qubit gate error
    n = 50
    gates = ghz(n)
    expt = dfe.generate_monte_carlo_state_dfe_experiment(None, gates, list(range(n)), n_terms=args.terms, seed=args.seed)
    p2s = np.array([0.0, 0.001, 0.002, 0.005, 0.01, 0.02])
    errors = np.stack([np.full(p2s.size, 0.0005), p2s], axis=1)
    fid, err = dfe.simulate_and_estimate_dfe_batch(expt, errors, args.shots, noise_class=by_arity(gates),
                                                   readout_flip=np.full(n, 0.01), calibrate=True, seed=args.seed)
    print(f"GHZ on {n} qubits, {expt.m} Monte Carlo settings, {args.shots} shots each, 49 CNOTs:")
    for p, f, e in zip(p2s, fid, err):
        print(f"  two-qubit gate error {p:.3f}: fidelity {f:.4f} +- {e:.4f}")

    # 3. a two-qubit process by both generators
    gates = [("H", (0,)), ("CNOT", (0, 1))]
    for name, expt in (("exhaustive", dfe.generate_exhaustive_process_dfe_experiment(None, gates, [0, 1])),
                       ("Monte Carlo", dfe.generate_monte_carlo_process_dfe_experiment(None, gates, [0, 1], n_terms=args.terms,
                                                                                       seed=args.seed))):
        fid, err = dfe.simulate_and_estimate_dfe_batch(expt, [[0.002, 0.02]], args.shots, noise_class=by_arity(gates),
                                                       seed=args.seed)
        print(f"H, CNOT as a process, {name} ({expt.m} settings): average gate fidelity {fid[0]:.4f} +- {err[0]:.4f}")


if __name__ == "__main__":
    main()
