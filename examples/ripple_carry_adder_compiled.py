"""The ripple-carry adder as the hardware runs it: compiled to native gates by ``fbx.compilation.basic_compile`` -- every Toffoli
its decomposition into 123 native gates, 12 of them CZ -- and simulated on a state vector with a Pauli error after every native
gate (``fbx_native_trajectories``).  The question it answers: which success probability does a given CZ error predict for the
1-, 2- and 3-bit adder?

Next to it stands the model of ``ripple_carry_adder_simulated.py``, classical bits with one error per SOURCE gate
(``predicted_adder_statistics``), where the caller has to say what a Toffoli's error is.  The natural guess gives a CNOT the
error p of its one CZ and the Toffoli the error ``1 - (1 - p)^12`` of its twelve.  The two curves differ where that guess does:
an error inside a decomposition is not a uniformly random Pauli on the gate's three qubits after it.

Only CZ errs here (the RX pulses and the virtual RZ are perfect), so that the CZ error is the only knob.

    python examples/ripple_carry_adder_compiled.py [--trajectories 512] [--plot adder.png]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "forest-benchmarking_amd"))

from fbx.classical_logic import reversible, ripple_carry_adder as rca  # noqa: E402

CZ_ERRORS = np.array([0.0, 0.001, 0.003, 0.01, 0.03])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trajectories", type=int, default=512)
    ap.add_argument("--plot", default=None, help="write the curves to this image file (needs matplotlib)")
    args = ap.parse_args()
    compiled_ce = np.stack([0.0 * CZ_ERRORS, 0.0 * CZ_ERRORS, CZ_ERRORS], axis=1)                     # (p_rx, p_rz, p_cz)
    source_ce = np.stack([0.0 * CZ_ERRORS, CZ_ERRORS, 1.0 - (1.0 - CZ_ERRORS) ** 12], axis=1)         # one-, two-, three-qubit gates
    curves = {}
    for n in (1, 2, 3):
        words, _, n_qubits, _, cls = rca.compiled_adder_circuit(n)
        gates, _ = rca.adder(*rca.default_adder_registers(n))
        arity = reversible.gate_arity(reversible.encode_reversible(gates, n_qubits))
        success, hamming = rca.compiled_adder_statistics_batch(n, compiled_ce, trajectories=args.trajectories, seed=2024)
        model, _ = rca.predicted_adder_statistics(n, source_ce, noise_class=arity - 1)
        # the standard error of a pair's success probability is at most 1 / (2 sqrt(T)); the mean over the pairs averages 4^n of them
        err = 0.5 / np.sqrt(args.trajectories * 4 ** n)
        print(f"{n}-bit adder: {len(gates)} gates -> {words.size} native gates ({int((cls == 2).sum())} CZ) on {n_qubits} qubits, "
              f"{4 ** n} pairs x {args.trajectories} trajectories")
        print("    CZ error   compiled, native noise (+- at most)   source gates, Toffoli at 1 - (1 - p)^12")
        for b, p in enumerate(CZ_ERRORS):
            print(f"    {p:8.3f}   {success[b].mean():.4f} (+- {err:.4f})                   {model[b].mean():.4f}")
        curves[n] = (success.mean(axis=1), model.mean(axis=1))
    if args.plot:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        fig, ax = plt.subplots(figsize=(6, 4))
        for n, (compiled, model) in curves.items():
            line, = ax.plot(CZ_ERRORS, compiled, "o-", label=f"{n}-bit, compiled")
            ax.plot(CZ_ERRORS, model, "s--", color=line.get_color(), label=f"{n}-bit, source-gate model")
        ax.set_xlabel("CZ error")
        ax.set_ylabel("success probability, mean over all pairs")
        ax.legend()
        fig.tight_layout()
        fig.savefig(args.plot)
        print("wrote", args.plot)


if __name__ == "__main__":
    main()
