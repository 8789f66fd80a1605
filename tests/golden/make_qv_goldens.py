"""Generate tests/golden/qv_cases.npz from the reference's quantum_volume.py (build machine only; needs the reference checkout).

The reference's own ``generate_abstract_qv_circuit`` (under ``np.random.seed``) supplies the circuits and its own
``collect_heavy_outputs`` the heavy lists; the simulator it drives is pyquil's NumpyWavefunctionSimulator, which is not installed
here -- ``_WavefunctionStandIn`` restates its published behaviour (``reset``, ``do_gate_matrix(matrix, qubits)``, ``.wf`` of shape
(2,) * n with axis q = qubit q, the matrix's row / column index split most-significant-first over ``qubits``), the way
``_ref_harness.lifted_pauli`` restates pyquil's tools.  The three scalar helpers (:211-397) are called in the reference itself.
Only arrays are stored.  Usage: python tests/golden/make_qv_goldens.py
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import _ref_harness as rh  # noqa: E402

WIDTHS = range(2, 11)
CIRCUITS = 4
MIN_GAP = 1e-7
_EINSUM = "abcdefghijklmnopqrstuvwxyz"


class _WavefunctionStandIn:
    def __init__(self, n_qubits):
        self.n_qubits = n_qubits
        self.reset()

    def reset(self):
        self.wf = np.zeros((2,) * self.n_qubits, dtype=np.complex128)
        self.wf[(0,) * self.n_qubits] = 1.0
        return self

    def do_gate_matrix(self, matrix, qubits):
        k, n = len(qubits), self.n_qubits
        tensor = np.asarray(matrix, dtype=np.complex128).reshape((2,) * (2 * k))
        state = list(_EINSUM[:n])
        outs = list(_EINSUM[n:n + k])
        result = list(state)
        for j, q in enumerate(qubits):
            result[int(q)] = outs[j]
        spec = "".join(outs) + "".join(state[int(q)] for q in qubits) + "," + "".join(state) + "->" + "".join(result)
        self.wf = np.einsum(spec, tensor, self.wf)
        return self


def load_quantum_volume():
    rh._install_stubs()
    inert = rh._Inert

    def mod(name, **attrs):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
        sys.modules[name].__dict__.update(attrs)

    try:
        import tqdm  # noqa: F401
    except ImportError:
        mod("tqdm", tqdm=lambda it, **k: it)
    mod("rpcq")
    mod("rpcq.messages", TargetDevice=inert)
    mod("rpcq._utils", RPCErrorError=type("RPCErrorError", (Exception,), {}))
    mod("pyquil.external")
    mod("pyquil.external.rpcq", CompilerISA=inert)
    mod("pyquil.quil", DefGate=inert, Pragma=inert)
    if rh.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, rh.REFERENCE_ROOT)
    return importlib.import_module("forest.benchmarking.quantum_volume")


def middle_gap(p):
    s = np.sort(p)
    N = len(s)
    return (s[N // 2] - s[N // 2 - 1]) / (0.5 * (s[N // 2] + s[N // 2 - 1]))


def main():
    qv = load_quantum_volume()
    out = {}
    for n in WIDTHS:
        perms, gates, heavy, probs, med, seeds = [], [], [], [], [], []
        seed = 1000 * n
        while len(perms) < CIRCUITS:
            np.random.seed(seed)
            p, g = qv.generate_abstract_qv_circuit(n)
            sim = _WavefunctionStandIn(n)
            hh = qv.collect_heavy_outputs(sim, p, g)
            pr = np.abs(sim.wf.reshape(-1)) ** 2
            if middle_gap(pr) >= MIN_GAP:                       # (a circuit with a tighter middle is re-seeded, never dropped later)
                table = np.zeros(1 << n, dtype=bool)
                table[hh] = True
                s = np.sort(pr)
                perms.append(np.asarray(p)); gates.append(g); heavy.append(table); probs.append(pr)
                med.append(0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])); seeds.append(seed)
            seed += 1
        out[f"w{n}_seeds"] = np.asarray(seeds)
        out[f"w{n}_permutations"] = np.stack(perms).astype(np.int64)
        out[f"w{n}_gates"] = np.stack(gates)
        out[f"w{n}_heavy"] = np.stack(heavy)
        out[f"w{n}_probabilities"] = np.stack(probs)
        out[f"w{n}_median"] = np.asarray(med)
    # scalar helpers, called in the reference
    rng = np.random.default_rng(7)
    args = np.asarray([(int(rng.integers(0, c * s + 1)), c, s) for c, s in
                       ((1, 1), (1, 1000), (100, 1000), (100, 500), (437, 1000), (200, 10), (3, 7), (1000, 100))], dtype=np.int64)
    args = np.concatenate([args, [(0, 10, 10), (100, 10, 10), (70000, 100, 1000)]])
    out["est_args"] = args
    out["est_out"] = np.asarray([qv.calculate_prob_est_and_err(int(h), int(c), int(s)) for h, c, s in args], dtype=np.float64)
    depths = np.repeat(np.arange(2, 8), 5)
    shots = np.where(depths % 2 == 0, 1000, 400)
    frac = {2: 0.85, 3: 0.8, 4: 0.78, 5: 0.7, 6: 0.66, 7: 0.55}
    hh = np.asarray([int(rng.binomial(s, frac[int(d)])) for d, s in zip(depths, shots)], dtype=np.int64)
    order = rng.permutation(len(depths))                        # circuits of different depths interleaved
    depths, shots, hh = depths[order], shots[order], hh[order]
    res = qv.get_prob_sample_heavy_by_depth([int(d) for d in depths], [int(h) for h in hh], [int(s) for s in shots])
    out["by_depth_depths"], out["by_depth_heavy"], out["by_depth_shots"] = depths, hh, shots
    out["by_depth_keys"] = np.asarray(list(res.keys()), dtype=np.int64)
    out["by_depth_values"] = np.asarray(list(res.values()), dtype=np.float64)
    out["qv_from_by_depth"] = np.asarray(qv.extract_quantum_volume_from_results(res))
    tables = {"first_fails": {2: (0.6, 0.55), 3: (0.9, 0.8), 4: (0.9, 0.8)},
              "middle_fails": {2: (0.9, 0.8), 3: (0.85, 0.75), 4: (0.7, 2 / 3), 5: (0.9, 0.85)},
              "none_fails": {4: (0.8, 0.7), 2: (0.9, 0.85), 3: (0.85, 0.75), 5: (0.75, 0.67)},
              "just_above": {2: (0.9, np.nextafter(2 / 3, 1.0))}}
    for name, t in tables.items():
        out[f"extract_{name}_depths"] = np.asarray(list(t.keys()), dtype=np.int64)
        out[f"extract_{name}_values"] = np.asarray(list(t.values()), dtype=np.float64)
        out[f"extract_{name}_qv"] = np.asarray(qv.extract_quantum_volume_from_results(t))
    path = os.path.join(HERE, "qv_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", {n: out[f"w{n}_seeds"].tolist() for n in WIDTHS})


if __name__ == "__main__":
    main()
