"""Generate tests/golden/readout_cases.npz from the reference's readout.py, classical_logic/ripple_carry_adder.py and
entangled_states.py (build machine only; needs the reference checkout).  Only arrays are stored: the shot records (the inputs) and
what the reference's own functions return for them.

The reference's ``estimate_confusion_matrix``, ``estimate_joint_confusion_in_set`` and ``estimate_joint_reset_confusion`` run
programs on a ``QuantumComputer``.  They run here against ``ReplayQC``, a stand-in written below that hands out the stored shot
arrays in the order in which the functions ask for them (their loops over groups, prepared bitstrings and trials); the pyquil
objects they build on the way are inert.  Usage: python tests/golden/make_readout_goldens.py
"""
import importlib
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
import _ref_harness as rh  # noqa: E402
import readout_cases as rc  # noqa: E402

READOUT_SHOTS = 200
RESET_TRIALS = 40
ADDER_SHOTS = 50
GHZ_SHOTS = 300


class Inert:
    """a pyquil object nobody looks into: programs, gates, memory references"""

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return Inert()

    def __getattr__(self, name):
        return Inert()

    def __getitem__(self, i):
        return Inert()

    def __add__(self, other):
        return Inert()

    __radd__ = __iadd__ = __add__


class _Result:
    def __init__(self, ro):
        self.ro = ro

    def get_register_map(self):
        return {"ro": self.ro}


class ReplayQC:
    """``qc.run`` returns the next stored array.  With ``echo_preparation`` a run that comes with a memory map is a state preparation
    whose measurement the caller only checks against the prepared bitstring (estimate_joint_reset_confusion): it succeeds at once."""

    def __init__(self, qubits, arrays, echo_preparation=False):
        self._qubits, self._queue, self._echo = list(qubits), list(arrays), echo_preparation
        self.compiler = self

    def qubits(self):
        return list(self._qubits)

    def compile(self, program):
        return program

    native_quil_to_executable = quil_to_native_quil = compile

    def run(self, executable, memory_map=None):
        if self._echo and memory_map:
            return _Result(np.asarray([[int(b) for b in memory_map["bitstr"]]]))
        return _Result(self._queue.pop(0))

    def exhausted(self):
        return not self._queue


def load_modules():
    rh._install_stubs()
    sys.modules["pyquil.simulation.tools"].all_bitstrings = \
        lambda n: np.array(list(itertools.product((0, 1), repeat=n)), dtype=int).reshape(2 ** n, n)
    if rh.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, rh.REFERENCE_ROOT)
    readout = importlib.import_module("forest.benchmarking.readout")
    adder = importlib.import_module("forest.benchmarking.classical_logic.ripple_carry_adder")
    ghz = importlib.import_module("forest.benchmarking.entangled_states")
    for name in ("Program", "RX", "RZ", "RESET", "MEASURE", "bitstring_prep", "parameterized_bitstring_prep"):
        setattr(readout, name, Inert if name == "Program" else Inert())
    return readout, adder, ghz


def main():
    readout, adder, ghz = load_modules()
    rng = np.random.default_rng(20241018)
    out = {}
    qubits = list(rc.GOLDEN_QUBITS)
    # single-qubit confusion matrices: two register arrays [shots, 1] per qubit
    zero = (rng.random((len(qubits), READOUT_SHOTS, 1)) < 0.06).astype(np.uint8)
    one = (rng.random((len(qubits), READOUT_SHOTS, 1)) < 0.91).astype(np.uint8)
    out["single_should_be_0"], out["single_should_be_1"] = zero, one
    out["single_confusion"] = np.stack([readout.estimate_confusion_matrix(ReplayQC(qubits, [zero[i], one[i]]), q, READOUT_SHOTS)
                                        for i, q in enumerate(qubits)])
    # joint confusion matrices and reset matrices of every group of 1, 2 and 3 of the 4 qubits
    for g in rc.GOLDEN_GROUP_SIZES:
        groups = list(itertools.combinations(qubits, g))
        shots = rc.sample_rows(rng, rc.random_confusion(rng, len(groups), g), READOUT_SHOTS)
        qc = ReplayQC(qubits, [shots[i, r] for i in range(len(groups)) for r in range(1 << g)])
        got = readout.estimate_joint_confusion_in_set(qc, qubits, num_shots=READOUT_SHOTS, joint_group_size=g)
        assert qc.exhausted() and list(got) == groups
        out[f"joint{g}_groups"] = np.asarray(groups)
        out[f"joint{g}_shots"] = shots
        out[f"joint{g}_confusion"] = np.stack([got[grp] for grp in groups])
        reset = rc.sample_rows(rng, rc.random_confusion(rng, len(groups), g, fidelity=0.0) * 0.2 + 0.8 * (np.arange(1 << g) == 0),
                               RESET_TRIALS)
        qc = ReplayQC(qubits, [reset[i, r, t][None] for i in range(len(groups)) for r in range(1 << g) for t in range(RESET_TRIALS)],
                      echo_preparation=True)
        got = readout.estimate_joint_reset_confusion(qc, qubits, num_trials=RESET_TRIALS, joint_group_size=g)
        assert qc.exhausted() and list(got) == groups
        out[f"reset{g}_shots"] = reset
        out[f"reset{g}_confusion"] = np.stack([got[grp] for grp in groups])
    # marginals of 2- and 3-qubit matrices: every non-empty subset, subsets given in every order, all_qubits permuted
    for n in (2, 3):
        mat = rc.random_confusion(rng, 1, n, fidelity=0.7)[0]
        out[f"marginal{n}_matrix"] = mat
        alls, subsets, results = [], [], []
        for all_q in itertools.permutations((5, 2, 7)[:n]):
            for k in range(1, n + 1):
                for subset in itertools.permutations(all_q, k):
                    alls.append(all_q)
                    subsets.append(tuple(subset) + (-1,) * (n - k))
                    results.append(readout.marginalize_confusion_matrix(mat, all_q, subset).ravel())
        out[f"marginal{n}_all_qubits"] = np.asarray(alls)
        out[f"marginal{n}_subsets"] = np.asarray(subsets)                       # padded with -1
        width = max(len(r) for r in results)
        out[f"marginal{n}_results"] = np.stack([np.pad(r, (0, width - len(r)), constant_values=np.nan) for r in results])
    # ripple-carry adder: results[4^n][shots][n + 1]
    for n in rc.GOLDEN_ADDER_BITS:
        ans = rc.adder_expected(n)
        res = ans[:, None, :] ^ (rng.random((ans.shape[0], ADDER_SHOTS, n + 1)) < 0.15).astype(np.uint8)
        res[0] = ans[0]                                                         # one addition that never fails
        out[f"adder{n}_results"] = res
        out[f"adder{n}_success"] = np.asarray(adder.get_success_probabilities_from_results(res.tolist()))
        out[f"adder{n}_hamming"] = np.asarray(adder.get_error_hamming_distributions_from_results(res.tolist()))
    # GHZ statistics
    for n in rc.GOLDEN_GHZ_WIDTHS:
        bits = (rng.integers(0, 2, size=(GHZ_SHOTS, 1)) ^ (rng.random((GHZ_SHOTS, n)) < 0.08)).astype(np.uint8)
        stats = ghz.ghz_state_statistics(bits)
        out[f"ghz{n}_bits"] = bits
        out[f"ghz{n}_stats"] = np.asarray([stats["bell"], stats["total"]], dtype=np.int64)
    path = os.path.join(HERE, "readout_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
