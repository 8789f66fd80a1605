"""What tests/test_native_cpu.py, tests/test_compilation_cpu.py and tests/test_native_gpu.py share: the test circuits of the
native-gate simulator, the cases that reach every path of its kernel, the reference's random programs, and the measurement
behind the tolerance of the device's probabilities.

THE TOLERANCE.  The device is compared with the numpy mirror (fbx.native_circuit) run on the restated Paulis.  The mirror is
itself a double-precision computation, so its own error is the yardstick: ``measure_mirror_deviation`` evaluates the same
trajectories of the circuits below with mpmath at 50 digits and returns the mirror's largest absolute deviation over every
probability of ``probs_mean``.  Measured on the CPU over all of ``CASES`` (77 052 values, 20 s; generic angles, so that no
product is exact by accident): 4.44e-16, reached by the marginal of the width-6 case; the widest cases stay below 1.4e-16 (the
error of a probability scales with the probability, and the probabilities of a state sum to 1).  MIRROR_DEVIATION = 4.5e-16.
The device makes the same roundings in another order (FMA contraction, its own cos and sin, another summation tree), so its
difference from the mirror is expected near 2 x that; it is allowed FACTOR = 8 x, the rest being margin for the tail over the
~10^5 values the GPU tests compare.  Neither number comes from the device's output.  tests/test_native_cpu.py repeats the
measurement on the narrow cases and holds it below MIRROR_DEVIATION.

That number belongs to the 8-gate circuits of ``CASES``.  The compiled adders of the adder tests are 293 to 709 gates long and
the mirror's deviation on them is 7 to 25 times larger (3.1e-15 to 1.13e-14; ``ADDER_MIRROR_DEVIATION`` below says why), so the
same procedure is applied to each of those circuits and each is held to FACTOR x ITS mirror's deviation: a tolerance per
circuit, none of them from the device.
"""
import numpy as np

MIRROR_DEVIATION = 4.5e-16
FACTOR = 8.0
TOL = FACTOR * MIRROR_DEVIATION

SEG = 8                                  # fbx.native_circuit.SEGMENT, restated: the tests straddle it
WAVE = 8                                 # fbx.native_circuit.WAVE_MAX_QUBITS, restated
INPUTS = np.array([0b000001, 0b100000], dtype=np.uint64)          # bit 0 set and bit 5 clear, and the other way round
CLASS_ERROR = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.3, 0.1, 0.5]])      # nothing errs, every gate errs, a mixture


def circuit(n, G, seed=0):
    """G native gates on n qubits with generic angles: every opcode, both operand orders, conditional gates on input bits 0 and
    5 (one-qubit and two-qubit), and from gate to gate other qubits."""
    rng = np.random.default_rng(1000 * n + 10 * G + seed)
    gates = []
    for l in range(G):
        q = int(rng.integers(n))
        angle = float(rng.uniform(-2 * np.pi, 2 * np.pi))
        kind = l % 8 if n >= 2 else (0, 2, 5, 4)[l % 4]
        if kind in (1, 3, 6, 7):
            r = int(rng.integers(n - 1))
            pair = (q, r if r < q else r + 1)
        if kind == 0:
            gates.append(("RX", (q,), angle))
        elif kind == 1:
            gates.append(("CZ", pair))
        elif kind == 2:
            gates.append(("RZ", (q,), angle))
        elif kind == 3:
            gates.append(("XY", pair, angle))
        elif kind == 4:
            gates.append(("RX", (q,), angle, 0))
        elif kind == 5:
            gates.append(("I", (q,)))
        elif kind == 6:
            gates.append(("CZ", pair, None, 5))
        else:
            gates.append(("XY", pair, angle, 0))
    return gates


def _case(n, G, T, out=None):
    return {"n": n, "G": G, "T": T, "out": list(range(n)) if out is None else out}


# widths: fewer amplitudes than lanes (1, 2, 3), exactly 64 (6), both teams (.., WAVE | WAVE + 1, ..), the widest; G: both parities
# of the two-gates-per-block rule; T: both sides of the segment; marginals on non-adjacent qubits in non-sorted order
CASES = ([_case(n, 8, SEG + 1) for n in (1, 2, 3, 6, 7, WAVE, WAVE + 1)]
         + [_case(13, 8, 5)]
         + [_case(n, G, SEG + 1) for n in (3, WAVE + 1) for G in (0, 1, 2, 7)]
         + [_case(n, 8, T) for n in (3, WAVE + 1) for T in (1, SEG - 1, SEG)]
         + [_case(3, 7, SEG + 1, [2, 0]), _case(6, 8, SEG + 1, [4, 0, 2]), _case(WAVE + 1, 8, SEG + 1, [7, 2, 5, 0]),
            _case(13, 7, 3, [12, 3, 8])])


def case_id(case):
    return "n%d-G%d-T%d-m%d" % (case["n"], case["G"], case["T"], len(case["out"]))


def restated(case, seed=11, first_item=0, first_input=0):
    """``restate_native_trajectories`` of a case: (words, angles, classes, the restatement)."""
    from fbx import native_circuit as nc
    words, angles = nc.encode_native(circuit(case["n"], case["G"]), case["n"])
    cls = nc.native_noise_classes(words)
    res = nc.restate_native_trajectories(words, angles, case["n"], INPUTS, case["out"], case["T"], CLASS_ERROR, cls, seed,
                                         first_item, first_input)
    return words, angles, cls, res


def circuit_mirror_deviation(words, angles, cls, n, inputs, out, T, class_error, seed, digits=50):
    """The largest absolute difference between the mirror's ``probs_mean`` of one circuit and an evaluation of the same
    trajectories -- the restated Paulis -- with mpmath at ``digits`` digits, over every item, input and output."""
    import mpmath
    from fbx import native_circuit as nc
    res = nc.restate_native_trajectories(words, angles, n, inputs, out, T, class_error, cls, seed)
    fields = [nc._fields(w) for w in words.tolist()]
    out = [int(q) for q in out]
    m, worst = len(out), 0.0
    with mpmath.workdps(digits):
        half = mpmath.mpf(1) / 2
        for b in range(res["paulis"].shape[0]):
            for r, word in enumerate(np.asarray(inputs).tolist()):
                total = [mpmath.mpf(0)] * (1 << n)
                for t in range(T):
                    state = [mpmath.mpc(0)] * (1 << n)
                    state[0] = mpmath.mpc(1)
                    for l, (op, q0, q1, cond, bit) in enumerate(fields):
                        if cond and not (word >> bit) & 1:
                            continue
                        state = _mp_gate(mpmath, state, n, op, q0, q1, mpmath.mpf(float(angles[l])) * half, int(res["paulis"][b, r, t, l]))
                    total = [s + a.real * a.real + a.imag * a.imag for s, a in zip(total, state)]
                marg = [mpmath.mpf(0)] * (1 << m)
                for i, v in enumerate(total):
                    marg[sum(((i >> (n - 1 - q)) & 1) << (m - 1 - c) for c, q in enumerate(out))] += v
                for j in range(1 << m):
                    worst = max(worst, abs(float(marg[j] / T - mpmath.mpf(float(res["probs_mean"][b, r, j])))))
    return worst


def measure_mirror_deviation(cases, digits=50):
    """``circuit_mirror_deviation`` over the circuits, inputs and noise of ``cases``: the largest of them."""
    from fbx import native_circuit as nc
    worst = 0.0
    for case in cases:
        words, angles = nc.encode_native(circuit(case["n"], case["G"]), case["n"])
        worst = max(worst, circuit_mirror_deviation(words, angles, nc.native_noise_classes(words), case["n"], INPUTS, case["out"],
                                                    case["T"], CLASS_ERROR, 11, digits))
    return worst


# The compiled adders of the GPU tests are hundreds of gates long, most of them RX(+-pi/2): the rounding of cos(pi/4) and
# sin(pi/4) enters every one of them with the same sign, so the mirror's deviation grows with the gate count and is measured
# per circuit (on the CPU, as above): noiseless, all 4^n inputs, one trajectory -- and the noisy 1-bit case of the statistics
# test.  Key: (n_bits, in_x_basis); value: (native gates, the mirror's largest deviation from mpmath).
ADDER_STATS_CLASS_ERROR = np.array([[0.02, 0.0, 0.05], [0.2, 0.01, 0.3]])
ADDER_STATS_T, ADDER_STATS_SEED = SEG + 1, 9
# Measured: 3.11e-15, 6.00e-15, 9.77e-15 and 1.13e-14, each on the weight of an expected answer (which the mirror puts BELOW 1:
# the error is a loss of norm), and 2.04e-15 for the statistics case; recorded rounded up.
ADDER_MIRROR_DEVIATION = {(1, False): (293, 3.2e-15), (1, True): (365, 6.0e-15), (2, False): (577, 9.8e-15), (2, True): (709, 1.14e-14)}
ADDER_STATS_MIRROR_DEVIATION = 2.1e-15
ADDER_STATS_TOL = FACTOR * ADDER_STATS_MIRROR_DEVIATION


def adder_mirror_deviation(n_bits, in_x_basis, digits=50):
    from fbx.classical_logic import ripple_carry_adder as rca
    words, angles, n, out, cls = rca.compiled_adder_circuit(n_bits, in_x_basis=in_x_basis)
    return int(words.size), circuit_mirror_deviation(words, angles, cls, n, np.arange(4 ** n_bits, dtype=np.uint64), out, 1, None, 0, digits)


def adder_stats_mirror_deviation(digits=50):
    from fbx.classical_logic import ripple_carry_adder as rca
    words, angles, n, out, cls = rca.compiled_adder_circuit(1)
    return circuit_mirror_deviation(words, angles, cls, n, np.arange(4, dtype=np.uint64), out, ADDER_STATS_T, ADDER_STATS_CLASS_ERROR,
                                    ADDER_STATS_SEED, digits)


def adder_tol(n_bits, in_x_basis):
    return FACTOR * ADDER_MIRROR_DEVIATION[(n_bits, in_x_basis)][1]


def _mp_gate(mp, state, n, op, q0, q1, half_angle, pauli):
    """One gate of the mirror's definition (include/fbx.h) and then its Pauli, on a list of mpc amplitudes (qubit 0 = the most
    significant index bit)."""
    c, s, j = mp.cos(half_angle), mp.sin(half_angle), mp.mpc(0, 1)
    p0, p1 = n - 1 - q0, n - 1 - q1
    new = list(state)
    if op == 1:                                                          # RX
        for i in range(1 << n):
            new[i] = c * state[i] - j * s * state[i ^ (1 << p0)]
    elif op == 2:                                                        # RZ
        for i in range(1 << n):
            new[i] = state[i] * (c + j * s if (i >> p0) & 1 else c - j * s)
    elif op == 3:                                                        # CZ
        for i in range(1 << n):
            new[i] = -state[i] if (i >> p0) & (i >> p1) & 1 else state[i]
    elif op == 4:                                                        # XY
        for i in range(1 << n):
            if ((i >> p0) ^ (i >> p1)) & 1:
                new[i] = c * state[i] + j * s * state[i ^ (1 << p0) ^ (1 << p1)]
    if pauli >= 0:
        digits = ((pauli >> 2, p0), (pauli & 3, p1)) if op >= 3 else ((pauli, p0),)
        for d, p in digits:
            if d >= 2:                                                   # Z part first: Y is X Z
                new = [-a if (i >> p) & 1 else a for i, a in enumerate(new)]
            if d in (1, 2):
                new = [new[i ^ (1 << p)] for i in range(1 << n)]
    return new


# --------------------------------------------------------------------------------------------------
# The reference's random programs (tests/test_compilation.py:96-154 of the reference, on gate lists)
# --------------------------------------------------------------------------------------------------
RANDOM_GATES = ("I", "X", "H", "T", "RX", "RY", "RZ", "CZ", "CNOT", "CCNOT", "SWAP")
RANDOM_ARITY = {"CZ": 2, "CNOT": 2, "SWAP": 2, "CCNOT": 3}
MAGIC = (-1.0, -0.5, 0.0, 0.5, 1.0)
RANDOM_WIDTHS, RANDOM_LENGTHS, RANDOM_REPEATS = (3, 4), (2, 50, 67), 10


def random_program(rng, n_qubits, length):
    """A gate drawn uniformly from the reference's set, on qubits drawn without replacement; RX takes one of its five magic
    angles, every other rotation an angle uniform in [-2 pi, 2 pi)."""
    prog = []
    for _ in range(length):
        name = RANDOM_GATES[int(rng.integers(len(RANDOM_GATES)))]
        qubits = tuple(int(q) for q in rng.choice(n_qubits, size=RANDOM_ARITY.get(name, 1), replace=False))
        if name == "RX":
            prog.append((name, qubits, MAGIC[int(rng.integers(5))] * np.pi))
        elif name in ("RY", "RZ"):
            prog.append((name, qubits, float(rng.uniform(-2 * np.pi, 2 * np.pi))))
        else:
            prog.append((name, qubits))
    return prog


def random_programs():
    """The programs of the reference's test_random_progs from one seeded generator: ``[(n_qubits, program)]``, 60 of them."""
    rng = np.random.default_rng(20241)
    return [(n, random_program(rng, n, length)) for n in RANDOM_WIDTHS for length in RANDOM_LENGTHS for _ in range(RANDOM_REPEATS)]


def assert_close_up_to_global_phase(actual, desired, atol=1e-12):
    from fbx.compilation import match_global_phase
    a, d = match_global_phase(np.asarray(actual), np.asarray(desired))
    np.testing.assert_allclose(a, d, rtol=1e-7, atol=atol)
