"""fbx.native_circuit without a GPU: the word, the numpy mirror against dense kron products, the density-matrix evaluation of
the noise model, and the restated stream of fbx_native_trajectories against both."""
import numpy as np
import pytest

import native_cases as cases
from fbx import native_circuit as nc
from fbx.compilation import gate_matrix

I2, X, Z = np.eye(2), np.array([[0.0, 1.0], [1.0, 0.0]]), np.diag([1.0, -1.0])
PAULI = [I2, X, X @ Z, Z]                                            # Y as X Z: the mirror's and the kernel's convention


def test_the_word():
    gates = [("I", (2,)), ("RX", (0,), 0.25), ("RZ", (12,), -3.0), ("CZ", (3, 11)), ("XY", (11, 3), 0.5), ("RX", (1,), np.pi, 63),
             ("CZ", (0, 1), None, 5), ("I", (4,), None, 0)]
    words, angles = nc.encode_native(gates, 13)
    assert words.dtype == np.uint32 and angles.dtype == np.float64
    assert words.tolist() == [0 | 2 << 3, 1, 2 | 12 << 3, 3 | 3 << 3 | 11 << 7, 4 | 11 << 3 | 3 << 7, 1 | 1 << 3 | 1 << 11 | 63 << 12,
                              3 | 1 << 7 | 1 << 11 | 5 << 12, 4 << 3 | 1 << 11]
    assert angles.tolist() == [0.0, 0.25, -3.0, 0.0, 0.5, np.pi, 0.0, 0.0]
    assert nc.decode_native(words, angles) == gates
    assert nc.encode_native(nc.decode_native(words, angles), 13)[0].tolist() == words.tolist()
    assert nc.native_noise_classes(words).tolist() == [0, 0, 1, 2, 2, 0, 2, 0]
    assert nc.check_words(words, 13) is not None and nc.encode_native([], 1)[0].size == 0


@pytest.mark.parametrize("gates,n", [
    ([("H", (0,))], 2), ([("RX", (0,), 0.1), ("RX", (2,), 0.1)], 2), ([("CZ", (0, 0))], 2), ([("CZ", (0,))], 2), ([("RX", (0, 1), 0.1)], 2),
    ([("RX", (0,))], 1), ([("RX", (0,), np.inf)], 1), ([("CZ", (0, 1), 0.5)], 2), ([("RX", (0,), 0.1, 64)], 1), ([("I", (-1,))], 1),
    ([("I", (0,))], 0), ([("I", (0,))], 14), (["RX"], 1)])
def test_encode_refusals(gates, n):
    with pytest.raises(ValueError):
        nc.encode_native(gates, n)


def test_check_words_refusals():
    ok = nc.encode_native([("RX", (1,), 0.1), ("CZ", (0, 1))], 2)[0]
    for l, w in ((0, 5), (0, 1 | 2 << 3), (0, 1 | 1 << 3 | 1 << 7), (1, 3 | 1 << 3 | 1 << 7), (1, 3 | 2 << 7), (0, 1 | 1 << 12), (0, 1 | 1 << 18)):
        bad = ok.copy()
        bad[l] = w
        with pytest.raises(ValueError, match=f"word {l} "):
            nc.check_words(bad, 2)
    with pytest.raises(ValueError):
        nc.check_words(ok, 2, [0.1])
    with pytest.raises(ValueError, match="gate 1"):
        nc.check_words(ok, 2, [0.1, np.nan])


def embed(matrix, qubits, n):
    """``matrix`` on ``qubits`` (first = most significant bit of its index) as a dense 2^n x 2^n matrix, qubit 0 the most
    significant bit: built entry by entry, independently of the mirror's tensordot."""
    N, k = 1 << n, len(qubits)
    full = np.zeros((N, N), dtype=np.complex128)
    for col in range(N):
        sub = sum(((col >> (n - 1 - q)) & 1) << (k - 1 - i) for i, q in enumerate(qubits))
        for out in range(1 << k):
            row = col
            for i, q in enumerate(qubits):
                row = (row & ~(1 << (n - 1 - q))) | (((out >> (k - 1 - i)) & 1) << (n - 1 - q))
            full[row, col] += matrix[out, sub]
    return full


def test_embed_is_kron():
    a, b = gate_matrix("RX", 0.3), gate_matrix("RZ", 1.1)
    assert np.allclose(embed(a, (0,), 2), np.kron(a, I2)) and np.allclose(embed(b, (1,), 2), np.kron(I2, b))
    assert np.allclose(embed(np.kron(a, b), (0, 1), 2), np.kron(a, b))
    assert np.allclose(embed(np.kron(a, b), (2, 0), 3), np.kron(np.kron(b, I2), a))


@pytest.mark.parametrize("n", [1, 2, 3])
def test_mirror_against_dense_products(n):
    rng = np.random.default_rng(n)
    state = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    state /= np.linalg.norm(state)
    one = [(name, (q,), 0.7 + q) if name != "I" else (name, (q,)) for name in ("I", "RX", "RZ") for q in range(n)]
    two = [(name, (a, b)) + ((1.3,) if name == "XY" else ()) for name in ("CZ", "XY") for a in range(n) for b in range(n) if a != b]
    for gate in one + two:
        words, angles = nc.encode_native([gate], n)
        k = len(gate[1])
        matrix = gate_matrix(gate[0], gate[2] if len(gate) > 2 else None)
        want = embed(matrix, gate[1], n) @ state
        assert np.abs(nc.apply_native(words, angles, n, state) - want).max() <= 1e-15
        for index in range(4 ** k):                                  # the Pauli after the gate: operand i has digit k - 1 - i
            pauli = np.ones((1, 1))
            for i in range(k):
                pauli = np.kron(pauli, PAULI[(index >> (2 * (k - 1 - i))) & 3])
            got = nc.apply_native(words, angles, n, state, 0, [index])
            assert np.abs(got - embed(pauli, gate[1], n) @ want).max() <= 1e-15
        # conditional: there with the bit set, absent -- Pauli and all -- without
        cw, ca = nc.encode_native([gate[:2] + (gate[2] if len(gate) > 2 else None, 3)], n)
        assert np.abs(nc.apply_native(cw, ca, n, state, 0b1000, [1]) - nc.apply_native(words, angles, n, state, 0, [1])).max() == 0.0
        assert np.array_equal(nc.apply_native(cw, ca, n, state, 0b0111, [1]), state)
    # gates compose from the left
    seq = one + two
    words, angles = nc.encode_native(seq, n)
    want = state
    for gate in seq:
        want = embed(gate_matrix(gate[0], gate[2] if len(gate) > 2 else None), gate[1], n) @ want
    assert np.abs(nc.apply_native(words, angles, n, state) - want).max() <= 1e-14


def test_marginal_distribution():
    p = np.arange(8, dtype=float)                                    # index = q0 q1 q2
    assert np.array_equal(nc.marginal_distribution(p, 3, [0, 1, 2]), p)
    assert np.array_equal(nc.marginal_distribution(p, 3, [2]), [0 + 2 + 4 + 6, 1 + 3 + 5 + 7])
    assert np.array_equal(nc.marginal_distribution(p, 3, [2, 0]), [0 + 2, 4 + 6, 1 + 3, 5 + 7])       # column 0 = qubit 2 = the high bit
    for bad in ([], [0, 0], [3], [0, 1, 2, 1]):
        with pytest.raises(ValueError):
            nc.marginal_distribution(p, 3, bad)


def test_exact_distribution_on_known_channels():
    # RX(pi) then a certain error: uniformly I, X, Y, Z -> the qubit is maximally mixed
    words, angles = nc.encode_native([("RX", (0,), np.pi)], 1)
    assert np.allclose(nc.exact_native_distribution(words, angles, 1, 0, [1.0]), [0.5, 0.5], atol=1e-15)
    assert np.allclose(nc.exact_native_distribution(words, angles, 1, 0, [0.2]), [0.1, 0.9], atol=1e-15)
    # classes: the error of RZ does not reach a gate of class 0; 255 is noiseless
    assert np.allclose(nc.exact_native_distribution(words, angles, 1, 0, [0.0, 1.0, 1.0], [0]), [0.0, 1.0], atol=1e-15)
    assert np.allclose(nc.exact_native_distribution(words, angles, 1, 0, [1.0], [255]), [0.0, 1.0], atol=1e-15)
    # a Bell pair, then a certain error on both qubits of a CZ: I / 4; a marginal of it
    bell = [("RX", (0,), np.pi / 2), ("RZ", (0,), -np.pi / 2), ("RX", (0,), -np.pi / 2), ("RZ", (0,), np.pi)]
    words, angles = nc.encode_native(bell + [("CZ", (0, 1))], 2)
    cls = nc.native_noise_classes(words)
    assert np.allclose(nc.exact_native_distribution(words, angles, 2, 0, [0, 0, 0], cls), [0.5, 0, 0.5, 0], atol=1e-15)
    assert np.allclose(nc.exact_native_distribution(words, angles, 2, 0, [0, 0, 1], cls), [0.25] * 4, atol=1e-15)
    assert np.allclose(nc.exact_native_distribution(words, angles, 2, 0, [0, 0, 0.4], cls, [1]), [0.8, 0.2], atol=1e-15)
    # a conditional gate exists, with its error site, only where the bit is set
    words, angles = nc.encode_native([("RX", (0,), np.pi, 2)], 1)
    assert np.allclose(nc.exact_native_distribution(words, angles, 1, 0b100, [0.2]), [0.1, 0.9], atol=1e-15)
    assert np.allclose(nc.exact_native_distribution(words, angles, 1, 0b011, [0.2]), [1.0, 0.0], atol=1e-15)


def test_restated_stream_properties():
    case = {"n": 3, "G": 8, "T": 9, "out": [2, 0]}
    words, angles, cls, res = cases.restated(case)
    assert res["paulis"].shape == (3, 2, 9, 8) and res["n_errors"].shape == (3, 2, 9) and not res["status"].any()
    assert (res["paulis"][0] == -1).all() and not res["n_errors"][0].any()
    # error 1: every gate that exists errs; with both inputs every gate exists for one of them
    exists = np.array([[not ((w >> 11) & 1) or (int(word) >> ((w >> 12) & 63)) & 1 for w in words.tolist()] for word in cases.INPUTS])
    assert exists.any(axis=0).all() and not exists.all()
    assert np.array_equal(res["paulis"][1] >= 0, np.broadcast_to(exists[:, None, :], (2, 9, 8)))
    two = np.isin(words & 7, (3, 4))
    assert res["paulis"][1][:, :, ~two].max() <= 3 and res["paulis"][1][:, :, two].max() > 3
    assert np.allclose(res["probs_mean"].sum(axis=2), 1.0, atol=1e-14)
    # an item, an input and a trajectory are what their global indices say
    sub = nc.restate_native_trajectories(words, angles, 3, cases.INPUTS[1:], [2, 0], 5, cases.CLASS_ERROR[2:], cls, 11, first_item=2, first_input=1)
    assert np.array_equal(sub["paulis"][0, 0], res["paulis"][2, 1, :5])
    other = nc.restate_native_trajectories(words, angles, 3, cases.INPUTS, [2, 0], 9, cases.CLASS_ERROR, cls, 12, probs=False)
    assert not np.array_equal(other["paulis"][2], res["paulis"][2]) and "probs_mean" not in other
    # a poisoned item
    for bad in (-0.1, 1.5, np.nan):
        ce = cases.CLASS_ERROR.copy()
        ce[1, 0] = bad
        got = nc.restate_native_trajectories(words, angles, 3, cases.INPUTS, [2, 0], 9, ce, cls, 11)
        assert got["status"].tolist() == [0, 1, 0] and np.isnan(got["probs_mean"][1]).all() and not got["n_errors"][1].any()
        assert np.array_equal(got["probs_mean"][2], res["probs_mean"][2])


def test_restated_mean_against_the_exact_distribution():
    """T = 4096 trajectories of a 2-qubit circuit of 6 gates with errors of order 0.1: every probability of the restated mean
    within 5 standard errors of the density-matrix answer, the standard error being that of a mean of T independent
    trajectories (sample deviation of the trajectories' own probabilities over sqrt(T)).  The seed was chosen here, on the
    CPU, as one for which this host-only computation satisfies the bound; a 5-sigma bound on 16 values fails for about one
    seed in 10^5, so nearly any would do."""
    T, seed = 4096, 3
    gates = [("RX", (0,), 0.7), ("RZ", (1,), 1.3), ("CZ", (0, 1)), ("XY", (1, 0), 0.9), ("I", (0,)), ("RX", (1,), -0.4, 0)]
    words, angles = nc.encode_native(gates, 2)
    cls = nc.native_noise_classes(words)
    ce = np.array([[0.1, 0.05, 0.15], [0.2, 0.0, 0.1]])
    res = nc.restate_native_trajectories(words, angles, 2, [1], [1, 0], T, ce, cls, seed)
    zero = np.array([1.0, 0, 0, 0], dtype=np.complex128)
    for b in range(2):
        exact = nc.exact_native_distribution(words, angles, 2, 1, ce[b], cls, [1, 0])
        assert abs(exact.sum() - 1.0) < 1e-14
        memo = {}
        per = np.empty((T, 4))
        for t in range(T):
            key = res["paulis"][b, 0, t].tobytes()
            if key not in memo:
                memo[key] = nc.marginal_distribution(np.abs(nc.apply_native(words, angles, 2, zero, 1, res["paulis"][b, 0, t])) ** 2, 2, [1, 0])
            per[t] = memo[key]
        assert np.abs(per.mean(axis=0) - res["probs_mean"][b, 0]).max() < 1e-13
        std_err = per.std(axis=0, ddof=1) / np.sqrt(T)
        sigmas = np.abs(res["probs_mean"][b, 0] - exact) / std_err
        print("item", b, "deviation in standard errors", sigmas)
        assert (std_err > 0).all() and sigmas.max() <= 5.0
        rate = (res["paulis"][b, 0] >= 0).mean(axis=0)
        want = np.array([ce[b, c] for c in cls])
        assert np.abs(rate - want).max() <= 5.0 * np.sqrt(0.25 / T)


def test_mirror_deviation_stays_below_the_recorded_value():
    """The measurement behind the GPU tests' tolerance, repeated on the narrow cases (a second or two)."""
    narrow = [c for c in cases.CASES if c["n"] <= 7]
    worst = cases.measure_mirror_deviation(narrow)
    print("mirror against mpmath:", worst)
    assert 0.0 < worst <= cases.MIRROR_DEVIATION
    assert cases.TOL == 8.0 * cases.MIRROR_DEVIATION
    # ... and on the shortest compiled adder and the statistics case, each against its own recorded value
    gates, worst = cases.adder_mirror_deviation(1, False)
    print("1-bit adder, Z basis:", gates, "gates,", worst)
    assert (gates, True) == (cases.ADDER_MIRROR_DEVIATION[(1, False)][0], 0.0 < worst <= cases.ADDER_MIRROR_DEVIATION[(1, False)][1])
    worst = cases.adder_stats_mirror_deviation()
    print("statistics case:", worst)
    assert 0.0 < worst <= cases.ADDER_STATS_MIRROR_DEVIATION


def test_constants_match_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "fbx.h")).read()
    source = open(os.path.join(root, "forest-benchmarking_amd", "csrc", "fbx_native.hip")).read()
    for name, op in nc.OPCODES.items():
        assert re.search(r"#define FBX_NAT_%s %d\b" % (name, op), header)
    assert re.search(r"#define FBX_NAT_WAVE_MAX_QUBITS %d\b" % nc.WAVE_MAX_QUBITS, header) and nc.WAVE_MAX_QUBITS == cases.WAVE
    assert re.search(r"NAT_SEG = %d;" % nc.SEGMENT, source) and nc.SEGMENT == cases.SEG
    assert "0x%08X" % nc.NATIVE_KEY_TAG in header and "0x%08Xu" % nc.NATIVE_KEY_TAG in source
    tags = re.findall(r"seed low \^\s*(0x[0-9A-F]{8})", header)
    assert tags.count("0x%08X" % nc.NATIVE_KEY_TAG) == 1                # no other stream uses the tag
