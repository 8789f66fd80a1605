"""The reversible-circuit sampler (csrc/fbx_reversible.hip) on the GPU: records, packed words and the fused histogram bit for bit
against the host restatement (which tests/test_reversible_cpu.py pins to a density-matrix simulation), noiseless adders up to 64
qubits, the histogram against fbx_bit_histogram, the stream properties, the poisoned-item and argument rules, and the public calls.
Shapes are the smallest that reach every path: shot counts on both sides of a wavefront (one unit per (item, input) or several: the
stored and the atomic form of the histogram), records of three bytes with odd shot counts (unaligned record starts), gate counts
of both parities."""
import ctypes as C
import functools

import numpy as np
import pytest

from fbx import _lib
from fbx.classical_logic import reversible as rev, ripple_carry_adder as rca

pytestmark = pytest.mark.gpu

SEED = 0xADDE5000C0FFEE
CLASS_ERROR = np.array([[0.02, 0.05, 0.11], [0.3, 0.2, 0.1], [0.0, 0.5, 0.0]])
MOST_SHOTS = 257


def readout(m):
    return np.array([[0.01 + 0.02 * j, 0.05 - 0.01 * j] for j in range(m)])


@functools.lru_cache(maxsize=None)
def circuit(n, in_x_basis):
    gates, out_qubits = rca.adder(*rca.default_adder_registers(n), in_x_basis=in_x_basis)
    words = rev.encode_reversible(gates, 2 * n + 2)
    return words, tuple(out_qubits), rev.gate_arity(words) - 1, rev.pack_records(rca.adder_expected_bits(n))


@functools.lru_cache(maxsize=None)
def restated(n, in_x_basis):
    """The restatement of the B = 3 noisy call at the largest shot count, computed once; fewer shots are its prefix."""
    words, out_qubits, cls, _ = circuit(n, in_x_basis)
    out = rev.restate_reversible_shots(words, 2 * n + 2, np.arange(4 ** n), out_qubits, MOST_SHOTS, CLASS_ERROR, cls, readout(n + 1),
                                       seed=SEED)
    out.setflags(write=False)
    return out


def sample(n, in_x_basis, shots, class_error=CLASS_ERROR, inputs=None, **kw):
    words, out_qubits, cls, expected = circuit(n, in_x_basis)
    inputs = np.arange(4 ** n) if inputs is None else inputs
    kw.setdefault("expected", expected[np.asarray(inputs, dtype=np.int64)])
    return rev.sample_reversible_shots(words, 2 * n + 2, inputs, out_qubits, shots, class_error, cls, readout(n + 1), SEED,
                                       bits=True, packed=True, counts=True, **kw)


# ------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize("shots", [1, 63, 64, 65, MOST_SHOTS])
@pytest.mark.parametrize("in_x_basis", [False, True])
@pytest.mark.parametrize("n", [1, 2])
def test_records_words_and_counts_equal_the_restatement(gpu, n, in_x_basis, shots):
    want = restated(n, in_x_basis)[:, :, :shots]
    got = sample(n, in_x_basis, shots)
    assert not got["status"].any()
    assert np.array_equal(got["packed"], want)
    assert got["bits"].shape == (3, 4 ** n, shots, n + 1)
    assert np.array_equal(got["bits"], rev.unpack_records(want, n + 1))
    assert np.array_equal(got["counts"], rev.weight_counts(want, circuit(n, in_x_basis)[3], n + 1))
    assert np.all(got["counts"].sum(axis=-1) == shots)


def test_device_pointer_form_equals_the_host_form(gpu):
    n, shots = 2, 65
    words, out_qubits, cls, expected = circuit(n, True)
    B, P, m = 3, 16, n + 1
    flips = np.ascontiguousarray(np.broadcast_to(readout(m), (B, m, 2)))
    with _lib.DeviceScope() as dev:
        d = [dev.upload(a) for a in (words, cls.astype(np.uint8), np.arange(P, dtype=np.uint64), np.array(out_qubits, dtype=np.uint8),
                                     expected, CLASS_ERROR, flips)]
        d_bits, d_words, d_counts, d_status = (dev.alloc(B * P * shots * m), dev.alloc(8 * B * P * shots),
                                               dev.alloc(8 * B * P * (m + 1)), dev.alloc(4 * B))
        _lib.check(_lib.lib().fbx_reversible_sample_shots_dev(2 * n + 2, words.size, d[0].ptr, d[1].ptr, 3, P, d[2].ptr, m, d[3].ptr,
                                                              d[4].ptr, B, shots, d[5].ptr, d[6].ptr, SEED, 0, 0, d_bits.ptr,
                                                              d_words.ptr, d_counts.ptr, d_status.ptr))
        _lib.synchronize()
        want = sample(n, True, shots)
        assert np.array_equal(d_bits.to_array(np.uint8, (B, P, shots, m)), want["bits"])
        assert np.array_equal(d_words.to_array(np.uint64, (B, P, shots)), want["packed"])
        assert np.array_equal(d_counts.to_array(np.int64, (B, P, m + 1)), want["counts"])
        assert np.array_equal(d_status.to_array(np.int32, (B,)), want["status"])


def test_each_output_alone(gpu):
    """Every output is optional: one at a time gives what all together give."""
    n, shots = 2, 65
    words, out_qubits, cls, expected = circuit(n, False)
    both = sample(n, False, shots)
    for key, kw in (("bits", dict(bits=True)), ("packed", dict(bits=False, packed=True)),
                    ("counts", dict(bits=False, counts=True, expected=expected))):
        got = rev.sample_reversible_shots(words, 2 * n + 2, np.arange(16), out_qubits, shots, CLASS_ERROR, cls, readout(n + 1), SEED, **kw)
        assert np.array_equal(got[key], both[key]), key


# ------------------------------------------------------------------ 2. noiseless runs
@pytest.mark.parametrize("in_x_basis", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_noiseless_adders_add(gpu, n, in_x_basis):
    results = rca.simulate_n_bit_adder_results(n, in_x_basis=in_x_basis, num_shots=70)
    assert results.shape == (4 ** n, 70, n + 1) and results.dtype == np.uint8
    assert np.array_equal(results, np.broadcast_to(rca.adder_expected_bits(n)[:, None, :], results.shape))
    assert rca.get_success_probabilities_from_results(results) == [1.0] * 4 ** n


@pytest.mark.parametrize("in_x_basis", [False, True])
def test_the_64_qubit_adder_adds(gpu, in_x_basis):
    """n = 31: 64 qubits, the z ancilla on bit 63, records of 32 columns."""
    n, ones = 31, 2 ** 31 - 1
    pairs = [(ones, 1), (ones, ones), (0, 0), (1, ones), (0x55555555, 0x2AAAAAAA), (0x12345678, 0x7EDCBA98), (2 ** 30, 2 ** 30)]
    inputs = np.array([(a << n) | b for a, b in pairs], dtype=np.uint64)
    gates, out_qubits = rca.adder(*rca.default_adder_registers(n), in_x_basis=in_x_basis)
    assert max(out_qubits) == 63
    words = rev.encode_reversible(gates, 64)
    want = np.array([[((a + b) >> (n - j)) & 1 for j in range(n + 1)] for a, b in pairs], dtype=np.uint8)
    expected = rev.pack_records(want)
    got = rev.sample_reversible_shots(words, 64, inputs, out_qubits, 3, expected=expected, packed=True, counts=True)
    assert np.array_equal(got["bits"][0], np.broadcast_to(want[:, None, :], (len(pairs), 3, n + 1)))
    assert np.array_equal(got["packed"][0], np.broadcast_to(expected[:, None], (len(pairs), 3)))
    assert np.array_equal(got["counts"][0, :, 0], np.full(len(pairs), 3)) and not got["counts"][0, :, 1:].any()
    assert np.array_equal(rev.gather_record(rev.evaluate(words, 64, inputs), out_qubits), expected)
    success, hamming = rca.simulate_adder_statistics_batch(n, np.zeros((1, 3)), in_x_basis=in_x_basis, num_shots=5, inputs=inputs)
    assert np.all(success == 1.0) and hamming.shape == (1, len(pairs), n + 2)


def test_a_64_column_record(gpu):
    """m = 64: every qubit is read, and the histogram has 65 entries."""
    gates = [("XIN", (q, q)) for q in range(64)] + [("CNOT", (0, 63)), ("CCNOT", (1, 2, 62))]
    words = rev.encode_reversible(gates, 64)
    inputs = np.array([0, 2 ** 64 - 1, 1, 6, 0x8000000000000001], dtype=np.uint64)
    out_qubits = list(range(63, -1, -1))
    state = rev.evaluate(words, 64, inputs)
    assert [int(s) for s in state] == [0, 2 ** 64 - 1 - 2 ** 63 - 2 ** 62, 1 + 2 ** 63, 6 + 2 ** 62, 1]
    records = rev.gather_record(state, out_qubits)
    got = rev.sample_reversible_shots(words, 64, inputs, out_qubits, 66, expected=~records, packed=True, counts=True)
    assert np.array_equal(got["packed"][0], np.broadcast_to(records[:, None], (5, 66)))
    assert np.array_equal(got["bits"][0], rev.unpack_records(got["packed"][0], 64))
    assert np.all(got["counts"][0, :, 64] == 66) and not got["counts"][0, :, :64].any()


# ------------------------------------------------------------------ 3. the fused histogram
@pytest.mark.parametrize("shots", [64, 100])
def test_counts_are_the_histogram_of_the_records(gpu, shots):
    """weight_counts / n_shots against fbx_bit_histogram over the same call's records, exactly; one wavefront per unit (stored)
    and two (added)."""
    got = sample(2, True, shots)
    want = rca.get_error_hamming_distributions_from_results_batch(got["bits"])
    assert np.array_equal(got["counts"] / float(shots), want)
    success, hamming = rca.simulate_adder_statistics_batch(2, CLASS_ERROR, in_x_basis=True, num_shots=shots,
                                                           readout_flip=readout(3), seed=SEED)
    assert np.array_equal(hamming, want) and np.array_equal(success, want[:, :, 0])
    assert np.array_equal(success, rca.get_success_probabilities_from_results_batch(got["bits"]))


# ------------------------------------------------------------------ 4. the stream
def test_a_record_depends_on_its_own_indices_only(gpu):
    full = sample(2, True, 130)
    item = sample(2, True, 130, class_error=CLASS_ERROR[1:2], first_item=1)
    for key in ("bits", "packed", "counts"):
        assert np.array_equal(item[key][0], full[key][1]), key
    inputs = np.arange(5, 16)
    part = sample(2, True, 130, inputs=inputs, first_input=5, expected=circuit(2, True)[3][5:])
    for key in ("bits", "packed", "counts"):
        assert np.array_equal(part[key], full[key][:, 5:]), key
    fewer = sample(2, True, 70)
    assert np.array_equal(fewer["bits"], full["bits"][:, :, :70]) and np.array_equal(fewer["packed"], full["packed"][:, :, :70])
    other = rev.sample_reversible_shots(*_call_args(2, True), 130, CLASS_ERROR, circuit(2, True)[2], readout(3), SEED + 1, packed=True)
    assert not np.array_equal(other["packed"], full["packed"])


def _call_args(n, in_x_basis):
    words, out_qubits, _, _ = circuit(n, in_x_basis)
    return words, 2 * n + 2, np.arange(4 ** n), out_qubits


# ------------------------------------------------------------------ 5. a poisoned item
@pytest.mark.parametrize("where", ["class_error", "readout_flip"])
@pytest.mark.parametrize("shots", [40, 100])
def test_a_poisoned_middle_item(gpu, where, shots):
    words, out_qubits, cls, expected = circuit(2, False)
    good = sample(2, False, shots)
    ce, flips = CLASS_ERROR.copy(), np.ascontiguousarray(np.broadcast_to(readout(3), (3, 3, 2)))
    if where == "class_error":
        ce[1, 2] = np.nan
    else:
        flips[1, 2, 1] = 1.5
    got = rev.sample_reversible_shots(words, 6, np.arange(16), out_qubits, shots, ce, cls, flips, SEED, expected=expected,
                                      packed=True, counts=True)
    assert list(got["status"]) == [0, 1, 0]
    assert not got["bits"][1].any() and not got["packed"][1].any() and not got["counts"][1].any()
    for key in ("bits", "packed", "counts"):
        assert np.array_equal(got[key][[0, 2]], good[key][[0, 2]]), key
    success, hamming = rca.simulate_adder_statistics_batch(2, ce, num_shots=shots, readout_flip=flips, seed=SEED)
    assert np.isnan(success[1]).all() and np.isnan(hamming[1]).all() and np.array_equal(hamming[0], good["counts"][0] / float(shots))


# ------------------------------------------------------------------ 6. refusals
def raw_call(**over):
    """fbx_reversible_sample_shots on a small valid call with some arguments replaced; the output buffers are filled with 7."""
    words, out_qubits, cls, expected = circuit(1, False)
    a = dict(n=4, G=words.size, words=words, cls=cls.astype(np.uint8), K=3, P=4, inputs=np.arange(4, dtype=np.uint64), m=2,
             out=np.array(out_qubits, dtype=np.uint8), expected=expected, B=2, shots=5, ce=np.zeros((2, 3)), flips=None, seed=1,
             first_item=0, first_input=0, bits=np.full(2 * 4 * 5 * 2, 7, dtype=np.uint8), packed=np.full(40, 7, dtype=np.uint64),
             counts=np.full(24, 7, dtype=np.int64), status=np.full(2, 7, dtype=np.int32))
    a.update(over)
    rc = _lib.lib().fbx_reversible_sample_shots(
        a["n"], a["G"], _lib.ptr(a["words"], C.c_uint32), _lib.ptr(a["cls"], C.c_uint8), a["K"], a["P"], _lib.ptr(a["inputs"], C.c_uint64),
        a["m"], _lib.ptr(a["out"], C.c_uint8), _lib.ptr(a["expected"], C.c_uint64), a["B"], a["shots"], _lib.dptr(a["ce"]),
        _lib.dptr(a["flips"]), a["seed"], a["first_item"], a["first_input"], _lib.ptr(a["bits"], C.c_uint8),
        _lib.ptr(a["packed"], C.c_uint64), _lib.ptr(a["counts"], C.c_int64), _lib.iptr(a["status"]))
    return rc, a


REFUSED = {
    "no qubits": dict(n=0), "65 qubits": dict(n=65), "no columns": dict(m=0), "65 columns": dict(m=65),
    "a word's qubit outside the width": dict(n=3),
    "an unknown micro-op": dict(words=np.array([7 | (1 << 3)] * 9, dtype=np.uint32)),
    "a repeated operand": dict(words=np.array([2 | (2 << 3) | (1 << 5) | (1 << 11)] * 9, dtype=np.uint32)),
    "out_qubits outside the width": dict(out=np.array([3, 4], dtype=np.uint8)),
    "no classes": dict(K=0), "17 classes": dict(K=17), "a class that is not below K": dict(K=2),
    "negative G": dict(G=-1), "negative B": dict(B=-1), "negative P": dict(P=-1), "negative shots": dict(shots=-1),
    "negative first_item": dict(first_item=-1), "negative first_input": dict(first_input=-1),
    "2^32 shots": dict(shots=2 ** 32), "an item index of 2^32": dict(first_item=2 ** 32 - 1),
    "an input index of 2^32": dict(first_input=2 ** 32 - 3),
    "a grid beyond 2^31 workgroups": dict(B=2 ** 16, P=2 ** 16, shots=2 ** 31),
    "counts without expected": dict(expected=None), "no output": dict(bits=None, packed=None, counts=None),
    "NULL words": dict(words=None), "NULL inputs": dict(inputs=None), "NULL out_qubits": dict(out=None),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refusals(gpu, what):
    rc, a = raw_call(**REFUSED[what])
    assert rc == _lib.FBX_ERR_BAD_ARG, what
    assert b"fbx_reversible_sample_shots" in _lib.lib().fbx_last_error()
    for key in ("bits", "packed", "counts", "status"):                  # before any buffer is touched
        assert a[key] is None or np.all(a[key] == 7), (what, key)


def test_the_device_pointer_form_refuses_too(gpu):
    with _lib.DeviceScope() as dev:
        buf = dev.alloc(4096)
        for over in (dict(K=0), dict(m=65), dict(counts=False, bits=False), dict(expected=False)):
            a = dict(K=3, m=2, counts=True, bits=True, expected=True)
            a.update(over)
            rc = _lib.lib().fbx_reversible_sample_shots_dev(4, 9, buf.ptr, None, a["K"], 4, buf.ptr, a["m"], buf.ptr,
                                                            buf.ptr if a["expected"] else None, 1, 5, None, None, 0, 0, 0,
                                                            buf.ptr if a["bits"] else None, None, buf.ptr if a["counts"] else None, None)
            assert rc == _lib.FBX_ERR_BAD_ARG, over


@pytest.mark.parametrize("empty", [dict(B=0), dict(P=0), dict(shots=0)])
def test_an_empty_call_does_nothing(gpu, empty):
    rc, a = raw_call(**empty)
    assert rc == _lib.FBX_OK
    for key in ("bits", "packed", "counts", "status"):
        assert np.all(a[key] == 7), key


def test_the_encoder_refuses_an_input_bit_of_64(gpu):
    """The word has six bits for XIN's input bit: an index of 64 cannot reach the library and is refused where words are made."""
    with pytest.raises(ValueError):
        rev.encode_reversible([("XIN", (0, 64))], 2)
    with pytest.raises(ValueError):
        rca.simulate_adder_statistics_batch(2, np.zeros((1, 3)), inputs=[16])
    with pytest.raises(ValueError):
        rca.simulate_n_bit_adder_results(2, gate_error=(0.1, 1.5, 0.0))


# ------------------------------------------------------------------ 7. the public wiring
@pytest.mark.parametrize("in_x_basis", [False, True])
def test_simulated_statistics_follow_the_predicted_ones(gpu, in_x_basis):
    """n = 2, 20 000 shots: every frequency within 6 sqrt(p (1 - p) / S) + 1 / S of its exact probability.  The bit-for-bit test
    above and the CPU test of the restatement give this for the kernel; here it is the public calls that are held to it."""
    S = 20000
    ce = np.array([[0.02, 0.05, 0.11], [0.001, 0.01, 0.03]])
    flips = np.array([[0.01, 0.04], [0.03, 0.02], [0.0, 0.06]])
    success, hamming = rca.simulate_adder_statistics_batch(2, ce, in_x_basis=in_x_basis, num_shots=S, readout_flip=flips, seed=SEED)
    p_success, p = rca.predicted_adder_statistics(2, ce, in_x_basis=in_x_basis, readout_flip=flips)
    assert hamming.shape == p.shape == (2, 16, 4)
    bound = 6.0 * np.sqrt(p * (1.0 - p) / S) + 1.0 / S
    print("largest deviation / bound:", float((np.abs(hamming - p) / bound).max()))
    assert np.all(np.abs(hamming - p) <= bound)
    assert np.all(np.abs(success - p_success) <= bound[:, :, 0])


def test_custom_noise_classes(gpu):
    """noise_class / class_error in place of the three default classes (here: only the Toffolis err): the records equal the
    restatement under the same classes."""
    words, out_qubits, cls, _ = circuit(2, False)
    custom = np.where(cls == 2, 0, 255).astype(np.uint8)
    results = rca.simulate_n_bit_adder_results(2, num_shots=90, noise_class=custom, class_error=[0.4], seed=SEED)
    want = rev.restate_reversible_shots(words, 6, np.arange(16), out_qubits, 90, np.array([[0.4]]), custom, None, seed=SEED)
    assert np.array_equal(results, rev.unpack_records(want[0], 3))
    assert 0.0 < np.mean(rca.get_success_probabilities_from_results(results)) < 1.0
