"""The Pauli-frame sampler (csrc/fbx_frames.hip) on the GPU: the reference outcome and every shot bit for bit against the host mirror
(which tests/test_frames_cpu.py pins to dense simulations), the stream properties, the poisoned-item and argument rules, and the
resident GHZ / graph-state chains.  Shapes are the smallest that reach every path: widths on both sides of 32 bits and at 64, gate
counts of both parities (the pairing of gates in a Philox block), shot counts on both sides of a wavefront and of a workgroup."""
import ctypes as C

import numpy as np
import pytest

import dfe_cases as dc
import frames_cases as fc
from fbx import _lib, clifford_circuit as cc, entangled_states as es, sampling

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE1234567


def reference_dev(gates, n):
    """fbx_clifford_reference_sample_dev on caller-owned buffers."""
    words = cc.encode_gates(gates, n)
    d_gates, d_ref = _lib.DeviceBuffer.from_array(words if words.size else np.zeros(1, dtype=np.uint32)), _lib.DeviceBuffer(8)
    try:
        _lib.check(_lib.lib().fbx_clifford_reference_sample_dev(n, words.size, d_gates.ptr, d_ref.ptr))
        return int(d_ref.to_array(np.uint64, (1,))[0])
    finally:
        d_gates.free()
        d_ref.free()


# ------------------------------------------------------------------ 7. the reference sample
def test_reference_sample_equals_the_mirror_on_the_dense_cases(gpu):
    for i, (n, gates, _) in enumerate(fc.case_circuits()):
        want = cc.reference_sample(gates, n)
        assert cc.reference_sample(gates, n, device=0) == want, (n, gates)
        if i % 8 == 0:
            assert reference_dev(gates, n) == want, (n, gates)


@pytest.mark.parametrize("n", [31, 32, 33, 63, 64])
def test_reference_sample_equals_the_mirror_at_the_mask_edges(gpu, n):
    nonzero = 0
    for n_gates in (0, 1, 2, 3, 300):
        for seed in range(3 if n_gates == 300 else 1):
            gates = fc.wide_circuit(n, n_gates, seed)
            want = cc.reference_sample(gates, n)
            assert cc.reference_sample(gates, n, device=0) == want, (n, n_gates, seed)
            assert reference_dev(gates, n) == want, (n, n_gates, seed)
            nonzero += want != 0
    assert nonzero >= 1
    assert cc.reference_sample([("X", (q,)) for q in range(n)], n, device=0) == 2 ** n - 1


# ------------------------------------------------------------------ 8. the shots
def noise_case(n, n_gates):
    """B = 3 items with distinct noise over K = 16 scattered classes (a fifth of the gates noiseless, class 3 without error in
    item 1, item 2 without gate noise at all) and asymmetric flips."""
    rng = np.random.default_rng(100 * n + n_gates)
    classes = rng.integers(0, 16, size=n_gates).astype(np.uint8)
    classes[rng.random(n_gates) < 0.2] = 255
    errors = rng.random((3, 16)) * 0.5
    errors[1, 3] = 0.0
    errors[2] = 0.0
    errors[0, 5] = 1.0
    flips = rng.random((3, n, 2)) * 0.3
    flips[1, 0] = (0.0, 1.0)
    return classes, errors, flips


@pytest.mark.parametrize("n", [1, 2, 5, 32, 33, 64])
def test_shots_equal_the_mirror_bit_for_bit(gpu, n):
    for n_gates in (0, 1, 2, 3, 57):
        gates = fc.wide_circuit(n, n_gates)
        classes, errors, flips = noise_case(n, n_gates)
        for with_flips in (False, True):
            rf = flips if with_flips else None
            want = cc.restate_frame_shots(gates, n, 1000, errors, classes, rf, seed=SEED, first_item=7)
            for shots in (1, 65, 1000):
                bits = sampling.sample_clifford_circuit_batch(gates, n, shots, errors, classes, rf, seed=SEED, first_item=7)
                words = sampling.sample_clifford_circuit_batch(gates, n, shots, errors, classes, rf, seed=SEED, first_item=7,
                                                               packed=True)
                assert bits.shape == (3, shots, n) and bits.dtype == np.uint8 and words.dtype == np.uint64
                assert np.array_equal(words, want[:, :shots]), (n, n_gates, with_flips, shots)
                assert np.array_equal(bits, cc.unpack_shots(want[:, :shots], n)), (n, n_gates, with_flips, shots)
    if n >= 2:
        assert len(np.unique(want)) > 3                       # the last case is not a constant


def test_both_outputs_of_one_call_agree(gpu):
    n, shots = 33, 300
    gates = fc.wide_circuit(n, 57)
    classes, errors, flips = noise_case(n, 57)
    words_in = cc.encode_gates(gates, n)
    ref = np.array([cc.reference_sample(gates, n)], dtype=np.uint64)
    bits, words, status = np.zeros((3, shots, n), dtype=np.uint8), np.zeros((3, shots), dtype=np.uint64), np.full(3, -1, dtype=np.int32)
    _lib.check(_lib.lib().fbx_clifford_sample_shots(n, 57, _lib.ptr(words_in, C.c_uint32), _lib.ptr(classes, C.c_uint8), 16,
                                                    _lib.ptr(ref, C.c_uint64), 3, shots, _lib.dptr(errors), _lib.dptr(flips), SEED, 0,
                                                    _lib.ptr(bits, C.c_uint8), _lib.ptr(words, C.c_uint64), _lib.iptr(status)))
    assert np.array_equal(words, cc.restate_frame_shots(gates, n, shots, errors, classes, flips, seed=SEED))
    assert np.array_equal(bits, cc.unpack_shots(words, n)) and not status.any()


# ------------------------------------------------------------------ 9. stream properties
def test_stream_properties(gpu):
    n, n_gates = 33, 57
    gates = fc.wide_circuit(n, n_gates)
    classes, errors, flips = noise_case(n, n_gates)
    draw = lambda **kw: sampling.sample_clifford_circuit_batch(gates, n, packed=True, seed=SEED, **kw)      # noqa: E731
    full = draw(shots=1000, class_error=errors, noise_class=classes, readout_flip=flips, first_item=7)
    tail = draw(shots=1000, class_error=errors[1:], noise_class=classes, readout_flip=flips[1:], first_item=8)
    assert np.array_equal(tail, full[1:])
    head = draw(shots=100, class_error=errors, noise_class=classes, readout_flip=flips, first_item=7)
    assert np.array_equal(head, full[:, :100])
    clean = draw(shots=1000, first_item=7)
    assert np.array_equal(draw(shots=1000, class_error=np.zeros((1, 16)), noise_class=classes, first_item=7), clean)
    assert np.array_equal(draw(shots=1000, class_error=np.zeros((1, 16)), noise_class=classes, readout_flip=np.zeros((n, 2)),
                               first_item=7), clean)
    assert np.array_equal(draw(shots=1000, class_error=errors[:1], noise_class=np.full(n_gates, 255, dtype=np.uint8), first_item=7),
                          clean)
    assert not np.array_equal(full[:1], clean)


# ------------------------------------------------------------------ 10. poisoned items and argument errors
@pytest.mark.parametrize("bad", [np.nan, -0.1, 1.5])
@pytest.mark.parametrize("where", ["class_error", "readout_flip"])
def test_poisoned_item_gets_zeros_and_its_neighbours_are_untouched(gpu, where, bad):
    n, n_gates, shots = 5, 57, 300
    gates = fc.wide_circuit(n, n_gates) + [("X", (0,))]
    classes, errors, flips = noise_case(n, n_gates + 1)
    clean_bits = sampling.sample_clifford_circuit_batch(gates, n, shots, errors, classes, flips, seed=SEED)
    clean_words = sampling.sample_clifford_circuit_batch(gates, n, shots, errors, classes, flips, seed=SEED, packed=True)
    assert clean_bits[1].any()
    if where == "class_error":
        errors = errors.copy()
        errors[1, 15] = bad
    else:
        flips = flips.copy()
        flips[1, n - 1, 1] = bad
    for packed, clean in ((False, clean_bits), (True, clean_words)):
        got, status = sampling.sample_clifford_circuit_batch(gates, n, shots, errors, classes, flips, seed=SEED, packed=packed,
                                                             return_status=True)
        assert status.tolist() == [0, 1, 0]
        assert not got[1].any() and np.array_equal(got[[0, 2]], clean[[0, 2]])
    with pytest.raises(ValueError, match="item 1"):
        sampling.sample_clifford_circuit_batch(gates, n, shots, errors, classes, flips, seed=SEED)


def test_argument_errors_leave_the_buffers_untouched(gpu):
    lib = _lib.lib()
    n, G, K, B, shots = 3, 4, 2, 2, 10
    gates = cc.encode_gates(dc.ghz_circuit(3) + [("S", (1,))], n)
    classes = np.array([0, 1, 255, 0], dtype=np.uint8)
    ref = np.zeros(1, dtype=np.uint64)
    errors, flips = np.full((B, K), 0.1), np.full((B, n, 2), 0.1)
    bits, words = np.full((B, shots, n), 7, dtype=np.uint8), np.full((B, shots), 7, dtype=np.uint64)
    status = np.full(B, 7, dtype=np.int32)
    good = dict(n=n, G=G, gates=gates, classes=classes, K=K, ref=ref, B=B, shots=shots, first=0, bits=bits, words=words)

    def call(**kw):
        a = dict(good, **kw)
        return lib.fbx_clifford_sample_shots(a["n"], a["G"], _lib.ptr(a["gates"], C.c_uint32), _lib.ptr(a["classes"], C.c_uint8), a["K"],
                                             _lib.ptr(a["ref"], C.c_uint64), a["B"], a["shots"], _lib.dptr(errors), _lib.dptr(flips), 1,
                                             a["first"], _lib.ptr(a["bits"], C.c_uint8), _lib.ptr(a["words"], C.c_uint64),
                                             _lib.iptr(status))
    bad_word, bad_pair = gates.copy(), gates.copy()
    bad_word[1] = 99
    bad_pair[1] = cc.OPCODES["CZ"] | (1 << 8) | (1 << 16)
    for kw in (dict(n=0), dict(n=65), dict(G=2 ** 31), dict(shots=2 ** 32), dict(K=0), dict(K=17), dict(B=-1), dict(shots=-1),
               dict(G=-1), dict(first=-1), dict(gates=None), dict(ref=None), dict(bits=None, words=None), dict(gates=bad_word),
               dict(gates=bad_pair), dict(classes=np.array([0, 2, 255, 0], dtype=np.uint8))):
        assert call(**kw) == _lib.FBX_ERR_BAD_ARG, kw
        assert lib.fbx_last_error()
        assert (bits == 7).all() and (words == 7).all() and (status == 7).all(), kw
    out = np.full(1, 7, dtype=np.uint64)
    for a in ((0, G, gates), (65, G, gates), (n, -1, gates), (n, G, None), (n, G, bad_word)):
        assert lib.fbx_clifford_reference_sample(a[0], a[1], _lib.ptr(a[2], C.c_uint32), _lib.ptr(out, C.c_uint64)) == _lib.FBX_ERR_BAD_ARG
        assert out[0] == 7
    assert lib.fbx_clifford_reference_sample(n, G, _lib.ptr(gates, C.c_uint32), None) == _lib.FBX_ERR_BAD_ARG
    # B == 0 and n_shots == 0 do nothing; the good call fills everything
    assert call(B=0) == 0 and call(shots=0) == 0
    assert (bits == 7).all() and (words == 7).all() and (status == 7).all()
    assert call() == 0
    assert (bits <= 1).all() and (words < 8).all() and not status.any()
    assert sampling.sample_clifford_circuit_batch(gates, n, 0).shape == (1, 0, n)


# ------------------------------------------------------------------ 11. the resident chains
@pytest.mark.parametrize("n", [5, 50])
def test_ghz_chain_equals_the_statistics_of_the_mirrors_shots(gpu, n):
    shots = 2000
    tree = [(q, q + 1) for q in range(n - 1)] if n == 50 else [(0, 1), (0, 2), (1, 3), (3, 4)]
    gates = es.create_ghz_program(tree)
    classes = np.array([255] + [q % 2 for q in range(n - 1)], dtype=np.uint8)
    errors = np.array([[0.0, 0.0], [0.01, 0.03], [0.2, 0.0]])
    flips = np.full((n, 2), 0.002)
    got = es.simulate_ghz_statistics_batch(tree, shots, errors, classes, flips, seed=SEED)
    bits = cc.unpack_shots(cc.restate_frame_shots(gates, n, shots, errors, classes, flips, seed=SEED), n)
    want = es.ghz_state_statistics_batch(bits)
    assert np.array_equal(want["bell"], (bits.sum(axis=2) % n == 0).sum(axis=1))
    assert np.array_equal(got["bell"], want["bell"]) and np.array_equal(got["total"], want["total"])
    assert got["bell"][0] < shots and got["bell"][2] < got["bell"][1] < shots
    ideal = es.simulate_ghz_statistics_batch(tree, shots, seed=SEED)
    assert ideal["bell"].tolist() == [shots] and ideal["total"].tolist() == [shots]
    ones = cc.unpack_shots(cc.restate_frame_shots(gates, n, shots, seed=SEED), n).all(axis=2).sum()
    assert 0.4 * shots < ones < 0.6 * shots                     # both branches of the GHZ state occur


def test_graph_state_chain_equals_the_parities_of_the_mirrors_shots(gpu):
    n, shots = 6, 2000
    graph = (list(range(n)), [(q, (q + 1) % n) for q in range(n)])
    state = es.create_graph_state(graph)
    classes = np.array([0] * n + [1] * n + [255], dtype=np.uint8)
    errors = np.array([[0.0, 0.0], [0.02, 0.05], [0.0, 0.3]])
    flips = np.full((n, 2), 0.01)
    got = es.simulate_graph_state_parities_batch(graph, shots, errors, classes, flips, seed=SEED)
    assert got.shape == (3, n)
    for i in range(n):
        rotation, measured = es.measure_graph_state(graph, i)
        words = cc.restate_frame_shots(state + rotation, n, shots, errors, classes, flips, seed=SEED + i)
        mask = np.uint64(sum(1 << q for q in measured))
        odd = (cc._popcount(words & mask) & np.uint64(1)).astype(np.int64).sum(axis=1)
        assert np.array_equal(got[:, i], ((shots - odd) - odd) / shots), i
    assert (got[0] < 1).all() and (got[2] < got[0]).all()
    assert np.array_equal(es.simulate_graph_state_parities_batch(graph, shots, seed=SEED), np.ones((1, n)))
    assert np.array_equal(es.simulate_graph_state_parities_batch(graph, shots, seed=SEED, theta=np.pi / 2), -np.ones((1, n)))
