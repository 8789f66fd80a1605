"""fbx.quantum_volume on the host (no GPU): the scalar helpers and the circuit generator against the reference's answers in
tests/golden/qv_cases.npz (tests/golden/make_qv_goldens.py), the pairing rules, the mask packing, argument errors, the synthetic shot
generator -- and the numpy restatement of tests/qv_cases.py pinned to the reference's heavy lists, so that the GPU tests above the
widths of the goldens do not compare the device with itself."""
import os

import numpy as np
import pytest

import qv_cases as qc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qv_cases.npz")
WIDTHS = range(2, 11)


@pytest.fixture(scope="module")
def gold():
    assert os.path.getsize(GOLDEN) <= 1024 * 1024
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_calculate_prob_est_and_err_matches_the_reference(gold):
    from fbx import quantum_volume as qv
    for (h, c, s), want in zip(gold["est_args"], gold["est_out"]):
        got = qv.calculate_prob_est_and_err(int(h), int(c), int(s))
        for g, w in zip(got, want):
            assert abs(g - w) <= 1e-15 * abs(w), (h, c, s, g, w)


def test_get_prob_sample_heavy_by_depth_matches_the_reference(gold):
    from fbx import quantum_volume as qv
    res = qv.get_prob_sample_heavy_by_depth([int(d) for d in gold["by_depth_depths"]], [int(h) for h in gold["by_depth_heavy"]],
                                            [int(s) for s in gold["by_depth_shots"]])
    assert list(res.keys()) == [int(k) for k in gold["by_depth_keys"]]
    for (est, low), (west, wlow) in zip(res.values(), gold["by_depth_values"]):
        assert abs(est - west) <= 1e-15 * abs(west) and abs(low - wlow) <= 1e-15 * abs(wlow)
    assert qv.extract_quantum_volume_from_results(res) == int(gold["qv_from_by_depth"])


def test_unequal_shot_counts_of_one_depth_are_refused():
    from fbx import quantum_volume as qv
    with pytest.raises(AssertionError, match="number of shots should be the same"):
        qv.get_prob_sample_heavy_by_depth([2, 3, 2], [10, 10, 10], [100, 100, 101])


@pytest.mark.parametrize("name", ["first_fails", "middle_fails", "none_fails", "just_above"])
def test_extract_quantum_volume_matches_the_reference(gold, name):
    from fbx import quantum_volume as qv
    table = {int(d): (float(v[0]), float(v[1])) for d, v in zip(gold[f"extract_{name}_depths"], gold[f"extract_{name}_values"])}
    assert qv.extract_quantum_volume_from_results(table) == int(gold[f"extract_{name}_qv"])


def test_extract_quantum_volume_breaks_at_two_thirds_inclusive():
    from fbx import quantum_volume as qv
    assert qv.extract_quantum_volume_from_results({2: (0.9, 0.8), 3: (0.7, 2 / 3), 4: (0.9, 0.9)}) == 4
    assert qv.extract_quantum_volume_from_results({2: (0.5, 0.4)}) == 2
    assert qv.extract_quantum_volume_from_results({}) == 2


@pytest.mark.parametrize("n", WIDTHS)
def test_generate_abstract_qv_circuit_reproduces_the_stored_circuits(gold, n):
    from fbx import quantum_volume as qv
    for k, seed in enumerate(gold[f"w{n}_seeds"]):
        np.random.seed(int(seed))
        perms, gates = qv.generate_abstract_qv_circuit(n)
        assert len(perms) == n and gates.shape == (n, n // 2, 4, 4)
        assert np.array_equal(np.asarray(perms), gold[f"w{n}_permutations"][k])
        assert np.abs(gates - gold[f"w{n}_gates"][k]).max() <= 1e-13


def test_generate_abstract_qv_circuit_equals_the_reference_bit_for_bit():
    import _ref_harness as rh
    if not rh.reference_available():
        pytest.skip("the reference checkout is not on this machine")
    import make_qv_goldens as mk
    ref = mk.load_quantum_volume()
    from fbx import quantum_volume as qv
    for n in (2, 3, 6, 9):
        np.random.seed(77 + n)
        rp, rg = ref.generate_abstract_qv_circuit(n)
        np.random.seed(77 + n)
        p, g = qv.generate_abstract_qv_circuit(n)
        assert all((a == b).all() for a, b in zip(p, rp)) and len(p) == len(rp)
        assert g.shape == rg.shape and (g == rg).all()


@pytest.mark.parametrize("n", WIDTHS)
def test_restatement_is_pinned_to_the_reference(gold, n):
    """tests/qv_cases.py::simulate + heavy_of against the reference's collect_heavy_outputs: heavy tables equal, probabilities and
    medians to the derived bound"""
    L = n * (n // 2)
    for k in range(len(gold[f"w{n}_seeds"])):
        pairs = qc.pairs_of(gold[f"w{n}_permutations"][k], "reference")
        want = gold[f"w{n}_probabilities"][k]
        assert qc.middle_gap(want) >= 1e-7
        p = qc.simulate(n, pairs, gold[f"w{n}_gates"][k].reshape(-1, 4, 4))
        med, heavy = qc.heavy_of(p)
        assert np.array_equal(heavy, gold[f"w{n}_heavy"][k])
        assert np.all(np.abs(p - want) <= qc.prob_bound(want, L))
        assert abs(med - gold[f"w{n}_median"][k]) <= qc.prob_bound(gold[f"w{n}_median"][k], L)
        assert abs(p.sum() - 1) <= 2 * qc.delta(L)


def test_exact_cases_hold_in_the_restatement():
    for n in (2, 3, 4, 7):
        for name, pairs, gates, idx in qc.basis_state_cases(n):
            p = qc.simulate(n, pairs, gates)
            assert p[idx] == 1.0 and p.sum() == 1.0, (n, name)
        kinds = ["all"] + (["all_but_last"] if n % 2 == 0 else [])
        for kind in kinds:
            pairs, gates, probs, med, heavy = qc.hadamard_case(n, kind)
            p = qc.simulate(n, pairs, gates)
            m, h = qc.heavy_of(p)
            assert np.array_equal(p, probs) and m == med and np.array_equal(h, heavy), (n, kind)


def test_pairing_rules():
    from fbx import quantum_volume as qv
    perm = np.array([[3, 0, 4, 1, 2], [1, 2, 3, 4, 0]])                  # odd width: the last position is idle
    ref = qv.layer_pairs(perm, "reference")
    dis = qv.layer_pairs(perm, "disjoint")
    assert ref.dtype == np.uint8 and ref.shape == (2, 2, 2)
    assert ref.tolist() == [[[3, 0], [0, 4]], [[1, 2], [2, 3]]]           # (perm[g], perm[g + 1]): neighbours overlap
    assert dis.tolist() == [[[3, 0], [4, 1]], [[1, 2], [3, 4]]]           # (perm[2 g], perm[2 g + 1])
    even = np.array([[2, 0, 3, 1]])
    assert qv.layer_pairs(even, "reference").tolist() == [[[2, 0], [0, 3]]]
    assert qv.layer_pairs(even, "disjoint").tolist() == [[[2, 0], [3, 1]]]
    for pairing in ("reference", "disjoint"):
        for n in (2, 5, 8):
            p = np.stack([np.random.default_rng(n).permutation(n) for _ in range(n)])
            assert np.array_equal(qv.layer_pairs(p, pairing).reshape(-1, 2), qc.pairs_of(p, pairing))
    with pytest.raises(ValueError):
        qv.layer_pairs(even, "paper")
    with pytest.raises(ValueError):
        qv.layer_pairs(np.array([[0, 0, 1, 2]]))
    with pytest.raises(ValueError):
        qv.layer_pairs(np.array([[0.0, 1.0]]))


@pytest.mark.parametrize("n", [2, 3, 5, 6, 7, 10])
def test_mask_packing_round_trip(n):
    from fbx import quantum_volume as qv
    rng = np.random.default_rng(n)
    table = rng.random((3, 1 << n)) < 0.5
    table[1] = False
    table[2] = True
    mask = qv.pack_heavy_mask(table)
    assert mask.dtype == np.uint64 and mask.shape == (3, max(1, (1 << n) // 64))
    for b in range(3):
        for i in range(1 << n):
            assert bool((int(mask[b, i // 64]) >> (i % 64)) & 1) == bool(table[b, i])
    assert np.array_equal(qv.unpack_heavy_mask(mask, n), table)
    with pytest.raises(ValueError):
        qv.unpack_heavy_mask(mask, n + 7)


def test_argument_errors_come_before_any_device_call(monkeypatch):
    from fbx import _lib, quantum_volume as qv

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    n = 4
    perms = np.stack([np.stack([np.arange(n)] * n)] * 2)
    gates = np.broadcast_to(np.eye(4, dtype=complex), (2, n, n // 2, 4, 4)).copy()
    with pytest.raises(ValueError):
        qv.collect_heavy_outputs_batch(perms, gates[:, :, :1])                    # gates of the wrong shape
    with pytest.raises(ValueError):
        qv.collect_heavy_outputs_batch(perms[0], gates)                           # not a batch
    with pytest.raises(ValueError):
        qv.collect_heavy_outputs_batch(perms, gates, pairing="nearest")
    bad = perms.copy(); bad[0, 0, 0] = 1                                          # not a permutation
    with pytest.raises(ValueError):
        qv.collect_heavy_outputs_batch(bad, gates)
    flat = np.broadcast_to(np.eye(4, dtype=complex), (1, 1, 4, 4))
    with pytest.raises(ValueError):
        qv.heavy_outputs_flat(3, [[(1, 1)]], flat)                                # equal qubits
    with pytest.raises(ValueError):
        qv.heavy_outputs_flat(3, [[(0, 3)]], flat)                                # index out of range
    with pytest.raises(ValueError):
        qv.heavy_outputs_flat(3, [[(0, 1)]], flat[:, :, :2])
    with pytest.raises(ValueError):
        qv.heavy_outputs_flat(3, [[(0, 1)]], flat, probabilities=False, median=False, mask=False, heavy_prob=False, heavy_count=False)
    bits = np.zeros((2, 10, 3), dtype=np.uint8)
    with pytest.raises(ValueError):
        qv.count_heavy_hitters_sampled_batch(bits, np.zeros((2, 4), dtype=bool))   # table of another width
    with pytest.raises(ValueError):
        qv.count_heavy_hitters_sampled_batch(bits, np.zeros((2, 2), dtype=np.uint64))
    with pytest.raises(ValueError):
        qv.count_heavy_hitters_sampled_batch(bits + 2, np.zeros((2, 8), dtype=bool))
    with pytest.raises(ValueError):
        qv.count_heavy_hitters_sampled_batch(bits[0], np.zeros((2, 8), dtype=bool))
    with pytest.raises(ValueError):
        qv.generate_abstract_qv_circuits_batch(1, 4, seed=1)


def test_no_device_fails_loudly_not_silently(gold):
    """Without a GPU the heavy outputs are an error (FBX_ERR_NO_DEVICE), never a host simulation."""
    import fbx
    from fbx import _lib, quantum_volume as qv
    if fbx.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(fbx.FbxError) as ei:
        qv.collect_heavy_outputs_batch(gold["w3_permutations"], gold["w3_gates"])
    assert ei.value.code == _lib.FBX_ERR_NO_DEVICE
    with pytest.raises(fbx.FbxError) as ei:
        qv.count_heavy_hitters_sampled_batch(np.zeros((1, 5, 3), dtype=np.uint8), np.zeros((1, 8), dtype=bool))
    assert ei.value.code == _lib.FBX_ERR_NO_DEVICE
    with pytest.raises(fbx.FbxError) as ei:
        qv.collect_heavy_outputs(None, list(gold["w3_permutations"][0]), gold["w3_gates"][0])
    assert ei.value.code == _lib.FBX_ERR_NO_DEVICE


def test_unsupported_widths_are_refused_without_a_device():
    import fbx
    from fbx import _lib, quantum_volume as qv
    perms = np.stack([np.stack([np.arange(14)] * 14)])
    gates = np.broadcast_to(np.eye(4, dtype=complex), (1, 14, 7, 4, 4)).copy()
    with pytest.raises(fbx.FbxError) as ei:
        qv.collect_heavy_outputs_batch(perms, gates)
    assert ei.value.code == _lib.FBX_ERR_UNSUPPORTED and "13" in str(ei.value)


def test_qv_shots_shapes_dtype_and_determinism():
    from fbx import synthetic
    rng = np.random.default_rng(0)
    p = rng.random((3, 32)); p /= p.sum(axis=1, keepdims=True)
    a = synthetic.qv_shots(p, 200, depolarizing=0.1, seed=5)
    assert a.shape == (3, 200, 5) and a.dtype == np.uint8 and set(np.unique(a)) <= {0, 1}
    assert np.array_equal(a, synthetic.qv_shots(p, 200, depolarizing=0.1, seed=5))
    assert not np.array_equal(a, synthetic.qv_shots(p, 200, depolarizing=0.1, seed=6))
    delta = np.zeros((1, 8)); delta[0, 0b110] = 1.0
    s = synthetic.qv_shots(delta, 50, seed=1)
    assert (s == np.array([1, 1, 0], dtype=np.uint8)).all()                      # first column = qubit 0 = most significant bit
    assert (qc.bit_array_to_int_rows(s[0]) == 6).all()
    flat = synthetic.qv_shots(delta, 4000, depolarizing=1.0, seed=2)
    assert abs(flat.mean() - 0.5) < 0.03
    assert synthetic.qv_shots(p, 0).shape == (3, 0, 5)
    with pytest.raises(ValueError):
        synthetic.qv_shots(p[:, :24], 10)
    with pytest.raises(ValueError):
        synthetic.qv_shots(p, 10, depolarizing=1.5)
    poisoned = p.copy(); poisoned[1] = np.nan
    with pytest.raises(ValueError, match=r"probabilities\[1\]"):
        synthetic.qv_shots(poisoned, 10)
    with pytest.raises(ValueError, match=r"probabilities\[2\]"):
        synthetic.qv_shots(np.vstack([p[:2], np.zeros((1, 32))]), 10)
