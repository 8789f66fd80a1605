"""The host restatements of fbx_tomo_simulate_symmetrized and fbx_tomo_simulate_calibration (include/fbx.h) without a GPU:
``synthetic.restate_symmetrized_tomography_counts`` and ``synthetic.restate_readout_calibration_counts`` on deterministic
confusion matrices with known answers, against the stream walked shot by shot (tomo_sim_symm_cases.pattern_loop, on the
oracle's Philox), the bookkeeping of patterns and shots, and the sampler guard of the GPU test on dense float64 distributions."""
import numpy as np
import pytest

import tomo_sim_cases as tc
import tomo_sim_symm_cases as ss
from tomo_sim_cases import B, FIRST, SEED


def z_type(n):
    """the 2^n - 1 Z-type observables of n qubits as Pauli codes [m, n]"""
    return np.array([[3 * ((k >> (n - 1 - q)) & 1) for q in range(n)] for k in range(1, 1 << n)], dtype=np.uint8)


def rows_for(p, conf, masks, symm_type):
    from fbx import synthetic
    return synthetic.symmetrized_pattern_distributions(p, conf, masks, symm_type)


# ------------------------------------------------------------------------------------------------ 1. deterministic matrices
@pytest.mark.parametrize("symm_type", (-1, 0))
def test_identity_matrix_merges_the_per_pattern_draws(symm_type):
    """C = identity: q_f = p for every pattern, and the merged histogram is the sum of the patterns' own draws, walked shot by
    shot with the counter (gid, group, (f << 27) | block) -- 23 shots over 4 patterns: s = 5, a tail block in every pattern"""
    from fbx import synthetic
    n, d, shots = 2, 4, 23
    paulis = np.array([[0, 3], [3, 0], [3, 3], [1, 0]], dtype=np.uint8)          # group 0: U = 3, group 1: U = 2
    group_of = np.array([0, 0, 0, 1])
    rng = np.random.default_rng(5)
    p = rng.dirichlet(np.ones(d), size=(B, 2))
    rows = rows_for(p, np.eye(d), [3, 2], symm_type)
    for g, U in enumerate((3, 2)):
        pats = ss.patterns_of(U, symm_type, n)
        assert np.array_equal(rows[:, g, pats], np.broadcast_to(p[:, g, None, :], (B, len(pats), d)))
        assert not rows[:, g, [f for f in range(d) if f not in pats]].any()
    e, c, se, hist = synthetic.restate_symmetrized_tomography_counts(rows, group_of, paulis, np.ones(4), shots, symm_type, SEED, FIRST)
    for b in range(B):
        for g, U in enumerate((3, 2)):
            pats = ss.patterns_of(U, symm_type, n)
            s = shots // len(pats)
            want = sum(ss.pattern_loop(p[b, g], f, s, SEED, FIRST + b, g, ss.TAG_MEASUREMENT) for f in pats)
            assert np.array_equal(hist[b, g], want) and want.sum() == s * len(pats)
    N0 = (shots // (4 if symm_type == -1 else 1)) * (4 if symm_type == -1 else 1)
    assert np.all(c[:, :3] == N0) and np.array_equal(e[:, 2], (hist[:, 0, [0, 3]].sum(axis=1) - hist[:, 0, [1, 2]].sum(axis=1)) / N0)


@pytest.mark.parametrize("symm_type", (-1, 0))
@pytest.mark.parametrize("n", (1, 2, 3))
def test_every_bit_read_inverted(n, symm_type):
    """the anti-diagonal permutation on |0...0> in the all-Z group: every shot of every pattern lands on outcome 2^n - 1"""
    from fbx import synthetic
    d, shots = 1 << n, 37
    paulis = z_type(n)
    p = np.zeros((B, 1, d)); p[:, 0, 0] = 1.0
    conf = np.eye(d)[::-1].copy()
    U = d - 1
    rows = rows_for(p, conf, [U], symm_type)
    pats = ss.patterns_of(U, symm_type, n)
    assert np.all(rows[:, 0, pats, d - 1] == 1.0) and np.all(rows[:, 0, :, :d - 1] == 0.0)
    e, c, se, hist = synthetic.restate_symmetrized_tomography_counts(rows, np.zeros(len(paulis), dtype=int), paulis, np.ones(len(paulis)),
                                                                    shots, symm_type, SEED, FIRST)
    N = (shots // len(pats)) * len(pats)
    assert np.all(hist[:, 0, d - 1] == N) and np.all(hist[:, 0, :d - 1] == 0) and np.all(c == N)
    weight = (paulis != 0).sum(axis=1)
    assert np.array_equal(e, np.broadcast_to((-1.0) ** weight, e.shape)) and np.all(se == 0.0)


def test_one_way_flip_is_removed_by_symmetrization():
    """P(1|0) = 1, P(0|1) = 0 on one qubit in |0>: unsymmetrized <Z> = -1; symmetrized, the flipped half of the shots reads 1,
    is recorded as 0, and the mean is exactly 0 with an even number of shots per pattern; so is the calibration's"""
    from fbx import synthetic
    conf = np.array([[0.0, 1.0], [0.0, 1.0]])
    paulis = np.array([[3]], dtype=np.uint8)
    p = np.zeros((B, 1, 2)); p[:, 0, 0] = 1.0
    args = (np.zeros(1, dtype=int), paulis, np.ones(1), 36)
    e0 = synthetic.restate_symmetrized_tomography_counts(rows_for(p, conf, [1], 0), *args, 0, SEED, FIRST)
    assert np.all(e0[0] == -1.0) and np.all(e0[1] == 36.0) and np.all(e0[3][:, 0] == [0, 36])
    e1 = synthetic.restate_symmetrized_tomography_counts(rows_for(p, conf, [1], -1), *args, -1, SEED, FIRST)
    assert np.all(e1[0] == 0.0) and np.all(e1[3][:, 0] == [18, 18]) and np.all(e1[2] == 1.0 / 6.0)       # sqrt(4 18 18 / 36) / 36
    mean, var, cnt, hist = synthetic.restate_readout_calibration_counts(conf, paulis, 36, -1, SEED, FIRST)
    assert mean.shape == (1, 1) and mean[0, 0] == 0.0 and cnt[0, 0] == 36.0 and var[0, 0] == 1.0 / 36.0
    mean0 = synthetic.restate_readout_calibration_counts(conf, paulis, 36, 0, SEED, FIRST)[0]
    assert mean0[0, 0] == -1.0


# ------------------------------------------------------------------------------------------------ 2. bookkeeping
def test_patterns_are_the_submasks_of_the_union():
    from fbx import synthetic
    for mask in range(32):
        got = synthetic.symmetrization_patterns(mask, -1)
        assert got == ss.patterns_of(mask, -1, 5) and len(got) == 1 << bin(mask).count("1")
        assert synthetic.symmetrization_patterns(mask, 0) == [0]
    for symm_type in (1, 2, 3, -2, 4):
        with pytest.raises(ValueError):
            synthetic.symmetrization_patterns(3, symm_type)


def test_floor_rule_counts_and_refusals():
    """1000 shots: a weight-3 union draws floor(1000 / 8) = 125 per pattern and reports 1000, a weight-2 union 250 and 1000;
    1003 shots: 125 x 8 = 1000 and 250 x 4 = 1000 -- fewer than asked for; 37 shots: 4 x 8 = 32 and 9 x 4 = 36, which differ
    between the groups of one call"""
    from fbx import synthetic
    n, d = 3, 8
    paulis = np.array([[3, 3, 3], [3, 0, 3], [0, 0, 3]], dtype=np.uint8)
    group_of = np.array([0, 1, 1])                                                  # U = 7 and U = 5
    p = np.random.default_rng(3).dirichlet(np.ones(d), size=(2, 2))
    conf = ss.correlated_confusion(n, 2)
    rows = rows_for(p, conf, [7, 5], -1)
    assert [f for f in range(d) if rows[0, 1, f].any()] == [0, 1, 4, 5]
    for shots, want in ((1000, (1000, 1000)), (1003, (1000, 1000)), (37, (32, 36)), (8, (8, 8))):
        e, c, se, hist = synthetic.restate_symmetrized_tomography_counts(rows, group_of, paulis, np.ones(3), shots, -1, SEED)
        assert np.all(c[:, 0] == want[0]) and np.all(c[:, 1:] == want[1])
        assert np.all(hist[:, 0].sum(axis=1) == want[0]) and np.all(hist[:, 1].sum(axis=1) == want[1])
        assert synthetic.shots_per_pattern(shots, 7, -1) == shots // 8 and synthetic.shots_per_pattern(shots, 5, -1) == shots // 4
        c0 = synthetic.restate_symmetrized_tomography_counts(rows_for(p, conf, [7, 5], 0), group_of, paulis, np.ones(3), shots, 0, SEED)[1]
        assert np.all(c0 == shots)
    with pytest.raises(ValueError, match="shots per flip pattern"):
        synthetic.restate_symmetrized_tomography_counts(rows, group_of, paulis, np.ones(3), 7, -1, SEED)       # s == 0 in group 0
    with pytest.raises(ValueError, match="shots per flip pattern"):
        synthetic.restate_readout_calibration_counts(conf, paulis, 7, -1, SEED)
    for symm_type in (1, 2, 3):
        with pytest.raises(ValueError, match="orthogonal"):
            synthetic.restate_symmetrized_tomography_counts(rows, group_of, paulis, np.ones(3), 1000, symm_type, SEED)
        with pytest.raises(ValueError, match="orthogonal"):
            synthetic.restate_readout_calibration_counts(conf, paulis, 1000, symm_type, SEED)
    cal = synthetic.restate_readout_calibration_counts(conf, paulis, 37, -1, SEED)
    assert np.array_equal(cal[2], np.broadcast_to([32.0, 36.0, 36.0], (2, 3)))         # weights 3, 2, 1: 4 x 8, 9 x 4, 18 x 2


def test_the_three_streams_differ_under_one_seed():
    """the same distribution, seed, item and unit number: the grouped call, the symmetrized measurement (one pattern, f = 0: the
    same counter words) and the calibration draw different histograms -- only the key tag tells them apart"""
    from fbx import synthetic
    paulis = np.array([[3]], dtype=np.uint8)
    flips = np.array([[0.3, 0.45]])
    conf = ss.kron_flips(flips)
    p = np.zeros((B, 1, 2)); p[:, 0, 0] = 1.0
    rows = rows_for(p, conf, [1], 0)                                                # row 0 = C[0] = (0.7, 0.3)
    assert np.array_equal(rows[:, 0, 0], np.broadcast_to(conf[0], (B, 2)))
    grouped = synthetic.restate_grouped_tomography_counts(rows[:, :, 0, :], np.zeros(1, dtype=int), paulis, np.ones(1), 1000, SEED, FIRST)[3]
    measured = synthetic.restate_symmetrized_tomography_counts(rows, np.zeros(1, dtype=int), paulis, np.ones(1), 1000, 0, SEED, FIRST)[3]
    calibrated = np.stack([synthetic.restate_readout_calibration_counts(conf, paulis, 1000, 0, SEED, FIRST + b)[3][0] for b in range(B)])
    assert not np.array_equal(grouped, measured) and not np.array_equal(grouped, calibrated) and not np.array_equal(measured, calibrated)
    for b in range(2):
        assert np.array_equal(measured[b, 0], ss.pattern_loop(conf[0], 0, 1000, SEED, FIRST + b, 0, ss.TAG_MEASUREMENT))
        assert np.array_equal(calibrated[b, 0], ss.pattern_loop(conf[0], 0, 1000, SEED, FIRST + b, 0, ss.TAG_CALIBRATION))
        assert np.array_equal(grouped[b, 0], ss.pattern_loop(conf[0], 0, 1000, SEED, FIRST + b, 0, ss.TAG_GROUPED))


def test_calibration_restatement_against_the_shot_loop():
    """two qubits, a correlated matrix, every pattern of every calibration walked shot by shot: q_f(r) = C[f][r ^ f]"""
    from fbx import synthetic
    n, d, shots = 2, 4, 23
    conf = ss.correlated_confusion(n)
    paulis = np.array([[0, 1], [2, 0], [3, 3]], dtype=np.uint8)
    mean, var, cnt, hist = synthetic.restate_readout_calibration_counts(conf, paulis, shots, -1, SEED, FIRST)
    for b in range(B):
        for c, z in enumerate((1, 2, 3)):
            pats = ss.patterns_of(z, -1, n)
            s = shots // len(pats)
            want = sum(ss.pattern_loop(conf[b, f, np.arange(d) ^ f], f, s, SEED, FIRST + b, c, ss.TAG_CALIBRATION) for f in pats)
            assert np.array_equal(hist[b, c], want)
            N = s * len(pats)
            kp = sum(int(want[o]) for o in range(d) if bin(o & z).count("1") % 2 == 0)
            assert mean[b, c] == (2 * kp - N) / N and cnt[b, c] == N and var[b, c] == 4 * kp * (N - kp) / N / N / N


def test_confusion_from_flips_is_the_kronecker_product():
    from fbx import readout
    flips = np.random.default_rng(2).uniform(0.0, 0.3, size=(B, 3, 2))
    got = readout.confusion_from_flips(flips)
    assert got.shape == (B, 8, 8) and np.allclose(got.sum(axis=2), 1.0)
    for b in range(B):
        assert np.array_equal(got[b], ss.kron_flips(flips[b]))
    assert np.array_equal(readout.confusion_from_flips(flips[0]), got[0])
    assert got[0][0, 1] == (1 - flips[0, 0, 0]) * (1 - flips[0, 1, 0]) * flips[0, 2, 0]       # drawn 000, read 001: qubit 2 flipped
    with pytest.raises(ValueError):
        readout.confusion_from_flips(np.zeros((3, 3)))


def test_correlated_matrices_are_far_from_products():
    for n in (2, 3, 4, 5):
        for b in range(B):
            assert ss.distance_from_products(ss.correlated_confusion(n)[b]) > 0.01
            assert ss.distance_from_products(ss.product_confusion(n)[b]) < 1e-14
        assert np.allclose(ss.correlated_confusion(n).sum(axis=2), 1.0)


# ------------------------------------------------------------------------------------------------ 3. the sampler guard, on the CPU
@pytest.mark.parametrize("case", ss.ALL_CASES)
def test_restatement_alone_stays_inside_the_z_bound(case):
    """the guard of the GPU test (test_merged_cells_follow_their_probabilities) with the restatement in place of the device,
    on dense float64 distributions: the seed and the cases keep every cell inside the bound, so a GPU failure of that test is
    the kernel's"""
    from fbx import synthetic
    des, g, unions = ss.design_of(case), ss.grouping_of(case), ss.unions_of(case)
    nb = ss.guard_items(des.n_qubits)
    conf = ss.correlated_confusion(des.n_qubits)[:nb]
    rows = ss.dense_patterns(ss.ideal(case)[:nb], conf, unions, -1).astype(np.float64)
    e, c, se, hist = synthetic.restate_symmetrized_tomography_counts(rows, g, des.paulis, des.coefs, 1000, -1, SEED, FIRST)
    per_group = np.array([(1000 // (1 << bin(u).count("1"))) << bin(u).count("1") for u in unions], dtype=np.float64)
    qbar = rows.sum(axis=2) / np.array([1 << bin(u).count("1") for u in unions], dtype=np.float64)[None, :, None]
    z, cells = ss.cell_z_scores(hist, qbar, per_group[None, :, None])
    bound = ss.z_bound(cells)
    print(f"{case}: {cells} cells, worst |z| {np.abs(z).max():.3f}, bound {bound:.3f}")
    assert cells >= 30 and np.all(np.abs(z) <= bound)
