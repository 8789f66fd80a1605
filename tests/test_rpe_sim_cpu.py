"""The host half of the simulated robust phase estimation (no device): synthetic.rpe_distributions against closed forms and
against mpmath matrix powers at 50 digits, synthetic.restate_rpe_counts on exact integer properties and against a shot-by-shot
restatement, the two settings helpers against the reference's settings written out by hand, and the end-to-end experiments of
tests/test_rpe_sim_gpu.py run through the host restatement -- which confirms their seeds."""
import math

import mpmath
import numpy as np
import pytest

import rpe_cases
import rpe_sim_cases as cases
from fbx import robust_phase_estimation as rpe
from fbx import synthetic

U = 2.0 ** -53


def test_rz_distributions_follow_the_closed_form():
    """RZ(theta), no change of basis, |+>: <X>_j = cos(2^j theta), <Y>_j = sin(2^j theta), with mpmath for K = 20.  The bound: the
    entries of the float64 matrix carry a relative rounding of u, which turns the rotation by at most 2 u; a squaring doubles the
    angle error it inherits and adds at most 4 u of its own, so depth j is off by at most 2^j (2 u + 4 u sum_i 2^-i) <= 2^j 10 u,
    and the last products add a few u: 2^j 16 u + 8 u."""
    gate, K, kw, _ = cases.distribution_cases()["1q_rz"]
    p = cases.mirror(gate, K, kw)[0]                               # [K, 2, 2]
    theta = mpmath.mpf(cases.THETA)
    for j in range(K):
        angle = mpmath.mpf(2) ** j * theta
        want = (float(mpmath.cos(angle)), float(mpmath.sin(angle)))
        bound = 2.0 ** j * 16 * U + 8 * U
        for basis in range(2):
            assert abs((p[j, basis, 0] - p[j, basis, 1]) - want[basis]) <= bound, (j, basis)
            assert abs(p[j, basis, 0] + p[j, basis, 1] - 1.0) <= bound


@pytest.mark.parametrize("name", ["1q_noisy_shared_basis", "1q_noisy_per_item_basis", "2q_diag_partner", "2q_diag_no_partner",
                                  "2q_shared_basis_partner_flips", "2q_per_item_basis_partner"])
def test_distributions_against_mpmath_matrix_powers(name):
    """The numpy mirror against 50-digit powers of the SAME float64 matrices.  One squaring of a matrix of norm about 1 loses at
    most D u per entry and a later squaring doubles what it inherits: depth j is within 2^j (D + 2) u of the exact power, and the
    two changes of basis and the flips add a few D u: (2^j + 4) (D + 2) u."""
    gate, K, kw, ref = cases.distribution_cases()[name]
    got = cases.mirror(gate, K, kw)
    D = gate.shape[-1]
    assert got.shape == ref.shape
    for j in range(K):
        assert np.abs(got[:, j] - ref[:, j]).max() <= (2.0 ** j + 4) * (D + 2) * U, j


def test_distribution_conventions():
    """|+>|1> under diag(1, 1, 1, e^{i phi}): the partner reads t = 1 every time and the xy qubit turns by phi; with the partner's
    flips swapped in the outcome moves with them; outcome = 2 s + t."""
    phi = 0.9
    gate = synthetic.pauli_transfer_matrix(np.diag([1, 1, 1, np.exp(1j * phi)]))
    init = synthetic.pauli_vector_of_state(np.kron([1, 1], [0, 1]) / math.sqrt(2))
    p = synthetic.rpe_distributions(gate, 2, init=init, xy_qubit=0, z_qubit=1)[0]
    for j in range(2):
        c, s = math.cos(2 ** j * phi), math.sin(2 ** j * phi)
        np.testing.assert_allclose(p[j, 0], [0, (1 + c) / 2, 0, (1 - c) / 2], atol=1e-15)
        np.testing.assert_allclose(p[j, 1], [0, (1 + s) / 2, 0, (1 - s) / 2], atol=1e-15)
    flipped = synthetic.rpe_distributions(gate, 1, init=init, xy_qubit=0, z_qubit=1, flips=[[0, 0], [0, 1]])[0]      # reads every 1 as 0
    np.testing.assert_allclose(flipped[0, 0], [(1 + math.cos(phi)) / 2, 0, (1 - math.cos(phi)) / 2, 0], atol=1e-15)
    # the other qubit as the rotated one: the same numbers with the roles of the tensor factors exchanged
    init2 = synthetic.pauli_vector_of_state(np.kron([0, 1], [1, 1]) / math.sqrt(2))
    q = synthetic.rpe_distributions(gate, 2, init=init2, xy_qubit=1, z_qubit=0)[0]
    np.testing.assert_allclose(q, p, atol=1e-15)
    alone = synthetic.rpe_distributions(gate, 1, init=init, xy_qubit=0)[0]
    np.testing.assert_allclose(alone[0, 0], [(1 + math.cos(phi)) / 2, (1 - math.cos(phi)) / 2], atol=1e-15)


# ------------------------------------------------------------------------------------------------ restate_rpe_counts
def _shot_by_shot(p, N, seed, gid, j, basis):
    """the histogram of one unit from the contract, one Philox block per shot"""
    c = np.cumsum(np.maximum(p, 0.0))
    thr = [int(math.floor(x / c[-1] * 2.0 ** 32)) for x in c[:-1]]
    k0, k1 = (seed & 0xFFFFFFFF) ^ 0x52504553, seed >> 32
    hist = [0] * len(p)
    for s in range(N):
        words = synthetic._philox4x32_10(gid & 0xFFFFFFFF, gid >> 32, 2 * j + basis, s >> 2, k0, k1)
        w = int(words[s & 3])
        hist[sum(t <= w for t in thr)] += 1
    return hist


def test_restated_counts_are_the_documented_stream():
    rng = np.random.default_rng(3)
    shots = [1, 3, 5, 1001]                                        # the tail of a block: 1, 3, 1 words; 1001 = 250 blocks + 1
    seed, first = (7 << 32) + 12345, 2 ** 33 + 5
    for M in (2, 4):
        p = rng.dirichlet(np.ones(M), size=(2, len(shots), 2))
        hist, moments = synthetic.restate_rpe_counts(p, shots, seed, first_item=first)
        assert hist.shape == (2, 4, 2, M) and moments.shape == (8, 2, 4)
        np.testing.assert_array_equal(hist.sum(axis=3), np.broadcast_to(np.array(shots)[None, :, None], (2, 4, 2)))
        for b in range(2):
            for j, N in enumerate(shots):
                for basis in range(2):
                    assert list(hist[b, j, basis]) == _shot_by_shot(p[b, j, basis], N, seed, first + b, j, basis), (M, b, j, basis)
        N = np.array(shots, dtype=np.float64)[None, :]
        odd = hist[..., 1] if M == 2 else hist[..., 2] + hist[..., 3]
        for basis in range(2):
            mean = ((N - odd[:, :, basis]) - odd[:, :, basis]) / N
            np.testing.assert_array_equal(moments[basis], mean)
            np.testing.assert_array_equal(moments[4 + basis], (1.0 - mean * mean) / N)
        if M == 2:
            assert np.isnan(moments[[2, 3, 6, 7]]).all()
        else:
            par = hist[..., 1] + hist[..., 2]
            for basis in range(2):
                mean = ((N - par[:, :, basis]) - par[:, :, basis]) / N
                np.testing.assert_array_equal(moments[2 + basis], mean)
                np.testing.assert_array_equal(moments[6 + basis], (1.0 - mean * mean) / N)


def test_certain_outcomes_give_all_or_nothing_counts():
    shots = [1, 3, 5, 1001]
    p = np.zeros((1, 4, 2, 4))
    p[0, :, 0, 2] = 1.0                                            # X basis: always s = 1, t = 0
    p[0, :, 1, 0] = 1.0                                            # Y basis: always s = 0, t = 0
    hist, moments = synthetic.restate_rpe_counts(p, shots, seed=99)
    np.testing.assert_array_equal(hist[0, :, 0], [[0, 0, N, 0] for N in shots])
    np.testing.assert_array_equal(hist[0, :, 1], [[N, 0, 0, 0] for N in shots])
    np.testing.assert_array_equal(moments[0, 0], -1.0); np.testing.assert_array_equal(moments[1, 0], 1.0)
    np.testing.assert_array_equal(moments[2, 0], -1.0); np.testing.assert_array_equal(moments[3, 0], 1.0)
    np.testing.assert_array_equal(moments[4:, 0], 0.0)
    p2 = np.zeros((1, 4, 2, 2)); p2[..., 1] = 1.0
    hist2, _ = synthetic.restate_rpe_counts(p2, shots, seed=99)
    np.testing.assert_array_equal(hist2[0, :, :, 1], [[N, N] for N in shots])
    # a negative probability is clamped to 0 before the running sum
    p3 = np.array([[[[-0.25, 1.0], [1.25, -0.25]]]])
    hist3, _ = synthetic.restate_rpe_counts(p3, 37, seed=1)
    np.testing.assert_array_equal(hist3[0, 0], [[0, 37], [37, 0]])
    with pytest.raises(ValueError):
        synthetic.restate_rpe_counts(np.zeros((1, 1, 2, 2)), 5, seed=1)
    with pytest.raises(ValueError):
        synthetic.restate_rpe_counts(p2, [1, 3, 0, 5], seed=1)


def test_counts_do_not_depend_on_the_batch():
    rng = np.random.default_rng(4)
    p = rng.dirichlet(np.ones(4), size=(8, 3, 2))
    whole = synthetic.restate_rpe_counts(p, [5, 8, 13], seed=2 ** 40 + 3)
    part = synthetic.restate_rpe_counts(p[5:], [5, 8, 13], seed=2 ** 40 + 3, first_item=5)
    np.testing.assert_array_equal(whole[0][5:], part[0])
    np.testing.assert_array_equal(whole[1][:, 5:], part[1])


# ------------------------------------------------------------------------------------------------ the settings helpers
def test_all_eigenvector_settings_are_the_reference_s():
    """robust_phase_estimation.py:111-126 by hand: every qubit in plusX; per X / Y qubit the terms X, X Z_q.., Y, Y Z_q.."""
    from fbx.observable_estimation import ExperimentSetting, PauliTerm, plusX
    cob = np.array([[1, 1], [1, -1]]) / math.sqrt(2)
    prep, pre_meas, settings = rpe.all_eigenvector_prep_meas_settings([3], cob)
    np.testing.assert_array_equal(prep, cob); np.testing.assert_array_equal(pre_meas, cob.conj().T)
    assert settings == [ExperimentSetting(plusX(3), PauliTerm({3: 'X'})), ExperimentSetting(plusX(3), PauliTerm({3: 'Y'}))]
    prep, pre_meas, settings = rpe.all_eigenvector_prep_meas_settings([0, 1], None)
    np.testing.assert_array_equal(prep, np.eye(4)); np.testing.assert_array_equal(pre_meas, np.eye(4))
    init = plusX(0) * plusX(1)
    want = [{0: 'X'}, {0: 'X', 1: 'Z'}, {0: 'Y'}, {0: 'Y', 1: 'Z'}, {1: 'X'}, {1: 'X', 0: 'Z'}, {1: 'Y'}, {1: 'Y', 0: 'Z'}]
    assert settings == [ExperimentSetting(init, PauliTerm(ops)) for ops in want]
    assert [str(s) for s in settings][:2] == ["X+_0 * X+_1→(1+0j)*X0", "X+_0 * X+_1→(1+0j)*X0Z1"]
    three = rpe.all_eigenvector_prep_meas_settings([0, 1, 2], None)[2]
    assert len(three) == 18 and three[1].observable == PauliTerm({0: 'X', 1: 'Z'}) and three[2].observable == PauliTerm({0: 'X', 2: 'Z'})
    with pytest.raises(ValueError):
        rpe.all_eigenvector_prep_meas_settings([0, 1], np.eye(2))


def test_pick_two_eigenvector_settings_are_the_reference_s():
    """robust_phase_estimation.py:129-149 by hand: the fixed qubit in plusZ / minusZ, the rotated one in plusX; I X, I Y, Z X, Z Y"""
    from fbx.observable_estimation import ExperimentSetting, PauliTerm, minusZ, plusX, plusZ
    for value, fixed_state in ((0, plusZ), (1, minusZ)):
        prep, pre_meas, settings = rpe.pick_two_eigenvecs_prep_meas_settings((4, value), 7)
        np.testing.assert_array_equal(prep, np.eye(4)); np.testing.assert_array_equal(pre_meas, np.eye(4))
        init = fixed_state(4) * plusX(7)
        want = [{7: 'X'}, {7: 'Y'}, {4: 'Z', 7: 'X'}, {4: 'Z', 7: 'Y'}]
        assert settings == [ExperimentSetting(init, PauliTerm(ops)) for ops in want]
    cob = synthetic.haar_unitary(4, np.random.RandomState(1))
    prep, pre_meas, _ = rpe.pick_two_eigenvecs_prep_meas_settings((0, 1), 1, cob)
    np.testing.assert_array_equal(prep, cob); np.testing.assert_array_equal(pre_meas, cob.conj().T)


def test_shot_schedule_is_acquire_rpe_data_s():
    np.testing.assert_array_equal(rpe.rpe_shot_schedule(8, min_shots=1), [18, 16, 13, 11, 8, 6, 3, 1])
    np.testing.assert_array_equal(rpe.rpe_shot_schedule(6), [500] * 6)
    np.testing.assert_array_equal(rpe.rpe_shot_schedule(3, multiplicative_factor=100, min_shots=200), [550, 300, 200])
    assert rpe.rpe_shot_schedule(4).dtype == np.int32


# ------------------------------------------------------------------------------------------------ the end-to-end seeds, on the host
def test_one_qubit_experiment_passes_on_the_host():
    """the reference's test_noiseless_rpe criterion for RZ(pi/4 - 0.5), K = 7, multiplicative_factor 10, through the host restatement"""
    gate = synthetic.pauli_transfer_matrix(cases.rz(cases.ONE_QUBIT_ANGLE))[None]
    shots = rpe.rpe_shot_schedule(cases.ONE_QUBIT_K, cases.ONE_QUBIT_FACTOR)
    phase = cases.host_phases(cases.host_moments(gate, cases.ONE_QUBIT_K, shots, cases.ONE_QUBIT_SEED))[0]
    bound = 2 * math.sqrt(rpe.get_variance_upper_bound(cases.ONE_QUBIT_K, cases.ONE_QUBIT_FACTOR))
    assert rpe_cases.circ_dist(phase, cases.ONE_QUBIT_ANGLE) <= bound


def test_cphase_experiment_passes_on_the_host():
    """diag(1, 1, 1, e^{i phi}) with every qubit in plusX: per X / Y qubit the relative phases 0 (partner selected in 0) and phi
    (partner in 1), within the reference tests' atol of 0.1; the call for the c-th X / Y qubit is global item c"""
    gate = synthetic.pauli_transfer_matrix(np.diag([1, 1, 1, np.exp(1j * cases.CPHASE_ANGLE)]))[None]
    shots = rpe.rpe_shot_schedule(cases.CPHASE_K)
    for c, (xy, z) in enumerate(((0, 1), (1, 0))):
        moments = cases.host_moments(gate, cases.CPHASE_K, shots, cases.CPHASE_SEED, first_item=c, xy_qubit=xy, z_qubit=z)
        for post_select, want in ((0, 0.0), (1, cases.CPHASE_ANGLE)):
            phase = cases.host_phases(moments, partner=True, post_select=post_select)[0]
            assert rpe_cases.circ_dist(phase, want) <= 0.1, (xy, post_select, phase)


def test_statistics_pass_on_the_host():
    """4096 uniform angles, K = 8, num_trials' own schedule: the rms circular error is below sqrt(get_variance_upper_bound(8))"""
    shots = rpe.rpe_shot_schedule(cases.STAT_K, min_shots=1)
    np.testing.assert_array_equal(shots, [18, 16, 13, 11, 8, 6, 3, 1])
    moments = cases.host_moments(cases.stat_gates(), cases.STAT_K, shots, cases.STAT_SEED)
    phases = rpe_cases.estimate_vec(moments[0], moments[1], np.sqrt(moments[4]), np.sqrt(moments[5]))
    rms = math.sqrt(np.mean(rpe_cases.circ_dist(phases, cases.stat_angles()) ** 2))
    bound = math.sqrt(rpe.get_variance_upper_bound(cases.STAT_K))
    print(f"host restatement: rms circular error {rms:.5f}, bound {bound:.5f}")
    assert abs(bound - 0.0195) < 5e-5
    assert rms <= bound
