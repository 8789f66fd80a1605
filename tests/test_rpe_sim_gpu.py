"""fbx_rpe_simulate on the GPU (include/fbx.h): the outcome distributions against mpmath, histograms and moments bit for bit
against the host restatement of the stream, the bit records against the histograms and against fbx_rpe_from_shots, the stream's
dependence on (seed, item, depth, basis) only -- across batches and across the two work splits of the shot kernel -- poisoned
items, the refusals, the reference's own end-to-end criteria through simulate_rpe_results -> robust_phase_estimate, the
statistics of 4096 experiments against get_variance_upper_bound, and the resident chain.

The shot kernel has ONE switch (csrc/fbx_rpe_sim.hip): from FBX_RPE_SIM_LANE_MIN_UNITS units = B x K x 2 on a lane takes a unit,
below a wavefront does.  Every other case here is on the wavefront side; test_both_sides_of_the_lane_switch crosses it.  The distributions have one kernel per number of qubits (a lane per item for one, a wavefront per item for two)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import rpe_cases
import rpe_sim_cases as cases
from fbx import robust_phase_estimation as rpe
from fbx import synthetic
from tomo_sim_cases import TAIL_SHOTS, TAIL_SHOTS_LANE

pytestmark = pytest.mark.gpu

SEED = (0x9E37 << 32) + 0x12345                      # above 2^32: both key words are in use
RAGGED = [1, 3, 5, 8, 1001]                          # the block tails, fewer blocks than lanes, more blocks than lanes
ASYMMETRIC_1Q = np.array([[0.08, 0.13]])
ASYMMETRIC_2Q = np.array([[0.08, 0.13], [0.02, 0.05]])


def simulate(gate, K, kw, **more):
    return rpe.simulate_rpe_batch(gate, prep=kw.get("prep"), pre_meas=kw.get("meas"), xy_qubit=kw.get("xy_qubit", 0),
                                  z_qubit=kw.get("z_qubit"), flips=kw.get("flips"), num_depths=K, **more)


# ------------------------------------------------------------------------------------------------ distributions
@pytest.mark.parametrize("name", ["1q_rz", "1q_noisy_shared_basis", "1q_noisy_per_item_basis", "2q_diag_partner",
                                  "2q_diag_no_partner", "2q_shared_basis_partner_flips", "2q_per_item_basis_partner"])
def test_distributions_against_mpmath(gpu, name):
    """prob_out against 50-digit matrix powers of the same float64 inputs.  The tolerance is not fixed in advance: per case the
    float64 numpy mirror is measured against mpmath and the device is allowed 8 x that (its dot products are summed in another
    order and with fused multiply-adds), with a floor of 2^-50.  Measured on an MI355X: DESIGN.md section 4.22."""
    gate, K, kw, ref = cases.distribution_cases()[name]
    mirror_err = float(np.abs(cases.mirror(gate, K, kw) - ref).max())
    _, _, probs = simulate(gate, K, kw, num_shots=1, return_probabilities=True)
    device_err = float(np.abs(probs - ref).max())
    print(f"rpe_sim distributions {name}: numpy mirror {mirror_err:.3e}, device {device_err:.3e}")
    assert probs.shape == ref.shape
    assert device_err <= max(8 * mirror_err, 2.0 ** -50)


# ------------------------------------------------------------------------------------------------ the stream
STREAM_CASES = {
    "1q": ("1q_noisy_shared_basis", None),
    "1q_flips": ("1q_noisy_per_item_basis", ASYMMETRIC_1Q),
    "2q_partner": ("2q_diag_partner", None),
    "2q_partner_flips": ("2q_per_item_basis_partner", ASYMMETRIC_2Q),
    "2q_alone_flips": ("2q_diag_no_partner", ASYMMETRIC_2Q),
}


@pytest.mark.parametrize("name", sorted(STREAM_CASES))
def test_counts_are_the_documented_stream(gpu, name):
    """hist_out and all eight moment planes equal the host restatement of the reported distributions: integers exactly, moments
    bit for bit"""
    case, flips = STREAM_CASES[name]
    gate, _, kw, _ = cases.distribution_cases()[case]
    kw = dict(kw, flips=flips)
    moments, shots, probs, hist = simulate(gate, len(RAGGED), kw, num_shots=RAGGED, seed=SEED, first_item=3,
                                           return_probabilities=True, return_histograms=True)
    np.testing.assert_array_equal(shots, RAGGED)
    want_hist, want_moments = synthetic.restate_rpe_counts(probs, RAGGED, SEED, first_item=3)
    np.testing.assert_array_equal(hist.astype(np.int64), want_hist)
    np.testing.assert_array_equal(moments, want_moments)          # (NaN planes without a partner compare equal)
    assert np.isnan(moments[2]).all() == (kw.get("z_qubit") is None)
    assert hist.sum() == probs.shape[0] * 2 * sum(RAGGED)


# ------------------------------------------------------------------------------------------------ records
@pytest.mark.parametrize("name,xy,z", [("1q_noisy_shared_basis", 0, None), ("2q_diag_partner", 0, 1), ("2q_diag_partner", 1, 0),
                                       ("2q_diag_no_partner", 1, None)])
def test_records_reproduce_the_histograms_and_feed_from_shots(gpu, name, xy, z):
    S, K = 37, 4
    gate, _, kw, _ = cases.distribution_cases()[name]
    kw = dict(kw, xy_qubit=xy, z_qubit=z, flips=ASYMMETRIC_2Q if gate.shape[-1] == 16 else ASYMMETRIC_1Q)
    moments, _, hist, xb, yb = simulate(gate, K, kw, num_shots=S, seed=SEED, return_histograms=True, return_records=True)
    n = xb.shape[-1]
    assert xb.shape == (gate.shape[0], K, S, n) and xb.dtype == np.uint8 and xb.max() <= 1 and yb.max() <= 1
    for basis, bits in enumerate((xb, yb)):
        outcome = bits[..., xy].astype(np.int64) if z is None else 2 * bits[..., xy].astype(np.int64) + bits[..., z]
        counted = np.stack([(outcome == o).sum(axis=2) for o in range(hist.shape[-1])], axis=-1)
        np.testing.assert_array_equal(counted, hist[:, :, basis].astype(np.int64))
        if n == 2 and z is None:
            assert not bits[..., 1 - xy].any()                      # a column nobody measures stays 0
    for post_select in (0, 1) if z is not None else (0,):
        _, stats = rpe.robust_phase_estimate_from_shots_batch(xb, yb, xy, z, post_select=post_select, return_stats=True)
        x, y, xz, yz, vx, vy, vxz, vyz = moments
        if z is None:
            want = np.stack([x, y, np.sqrt(vx), np.sqrt(vy)], axis=-1)
        else:
            sign = 1.0 if post_select == 0 else -1.0
            want = np.stack([x + sign * xz, y + sign * yz, np.sqrt(np.sqrt(vxz) ** 2 + np.sqrt(vx) ** 2),
                             np.sqrt(np.sqrt(vyz) ** 2 + np.sqrt(vy) ** 2)], axis=-1)
        np.testing.assert_array_equal(stats["moments"], want)


def test_ragged_records_are_refused(gpu):
    gate, _, kw, _ = cases.distribution_cases()["1q_rz"]
    with pytest.raises(ValueError):
        simulate(gate, 3, kw, num_shots=[5, 5, 6], return_records=True)
    lib = gpu.lib()
    shots = np.array([5, 5, 6], dtype=np.int32)
    bits = np.zeros(3 * 6, dtype=np.uint8)
    g = np.ascontiguousarray(gate)
    rc = lib.fbx_rpe_simulate(1, 1, 3, gpu.dptr(g), None, None, 0, None, 0, -1, None, gpu.iptr(shots), 1, 0, None, None, None,
                              gpu.ptr(bits, C.c_uint8), None, None)
    assert rc == gpu.FBX_ERR_BAD_ARG and b"ragged" in lib.fbx_last_error()


# ------------------------------------------------------------------------------------------------ batch independence, dispatch
@pytest.mark.parametrize("two_qubits", [False, True])
def test_items_do_not_depend_on_the_batch(gpu, two_qubits):
    rng = np.random.RandomState(8)
    if two_qubits:
        gate = np.stack([cases.diagonal_gate_ptm(*rng.uniform(0, 6, 3), 0.01) for _ in range(8)])
        kw = dict(xy_qubit=1, z_qubit=0, flips=rng.uniform(0, 0.2, (8, 2, 2)))
    else:
        gate = np.stack([cases.noisy_rotation_ptm((0.3, 0.1, 0.9), a, 0.01, 0.02) for a in rng.uniform(0, 6, 8)])
        kw = dict(flips=rng.uniform(0, 0.2, (8, 1, 2)))
    whole = simulate(gate, 5, kw, num_shots=RAGGED, seed=SEED, return_probabilities=True, return_histograms=True)
    part = simulate(gate[5:], 5, dict(kw, flips=kw["flips"][5:]), num_shots=RAGGED, seed=SEED, first_item=5,
                    return_probabilities=True, return_histograms=True)
    np.testing.assert_array_equal(whole[0][:, 5:], part[0])
    np.testing.assert_array_equal(whole[2][5:], part[2])
    np.testing.assert_array_equal(whole[3][5:], part[3])


def lane_min_units():
    """the switch of the shot kernel, read from the source and from the binding, which must agree"""
    from fbx import _lib
    src = os.path.join(os.path.dirname(_lib.__file__), "..", "csrc", "fbx_rpe_sim.hip")
    value = int(re.search(r"#define\s+FBX_RPE_SIM_LANE_MIN_UNITS\s+(\d+)", open(src).read()).group(1))
    assert value == _lib.RPE_SIM_LANE_MIN_UNITS
    return value


@pytest.mark.parametrize("two_qubits", [False, True])
def test_both_sides_of_the_lane_switch(gpu, two_qubits):
    """one call large enough for the lane form against slices small enough for the wavefront form, item for item; 1 shot and,
    in a second pass, the ragged tail of the schedule on the last slice only"""
    K = 8
    B = lane_min_units() // (2 * K)
    assert B * K * 2 >= lane_min_units() and (B - 1) * K * 2 < lane_min_units()
    rng = np.random.RandomState(9)
    angles = rng.uniform(0, 2 * math.pi, B)
    if two_qubits:
        base = synthetic.pauli_transfer_matrix(np.diag([1, 1, 1, 1j]))
        gate = np.broadcast_to(base, (B, 16, 16)).copy()
        gate[:, 0, 0] = 1.0 - 1e-3 * rng.uniform(0, 1, B)         # items differ: a little trace loss each
        kw = dict(xy_qubit=0, z_qubit=1)
    else:
        c, s = np.cos(angles), np.sin(angles)
        gate = np.zeros((B, 4, 4))
        gate[:, 0, 0] = gate[:, 3, 3] = 1.0
        gate[:, 1, 1] = c; gate[:, 1, 2] = -s; gate[:, 2, 1] = s; gate[:, 2, 2] = c
        kw = {}
    for shots in (1, [7, 1, 3, 2, 5, 1, 4, 9]):
        big = simulate(gate, K, kw, num_shots=shots, seed=SEED, return_probabilities=True, return_histograms=True)
        for lo in (0, B // 2 - 3, B - 100):
            small = simulate(gate[lo:lo + 100], K, kw, num_shots=shots, seed=SEED, first_item=lo, return_probabilities=True,
                             return_histograms=True)
            np.testing.assert_array_equal(big[0][:, lo:lo + 100], small[0])
            np.testing.assert_array_equal(big[2][lo:lo + 100], small[2])
            np.testing.assert_array_equal(big[3][lo:lo + 100], small[3])
        assert big[3].sum() == B * 2 * int(np.sum(np.broadcast_to(shots, (K,))))


def _tail_call(batch, shots):
    """the smallest experiment (one qubit, one depth) with flips, with and without records -- two instantiations of the shot
    kernel, and the records take the shot index from the walk"""
    rng = np.random.RandomState(10)
    angles = rng.uniform(0, 2 * math.pi, batch)
    c, s = np.cos(angles), np.sin(angles)
    gate = np.zeros((batch, 4, 4))                              # a shrunk turn about z, another one per item
    gate[:, 0, 0] = gate[:, 3, 3] = 1.0
    gate[:, 1, 1] = 0.9 * c; gate[:, 1, 2] = -0.9 * s; gate[:, 2, 1] = 0.9 * s; gate[:, 2, 2] = 0.9 * c
    kw = dict(flips=rng.uniform(0, 0.2, (batch, 1, 2)))
    moments, _, probs, hist = simulate(gate, 1, kw, num_shots=shots, seed=SEED, first_item=3, return_probabilities=True,
                                       return_histograms=True)
    want_hist, want_moments = synthetic.restate_rpe_counts(probs, shots, SEED, first_item=3)
    np.testing.assert_array_equal(hist.astype(np.int64), want_hist)
    np.testing.assert_array_equal(moments, want_moments)
    m2, _, h2, xb, yb = simulate(gate, 1, kw, num_shots=shots, seed=SEED, first_item=3, return_histograms=True, return_records=True)
    np.testing.assert_array_equal(h2, hist)
    np.testing.assert_array_equal(m2, moments)
    assert xb.shape == yb.shape == (batch, 1, shots, 1)
    for basis, bits in enumerate((xb, yb)):
        np.testing.assert_array_equal(bits[..., 0].astype(np.int64).sum(axis=2), want_hist[:, :, basis, 1])
    return want_hist


@pytest.mark.parametrize("shots", TAIL_SHOTS)
def test_tail_block_on_the_wavefront_split(gpu, shots):
    """who owns the last, partial Philox block (tomo_sim_cases.TAIL_SHOTS): 3 x 1 x 2 units, a wavefront each"""
    _tail_call(3, shots)


@pytest.mark.parametrize("shots", TAIL_SHOTS_LANE)
def test_tail_block_on_the_lane_split(gpu, shots):
    """... and lane_min_units() units = B x 1 x 2, a lane each"""
    hist = _tail_call(lane_min_units() // 2, shots)
    assert len(np.unique(hist[..., 1])) > 2                  # (counts that vary: the comparison is not of constants)


# ------------------------------------------------------------------------------------------------ poison, limits
@pytest.mark.parametrize("two_qubits", [False, True])
def test_poisoned_items_are_reported_and_contained(gpu, two_qubits):
    """B = 4: a NaN in item 1's gate, a flip of 1.5 on item 2, an all-zero matrix for item 3 -- data errors reported through
    status, NaN / 0 outputs for them, item 0 bit-identical to the clean call"""
    if two_qubits:
        gate = np.stack([cases.diagonal_gate_ptm(0.3 + b, 1.0, 2.0, 0.01) for b in range(4)])
        kw, flips = dict(xy_qubit=0, z_qubit=1), np.broadcast_to(ASYMMETRIC_2Q, (4, 2, 2)).copy()
    else:
        gate = np.stack([cases.noisy_rotation_ptm((0.3, 0.1, 0.9), 0.5 + b, 0.01, 0.02) for b in range(4)])
        kw, flips = {}, np.broadcast_to(ASYMMETRIC_1Q, (4, 1, 2)).copy()
    S, K = 9, 3
    flags = dict(num_shots=S, seed=SEED, return_probabilities=True, return_histograms=True, return_records=True, return_status=True)
    clean = simulate(gate, K, dict(kw, flips=flips), **flags)
    assert not clean[-1].any()
    bad_gate, bad_flips = gate.copy(), flips.copy()
    bad_gate[1, 1, 2] = np.nan
    bad_flips[2, 0, 1] = 1.5
    bad_gate[3] = 0.0
    moments, _, probs, hist, xb, yb, status = simulate(bad_gate, K, dict(kw, flips=bad_flips), **flags)
    np.testing.assert_array_equal(status, [0, 1, 1, 1])
    assert np.isnan(moments[:, 1:]).all() and np.isnan(probs[1:]).all()
    assert not hist[1:].any() and not xb[1:].any() and not yb[1:].any()
    for got, want in zip((moments[:, :1], probs[:1], hist[:1], xb[:1], yb[:1]),
                         (clean[0][:, :1], clean[2][:1], clean[3][:1], clean[4][:1], clean[5][:1])):
        np.testing.assert_array_equal(got, want)
    with pytest.raises(ValueError):
        simulate(bad_gate, K, dict(kw, flips=bad_flips), num_shots=S)
    inf_gate = gate.copy()
    inf_gate[2] *= 1e200                                           # finite input, a power that overflows
    assert list(simulate(inf_gate, 4, kw, num_shots=S, return_status=True)[-1]) == [0, 0, 1, 0]


def test_limits_raise_the_documented_errors(gpu):
    from fbx import FbxError
    gate, _, kw, _ = cases.distribution_cases()["1q_rz"]
    with pytest.raises(ValueError):
        simulate(gate, 0, kw, num_shots=5)
    with pytest.raises(FbxError) as e:
        simulate(gate, 63, kw, num_shots=5)
    assert e.value.code == gpu.FBX_ERR_UNSUPPORTED
    assert simulate(gate, 62, kw, num_shots=1)[0].shape == (8, 1, 62)          # every depth the analysis accepts
    with pytest.raises(FbxError) as e:
        rpe.simulate_rpe_batch(np.eye(8, dtype=complex)[None], num_depths=2, num_shots=5)
    assert e.value.code == gpu.FBX_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        simulate(gate, 3, kw, num_shots=[5, 0, 5])
    with pytest.raises(ValueError):
        simulate(gate, 3, dict(kw, z_qubit=0), num_shots=5)        # the partner is the rotated qubit
    with pytest.raises(ValueError):
        simulate(gate, 3, dict(kw, xy_qubit=1), num_shots=5)
    lib = gpu.lib()
    g = np.ascontiguousarray(np.zeros((1, 64, 64)))
    shots = np.full(3, 5, dtype=np.int32)
    out = np.empty(8 * 3)
    rc = lib.fbx_rpe_simulate(3, 1, 3, gpu.dptr(g), None, None, 0, None, 0, -1, None, gpu.iptr(shots), 1, 0, None, None,
                              gpu.dptr(out), None, None, None)
    assert rc == gpu.FBX_ERR_UNSUPPORTED
    g1 = np.ascontiguousarray(gate)
    rc = lib.fbx_rpe_simulate(1, 1, 3, gpu.dptr(g1), None, None, 0, None, 0, -1, None, gpu.iptr(shots), 1, 0, None, None, None,
                              None, None, None)
    assert rc == gpu.FBX_ERR_BAD_ARG and b"every output is NULL" in lib.fbx_last_error()


# ------------------------------------------------------------------------------------------------ end to end, reference structure
def test_one_qubit_experiment_in_the_reference_structure(gpu):
    """the reference's test_noiseless_rpe: RZ(pi/4 - 0.5), K = 7, multiplicative_factor 10; the estimate within
    2 sqrt(get_variance_upper_bound(7, 10)) of the angle (seed confirmed on the host: tests/test_rpe_sim_cpu.py)"""
    q = 3
    results = rpe.simulate_rpe_results(cases.rz(cases.ONE_QUBIT_ANGLE), None, [q], num_depths=cases.ONE_QUBIT_K,
                                       multiplicative_factor=cases.ONE_QUBIT_FACTOR, seed=cases.ONE_QUBIT_SEED)
    assert len(results) == cases.ONE_QUBIT_K and all(len(layer) == 2 for layer in results)
    assert [r.setting.observable[q] for r in results[0]] == ['X', 'Y'] and results[0][0].total_counts == 500
    phase = rpe.robust_phase_estimate(results, [q])
    bound = 2 * math.sqrt(rpe.get_variance_upper_bound(cases.ONE_QUBIT_K, cases.ONE_QUBIT_FACTOR))
    assert rpe_cases.circ_dist(phase, cases.ONE_QUBIT_ANGLE) <= bound
    # the same numbers as the host restatement: the structure only rearranges the moments
    gate = synthetic.pauli_transfer_matrix(cases.rz(cases.ONE_QUBIT_ANGLE))[None]
    shots = rpe.rpe_shot_schedule(cases.ONE_QUBIT_K, cases.ONE_QUBIT_FACTOR)
    probs = rpe.simulate_rpe_batch(gate, num_depths=cases.ONE_QUBIT_K, num_shots=shots, seed=cases.ONE_QUBIT_SEED,
                                   return_probabilities=True)[2]
    host = synthetic.restate_rpe_counts(probs, shots, cases.ONE_QUBIT_SEED)[1]
    assert [r.expectation for layer in results for r in layer] == [host[basis, 0, j] for j in range(cases.ONE_QUBIT_K) for basis in (0, 1)]


def test_cphase_experiment_in_the_reference_structure(gpu):
    """diag(1, 1, 1, e^{i phi}) through all_eigenvector_prep_meas_settings: robust_phase_estimate returns the relative phases
    {0, phi} for each X / Y qubit within 0.1, the atol of the reference's tests"""
    qubits = [0, 1]
    U = np.diag([1, 1, 1, np.exp(1j * cases.CPHASE_ANGLE)])
    results = rpe.simulate_rpe_results(U, None, qubits, num_depths=cases.CPHASE_K, seed=cases.CPHASE_SEED)
    assert len(results) == cases.CPHASE_K and all(len(layer) == 8 for layer in results)
    order = [r.setting.observable.operations_as_set() for r in results[0]]
    assert order == [frozenset(s) for s in ([(0, 'X')], [(0, 'X'), (1, 'Z')], [(0, 'Y')], [(0, 'Y'), (1, 'Z')],
                                            [(1, 'X')], [(1, 'X'), (0, 'Z')], [(1, 'Y')], [(1, 'Y'), (0, 'Z')])]
    phases = rpe.robust_phase_estimate(results, qubits)
    assert len(phases) == 4
    for got, want in zip(phases, (0.0, cases.CPHASE_ANGLE, 0.0, cases.CPHASE_ANGLE)):
        assert rpe_cases.circ_dist(got, want) <= 0.1, phases
    # the pick-two experiment on the same gate: qubit 0 fixed in |1>, qubit 1 rotated -- one phase, phi
    _, _, settings = rpe.pick_two_eigenvecs_prep_meas_settings((0, 1), 1)
    fixed = rpe.simulate_rpe_results(U, None, qubits, num_depths=cases.CPHASE_K, settings=settings, seed=cases.CPHASE_SEED)
    assert all(len(layer) == 4 for layer in fixed)
    picked = rpe.robust_phase_estimate(fixed, qubits)
    assert len(picked) == 1 and rpe_cases.circ_dist(picked[0], cases.CPHASE_ANGLE) <= 0.1, picked


# ------------------------------------------------------------------------------------------------ statistics, resident chain
def test_rms_error_is_below_the_variance_bound(gpu):
    """4096 uniform angles, K = 8, no noise, num_trials' own schedule 18, 16, 13, 11, 8, 6, 3, 1: the rms circular error is at
    most sqrt(get_variance_upper_bound(8)) = 0.0195 (a numpy Monte Carlo of the experiment gives 0.0088-0.0092; seed confirmed on
    the host)"""
    angles = cases.stat_angles()
    phases, depth, err = rpe.simulate_and_estimate_rpe_batch(cases.stat_gates(), num_depths=cases.STAT_K, min_shots=1,
                                                             seed=cases.STAT_SEED, true_phases=angles)
    rms = math.sqrt(np.mean(err ** 2))
    bound = math.sqrt(rpe.get_variance_upper_bound(cases.STAT_K))
    print(f"rpe_sim statistics: rms circular error {rms:.5f}, bound {bound:.5f}, cut short {int((depth < cases.STAT_K).sum())}")
    np.testing.assert_array_equal(err, rpe_cases.circ_dist(phases, angles))
    assert rms <= bound


@pytest.mark.parametrize("two_qubits", [False, True])
def test_resident_chain_equals_the_two_calls(gpu, two_qubits):
    if two_qubits:
        gate, _, kw, _ = cases.distribution_cases()["2q_shared_basis_partner_flips"]
    else:
        gate, _, kw, _ = cases.distribution_cases()["1q_noisy_shared_basis"]
    args = dict(prep=kw.get("prep"), pre_meas=kw.get("meas"), xy_qubit=kw.get("xy_qubit", 0), z_qubit=kw.get("z_qubit"),
                flips=kw.get("flips"), num_depths=9, multiplicative_factor=3.0, min_shots=20, seed=SEED, first_item=2)
    m, _ = rpe.simulate_rpe_batch(gate, **args)
    for post_select in (0, 1) if two_qubits else (0,):
        partner = (m[2], m[3], m[6], m[7]) if two_qubits else (None,) * 4
        want, stats = rpe.estimate_phase_from_moments_batch(m[0], m[1], m[4], m[5], *partner, post_select=post_select,
                                                            errors_are_variances=True, return_stats=True)
        got, depth = rpe.simulate_and_estimate_rpe_batch(gate, post_select=post_select, **args)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(depth, stats["depth_reached"])
