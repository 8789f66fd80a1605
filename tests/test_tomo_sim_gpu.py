"""fbx_tomo_simulate on the GPU (include/fbx.h): exact means against dense numpy and a brute-force readout model, counts bit for
bit against the host restatement of the stream, on both sides of the kernel's one switch; a value depends on (seed, item,
setting) only; known answers; guards on the sampler that do not use the restatement; poisoned items; and the consumers.

The kernel has ONE switch (csrc/fbx_tomo_sim.hip): from LANE_MIN_UNITS = 131072 units (B x m) on a lane takes a setting, below a
wavefront does.  B = 5 of every design here is on the wavefront side; test_both_sides_of_the_lane_switch crosses it."""
import functools

import numpy as np
import pytest

import sampling_cases as sc
import tomo_sim_cases as tc
from tomo_sim_cases import B, FIRST, SEED, SHOTS

pytestmark = pytest.mark.gpu

LANE_MIN_UNITS = 131072
ALL_CASES = tc.PROCESS_CASES + tuple(f"state-{n}" for n in tc.STATE_CASES)


def design_of(case):
    from fbx.design import state_design
    return state_design(int(case[6:])) if case.startswith("state") else tc.process_case_design(case)


def flips_of(case, on):
    return sc.asymmetric_flips(design_of(case).n_qubits, B, seed=5) if on else None


@functools.lru_cache(maxsize=None)
def device(case, with_flips=False, shots=SHOTS):
    """(expectations, counts, std_errs, exact) of the B-item call that the tests share"""
    from fbx import tomography as t
    des, kw = design_of(case), dict(readout_flip=flips_of(case, with_flips), seed=SEED, first_item=FIRST, return_std_errs=True,
                                    return_exact=True)
    if case.startswith("state"):
        out = t.simulate_state_tomography_batch(des, tc.mixed_states(des.n_qubits), shots, **kw)
    else:
        out = t.simulate_process_tomography_batch(des, tc.damped_kraus(des.n_qubits), shots, rep="kraus", **kw)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def host(case, with_flips=False, shots=SHOTS):
    """the restatement from the device's exact means (mu = exact / c exactly: the coefficients are powers of two)"""
    from fbx import synthetic
    return synthetic.restate_tomography_counts(device(case, with_flips, shots)[3], design_of(case).coefs, shots, SEED, FIRST)


def check_counts(got, want, coefs, shots):
    """test 2: expectations bit for bit, counts == N, std_err within 8 ulp of the integer formula and exactly 0 at the ends"""
    e, c, s, _ = got
    we, wc, ws, kp = want
    bad = np.argwhere(e != we)
    assert bad.size == 0, f"{len(bad)} expectations differ, first at (item, setting) {bad[0].tolist()}: {e[tuple(bad[0])]!r} != {we[tuple(bad[0])]!r}"
    assert np.array_equal(c, wc) and np.all(c == float(shots))
    _, exact_s = tc.moments(kp, shots, np.broadcast_to(coefs, kp.shape))
    rel = np.abs(s - exact_s) / np.where(exact_s > 0, exact_s, 1.0)
    print(f"std_err: worst relative excursion {rel.max() / 2.0 ** -53:.2f} x 2^-53")
    assert np.all(rel <= 8 * 2.0 ** -53)
    ends = (kp == 0) | (kp == shots)
    assert np.all(s[ends] == 0.0)


# ------------------------------------------------------------------------------------------------ 1. exact means
@pytest.mark.parametrize("case", tc.PROCESS_CASES)
def test_exact_means_of_channels(gpu, case):
    from fbx import tomography as t
    from fbx_oracle import superops
    des, kraus = design_of(case), tc.damped_kraus(design_of(case).n_qubits)
    want, tol = tc.kraus_means(des, kraus), tc.tolerance(des)[None, :]
    got = device(case)[3]
    ptm = np.array([np.real(superops.kraus2pauli_liouville(list(k))) for k in kraus])
    again = t.simulate_process_tomography_batch(des, ptm, SHOTS, seed=SEED, first_item=FIRST, return_exact=True)[2]
    for name, x in (("kraus", got), ("pauli_liouville", again)):
        worst = (np.abs(x - want) / tol).max()
        print(f"{case} rep={name}: worst excursion {worst:.4f} of the tolerance")
        assert worst <= 1.0
    assert np.abs(want).max() > 0.5 and (np.abs(want) > 1e-3).mean() > 0.5      # (the case is not degenerate)


@pytest.mark.parametrize("n", tc.STATE_CASES)
def test_exact_means_of_states(gpu, n):
    des = design_of(f"state-{n}")
    want, tol = tc.state_means(des, tc.mixed_states(n)), tc.tolerance(des)[None, :]
    worst = (np.abs(device(f"state-{n}")[3] - want) / tol).max()
    print(f"state n={n}: worst excursion {worst:.4f} of the tolerance")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 2. counts bit for bit
@pytest.mark.parametrize("with_flips", (False, True))
@pytest.mark.parametrize("case", ALL_CASES)
def test_counts_bit_for_bit(gpu, case, with_flips):
    check_counts(device(case, with_flips), host(case, with_flips), design_of(case).coefs, SHOTS)
    kp = host(case, with_flips)[3]
    assert len(np.unique(kp)) > 10                       # (counts that vary: the comparison is not of constants)


# ------------------------------------------------------------------------------------------------ 3. both sides of every switch
@pytest.mark.parametrize("shots", (1, 3, 4, 70001))
def test_shot_counts_around_a_block(gpu, shots):
    check_counts(device("1q-pauli", True, shots), host("1q-pauli", True, shots), design_of("1q-pauli").coefs, shots)


def test_both_sides_of_the_lane_switch(gpu):
    """LANE_MIN_UNITS: 243 x 540 units take a lane each, 242 x 540 a wavefront each; the common items agree bit for bit and both
    equal the restatement (37 shots: nine blocks and a tail of one)"""
    from fbx import synthetic, tomography as t
    des, shots = design_of("2q-pauli"), 37
    big = LANE_MIN_UNITS // des.m + 1
    assert big * des.m >= LANE_MIN_UNITS > (big - 1) * des.m
    us = tc.unitaries(2, big)
    flips = sc.asymmetric_flips(2, big, seed=7)
    kw = dict(rep="unitary", seed=SEED, first_item=FIRST, return_std_errs=True, return_exact=True)
    lane = t.simulate_process_tomography_batch(des, us, shots, readout_flip=flips, **kw)
    wave = t.simulate_process_tomography_batch(des, us[:big - 1], shots, readout_flip=flips[:big - 1], **kw)
    for a, b in zip(lane, wave):
        assert np.array_equal(a[:big - 1], b)
    check_counts(lane, synthetic.restate_tomography_counts(lane[3], des.coefs, shots, SEED, FIRST), des.coefs, shots)


def _tail_call(batch, shots, first_item):
    """the smallest design (one-qubit SIC, 12 settings) with flips: the device's outputs and the restatement of the same items"""
    from fbx import synthetic, tomography as t
    des = design_of("1q-sic")
    got = t.simulate_process_tomography_batch(des, tc.unitaries(1, batch), shots, rep="unitary", seed=SEED, first_item=first_item,
                                              readout_flip=sc.asymmetric_flips(1, batch, seed=7), return_std_errs=True,
                                              return_exact=True)
    return des, got, lambda lo, hi: synthetic.restate_tomography_counts(got[3][lo:hi], des.coefs, shots, SEED, first_item + lo)


@pytest.mark.parametrize("shots", tc.TAIL_SHOTS)
def test_tail_block_on_the_wavefront_split(gpu, shots):
    """who owns the last, partial Philox block (tomo_sim_cases.TAIL_SHOTS): 3 x 12 units, a wavefront each"""
    des, got, restate = _tail_call(3, shots, FIRST)
    check_counts(got, restate(0, 3), des.coefs, shots)


@pytest.mark.parametrize("shots", tc.TAIL_SHOTS_LANE)
def test_tail_block_on_the_lane_split(gpu, shots):
    """... and 10923 x 12 >= LANE_MIN_UNITS units, a lane each: the first and the last items against the restatement"""
    big = LANE_MIN_UNITS // 12 + 1
    des, got, restate = _tail_call(big, shots, FIRST)
    assert des.m == 12 and big * des.m >= LANE_MIN_UNITS > (big - 1) * des.m
    for lo, hi in ((0, 40), (big - 40, big)):
        check_counts([a[lo:hi] for a in got], restate(lo, hi), des.coefs, shots)


# ------------------------------------------------------------------------------------------------ 4. (seed, g, k) only
def test_a_value_depends_on_seed_item_and_setting_only(gpu):
    from fbx import _lib, sampling, tomography as t
    case = "2q-sic"
    des, kraus, full = design_of(case), tc.damped_kraus(2), device(case, True)
    flips = flips_of(case, True)
    kw = dict(rep="kraus", seed=SEED, return_std_errs=True, return_exact=True)
    part = t.simulate_process_tomography_batch(des, kraus[2:4], SHOTS, readout_flip=flips[2:4], first_item=FIRST + 2, **kw)
    one = t.simulate_process_tomography_batch(des, kraus[:1], SHOTS, readout_flip=flips[:1], first_item=FIRST, **kw)
    for a, p, o in zip(full, part, one):
        assert np.array_equal(a[2:4], p) and np.array_equal(a[:1], o)
    other = t.simulate_process_tomography_batch(des, kraus, SHOTS, readout_flip=flips, first_item=FIRST, **{**kw, "seed": SEED + 1})
    assert np.array_equal(other[3], full[3]) and (other[0] != full[0]).mean() > 0.5
    # the _dev form on DeviceBuffers
    from fbx.operator_tools.superoperator_transformations import convert_batch
    ptm = np.ascontiguousarray(convert_batch("kraus", "pauli_liouville", kraus).real)
    DB, m = _lib.DeviceBuffer, des.m
    d_t, d_f = DB.from_array(ptm), DB.from_array(flips)
    outs = [DB(B * m * 8) for _ in range(4)]
    d_st = DB(B * 4)
    _lib.check(_lib.lib().fbx_tomo_simulate_dev(des.handle, B, d_t.ptr, SHOTS, d_f.ptr, SEED, FIRST, outs[0].ptr, outs[1].ptr,
                                                outs[2].ptr, outs[3].ptr, d_st.ptr))
    _lib.synchronize()
    for a, buf in zip(full, outs):
        assert np.array_equal(a, buf.to_array(np.float64, (B, m)))
    assert not d_st.to_array(np.int32, (B,)).any()
    for buf in [d_t, d_f, d_st] + outs:
        buf.free()
    # the key tag: fbx_sample_bitstrings under the same seed and item ids, drawing the one-qubit distribution of setting 0,
    # does not reproduce the counts of setting 0
    des1 = design_of("1q-pauli")
    e1, _, _, x1 = device("1q-pauli")
    q = np.clip(0.5 * (x1[:, 0] / des1.coefs[0]) + 0.5, 0, 1)
    bits = sampling.sample_bitstrings_batch(np.stack([q, 1 - q], axis=1), SHOTS, seed=SEED, first_item=FIRST)
    k_plus_sampler = SHOTS - bits[:, :, 0].sum(axis=1, dtype=np.int64)
    k_plus = np.rint((e1[:, 0] / des1.coefs[0] + 1) / 2 * SHOTS).astype(np.int64)
    assert not np.array_equal(k_plus, k_plus_sampler)
    # ... and the restatement with the untagged key (seed low ^ tag ^ tag) gives other counts than the device
    from fbx import synthetic
    untagged = synthetic.restate_tomography_counts(x1, des1.coefs, SHOTS, SEED ^ tc.KEY_TAG, FIRST)[0]
    assert (untagged != e1).mean() > 0.5 and np.array_equal(host("1q-pauli")[0], e1)


# ------------------------------------------------------------------------------------------------ 5. known answers
@pytest.mark.parametrize("n", (1, 2))
def test_identity_channel_known_answers(gpu, n):
    from fbx import tomography as t
    des, at = tc.with_identity_observable(n)
    D = 4 ** n
    ptm = np.broadcast_to(np.eye(D), (B, D, D))
    kw = dict(seed=SEED, first_item=FIRST, return_std_errs=True, return_exact=True)
    e, c, s, x = t.simulate_process_tomography_batch(des, ptm, SHOTS, **kw)
    # every mean is 0 or +-1; the design's Bloch table holds (1 / sqrt 2)^2 * 2 for the X and Y states: +-1 to a rounding
    sure = np.abs(np.abs(x) - 1.0) <= 4 * tc.EPS
    sure[:, at] = False
    assert np.all((x == 0.0) | sure | (np.arange(des.m) == at)[None, :]) and (x == 0.0).any() and (x[sure] > 0).any() and (x[sure] < 0).any()
    assert np.all(x[:, at] == -0.5) and np.all(e[:, at] == -0.5) and np.all(s[:, at] == 0.0)       # exactly its coefficient
    assert np.all(e[sure] == np.sign(x[sure])) and np.all(s[sure] == 0.0) and np.all(c == float(SHOTS))
    assert np.all(np.abs(e[x == 0.0]) < 0.2) and np.all(s[x == 0.0] > 0.0)
    # flips [1, 1] on every qubit: (-1)^weight exactly; flips of zeros: the call without flips, bit for bit
    weight = (des.paulis != 0).sum(axis=1)
    xf = t.simulate_process_tomography_batch(des, ptm, SHOTS, readout_flip=np.ones((n, 2)), **kw)[3]
    assert np.array_equal(xf, (-1.0) ** weight[None, :] * x)
    zero = t.simulate_process_tomography_batch(des, ptm, SHOTS, readout_flip=np.zeros((B, n, 2)), **kw)
    for a, b in zip(zero, (e, c, s, x)):
        assert np.array_equal(a, b)


def test_zero_flips_equal_no_flips_on_a_generic_channel(gpu):
    from fbx import tomography as t
    des = design_of("3q-shuffled")
    zero = t.simulate_process_tomography_batch(des, tc.damped_kraus(3), SHOTS, rep="kraus", readout_flip=np.zeros((3, 2)), seed=SEED,
                                               first_item=FIRST, return_std_errs=True, return_exact=True)
    for a, b in zip(zero, device("3q-shuffled")):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 6. the readout model
@pytest.mark.parametrize("case", ("2q-pauli", "3q-shuffled"))
def test_readout_model_against_brute_force(gpu, case):
    des = design_of(case)
    flips = flips_of(case, True)
    want = tc.flipped_means(des, tc.process_outputs(des, tc.damped_kraus(des.n_qubits)), flips)
    got = device(case, True)[3]
    worst = (np.abs(got - want) / tc.tolerance(des)[None, :]).max()
    print(f"{case} with flips: worst excursion {worst:.4f} of the tolerance")
    assert worst <= 1.0
    assert np.abs(got - device(case)[3]).max() > 0.1       # (the flips matter)


# ------------------------------------------------------------------------------------------------ 7. guards without the restatement
def test_sampler_guards(gpu):
    des = design_of("2q-pauli")
    e, _, _, x = device("2q-pauli")
    M = e.size
    assert M == 2700
    bound = 2.0 * np.sqrt(np.log(2 * M / 1e-9) / (2 * SHOTS))
    print(f"Hoeffding: worst |expect - exact| {np.abs(e - x).max():.4f}, bound {bound:.4f}")
    assert np.all(np.abs(e - x) <= bound)
    mu = x / des.coefs[None, :]
    q = np.floor(np.clip(0.5 * mu + 0.5, 0, 1) * 2.0 ** 32) * 2.0 ** -32
    k_plus = np.rint((e / des.coefs[None, :] + 1) / 2 * SHOTS)
    z = tc.z_score(k_plus, q, SHOTS)
    print(f"z = {z:.3f}")
    assert abs(z) < 6.0


# ------------------------------------------------------------------------------------------------ 8. poisoned items, bad arguments
def _poison_check(clean, got, status, bad):
    good = [b for b in range(B) if b != bad]
    assert status.tolist() == [int(b == bad) for b in range(B)]
    e, c, s, x = got
    assert np.all(np.isnan(e[bad])) and np.all(np.isnan(s[bad])) and np.all(np.isnan(x[bad])) and np.all(c[bad] == float(SHOTS))
    for a, b in zip(got, clean):
        assert np.array_equal(a[good], b[good])


@pytest.mark.parametrize("what", ("nan-ptm", "flip-1.5", "flip-nan"))
def test_poisoned_channel(gpu, what):
    from fbx import tomography as t
    from fbx.operator_tools.superoperator_transformations import convert_batch
    case, bad = "2q-sic", 3
    des = design_of(case)
    ptm = np.ascontiguousarray(convert_batch("kraus", "pauli_liouville", tc.damped_kraus(2)).real)
    flips = flips_of(case, True).copy()
    kw = dict(seed=SEED, first_item=FIRST, return_std_errs=True, return_exact=True)
    clean = t.simulate_process_tomography_batch(des, ptm, SHOTS, readout_flip=flips, **kw)
    if what == "nan-ptm":
        ptm[bad, 7, 9] = np.nan
    else:
        flips[bad, 1, 0] = 1.5 if what == "flip-1.5" else np.nan
    *got, status = t.simulate_process_tomography_batch(des, ptm, SHOTS, readout_flip=flips, return_status=True, **kw)
    _poison_check(clean, got, status, bad)
    with pytest.raises(ValueError, match="item 3"):
        t.simulate_process_tomography_batch(des, ptm, SHOTS, readout_flip=flips, **kw)


def test_poisoned_state(gpu):
    from fbx import tomography as t
    des, bad = design_of("state-3"), 1
    rho = tc.mixed_states(3).copy()
    rho[bad, 5, 2] = complex(0.0, np.inf)
    *got, status = t.simulate_state_tomography_batch(des, rho, SHOTS, seed=SEED, first_item=FIRST, return_std_errs=True,
                                                     return_exact=True, return_status=True)
    _poison_check(device("state-3"), got, status, bad)


def test_bad_arguments_and_exact_only(gpu):
    from fbx import _lib
    des = design_of("1q-pauli")
    lib, m = _lib.lib(), des.m
    ptm = np.ascontiguousarray(np.broadcast_to(np.eye(4), (B, 4, 4)))
    out = [np.full((B, m), -7.0) for _ in range(4)]
    st = np.full(B, -7, dtype=np.int32)
    p, ip = _lib.dptr, _lib.iptr

    def call(design=des.handle, batch=B, truth=ptm, shots=SHOTS, first=FIRST, outs=(0, 1, 2, 3)):
        ptrs = [p(out[i]) if i in outs else None for i in range(4)]
        return lib.fbx_tomo_simulate(design, batch, p(truth), shots, None, SEED, first, *ptrs, ip(st))
    for kw in (dict(batch=-1), dict(shots=-1), dict(shots=2 ** 32), dict(first=-1), dict(truth=None), dict(outs=()),
               dict(shots=0), dict(shots=0, outs=(1, 3)), dict(design=None)):
        assert call(**kw) == _lib.FBX_ERR_BAD_ARG, kw
        assert lib.fbx_last_error()
    assert all(np.all(o == -7.0) for o in out) and np.all(st == -7)          # refused before any buffer was touched
    assert call(batch=0) == _lib.FBX_OK and all(np.all(o == -7.0) for o in out)
    assert call(shots=0, outs=(3,)) == _lib.FBX_OK                           # the exact-expectations-only mode
    assert np.all(out[0] == -7.0) and np.all(st == 0)
    assert set(np.unique(np.round(out[3], 12))) == {0.0, 1.0, -1.0}
    assert call(outs=(1,)) == _lib.FBX_OK and np.all(out[1] == float(SHOTS)) and np.all(out[0] == -7.0)


# ------------------------------------------------------------------------------------------------ 9. consumers
@pytest.mark.parametrize("n", (1, 2))
def test_results_feed_the_reference_signature_estimators(gpu, n):
    from fbx import tomography as t
    from fbx.direct_fidelity_estimation import estimate_dfe
    qubits = list(range(n))
    u = tc.unitaries(n, 1)[0]
    res = t.simulate_tomography_results(qubits, "process", u, 2000, rep="unitary", seed=SEED, readout_flip=np.full((n, 2), 0.01))
    assert len(res) == len(t.generate_process_tomography_settings(qubits)) and all(r.total_counts == 2000 for r in res)
    choi = t.pgdb_process_estimate(res, qubits)
    assert choi.shape == (4 ** n, 4 ** n) and np.all(np.isfinite(choi)) and np.allclose(choi, choi.conj().T)
    f, err = estimate_dfe(res, "process")
    assert np.isfinite(f) and err > 0
    psi = u[:, :1]
    sres = t.simulate_tomography_results(qubits, "state", psi @ psi.conj().T, 2000, seed=SEED)
    rho = t.linear_inv_state_estimate(sres, qubits)
    assert rho.shape == (2 ** n, 2 ** n) and np.real(psi.conj().T @ rho @ psi)[0, 0] > 0.9
    fs, errs = estimate_dfe(sres, "state")
    assert np.isfinite(fs) and errs > 0


def test_resident_loop_equals_the_composed_calls(gpu):
    from fbx import distance_measures as dm, tomography as t
    from fbx.operator_tools.superoperator_transformations import convert_batch
    des, us = design_of("2q-pauli"), tc.unitaries(2, 8)
    flips = sc.asymmetric_flips(2, 8, seed=9) * 0.125
    choi, fid = t.simulate_and_estimate_process_batch(des, us, 1000, rep="unitary", readout_flip=flips, seed=SEED, first_item=FIRST)
    e, c = t.simulate_process_tomography_batch(des, us, 1000, rep="unitary", readout_flip=flips, seed=SEED, first_item=FIRST)
    want = t.pgdb_process_estimate_batch(des, e, c)
    truth = convert_batch("kraus", "pauli_liouville", us[:, None]).real.astype(np.complex128)
    want_fid = dm.process_fidelity_batch(truth, convert_batch("choi", "pauli_liouville", want))
    assert np.array_equal(choi, want) and np.array_equal(fid, want_fid)
    assert np.all((fid > 0.5) & (fid <= 1.0 + 1e-9))


def test_more_shots_give_a_better_estimate(gpu):
    """The direction only, on unitary truths at 100 and at 10^5 shots.  The process fidelity is LINEAR in the estimate
    (tr(R_truth^T R_est) / d^2), and linear inversion is unbiased: its fidelity to a unitary truth scatters on both sides of 1, so
    "better" for it is "closer to 1" (root mean square over the items: the scatter shrinks with sqrt(1000)).  PGDB estimates are
    physical, their fidelity cannot pass 1, and there the fidelity of every item rises."""
    from fbx import tomography as t
    des, us = design_of("2q-pauli"), tc.unitaries(2, 8)
    rms = {}
    for shots in (100, 10 ** 5):
        _, f = t.simulate_and_estimate_process_batch(des, us, shots, rep="unitary", seed=SEED, estimator="linear_inv")
        rms[shots] = float(np.sqrt(np.mean((1.0 - f) ** 2)))
        print(f"linear inversion, {shots} shots: fidelity to truth {f}")
    assert rms[10 ** 5] < rms[100]
    _, few = t.simulate_and_estimate_process_batch(des, us, 100, rep="unitary", seed=SEED)
    _, many = t.simulate_and_estimate_process_batch(des, us, 10 ** 5, rep="unitary", seed=SEED)
    print("pgdb, 100 shots:", few, "10^5 shots:", many)
    assert np.all(many > few) and np.all(many <= 1.0 + 1e-9)
