"""The DFE kernels (csrc/fbx_dfe.hip) on the GPU: bit for bit against the host mirror, against dense matrices and a
density-matrix simulation where those fit, and the shot counts against the restated stream.  Shapes are the smallest that
reach every path: widths on both sides of 32 bits and at 64, batches that are no multiple of a wavefront, both sides of the
lane / wavefront switch of the simulation."""
import ctypes as C
import functools

import numpy as np
import pytest

import dfe_cases as dc
from fbx import _lib, clifford_circuit as cc, direct_fidelity_estimation as dfe, synthetic
from fbx.observable_estimation import calibrate_expectations_batch
from tomo_sim_cases import TAIL_SHOTS, TAIL_SHOTS_LANE

pytestmark = pytest.mark.gpu

PAIRS = {64: [(31, 32), (0, 63), (62, 63)], 33: [(31, 32), (0, 32)], 32: [(0, 31), (30, 31)]}


def circuit(n, n_gates, seed=0):
    return dc.random_circuit(np.random.default_rng(1000 * n + n_gates + seed), n, n_gates, PAIRS.get(n, ()))


# ------------------------------------------------------------------ 1. conjugation
@pytest.mark.parametrize("n", [1, 2, 3, 32, 33, 64])
def test_conjugation_equals_the_mirror_bit_for_bit(gpu, n):
    rng = np.random.default_rng(n)
    for n_gates in (0, 1, 300):
        gates = circuit(n, n_gates)
        if n_gates == 300 and n in PAIRS:
            assert all(any(set(q) == set(p) for _, q in gates) for p in PAIRS[n])
        for M in (1, 63, 1000):
            x, z, s = dc.random_paulis(rng, n, M)
            for inverse in (False, True):
                want = cc.conjugate_paulis(gates, n, x, z, s, inverse=inverse)
                got = cc.conjugate_paulis(gates, n, x, z, s, inverse=inverse, device=0)
                for a, b in zip(got, want):
                    assert a.dtype == b.dtype and np.array_equal(a, b), (n, n_gates, M, inverse)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_conjugation_against_dense(gpu, n):
    gates = circuit(n, 40)
    labels = dc.all_labels(n)
    x, z = cc.paulis_from_labels(labels)
    xo, zo, so = cc.conjugate_paulis(gates, n, x, z, device=0)
    u = dc.dense_circuit(gates, n)
    for lab, out, s in zip(labels, cc.labels_from_paulis(n, xo, zo), so):
        assert np.abs(u @ dc.dense_pauli(lab) @ u.conj().T - dc.dense_pauli(out, s)).max() < 1e-12, lab


def test_conjugation_known_answer_ghz_64(gpu):
    """H on qubit 0, then a CNOT chain of 63: Z_0 goes to X on every qubit, Z_j to Z_{j-1} Z_j."""
    gates = dc.ghz_circuit(64)
    z = np.uint64(1) << np.arange(64, dtype=np.uint64)
    xo, zo, so = cc.conjugate_paulis(gates, 64, np.zeros(64, dtype=np.uint64), z, device=0)
    assert xo[0] == np.uint64(2 ** 64 - 1) and zo[0] == 0 and not so.any()
    assert not xo[1:].any() and np.array_equal(zo[1:], z[1:] | z[:-1])


# ------------------------------------------------------------------ 2. settings
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("kind", ["state", "process"])
def test_exhaustive_settings_equal_the_reference_loops(gpu, kind, n):
    gates = circuit(n, 25)
    make = dfe.generate_exhaustive_process_dfe_experiment if kind == "process" else dfe.generate_exhaustive_state_dfe_experiment
    expt = make(None, gates, list(range(n)))
    assert dc.settings_as_tuples(n, expt) == dc.reference_settings(kind, n, gates)


@pytest.mark.parametrize("n", [1, 5, 64])
@pytest.mark.parametrize("kind", ["state", "process"])
def test_monte_carlo_settings_equal_the_restated_stream(gpu, kind, n):
    gates = circuit(n, 100)
    seed = 0xC0FFEE1234567 + n
    make = dfe.generate_monte_carlo_process_dfe_experiment if kind == "process" else dfe.generate_monte_carlo_state_dfe_experiment
    expt = make(None, gates, list(range(n)), n_terms=500, seed=seed)
    want = cc.restate_dfe_settings(n, kind, 500, seed, gates)
    for name, arr in want.items():
        assert np.array_equal(getattr(expt, name), arr), (kind, n, name)
    if n == 1:
        assert dc.monte_carlo_inputs(kind, 1, 500, seed)[2] > 100     # the rejection loop was exercised


@pytest.mark.parametrize("kind,n,n_terms", [("state", 3, 0), ("process", 3, 0), ("state", 33, 300), ("process", 33, 300),
                                            ("state", 64, 300), ("process", 64, 300)])
def test_without_noise_every_setting_has_expectation_one(gpu, kind, n, n_terms):
    """sigma * c == +1 for every setting of all four generators: the whole sign bookkeeping (conjugation forwards, propagation
    backwards, eigenvalue bits, observable sign).  exact_out is 1.0 exactly."""
    gates = circuit(n, 200, seed=1)
    expt = dfe._generate(kind, gates, list(range(n)), n_terms, 77)
    sigma, _ = expt.propagate()
    assert np.array_equal(sigma * (1 - 2 * expt.obs_sign.astype(np.int64)), np.ones(expt.m, dtype=np.int64))
    exact = dfe.simulate_dfe_batch(expt, np.zeros((2, 1)), 0)
    assert np.array_equal(exact, np.ones((2, expt.m)))


# ------------------------------------------------------------------ 3. propagation
def experiment_from(kind, n, gates, arrays):
    return dfe.DfeExperiment(kind, list(range(n)), gates, arrays)


@pytest.mark.parametrize("n", [3, 33, 64])
def test_propagation_equals_the_mirror(gpu, n):
    gates = circuit(n, 300, seed=2)
    rng = np.random.default_rng(n)
    expt = experiment_from("process", n, gates, cc.restate_dfe_settings(n, "process", 333, 9, gates))
    with_noiseless = rng.integers(0, 16, size=300).astype(np.uint8)
    with_noiseless[rng.random(300) < 0.2] = 255
    for K, classes in ((1, None), (1, np.where(with_noiseless == 255, 255, 0).astype(np.uint8)), (16, with_noiseless),
                       (3, rng.integers(0, 3, size=300).astype(np.uint8))):
        sigma, touches = expt.propagate(classes, K)
        want_sigma, want_touches = cc.propagate_settings(gates, n, expt.in_x, expt.in_z, expt.in_minus, expt.obs_x, expt.obs_z,
                                                         classes, K)
        assert sigma.dtype == np.int8 and touches.dtype == np.uint32 and touches.shape == (333, K)
        assert np.array_equal(sigma, want_sigma) and np.array_equal(touches, want_touches), (n, K)
        assert touches.sum() > 0


@pytest.mark.parametrize("n", [2, 3, 4])
def test_propagation_against_dense(gpu, n):
    """A gate is touched iff fully depolarizing its qubits changes the back-propagated matrix; settings that are not
    stabilizers (a wrong in-state label where the arriving Pauli acts) give sigma == 0."""
    gates, classes, s, wrong, want_sigma, want_touches = dc.propagation_case(n)
    sigma, touches = experiment_from("process", n, gates, s).propagate(classes, 3)
    assert np.array_equal(touches, want_touches)
    assert np.abs(sigma - want_sigma).max() < 1e-12
    assert (sigma[wrong] == 0).sum() > 0 and set(sigma[~wrong].tolist()) <= {-1, 1}


# ------------------------------------------------------------------ 4. exact means against the product formula
@pytest.mark.parametrize("n,K", [(3, 1), (33, 5), (64, 16)])
def test_exact_means_against_the_product_formula(gpu, n, K):
    """|got - want| <= (G + n + K + 4) 2^-52 |want|: one rounding per factor, whichever way the powers are formed."""
    G, B = 300, 3
    gates = circuit(n, G, seed=3)
    rng = np.random.default_rng(50 + n)
    classes = rng.integers(0, K, size=G).astype(np.uint8)
    expt = dfe.generate_monte_carlo_process_dfe_experiment(None, gates, list(range(n)), n_terms=301, seed=4)
    p, f = rng.uniform(0.0, 0.02, size=(B, K)), rng.uniform(0.0, 0.05, size=(B, n))
    sigma, touches = expt.propagate(classes, K)
    support = expt.obs_x | expt.obs_z
    on = np.array([[(int(sv) >> q) & 1 for q in range(n)] for sv in support.tolist()], dtype=bool)
    for flips, calibrate in ((None, False), (f, False), (f, True)):
        got = dfe.simulate_dfe_batch(expt, p, 0, noise_class=classes, readout_flip=flips, calibrate=calibrate)
        worst = 0.0
        for b in range(B):
            want = np.ones(expt.m) if calibrate else (1 - 2 * expt.obs_sign.astype(float)) * sigma
            if not calibrate:
                want = want * np.prod(np.power(1.0 - p[b][None, :], touches), axis=1)
            if flips is not None:
                want = want * np.prod(np.where(on, 1.0 - 2.0 * f[b][None, :], 1.0), axis=1)
            bound = (G + n + K + 4) * 2.0 ** -52 * np.abs(want)
            assert np.all(want != 0)
            worst = max(worst, float((np.abs(got[b] - want) / bound).max()))
        print(f"n = {n}, K = {K}, flips {flips is not None}, calibration {calibrate}: worst excursion {worst:.3f} of the bound")
        assert worst <= 1.0


# ------------------------------------------------------------------ 5. exact means against a density-matrix simulation
@functools.lru_cache(maxsize=None)
def dense_case(kind, n):
    """16 gates in 3 classes (every seventh noiseless), p in [0.01, 0.1], flips in [0.01, 0.05]: worst case |mu| >= 0.9^16 *
    0.9^4 = 0.12.  The exhaustive settings come from the host mirror, the dense means from dfe_cases."""
    rng = np.random.default_rng(60 + 10 * n + (kind == "process"))
    gates = circuit(n, 16, seed=5)
    classes = rng.integers(0, 3, size=16).astype(np.uint8)
    classes[::7] = 255
    p, f = rng.uniform(0.01, 0.1, size=3), rng.uniform(0.01, 0.05, size=n)
    s = cc.restate_dfe_settings(n, kind, 0, 0, gates)
    tuples = dc.settings_as_tuples(n, s)
    with_flips = dc.dense_exact_means(n, tuples, gates, classes, p, f)
    without = dc.dense_exact_means(n, tuples, gates, classes, p, None)
    d = 2 ** n
    if kind == "state":
        psi = dc.dense_circuit(gates, n)[:, 0]
        rho = dc.noisy_channel(dc.product_state("Z" * n, (0,) * n), gates, n, classes, p)
        fidelity = float((psi.conj() @ rho @ psi).real)
    else:
        u = dc.dense_circuit(gates, n)
        r_u = dc.pauli_transfer_matrix(lambda a: u @ a @ u.conj().T, n)
        r_e = dc.pauli_transfer_matrix(lambda a: dc.noisy_channel(a, gates, n, classes, p), n)
        fidelity = float((np.trace(r_u.T @ r_e) + d) / (d * d + d))
    return gates, classes, p, f, s, with_flips, without, fidelity


@pytest.mark.parametrize("kind,n", [("state", 3), ("state", 4), ("process", 1), ("process", 2)])
def test_exact_means_and_fidelity_against_a_density_matrix(gpu, kind, n):
    """Within 1e-10 absolute: the dense fp64 chain rounds below 16 * 40 * 17 * 2^-53, about 1e-12, and a wrong count or sign
    moves a mean by at least 0.01 |mu| with |mu| >= 0.1 here (asserted).  The exhaustive exact means without flips give the
    true fidelity: <psi| rho |psi> for a state, (tr R_U^T R_E + d) / (d^2 + d) for a process."""
    gates, classes, p, f, s, with_flips, without, fidelity = dense_case(kind, n)
    expt = experiment_from(kind, n, gates, s)
    got = dfe.simulate_dfe_batch(expt, p[None], 0, noise_class=classes, readout_flip=f)[0]
    plain = dfe.simulate_dfe_batch(expt, p[None], 0, noise_class=classes)[0]
    assert np.abs(with_flips).min() >= 0.1
    print(f"{kind} n = {n}: max |device - dense| = {np.abs(got - with_flips).max():.3e} with flips, "
          f"{np.abs(plain - without).max():.3e} without")
    assert np.abs(got - with_flips).max() <= 1e-10 and np.abs(plain - without).max() <= 1e-10
    d = 2.0 ** n
    if kind == "state":
        estimate = (d - 1) / d * plain.mean() + 1 / d
    else:
        p_mean = (d * d - 1) / (d * d) * plain.mean() + 1 / (d * d)
        estimate = (d * d * p_mean + d) / (d * d + d)
    print(f"{kind} n = {n}: fidelity {fidelity:.12f}, from the exhaustive exact means {estimate:.12f}")
    assert abs(estimate - fidelity) <= 1e-10


# ------------------------------------------------------------------ 6. counts against the restated stream
@functools.lru_cache(maxsize=None)
def ghz5():
    """n = 5, m = 31 exhaustive state settings of a GHZ circuit followed by 20 random gates, two noise classes."""
    gates = dc.ghz_circuit(5) + circuit(5, 20, seed=6)
    classes = np.array([0 if len(q) == 1 else 1 for _, q in gates], dtype=np.uint8)
    return dfe.generate_exhaustive_state_dfe_experiment(None, gates, list(range(5))), classes


def signs(expt):
    return 1.0 - 2.0 * expt.obs_sign.astype(np.float64)


@pytest.mark.parametrize("shots", [1, 3, 4, 70001])
@pytest.mark.parametrize("flips", [False, True])
def test_counts_equal_the_restated_stream(gpu, shots, flips):
    expt, classes = ghz5()
    rng = np.random.default_rng(shots)
    p = rng.uniform(0.0, 0.1, size=(2, 2))
    f = rng.uniform(0.0, 0.1, size=(2, 5)) if flips else None
    e, c, se, exact = dfe.simulate_dfe_batch(expt, p, shots, noise_class=classes, readout_flip=f, seed=2024, first_item=5,
                                             return_std_errs=True, return_exact=True)
    we, wc, wse, _ = synthetic.restate_dfe_counts(exact, signs(expt), shots, 2024, first_item=5)
    assert np.array_equal(e, we) and np.array_equal(c, wc) and np.array_equal(se, wse)
    assert np.array_equal(exact, dfe.simulate_dfe_batch(expt, p, 0, noise_class=classes, readout_flip=f))


def test_calibration_mode_has_a_stream_of_its_own(gpu):
    expt, classes = ghz5()
    p, f = np.full((2, 2), 0.03), np.full((2, 5), 0.04)
    kw = dict(noise_class=classes, readout_flip=f, seed=11, return_std_errs=True, return_exact=True)
    e, c, se, exact = dfe.simulate_dfe_batch(expt, p, 400, **kw)
    ce, cc_, cse, cexact = dfe.simulate_dfe_batch(expt, p, 400, calibrate=True, **kw)
    support = expt.obs_x | expt.obs_z
    weight = np.array([bin(int(v)).count("1") for v in support.tolist()])
    assert np.abs(cexact - 0.92 ** weight[None, :]).max() < 1e-14                 # the readout product alone, coefficient 1
    ones = np.ones(expt.m)
    we, _, wse, _ = synthetic.restate_dfe_counts(cexact, ones, 400, 11, key_tag=synthetic.DFE_CALIBRATION_KEY_TAG)
    assert np.array_equal(ce, we) and np.array_equal(cse, wse) and np.array_equal(cc_, c)
    assert not np.array_equal(ce, synthetic.restate_dfe_counts(cexact, ones, 400, 11)[0])


def test_both_sides_of_the_lane_wavefront_switch_give_the_same_bits(gpu):
    """m = 31: B = 4228 is 131068 units (a wavefront each), B = 4229 is 131099 (a lane each); the common items are equal bit
    for bit, and equal to the restated stream."""
    expt, classes = ghz5()
    rng = np.random.default_rng(8)
    p, f = rng.uniform(0.0, 0.1, size=(4229, 2)), rng.uniform(0.0, 0.1, size=(4229, 5))
    assert 4228 * expt.m < 131072 <= 4229 * expt.m
    kw = dict(noise_class=classes, seed=99, return_std_errs=True, return_exact=True)
    lane = dfe.simulate_dfe_batch(expt, p, 7, readout_flip=f, **kw)
    wave = dfe.simulate_dfe_batch(expt, p[:4228], 7, readout_flip=f[:4228], **kw)
    for a, b in zip(lane, wave):
        assert np.array_equal(a[:4228], b)
    we, _, wse, _ = synthetic.restate_dfe_counts(lane[3][4200:], signs(expt), 7, 99, first_item=4200)
    assert np.array_equal(lane[0][4200:], we) and np.array_equal(lane[2][4200:], wse)


def _tail_call(batch, shots):
    """the smallest experiment (one qubit, m = 1 exhaustive state setting, one noise class) with flips: the device's outputs and
    the restatement of items [lo, hi)"""
    gates = circuit(1, 6, seed=3)
    expt = dfe.generate_exhaustive_state_dfe_experiment(None, gates, [0])
    assert expt.m == 1
    rng = np.random.default_rng(17)
    p, f = rng.uniform(0.0, 0.1, size=(batch, 1)), rng.uniform(0.0, 0.3, size=(batch, 1))
    got = dfe.simulate_dfe_batch(expt, p, shots, noise_class=np.zeros(len(gates), dtype=np.uint8), readout_flip=f, seed=2024,
                                 first_item=5, return_std_errs=True, return_exact=True)
    return got, lambda lo, hi: synthetic.restate_dfe_counts(got[3][lo:hi], signs(expt), shots, 2024, first_item=5 + lo)


@pytest.mark.parametrize("shots", TAIL_SHOTS)
def test_tail_block_on_the_wavefront_split(gpu, shots):
    """who owns the last, partial Philox block (tomo_sim_cases.TAIL_SHOTS): 3 x 1 units, a wavefront each"""
    (e, c, se, _), restate = _tail_call(3, shots)
    we, wc, wse, _ = restate(0, 3)
    assert np.array_equal(e, we) and np.array_equal(c, wc) and np.array_equal(se, wse)


@pytest.mark.parametrize("shots", TAIL_SHOTS_LANE)
def test_tail_block_on_the_lane_split(gpu, shots):
    """... and 131072 x 1 units, a lane each: the first and the last items against the restatement"""
    (e, c, se, _), restate = _tail_call(131072, shots)
    for lo, hi in ((0, 200), (131072 - 200, 131072)):
        we, wc, wse, kp = restate(lo, hi)
        assert np.array_equal(e[lo:hi], we) and np.array_equal(c[lo:hi], wc) and np.array_equal(se[lo:hi], wse)
        assert len(np.unique(kp)) > 2                        # (counts that vary: the comparison is not of constants)


def test_a_later_call_repeats_the_items_of_an_earlier_one(gpu):
    expt, classes = ghz5()
    p = np.random.default_rng(9).uniform(0.0, 0.1, size=(4, 2))
    kw = dict(noise_class=classes, seed=5, return_std_errs=True)
    whole = dfe.simulate_dfe_batch(expt, p, 50, first_item=10, **kw)
    part = dfe.simulate_dfe_batch(expt, p[1:3], 50, first_item=11, **kw)
    for a, b in zip(whole, part):
        assert np.array_equal(a[1:3], b)
    assert not np.array_equal(whole[0][0], whole[0][1])


# ------------------------------------------------------------------ 7. Monte Carlo against exhaustive
@pytest.mark.parametrize("kind", ["state", "process"])
def test_monte_carlo_estimate_is_near_the_exhaustive_one(gpu, kind):
    """Exact means, n = 4, 200 terms, fixed seed: the Monte Carlo settings are uniform draws from the exhaustive ones, so the
    estimate is within 6 sqrt(v / 200) (d - 1) / d of the exhaustive one, v the population variance of the exhaustive means;
    (d - 1) / d is the slope of both estimators in the mean."""
    n, d = 4, 16.0
    gates = circuit(n, 30, seed=7)
    classes = np.array([0 if len(q) == 1 else 1 for _, q in gates], dtype=np.uint8)
    p = np.array([[0.02, 0.08]])
    gen = ((dfe.generate_exhaustive_process_dfe_experiment, dfe.generate_monte_carlo_process_dfe_experiment) if kind == "process"
           else (dfe.generate_exhaustive_state_dfe_experiment, dfe.generate_monte_carlo_state_dfe_experiment))
    full = dfe.simulate_dfe_batch(gen[0](None, gates, list(range(n))), p, 0, noise_class=classes)[0]
    some = dfe.simulate_dfe_batch(gen[1](None, gates, list(range(n)), n_terms=200, seed=31), p, 0, noise_class=classes)[0]
    v = full.var()
    assert v > 0 and some.shape == (200,)
    bound = 6 * np.sqrt(v / 200) * (d - 1) / d
    diff = abs(some.mean() - full.mean()) * (d - 1) / d
    print(f"{kind}: exhaustive mean {full.mean():.6f}, Monte Carlo {some.mean():.6f}, difference {diff:.3e} of a bound {bound:.3e}")
    assert diff <= bound


# ------------------------------------------------------------------ 8. poison and refusals
def test_poisoned_items_leave_their_neighbours_untouched(gpu):
    expt, classes = ghz5()
    rng = np.random.default_rng(12)
    p, f = rng.uniform(0.0, 0.1, size=(4, 2)), rng.uniform(0.0, 0.1, size=(4, 5))
    p[1, 1], f[2, 3] = np.nan, 1.5
    kw = dict(noise_class=classes, seed=3, return_std_errs=True, return_exact=True)
    e, c, se, exact, status = dfe.simulate_dfe_batch(expt, p, 90, readout_flip=f, return_status=True, **kw)
    assert status.tolist() == [0, 1, 1, 0]
    for b in (1, 2):
        assert np.isnan(e[b]).all() and np.isnan(se[b]).all() and np.isnan(exact[b]).all() and np.all(c[b] == 90.0)
    for b in (0, 3):
        alone = dfe.simulate_dfe_batch(expt, p[b:b + 1], 90, readout_flip=f[b:b + 1], first_item=b, **kw)
        for got, want in zip((e, c, se, exact), alone):
            assert np.array_equal(got[b], want[0])
    with pytest.raises(ValueError):
        dfe.simulate_dfe_batch(expt, p, 90, readout_flip=f, **kw)
    with pytest.raises(ValueError):
        dfe.simulate_and_estimate_dfe_batch(expt, p, 90, readout_flip=f, noise_class=classes, seed=3)


def test_every_bad_argument_of_the_c_abi_is_a_value_error(gpu):
    lib = _lib.lib()
    u64, u32, u8, i8 = C.c_uint64, C.c_uint32, C.c_uint8, C.c_int8
    P = _lib.ptr
    x, z, s = np.zeros(4, dtype=np.uint64), np.ones(4, dtype=np.uint64), np.zeros(4, dtype=np.uint8)
    xo, zo, so = x.copy(), z.copy(), s.copy()

    def word(op, q0, q1=0, extra=0):
        return np.array([op | (q0 << 8) | (q1 << 16) | extra], dtype=np.uint32)

    def conjugate(n, gates, G=None, M=4, x_in=x):
        return lib.fbx_clifford_conjugate(n, len(gates) if G is None else G, P(gates, u32), 0, M, P(x_in, u64), P(z, u64), P(s, u8),
                                          P(xo, u64), P(zo, u64), P(so, u8))
    good = word(0, 0)
    assert conjugate(2, good) == _lib.FBX_OK
    bad = [conjugate(2, word(0, 2)), conjugate(2, word(12, 0, 2)), conjugate(2, word(12, 1, 1)), conjugate(2, word(15, 0)),
           conjugate(2, word(0, 0, 0, 1 << 24)), conjugate(0, good), conjugate(65, good), conjugate(2, good, G=-1),
           conjugate(2, good, M=-1), conjugate(2, good, x_in=None), lib.fbx_clifford_conjugate(2, 1, None, 0, 4, P(x, u64), P(z, u64),
                                                                                             P(s, u8), P(xo, u64), P(zo, u64), P(so, u8))]
    a = {k: np.zeros(3, dtype=np.uint64) for k in "abcde"}
    sg = np.zeros(3, dtype=np.uint8)

    def settings(n, kind, n_terms, m, gates=good, first=a["a"]):
        return lib.fbx_dfe_settings(n, kind, n_terms, 1, len(gates), P(gates, u32), m, P(first, u64), P(a["b"], u64), P(a["c"], u64),
                                    P(a["d"], u64), P(a["e"], u64), P(sg, u8))
    assert settings(2, _lib.KIND_STATE, 0, 3) == _lib.FBX_OK
    bad += [settings(2, _lib.KIND_STATE, 0, 2), settings(1, _lib.KIND_PROCESS, 0, 3), settings(2, _lib.KIND_STATE, 3, 2),
            settings(2, 7, 0, 3), settings(2, _lib.KIND_STATE, -1, 3), settings(2, _lib.KIND_STATE, 0, 3, gates=word(13, 0, 5)),
            settings(2, _lib.KIND_STATE, 0, 3, first=None), settings(40, _lib.KIND_STATE, 0, 3)]
    ones, none = np.full(3, 3, dtype=np.uint64), np.zeros(3, dtype=np.uint64)      # in-state labels X X, and an in_z without bits
    sigma, touches = np.zeros(3, dtype=np.int8), np.zeros((3, 2), dtype=np.uint32)

    def propagate(K=2, classes=None, in_x=ones, gates=good, m=3, out=sigma):
        return lib.fbx_dfe_propagate(2, len(gates), P(gates, u32), P(classes, u8), K, m, P(in_x, u64), P(none, u64), P(a["c"], u64),
                                     P(a["d"], u64), P(a["e"], u64), P(sg, u8), P(out, i8), P(touches, u32))
    assert propagate() == _lib.FBX_OK and propagate(classes=np.array([255], dtype=np.uint8)) == _lib.FBX_OK
    bad += [propagate(classes=np.array([2], dtype=np.uint8)), propagate(K=0), propagate(K=17),
            propagate(in_x=np.array([3, 1, 3], dtype=np.uint64)), propagate(gates=word(3, 9)), propagate(m=-1), propagate(out=None)]
    out = np.zeros((2, 3))
    p = np.zeros((2, 2))

    def simulate(shots=5, expect=out, exact=None, B=2, m=3, K=2, sig=sigma, first_item=0):
        return lib.fbx_dfe_simulate(2, m, K, P(sig, i8), P(touches, u32), P(a["d"], u64), P(a["e"], u64), P(sg, u8), B, _lib.dptr(p),
                                    None, 0, shots, 1, first_item, _lib.dptr(expect), None, None, _lib.dptr(exact), None)
    assert simulate() == _lib.FBX_OK and simulate(shots=0, expect=None, exact=out) == _lib.FBX_OK
    bad += [simulate(shots=2 ** 32), simulate(shots=0), simulate(shots=-1), simulate(expect=None), simulate(B=-1), simulate(m=-1),
            simulate(K=17), simulate(sig=None), simulate(first_item=-1)]
    fid, err = np.zeros(2), np.zeros(2)

    def chain(shots=5, kind=_lib.KIND_STATE, fidelity=fid, m=3):
        return lib.fbx_dfe_simulate_fidelity(2, m, 2, P(sigma, i8), P(touches, u32), P(a["d"], u64), P(a["e"], u64), P(sg, u8), 2,
                                             _lib.dptr(p), None, shots, 1, 0, kind, 0, _lib.dptr(fidelity), _lib.dptr(err), None)
    assert chain() == _lib.FBX_OK
    bad += [chain(shots=0), chain(shots=2 ** 32), chain(kind=5), chain(fidelity=None), chain(m=0)]
    for i, rc in enumerate(bad):
        assert rc == _lib.FBX_ERR_BAD_ARG, (i, rc)
        with pytest.raises(ValueError):
            _lib.check(rc)


# ------------------------------------------------------------------ 9. the resident chain
@pytest.mark.parametrize("calibrate", [False, True])
@pytest.mark.parametrize("kind", ["state", "process"])
def test_the_resident_chain_equals_the_composition_through_the_host(gpu, kind, calibrate):
    """To the last bit: the chain runs the kernels of the separate calls -- the same simulation kernel, the same squaring
    (one product, rounded once, as numpy's), the calibrate kernel, and dfe_item, the reduction fbx_dfe_estimate itself is
    made of (fbx_sim_shared.hpp) -- on the same values in the same order."""
    if kind == "state":
        expt, classes = ghz5()
    else:
        gates = circuit(2, 20, seed=8)
        classes = np.array([0 if len(q) == 1 else 1 for _, q in gates], dtype=np.uint8)
        expt = dfe.generate_exhaustive_process_dfe_experiment(None, gates, [0, 1])
    rng = np.random.default_rng(13)
    B = 3
    p, f = rng.uniform(0.0, 0.1, size=(B, 2)), rng.uniform(0.0, 0.1, size=(B, expt.n_qubits))
    kw = dict(noise_class=classes, readout_flip=f, seed=21, first_item=2)
    fid, err = dfe.simulate_and_estimate_dfe_batch(expt, p, 500, calibrate=calibrate, **kw)
    e, _, se = dfe.simulate_dfe_batch(expt, p, 500, return_std_errs=True, **kw)
    if calibrate:
        ce, _, cse = dfe.simulate_dfe_batch(expt, p, 500, calibrate=True, return_std_errs=True, **kw)
        pairs = [calibrate_expectations_batch(e[b], se[b], ce[b], cse[b] ** 2) for b in range(B)]
        e, se = np.vstack([a for a, _ in pairs]), np.vstack([b for _, b in pairs])
    want_fid, want_err = dfe.estimate_dfe_batch(e, se, expt.n_qubits, kind)
    assert np.array_equal(fid, want_fid) and np.array_equal(err, want_err)
    assert np.all(np.isfinite(fid)) and np.all(err > 0)


def test_the_resident_chain_at_40_qubits_against_the_formula(gpu):
    """n = 40 is above the 30 qubits of fbx_dfe_estimate, so the chain is checked against estimate_dfe's formula in numpy.  The
    two sum m = 150 terms in different orders: each sum is within (m - 1) 2^-53 sum|e| of the true one, and the formula adds
    a few roundings -- 4 ulp of the result are allowed for them."""
    n, m = 40, 150
    gates = dc.ghz_circuit(n) + circuit(n, 60, seed=9)
    classes = np.array([0 if len(q) == 1 else 1 for _, q in gates], dtype=np.uint8)
    expt = dfe.generate_monte_carlo_state_dfe_experiment(None, gates, list(range(n)), n_terms=m, seed=17)
    p = np.array([[0.001, 0.004], [0.0, 0.0]])
    kw = dict(noise_class=classes, seed=23)
    fid, err = dfe.simulate_and_estimate_dfe_batch(expt, p, 300, **kw)
    e, _, se = dfe.simulate_dfe_batch(expt, p, 300, return_std_errs=True, **kw)
    d = 2.0 ** n
    want_fid = (d - 1) / d * e.mean(axis=1) + 1.0 / d
    want_err = np.sqrt((d - 1) ** 2 / d ** 2 * (se ** 2).sum(axis=1) / m ** 2)
    tol_fid = 2 * (m - 1) * 2.0 ** -53 * np.abs(e).sum(axis=1) / m + 4 * np.spacing(want_fid)
    tol_err = 2 * (m - 1) * 2.0 ** -53 * want_err + 4 * np.spacing(want_err)
    assert np.all(np.abs(fid - want_fid) <= tol_fid) and np.all(np.abs(err - want_err) <= tol_err)
    assert fid[1] == 1.0 and err[1] == 0.0 and 0.5 < fid[0] < 1.0
    with pytest.raises(ValueError):
        dfe.estimate_dfe_batch(e, se, n, "state")
