"""The host half of simulated tomography: ``synthetic.restate_tomography_counts`` against the stream of ``fbx_tomo_simulate``
(include/fbx.h) stated shot by shot on the oracle's Philox (tests/tomo_sim_cases.py), its corners, the distribution of its counts,
and the argument checks of the wrappers, which refuse before they touch the library."""
import numpy as np
import pytest

import tomo_sim_cases as tc


def test_restatement_equals_the_shot_by_shot_loop():
    from fbx import synthetic
    rng = np.random.default_rng(3)
    coefs = np.array([1.0, -1.0, 0.5, -2.0, 1.0, 0.5, -1.0])
    mu = rng.uniform(-1.0, 1.0, size=(2, 7))
    shots, first = 203, 3                                  # 50 blocks and a tail of three shots
    e, c, s, kp = synthetic.restate_tomography_counts(mu * coefs, coefs, shots, tc.SEED, first)
    want = np.array([[tc.count_loop((mu[b, k] * coefs[k]) / coefs[k], shots, tc.SEED, first + b, k) for k in range(7)]
                     for b in range(2)])
    assert kp.dtype == np.int64 and np.array_equal(kp, want)
    we, ws = tc.moments(want, shots, coefs[None, :])
    assert np.array_equal(e, we) and np.array_equal(s, ws)
    assert np.array_equal(c, np.full((2, 7), float(shots)))
    assert 0 < kp.min() and kp.max() < shots               # (the case is not degenerate)
    # a call from first + 1 repeats item 1, and another seed or the untagged key gives other counts
    assert np.array_equal(synthetic.restate_tomography_counts(mu[1:] * coefs, coefs, shots, tc.SEED, first + 1)[3], kp[1:])
    assert not np.array_equal(synthetic.restate_tomography_counts(mu * coefs, coefs, shots, tc.SEED + 1, first)[3], kp)
    assert not np.array_equal(synthetic.restate_tomography_counts(mu * coefs, coefs, shots, tc.SEED ^ tc.KEY_TAG, first)[3], kp)


@pytest.mark.parametrize("shots", (1, 3, 4, 4099))
def test_restatement_corners(shots):
    from fbx import synthetic
    mu = np.array([[1.0, -1.0, 0.0, 1.0 + 2.0 ** -40, -1.5]])
    coefs = np.array([1.0, 1.0, 1.0, 1.0, 1.0])
    e, c, s, kp = synthetic.restate_tomography_counts(mu, coefs, shots, tc.SEED)
    assert kp[0, 0] == shots and kp[0, 1] == 0            # t = 2^32: every word is below it; t = 0: none is
    assert kp[0, 3] == shots and kp[0, 4] == 0            # clamped, not refused
    assert e[0, 0] == 1.0 and e[0, 1] == -1.0 and s[0, 0] == 0.0 and s[0, 1] == 0.0
    # mu = 0: t = 2^31, the shot counts +1 iff the top bit of its word is clear
    assert kp[0, 2] == tc.count_loop(0.0, shots, tc.SEED, 0, 2)
    key = np.array([(tc.SEED & 0xFFFFFFFF) ^ tc.KEY_TAG, tc.SEED >> 32], dtype=np.uint32)
    words = np.concatenate([tc.philox4x32_10(np.array([0, 0, 2, j], dtype=np.uint32), key) for j in range((shots + 3) // 4)])
    assert kp[0, 2] == int((words[:shots] >> 31 == 0).sum())
    assert np.all(c == shots)


def test_restatement_counts_are_binomial():
    from fbx import synthetic
    m, shots = 2000, 4099
    mu = np.linspace(-0.999, 0.999, m)[None, :]
    kp = synthetic.restate_tomography_counts(mu, np.ones(m), shots, tc.SEED, tc.FIRST)[3]
    q = np.floor((0.5 * mu + 0.5) * 2.0 ** 32) * 2.0 ** -32   # the probability the stream realises
    z = tc.z_score(kp, q, shots)
    print(f"z = {z:.3f} over {m} settings of {shots} shots")
    assert abs(z) < 6.0


def test_restatement_refuses_bad_arguments():
    from fbx import synthetic
    for kw in (dict(shots=0), dict(shots=2 ** 32), dict(first_item=-1), dict(coefs=np.array([1.0, 0.0]))):
        args = dict(exact=np.zeros((1, 2)), coefs=np.ones(2), shots=5, seed=1, first_item=0)
        args.update(kw)
        with pytest.raises(ValueError):
            synthetic.restate_tomography_counts(**args)


def test_existing_synthetic_streams_are_unchanged():
    from fbx import synthetic
    e, c = synthetic.sample_expectations(np.array([[0.25, -0.5, 0.0]]), 100)
    rs = np.random.RandomState(2000)
    assert np.array_equal(e[0], 2 * rs.binomial(100, np.array([0.625, 0.25, 0.5])) / 100 - 1) and np.all(c == 100.0)


# ------------------------------------------------------------------------------------------------ the wrappers refuse first
@pytest.fixture()
def no_library(monkeypatch):
    """any touch of the library fails the test"""
    from fbx import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "check", boom)


def test_process_wrapper_refuses_bad_arguments(no_library):
    from fbx import tomography as t
    from fbx.design import process_design, state_design
    des = process_design(1)
    ptm = np.eye(4)[None]
    with pytest.raises(ValueError, match="rep"):
        t.simulate_process_tomography_batch(des, ptm, 10, rep="chi")
    with pytest.raises(ValueError, match="process design"):
        t.simulate_process_tomography_batch(state_design(1), ptm, 10)
    for bad, rep in ((np.eye(3)[None], "pauli_liouville"), (np.eye(4)[None] * 1j, "pauli_liouville"), (np.eye(4)[None], "unitary"),
                     (np.eye(3)[None], "kraus"), (np.eye(2)[None], "choi"), (np.zeros((2, 0, 2, 2)), "kraus")):
        with pytest.raises(ValueError):
            t.simulate_process_tomography_batch(des, bad, 10, rep=rep)
    for kw in (dict(shots=0), dict(shots=2 ** 32), dict(shots=10, first_item=-1), dict(shots=10, readout_flip=np.zeros((2, 2))),
               dict(shots=10, readout_flip=np.zeros((3, 1, 2)))):
        with pytest.raises(ValueError):
            t.simulate_process_tomography_batch(des, ptm, **kw)
    with pytest.raises(ValueError, match="estimator"):
        t.simulate_and_estimate_process_batch(des, ptm, 10, estimator="mle")
    with pytest.raises(ValueError, match="does not take"):
        t.simulate_and_estimate_process_batch(des, ptm, 10, estimator="linear_inv", max_iters=3)
    with pytest.raises(ValueError, match="rep"):
        t.simulate_and_estimate_process_batch(des, ptm, 10, rep="chi")


def test_state_wrapper_and_results_refuse_bad_arguments(no_library):
    from fbx import tomography as t
    from fbx.design import process_design, state_design
    des = state_design(2)
    with pytest.raises(ValueError, match="state design"):
        t.simulate_state_tomography_batch(process_design(1), np.eye(2)[None] / 2, 10)
    with pytest.raises(ValueError, match="states must be"):
        t.simulate_state_tomography_batch(des, np.eye(2)[None] / 2, 10)
    with pytest.raises(ValueError):
        t.simulate_state_tomography_batch(des, np.eye(4)[None] / 4, 0)
    with pytest.raises(ValueError):
        t.simulate_state_tomography_batch(des, np.eye(4)[None] / 4, 10, readout_flip=np.zeros((1, 2)))
    with pytest.raises(ValueError, match="kind"):
        t.simulate_tomography_results([0], "channel", np.eye(4), 10)
    with pytest.raises(ValueError, match="does not take"):
        t.simulate_tomography_results([0], "process", np.eye(4), 10, first_item=2)
    with pytest.raises(ValueError, match="Unknown basis"):
        t.simulate_tomography_results([0], "process", np.eye(4), 10, in_basis="bell")
