"""fbx.robust_phase_estimation on the host (no GPU): the experiment-design helpers against the reference's tables in
tests/golden/rpe_cases.npz (tests/golden/make_rpe_goldens.py), the numpy restatement of tests/rpe_cases.py pinned to the reference's
phases, bloch data and stopping depths (so that GPU tests on other shapes do not compare the device with itself), the selection
logic of robust_phase_estimate against the restatement, argument errors, and the loud failure without a device."""
import os

import numpy as np
import pytest

import rpe_cases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rpe_cases.npz")


@pytest.fixture(scope="module")
def gold():
    assert os.path.getsize(GOLDEN) <= 256 * 1024
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_module_offers_the_reference_names():
    from fbx import robust_phase_estimation as rpe
    for name in ("get_additive_error_factor", "num_trials", "_p_max", "_xci", "get_variance_upper_bound",
                 "bloch_rotation_to_eigenvectors", "get_change_of_basis_from_eigvecs", "estimate_phase_from_moments",
                 "robust_phase_estimate", "estimate_phase_from_moments_batch", "robust_phase_estimate_from_shots_batch",
                 "phase_variance_batch"):
        assert callable(getattr(rpe, name)), name
    for name in ("generate_rpe_experiments", "acquire_rpe_data", "do_rpe", "change_of_basis_matrix_to_quil", "plot_rpe_iterations"):
        assert not hasattr(rpe, name), name


def test_host_tables_match_the_reference(gold):
    from fbx import robust_phase_estimation as rpe
    for (d, m, f, a), want in zip(gold["num_trials_args"], gold["num_trials_out"]):
        assert rpe.num_trials(int(d), int(m), f, a if a else None) == int(want), (d, m, f, a)
    for (n, f, a), want in zip(gold["variance_args"], gold["variance_out"]):
        assert rpe.get_variance_upper_bound(int(n), f, a if a else None) == want, (n, f, a)
    for (m, a), want in zip(gold["factor_args"], gold["factor_out"]):
        assert rpe.get_additive_error_factor(m, a) == want, (m, a)
    for m, want in zip(gold["p_max_args"], gold["p_max_out"]):
        assert rpe._p_max(int(m)) == want
    for h, want in enumerate(gold["xci_out"]):
        assert rpe._xci(h) == want


def test_eigenvector_helpers_match_the_reference(gold):
    from fbx import robust_phase_estimation as rpe
    for (t, p), vecs, cob in zip(gold["eigvec_angles"], gold["eigvecs"], gold["change_of_basis"]):
        e1, e2 = rpe.bloch_rotation_to_eigenvectors(t, p)
        assert e1.shape == (2, 1) and e2.shape == (2, 1)
        assert np.array_equal(np.hstack([e1, e2]), vecs)
        assert np.array_equal(rpe.get_change_of_basis_from_eigvecs((e1, e2)), cob)
        assert np.array_equal(rpe.get_change_of_basis_from_eigvecs([e1[:, 0], e2.T]), cob)          # 1-d and row vectors
    q = gold["eigvecs_4"]
    assert np.array_equal(rpe.get_change_of_basis_from_eigvecs([q[:, i] for i in range(4)]), gold["change_of_basis_4"])
    with pytest.raises(AssertionError):
        rpe.get_change_of_basis_from_eigvecs([q[:, i] for i in range(3)])


@pytest.mark.parametrize("K", rc.GOLDEN_DEPTHS)
def test_restatement_is_pinned_to_the_reference(gold, K):
    """tests/rpe_cases.py::estimate against the reference's estimate_phase_from_moments: the same libm, so ==; and every stored set
    keeps the margins the generator promised"""
    x, y, xe, ye = (gold[f"k{K}_{n}"] for n in ("x", "y", "x_err", "y_err"))
    assert x.shape == (50, K)
    phase, depth, bloch, margins = rc.estimate_batch(x, y, xe, ye)
    assert all(rc.safe(m) for m in margins)
    assert np.array_equal(depth, gold[f"k{K}_depth_reached"])
    assert np.array_equal(phase, gold[f"k{K}_phase"])
    assert np.array_equal(bloch, gold[f"k{K}_bloch"], equal_nan=True)
    assert rc.circ_dist(rc.estimate_vec(x, y, xe, ye), phase).max() <= 1e-12
    assert ((depth < K).sum() >= 5) and (depth == K).sum() >= 5              # both kinds of item are present
    full = depth == K                                                        # an uncut estimate lands near the phase it came from
    assert np.all(rc.circ_dist(phase[full], gold[f"k{K}_true_phase"][full]) < 8.0 / 2 ** K + 0.5)


def test_restatement_exact_cases():
    """what the GPU test asks of the device with ==, asked of the restatement first"""
    K = 7
    one, zero, err = np.ones(K), np.zeros(K), np.full(K, 0.01)
    assert rc.estimate(one, zero, err, err)[:2] == (0.0, K)
    xs = np.array([-1.0] + [1.0] * (K - 1))                                 # cos(2^j pi)
    for y0 in (0.0, -0.0):
        assert rc.estimate(xs, np.full(K, y0), err, err)[:2] == (np.pi, K)
    assert rc.estimate([0.0], [0.0], [1.0], [1.0])[:2] == (0.0, 0)
    r_std = np.hypot(0.3, 0.4)                                              # 0.5 exactly: r == r_std does not stop
    assert rc.estimate([0.5], [0.0], [0.3], [0.4])[1] == 1 and r_std == 0.5
    assert rc.estimate([np.nextafter(0.5, 0)], [0.0], [0.3], [0.4])[1] == 0


@pytest.mark.parametrize("name", rc.RESULT_STRUCTURES)
def test_selection_logic_matches_the_reference(gold, name):
    """robust_phase_estimate's host half: the sequences it selects, run through the restatement, give the reference's phases in
    the reference's order (the launch itself is the GPU test's)"""
    from fbx import robust_phase_estimation as rpe
    results, qubits = rc.fbx_results(gold, name)
    inputs = rpe._phase_inputs(results, qubits)
    want = gold[f"{name}_phases"]
    assert len(inputs) == len(want) == {"all_eigvecs": 4, "fixed_one": 1, "fixed_zero": 1}[name]
    for item, w in zip(inputs, want):
        phase, used, _, margins = rc.estimate(*item)
        assert rc.safe(margins) and phase == w


def test_single_qubit_selection():
    from fbx import observable_estimation as oe, robust_phase_estimation as rpe
    state = oe.TensorProductState((oe._OneQState("X", 0, 3),))
    results = [[oe.ExperimentResult(oe.ExperimentSetting(state, oe.PauliTerm({3: p})), e, 100, std_err=s)
                for p, e, s in (("X", 0.5 + d, 0.1), ("Y", 0.25 - d, 0.2))] for d in (0.0, 0.125)]
    assert rpe._phase_inputs(results, [3]) == [([0.5, 0.625], [0.25, 0.125], [0.1, 0.1], [0.2, 0.2])]


def test_argument_errors_come_before_any_device_call(monkeypatch):
    from fbx import _lib, robust_phase_estimation as rpe

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    a = np.zeros((3, 4))
    with pytest.raises(ValueError):
        rpe.estimate_phase_from_moments_batch(a, a, a, a[:, :3])
    with pytest.raises(ValueError):
        rpe.estimate_phase_from_moments_batch(a[0], a[0], a[0], a[0])
    with pytest.raises(ValueError):
        rpe.estimate_phase_from_moments_batch(a, a, a, a, xz=a)
    with pytest.raises(ValueError):
        rpe.estimate_phase_from_moments_batch(a, a, a, a, post_select=2)
    with pytest.raises(ValueError):
        rpe.estimate_phase_from_moments_batch(a[:, :0], a[:, :0], a[:, :0], a[:, :0])
    bits = np.zeros((2, 3, 10, 2), dtype=np.uint8)
    with pytest.raises(ValueError):
        rpe.robust_phase_estimate_from_shots_batch(bits, bits[:1], 0)
    with pytest.raises(ValueError):
        rpe.robust_phase_estimate_from_shots_batch(bits, bits, 2)
    with pytest.raises(ValueError):
        rpe.robust_phase_estimate_from_shots_batch(bits, bits, 1, zcol=1)
    with pytest.raises(ValueError):
        rpe.robust_phase_estimate_from_shots_batch(bits + 2, bits, 0)
    with pytest.raises(ValueError):
        rpe.robust_phase_estimate_from_shots_batch(bits, bits, 0, zcol=1, post_select=3)
    with pytest.raises(ValueError):
        rpe.robust_phase_estimate_from_shots_batch(np.zeros((1, 1, 4, 9), dtype=np.uint8), np.zeros((1, 1, 4, 9), dtype=np.uint8), 0)
    with pytest.raises(ValueError):
        rpe.phase_variance_batch(a, a, a, a, 500, n_resamples=0)
    with pytest.raises(ValueError):
        rpe.phase_variance_batch(a, a, a, a, 0, n_resamples=10)
    with pytest.raises(ValueError):
        rpe.circular_stats(np.zeros(5))


def test_c_abi_argument_errors():
    """FBX_REQUIRE in the library itself, before a device is looked for; more than 62 depths is unsupported, not a bad argument"""
    import ctypes as C
    import fbx
    from fbx import _lib, robust_phase_estimation as rpe
    lib = _lib.lib()
    a, out = np.zeros(4), np.zeros(4)
    p, o = _lib.dptr(a), _lib.dptr(out)
    assert lib.fbx_rpe_phase(1, 0, p, p, p, p, 0, None, None, None, None, 0, o, None, None) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_rpe_phase(-1, 2, p, p, p, p, 0, None, None, None, None, 0, o, None, None) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_rpe_phase(1, 2, p, p, p, p, 0, None, None, None, None, 0, None, None, None) == _lib.FBX_ERR_BAD_ARG
    assert b"no output" in lib.fbx_last_error()
    assert lib.fbx_rpe_phase(1, 2, p, p, p, p, 0, p, None, None, None, 0, o, None, None) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_rpe_phase(1, 2, p, p, p, p, 0, None, None, None, None, 2, o, None, None) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_rpe_phase(1, 2, None, p, p, p, 0, None, None, None, None, 0, o, None, None) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_rpe_phase(1, 63, p, p, p, p, 0, None, None, None, None, 0, o, None, None) == _lib.FBX_ERR_UNSUPPORTED
    assert b"62" in lib.fbx_last_error()
    bits = np.zeros(64, dtype=np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
    for args in ((0, 1, 1, 4, 0, -1, 0), (9, 1, 1, 4, 0, -1, 0), (2, 1, 1, 0, 0, -1, 0), (2, 1, 1, 4, 2, -1, 0), (2, 1, 1, 4, 0, 0, 0),
                 (2, 1, 1, 4, 0, 2, 0), (2, 1, 1, 4, 0, 1, 2), (2, 1, 0, 4, 0, -1, 0)):
        n, B, K, shots, col, zcol, ps = args
        assert lib.fbx_rpe_from_shots(n, B, K, shots, bits, bits, col, zcol, ps, o, None, None, None) == _lib.FBX_ERR_BAD_ARG, args
    assert lib.fbx_rpe_from_shots(2, 1, 1, 4, bits, bits, 0, -1, 0, None, None, None, None) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_rpe_from_shots(2, 1, 63, 4, bits, bits, 0, -1, 0, o, None, None, None) == _lib.FBX_ERR_UNSUPPORTED
    assert lib.fbx_circular_stats(-1, 1, p, o, None, None) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_circular_stats(2, 2, None, o, None, None) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_circular_stats(2, 2, p, None, None, None) == _lib.FBX_ERR_BAD_ARG
    big = np.zeros((1, 63))
    with pytest.raises(fbx.FbxError) as ei:
        rpe.estimate_phase_from_moments_batch(big, big, big, big)
    assert ei.value.code == _lib.FBX_ERR_UNSUPPORTED


def test_no_device_fails_loudly_not_silently(gold):
    """Without a GPU the estimates are an error (FBX_ERR_NO_DEVICE), never a host computation; with one they run."""
    import fbx
    from fbx import _lib, robust_phase_estimation as rpe
    x, y, xe, ye = (gold[f"k5_{n}"][:3] for n in ("x", "y", "x_err", "y_err"))
    bits = np.zeros((2, 3, 20, 2), dtype=np.uint8)
    results, qubits = rc.fbx_results(gold, "fixed_one")
    calls = (lambda: rpe.estimate_phase_from_moments_batch(x, y, xe, ye),
             lambda: rpe.estimate_phase_from_moments(list(x[0]), list(y[0]), list(xe[0]), list(ye[0])),
             lambda: rpe.robust_phase_estimate(results, qubits),
             lambda: rpe.robust_phase_estimate_from_shots_batch(bits, bits, 0, zcol=1),
             lambda: rpe.phase_variance_batch(x, y, xe, ye, 500, n_resamples=4, seed=1),
             lambda: rpe.circular_stats(np.zeros((4, 2))))
    for call in calls:
        if fbx.device_count() > 0:
            call()
        else:
            with pytest.raises(fbx.FbxError) as ei:
                call()
            assert ei.value.code == _lib.FBX_ERR_NO_DEVICE
