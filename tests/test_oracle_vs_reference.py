"""The CPU oracle and the shim against the reference itself: tests/golden/oracle_cases.npz holds the reference's own answers
on exactly the inputs presented here (make_goldens.py --oracle-cases, which runs the reference)."""
import os
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ref():
    with np.load(os.path.join(HERE, "golden", "oracle_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def _settings(texts):
    from fbx import observable_estimation as oe
    return [oe.ExperimentSetting.from_str(str(s)) for s in texts]


def _results(settings, e, c):
    from fbx import observable_estimation as oe
    return [oe.ExperimentResult(setting=s, expectation=float(e[k]), std_err=0.0, total_counts=int(c[k]))
            for k, s in enumerate(settings)]


def test_flatten_results_matches_canonical_designs(ref):
    from fbx_oracle import design as od
    for n, qubits in ((1, [3]), (2, [0, 1]), (2, [5, 2])):
        for basis in ("pauli", "sic"):
            settings = _settings(ref[f"process_settings_{'_'.join(map(str, qubits))}_{basis}"])
            res = _results(settings, np.zeros(len(settings)), np.ones(len(settings)))
            d, _, _ = od.flatten_results(res, qubits, "process")
            c = od.process_design(n, basis)
            assert (d.in_labels == c.in_labels).all() and (d.paulis == c.paulis).all()


def test_design_matrix_and_counts_vector(ref):
    from fbx_oracle import design as od, estimators as oe
    rs = np.random.RandomState(0)
    for n, basis in ((1, "pauli"), (2, "sic")):
        m = len(ref[f"process_settings_{'_'.join(map(str, range(n)))}_{basis}"])
        e = rs.uniform(-1, 1, m); c = rs.randint(100, 1000, m)
        key = f"extract_{n}q_{basis}"
        assert np.array_equal(e, ref[key + "_e"]) and np.array_equal(c, ref[key + "_c"])
        d = od.process_design(n, basis)
        assert np.array_equal(ref[key + "_A"], oe.design_matrix_A(d))
        assert np.array_equal(ref[key + "_n"], oe.counts_vector(e, c))


def test_pgdb_bitwise_equal_incl_general_designs(ref):
    from fbx_oracle import design as od, estimators as oe
    from fbx import synthetic
    qubits = [0]
    _, _, e, c = synthetic.process_batch(1, "sic", 2, first_item=40)
    assert np.array_equal(e, ref["pgdb_e"]) and np.array_equal(c, ref["pgdb_c"])
    settings = _settings(ref["process_settings_0_sic"])
    for b in range(2):
        res = _results(settings, e[b], c[b])
        d, ee, cc = od.flatten_results(res, qubits, "process")
        assert np.array_equal(ref[f"pgdb_tp_{b}"], oe.pgdb_process_estimate(d, ee, cc))
        perm = np.random.RandomState(b).permutation(len(res))
        res2 = [res[i] for i in perm] + [res[1]]
        d, ee, cc = od.flatten_results(res2, qubits, "process")
        assert np.array_equal(ref[f"pgdb_tni_{b}"], oe.pgdb_process_estimate(d, ee, cc, trace_preserving=False))


def test_state_estimators_bitwise(ref):
    from fbx_oracle import design as od, estimators as oe
    from fbx import synthetic
    qubits = [0, 1]
    _, _, e, c = synthetic.state_batch(2, 2, first_item=7, mixed=0.05)
    assert np.array_equal(e, ref["state_e"]) and np.array_equal(c, ref["state_c"])
    settings = _settings(ref["state_settings_0_1"])
    for b in range(2):
        res = _results(settings, e[b], c[b])
        d, ee, cc = od.flatten_results(res, qubits, "state")
        assert np.allclose(ref[f"state_linv_{b}"], oe.linear_inv_state_estimate(d, ee), atol=1e-15)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert np.array_equal(ref[f"state_mle30_{b}"], oe.iterative_mle_state_estimate(d, ee, cc, maxiter=30))
        rho = ref[f"state_rho_{b}"]                                    # both sides evaluated on the same estimate
        assert np.array_equal(ref[f"state_R_{b}"], oe.R_operator(rho, d, ee))
        assert float(ref[f"state_loglik_{b}"]) == oe.state_log_likelihood(rho, d, ee, cc)


def test_operator_tools_random(ref):
    from fbx_oracle import superops as so, measures as om
    rs = np.random.RandomState(5)
    for d in (2, 4):
        D = d * d
        x = rs.randn(D, D) + 1j * rs.randn(D, D)
        assert np.array_equal(x, ref[f"ot{d}_x"])
        h = x + x.conj().T
        for name in ("choi2superop", "superop2choi", "choi2pauli_liouville", "pauli_liouville2choi",
                     "superop2pauli_liouville", "pauli_liouville2superop", "chi2choi", "chi2pauli_liouville",
                     "chi2superop", "proj_choi_to_trace_preserving", "proj_choi_to_trace_non_increasing",
                     "proj_choi_to_completely_positive"):
            assert np.allclose(ref[f"ot{d}_{name}"], getattr(so, name)(x), atol=1e-13), name
        for name in ("choi2chi", "superop2chi", "pauli_liouville2chi", "proj_choi_to_physical", "proj_choi_to_unitary"):
            arg = ref[f"ot{d}_arg_{name}"]                          # h, or the reference's own transform of it
            if name == "choi2chi":
                assert np.array_equal(arg, h)
            assert np.allclose(ref[f"ot{d}_{name}"], getattr(so, name)(arg), atol=1e-12), name
        assert np.array_equal(ref[f"ot{d}_computational2pauli_basis_matrix"], so.computational2pauli_basis_matrix(d))
        g = rs.randn(d, d) + 1j * rs.randn(d, d)
        rho = g @ g.conj().T; rho /= np.trace(rho)
        g = rs.randn(d, d) + 1j * rs.randn(d, d)
        sig = g @ g.conj().T; sig /= np.trace(sig)
        assert np.array_equal(rho, ref[f"dm{d}_rho"]) and np.array_equal(sig, ref[f"dm{d}_sigma"])
        for name in ("fidelity", "trace_distance", "bures_distance", "bures_angle", "hilbert_schmidt_ip"):
            assert np.isclose(ref[f"dm{d}_{name}"], getattr(om, name)(rho, sig), atol=1e-13), name
        assert np.isclose(ref[f"dm{d}_purity"], om.purity(rho))
        assert np.allclose(ref[f"dm{d}_watrous_bounds"], om.watrous_bounds(h))


def test_shots_to_obs_moments(ref):
    from fbx_oracle import acquisition as oa
    rs = np.random.RandomState(9)
    qubits = [3, 0, 5]
    bits = (rs.uniform(size=(500, 3)) < 0.3).astype(int)
    assert np.array_equal(bits, ref["shots_bits"])
    for k, (ops, coef) in enumerate((({3: "X", 5: "Z"}, 1.0), ({0: "Y"}, -0.7), ({}, 2.0), ({3: "Z", 0: "Z", 5: "Z"}, 1.0))):
        mask = [1 if q in ops else 0 for q in qubits]
        for prior in (False, True):
            got = oa.shots_to_obs_moments(bits, mask, coef, prior)
            assert np.allclose(ref[f"shots_{k}_{int(prior)}"], got, rtol=0, atol=1e-15)
    assert float(ref["ratio_variance"]) == oa.ratio_variance(1.0, 0.1, 2.0, 0.05) == 0.028125


def test_setting_generators_and_text_forms_match_the_reference(ref):
    """The shim's settings come from its design tables and its record classes are its own code; what must
    agree with the reference is the ORDER of the settings and every text form (the interchange schema)."""
    from fbx import tomography as T, observable_estimation as oe
    for qubits in ([0], [3, 1], [2, 0, 1]):
        key = "_".join(map(str, qubits))
        mine = T.generate_state_tomography_settings(qubits)
        assert [str(s) for s in mine] == list(ref[f"state_settings_{key}"])
        if len(qubits) == 3:
            continue
        for basis in ("pauli", "sic"):
            mine = T.generate_process_tomography_settings(qubits, basis)
            theirs = [str(s) for s in ref[f"process_settings_{key}_{basis}"]]
            assert [str(s) for s in mine] == theirs
            # text -> object -> text through both implementations
            sampled = theirs[:: max(1, len(theirs) // 7)]
            for s, back in zip(sampled, ref[f"process_roundtrip_{key}_{basis}"]):
                assert str(oe.ExperimentSetting.from_str(s)) == s
                assert str(back) == str(oe.ExperimentSetting.from_str(s))
    with pytest.raises(ValueError):
        T.generate_process_tomography_settings([0], "bogus")
    # record serialisation: same keys and values as the reference's
    ms = oe.ExperimentSetting.from_str(str(ref["record_setting"]))
    mr = oe.ExperimentResult(setting=ms, expectation=0.25, std_err=0.01, total_counts=500, raw_expectation=0.2)
    import json
    assert json.loads(json.dumps(mr, cls=oe.OperatorEncoder)) == json.loads(str(ref["record_json"]))
    for text, want in zip(ref["oneq_texts"], ref["oneq_strs"]):
        assert str(oe._OneQState.from_str(str(text))) == str(want)
    assert list(ref["oneq_bad_raises"]) == [True] * len(ref["oneq_bad"])
    for bad in ref["oneq_bad"]:
        with pytest.raises(ValueError):
            oe._OneQState.from_str(str(bad))
    assert oe.plusX(0) * oe.minusZ(1) == oe.minusZ(1) * oe.plusX(0)
    assert hash(oe.zeros_state([0, 1])) == hash(oe.plusZ(1) * oe.plusZ(0))


def test_beta_resampling_keeps_the_reference_draw_order(ref):
    from fbx import tomography as T, observable_estimation as oe
    settings_m = T.generate_state_tomography_settings([0, 1])
    rs = np.random.RandomState(3)
    e = rs.uniform(-0.9, 0.9, size=len(settings_m))
    assert np.array_equal(e, ref["beta_e"])
    res_m = [oe.ExperimentResult(setting=s, expectation=float(x), std_err=0.0, total_counts=300) for s, x in zip(settings_m, e)]
    np.random.seed(77)
    got = [r.expectation for r in T._resample_expectations_with_beta(res_m)]
    assert got == list(ref["beta_resampled"])
