"""The structured Choi-projection cases (tests/proj_cases.py) and their fixture (tests/golden/proj_cases.npz) without a GPU: the
builders still produce the fixture's inputs, the fixture is the one the generator wrote, the Dykstra references are defined by
the mathematics (no stopping-functional value near the threshold, at most 300 iterations), and the float64 oracle meets every
bound tests/test_proj_structured_gpu.py puts on the device -- the bounds are attainable without the code under test."""
import numpy as np
import pytest

import linalg_cases as lc
import proj_cases as pc


@pytest.fixture(scope="module")
def gold():
    return pc.gold()


def test_fixture_is_the_generators(gold):
    assert pc.fixture_digest(gold["arrays"]) == pc.FIXTURE_DIGEST, "an array of tests/golden/proj_cases.npz was altered"
    assert gold["c_p"] >= 1.0 and gold["c_d"] >= 1.0


def test_every_case_hash(gold):
    cases = pc.all_cases()
    assert list(cases) == list(gold["sha"])
    pc.check_hashes(cases, gold)


def test_a_perturbed_case_is_noticed(gold):
    key, a = next(iter(pc.cp_cases(4).items()))
    b = np.array(a)
    b.real[1, 2] = np.nextafter(b.real[1, 2], 1.0)
    with pytest.raises(AssertionError):
        pc.check_hashes({key: b}, gold)
    arrays = dict(gold["arrays"])
    bumped = np.array(arrays["cp_" + key])
    bumped.real[0, 0] = np.nextafter(bumped.real[0, 0], 1.0)
    arrays["cp_" + key] = bumped
    assert pc.fixture_digest(arrays) != pc.FIXTURE_DIGEST


def test_family_properties():
    """what the families promise: Hermitian parts of the cp family are linalg_cases' matrices to rounding, the unitary's Choi
    matrix has rank 1 and trace d, P = I gives a partial trace that is exactly I, tpx has an exact projection"""
    for D in (4, 16, 64):
        for key, x in pc.cp_cases(D).items():
            name = pc.family_of(key)
            if name != "negdef":
                h = lc.build(name, D)
                assert pc.norm_ld(pc.hermitise_ld(x) - h) <= 2 * pc.EPS * pc.norm_ld(h), key
            if name not in pc.NO_ANTI:
                anti = (x.astype(np.clongdouble) - x.astype(np.clongdouble).conj().T) / 2
                assert abs(pc.norm_ld(anti) / pc.norm_ld(pc.hermitise_ld(x)) - 0.25) < 1e-12, key
    for d in pc.DIMS:
        u = pc.channel_cases(d)[f"ch_d{d}_unitary"]
        w = np.linalg.eigvalsh(u)
        assert abs(w[-1] - d) < 1e-13 and np.abs(w[:-1]).max() < 1e-14
        assert pc.norm_ld(pc.tr_out_ld(pc.channel_cases(d)[f"ch_d{d}_tpnotcp"], d) - np.eye(d)) < 1e-13
        assert np.linalg.eigvalsh(pc.channel_cases(d)[f"ch_d{d}_tpnotcp"])[0] < -0.1
        if d != 3:
            assert np.array_equal(pc.tr_out_ld(pc.tni_cases(d)[f"tni_d{d}_eye"], d), np.eye(d))
        assert pc.norm_ld(pc.tr_out_ld(u, d) - np.eye(d)) < 1e-14
        x = pc.tpx_cases(d)[f"tpx_d{d}"]
        assert np.abs(x.real).max() < 2 ** 20 and np.abs(x.imag).max() < 2 ** 20
        assert np.array_equal(x.real, np.rint(x.real)) and np.array_equal(x.imag, np.rint(x.imag))


def test_dykstra_references_are_defined_by_the_mathematics(gold):
    """no stored stopping-functional value within a relative 1e-6 of the threshold, at most 300 iterations, every value but the
    last at or above the threshold; the same for the oracle's own sequences at d = 8, where there is no mpmath reference"""
    closest = 1.0
    for d in pc.DIMS:
        for kind in ("ptp", "ptni"):
            for key in pc.channel_cases(d):
                seq = gold["arrays"][f"dykseq_{kind}_{key}"] if d < 8 else pc.oracle_dykstra(key, kind == "ptp")[2]
                assert pc.sequence_is_clear(seq), (kind, key)
                assert len(seq) <= pc.DYKSTRA_MAX_ITERS, (kind, key, len(seq))
                assert (seq[:-1] >= pc.DYKSTRA_THRESHOLD).all() and seq[-1] < pc.DYKSTRA_THRESHOLD, (kind, key)
                closest = min(closest, float(np.abs(seq / pc.DYKSTRA_THRESHOLD - 1.0).min()))
    print("closest approach of a stopping-functional value to the threshold, relative:", closest)


def test_a_sequence_near_the_threshold_is_noticed(gold):
    seq = np.array(gold["arrays"]["dykseq_ptp_ch_d4_cp17"])
    assert pc.sequence_is_clear(seq)
    for rel in (5e-7, -5e-7, 0.0):
        moved = seq.copy()
        moved[len(seq) // 2] = pc.DYKSTRA_THRESHOLD * (1.0 + rel)
        assert not pc.sequence_is_clear(moved)


def test_stored_norms(gold):
    for D in pc.CP_SIZES:
        for key, x in pc.cp_inputs(D).items():
            if "normh_" + key in gold["norm"]:
                assert abs(pc.norm_ld(pc.hermitise_ld(x)) - gold["norm"]["normh_" + key]) <= 4 * pc.EPS * gold["norm"]["normh_" + key]
    for d in pc.DIMS:
        for key, x in pc.tni_inputs(d).items():
            assert abs(pc.norm_ld(pc.tr_out_ld(x, d)) - gold["norm"]["normp_" + key]) <= 4 * pc.EPS * gold["norm"]["normp_" + key]


@pytest.mark.parametrize("D", pc.CP_SIZES)
def test_oracle_meets_the_cp_bound(gold, D):
    keys, xs = pc.shuffled(pc.cp_inputs(D), D)
    got = [pc.oracle_single("cp", x) for x in xs]
    assert pc.check_cp("oracle", keys, xs, got, gold) <= 1.0
    assert pc.check_twice("oracle", "cp", keys, xs, got, [pc.oracle_single("cp", y) for y in got], gold) <= 1.0


@pytest.mark.parametrize("d", pc.DIMS)
def test_oracle_meets_the_tni_and_tp_bounds(gold, d):
    keys, xs = pc.shuffled(pc.tni_inputs(d), d)
    for kind in ("tni", "tp"):
        got = [pc.oracle_single(kind, x) for x in xs]
        assert (pc.check_tni("oracle", keys, xs, got, gold) if kind == "tni" else pc.check_tp("oracle", keys, xs, got)) <= 1.0
        assert pc.check_twice("oracle", kind, keys, xs, got, [pc.oracle_single(kind, y) for y in got], gold) <= 1.0
    x = pc.tpx_cases(d)[f"tpx_d{d}"]
    for b in range(len(x)):
        want = pc.tp_projection(x[b], d)
        assert np.array_equal(want.astype(np.clongdouble), pc.tp_reference_ld(x[b], d)[0]), "the integer family is not exact"
        assert np.array_equal(pc.oracle_single("tp", x[b]), want)


@pytest.mark.parametrize("kind", ["ptp", "ptni"])
@pytest.mark.parametrize("d", pc.DIMS)
def test_oracle_meets_the_dykstra_bound(gold, d, kind):
    """the recorded oracle iteration is fbx_oracle.superops.proj_choi_to_physical itself, bit for bit"""
    from fbx_oracle import superops as so
    keys, xs = pc.shuffled(pc.channel_cases(d), d)
    runs = [pc.oracle_dykstra(key, kind == "ptp") for key in keys]
    if d < 8:
        for x, run in zip(xs, runs):
            want, n = so.proj_choi_to_physical(np.array(x), kind == "ptp", return_iters=True)
            assert n == run[1] and np.array_equal(want, run[0])
    assert pc.check_dykstra("oracle", kind, keys, xs, [r[0] for r in runs], [r[1] for r in runs], gold) <= 1.0
