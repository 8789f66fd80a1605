"""fbx.classical_logic.ripple_carry_adder and fbx.entangled_states on the GPU: the reference-named functions against the
reference's own outputs (tests/golden/readout_cases.npz), bit for bit against numpy's counts / n_shots on the model's counts
(tests/readout_cases.py), and the batch forms against their per-experiment calls.

Bound against the reference: it adds 1 / n_shots once per matching shot -- at most n_shots rounded additions into a sum of at most
1 -- so each of its probabilities is within n_shots 2^-52 of counts / n_shots, which the device returns correctly rounded."""
import os

import numpy as np
import pytest

import readout_cases as rc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "readout_cases.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("n_bits", rc.GOLDEN_ADDER_BITS)
def test_adder_against_the_reference(gpu, gold, n_bits):
    from fbx.classical_logic import ripple_carry_adder as rca
    res = gold[f"adder{n_bits}_results"]
    shots = res.shape[1]
    success = rca.get_success_probabilities_from_results(res.tolist())
    hamming = rca.get_error_hamming_distributions_from_results(res)
    assert isinstance(success, list) and isinstance(success[0], float) and len(success) == 4 ** n_bits
    assert isinstance(hamming, list) and isinstance(hamming[0], list) and len(hamming[0]) == n_bits + 2
    assert np.abs(np.asarray(success) - gold[f"adder{n_bits}_success"]).max() <= shots * rc.EPS
    assert np.abs(np.asarray(hamming) - gold[f"adder{n_bits}_hamming"]).max() <= shots * rc.EPS
    counts = rc.histogram(res, expected=rc.adder_expected(n_bits), kind=rc.WEIGHT)
    assert np.array_equal(np.asarray(hamming), counts / shots)                     # bit for bit numpy's division
    assert success == [row[0] for row in hamming] and success[0] == 1.0


def test_adder_batch_against_per_experiment_calls(gpu):
    from fbx import synthetic
    from fbx.classical_logic import ripple_carry_adder as rca
    for n_bits, shots in ((1, 17), (2, 1000), (4, 33)):
        runs = np.stack([synthetic.adder_shots(n_bits, p, shots, seed=70 + e) for e, p in enumerate((0.0, 0.05, 0.3))])
        success = rca.get_success_probabilities_from_results_batch(runs)
        hamming = rca.get_error_hamming_distributions_from_results_batch(runs)
        assert success.shape == (3, 4 ** n_bits) and hamming.shape == (3, 4 ** n_bits, n_bits + 2)
        assert (success[0] == 1.0).all() and np.array_equal(success, hamming[:, :, 0])
        expected = np.tile(rc.adder_expected(n_bits), (3, 1))
        counts = rc.histogram(runs.reshape(-1, shots, n_bits + 1), expected=expected, kind=rc.WEIGHT)
        assert np.array_equal(hamming.reshape(counts.shape), counts / shots)
        for e in range(3):
            assert rca.get_success_probabilities_from_results(runs[e]) == success[e].tolist()
            assert rca.get_error_hamming_distributions_from_results(runs[e]) == hamming[e].tolist()


@pytest.mark.parametrize("n", rc.GOLDEN_GHZ_WIDTHS)
def test_ghz_statistics_against_the_reference(gpu, gold, n):
    from fbx import entangled_states as es
    bits = gold[f"ghz{n}_bits"]
    got = es.ghz_state_statistics(bits)
    assert got == {"bell": int(gold[f"ghz{n}_stats"][0]), "total": int(gold[f"ghz{n}_stats"][1])}
    assert isinstance(got["bell"], int) and isinstance(got["total"], int)
    assert es.ghz_state_statistics(bits.tolist()) == got


def test_ghz_batch(gpu):
    from fbx import entangled_states as es, synthetic
    for n, shots in ((1, 9), (4, 1000), (12, 4099)):
        bits = np.stack([synthetic.ghz_shots(n, p, shots, seed=s) for s, p in enumerate((0.0, 0.02, 0.5, 0.2, 0.1))])
        got = es.ghz_state_statistics_batch(bits)
        want = ((bits == 0).all(axis=2) | (bits == 1).all(axis=2)).sum(axis=1)
        assert got["bell"].dtype == np.int64 and np.array_equal(got["bell"], want) and got["bell"][0] == shots
        assert np.array_equal(got["total"], np.full(5, shots))
        for b in range(5):
            assert es.ghz_state_statistics(bits[b]) == {"bell": int(want[b]), "total": shots}
