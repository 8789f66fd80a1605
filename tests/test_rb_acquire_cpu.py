"""The host side of the RB / unitarity acquisition (no GPU): the numpy mirror of the outcome distributions against a dense
density-matrix measurement, the integer restatement of the shots against a scalar shot-by-shot loop, the rule that assigns every
Pauli to one measured basis, the refusals of the Python wrappers, and the seed of the GPU statistical test on the host."""
import itertools

import numpy as np
import pytest

import rb_acquire_cases as cases
from fbx import randomized_benchmarking as rb
from fbx import synthetic


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("mode", ["standard", "unitarity"])
def test_distributions_against_dense_measurement(n, mode):
    rs = np.random.RandomState(11 + n)
    vectors = rs.uniform(-0.4, 0.4, size=(3, 4, 4 ** n))
    vectors[..., 0] = rs.uniform(0.8, 1.0, size=(3, 4))              # a map that loses trace loses it in the distribution
    flips = rs.uniform(0.0, 0.2, size=(3, n, 2))
    for fl in (None, flips[0], flips):
        got = synthetic.rb_outcome_distributions(vectors, n, mode, fl)
        bases = synthetic.rb_measured_bases(n, mode)
        assert got.shape == (3, 4, len(bases), 2 ** n)
        for e, q in itertools.product(range(3), range(4)):
            f = None if fl is None else (fl if fl.ndim == 2 else fl[e])
            for b, digits in enumerate(bases):
                want = cases.dense_measurement(vectors[e, q], n, digits, f)
                np.testing.assert_allclose(got[e, q, b], want, rtol=0, atol=1e-15)
        np.testing.assert_allclose(got.sum(axis=-1), np.broadcast_to(vectors[..., :1], got.shape[:-1]), rtol=0, atol=1e-15)
    wide = synthetic.rb_outcome_distributions(vectors.astype(np.longdouble), n, mode, flips)
    assert wide.dtype == np.longdouble
    np.testing.assert_allclose(wide.astype(np.float64), synthetic.rb_outcome_distributions(vectors, n, mode, flips), rtol=0, atol=1e-15)


def test_basis_rule_covers_every_pauli_once():
    """unitarity: every non-identity Pauli is assigned exactly one of the 3^n bases, that basis measures its non-identity factors
    and has Z on the idle qubits, and the parity mask is its support; standard: the I/Z products, all from the one basis"""
    for n in (1, 2):
        assign = synthetic.rb_pauli_assignment(n, "unitarity")
        bases = synthetic.rb_measured_bases(n, "unitarity")
        assert [k for k, _, _ in assign] == list(range(1, 4 ** n)) and len(bases) == 3 ** n
        for k, basis, mask in assign:
            digits = [(k >> (2 * (n - 1 - q))) & 3 for q in range(n)]
            assert basis == rb.unitarity_basis_of_pauli(n, k)
            assert sum(d * 3 ** (n - 1 - q) for q, d in enumerate(x - 1 for x in bases[basis])) == basis     # base 3, qubit 0 first
            for q in range(n):
                assert bases[basis][q] == (digits[q] if digits[q] else 3)
                assert bool(mask >> (n - 1 - q) & 1) == bool(digits[q])
        # every basis is used, the all-Z one by the most Paulis
        used = [b for _, b, _ in assign]
        assert set(used) == set(range(3 ** n)) and used.count(3 ** n - 1) == 2 ** n - 1
        std = synthetic.rb_pauli_assignment(n, "standard")
        assert [k for k, _, _ in std] == list(rb.z_product_indices(n)) and all(b == 0 for _, b, _ in std)
    assert [m for _, _, m in synthetic.rb_pauli_assignment(2, "standard")] == [1, 2, 3]                # IZ, ZI, ZZ


def _scalar_restatement(probs, N, mode, seed, first_item):
    """shot by shot, scalar Python: the contract read literally"""
    E, Q, NB, M = probs.shape
    n = {2: 1, 4: 2}[M]
    hist = np.zeros(probs.shape, dtype=np.int64)
    k0, k1 = (seed & 0xFFFFFFFF) ^ 0x52424151, seed >> 32
    for e, q, b in itertools.product(range(E), range(Q), range(NB)):
        c = np.cumsum(np.maximum(probs[e, q, b], 0.0))
        thr = [int(np.floor(c[o] / c[-1] * 2.0 ** 32)) for o in range(M - 1)]
        gid = first_item + e
        for s in range(N):
            words = synthetic._philox4x32_10(gid & 0xFFFFFFFF, gid >> 32, q * NB + b, s >> 2, k0, k1)
            w = int(words[s & 3])
            hist[e, q, b, sum(t <= w for t in thr)] += 1
    assign = synthetic.rb_pauli_assignment(n, mode)
    expect = np.empty((E, Q, len(assign)))
    for col, (_, basis, mask) in enumerate(assign):
        for e, q in itertools.product(range(E), range(Q)):
            n_odd = sum(int(hist[e, q, basis, o]) for o in range(M) if bin(o & mask).count("1") & 1)
            expect[e, q, col] = ((N - n_odd) - n_odd) / N
    return hist, expect


@pytest.mark.parametrize("n,mode,N", [(1, "standard", 5), (2, "standard", 7), (1, "unitarity", 4), (2, "unitarity", 6)])
def test_restatement_against_a_scalar_loop(n, mode, N):
    rs = np.random.RandomState(5 + n)
    NB = len(synthetic.rb_measured_bases(n, mode))
    probs = rs.dirichlet(np.ones(2 ** n), size=(2, 3, NB))
    probs[0, 0, 0] = [1.0] + [0.0] * (2 ** n - 1)                     # thresholds of 2^32: reached by no word
    probs[1, 2, NB - 1, 0] = -1e-3                                     # clamped to 0 before the running sum
    seed = (7 << 32) + 99
    hist, expect, std_err = synthetic.restate_rb_counts(probs, N, mode, seed, first_item=(1 << 32) + 2)
    want_hist, want_expect = _scalar_restatement(probs, N, mode, seed, (1 << 32) + 2)
    np.testing.assert_array_equal(hist, want_hist)
    np.testing.assert_array_equal(expect, want_expect)
    np.testing.assert_array_equal(std_err, np.sqrt((1.0 - expect * expect) / N))
    assert (hist.sum(axis=-1) == N).all() and hist[0, 0, 0, 0] == N and hist[1, 2, NB - 1, 0] == 0
    if (n, mode) == (2, "standard"):                                   # ZZ is the product of IZ and ZI shot by shot
        np.testing.assert_array_equal(N * expect[..., 2], hist[:, :, 0, 0] - hist[:, :, 0, 1] - hist[:, :, 0, 2] + hist[:, :, 0, 3])


def test_wrappers_refuse_before_touching_the_library(monkeypatch):
    """bad shapes and depths raise with the reference's messages before the library is asked for: ``_lib.lib`` is replaced by a
    function that fails the test"""
    from fbx import _lib

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    eye1, eye2 = np.eye(4), np.eye(16)
    depth_message = "Sequence depth must be at least 2 for rb sequences, or at least 1 for unitarity sequences."
    with pytest.raises(ValueError, match="No RB gateset for more than two qubits."):
        rb.generate_unitarity_experiment_sequences(None, [0, 1, 2], [2], 1)
    with pytest.raises(ValueError) as err:
        rb.generate_unitarity_experiment_sequences(None, [0], [2, 0], 3, random_seed=1)
    assert str(err.value) == depth_message
    with pytest.raises(ValueError, match="num_sequences must be positive"):
        rb.generate_unitarity_experiment_sequences(None, [0], [2], 0)
    for call, kw in ((rb.simulate_rb_acquisition_batch, {}), (rb.simulate_and_fit_rb_batch, {})):
        with pytest.raises(ValueError) as err:
            call(1, [2, 1], 3, eye1, **kw)
        assert str(err.value) == depth_message
    for call in (rb.simulate_unitarity_acquisition_batch, rb.simulate_and_fit_unitarity_batch):
        with pytest.raises(ValueError) as err:
            call(1, [1, 0], 3, eye1)
        assert str(err.value) == depth_message
    with pytest.raises(ValueError, match="No RB gateset for more than two qubits."):
        rb.simulate_rb_acquisition_batch(3, [2], 1, np.eye(64))
    with pytest.raises(ValueError, match=r"noise_ptms must be \[G, 16, 16\] or \[E, G, 16, 16\]"):
        rb.simulate_rb_acquisition_batch(2, [2], 1, eye1)
    with pytest.raises(ValueError, match="two noise PTMs"):
        rb.simulate_rb_acquisition_batch(1, [2], 1, eye1, interleaved_gate=cases.interleaved_gate(1))
    with pytest.raises(ValueError, match="not a valid 1-qubit Clifford element word"):
        rb.simulate_rb_acquisition_batch(1, [2], 1, np.array([eye1, eye1]), interleaved_gate=0)
    with pytest.raises(ValueError, match="num_sequences must be positive"):
        rb.simulate_unitarity_acquisition_batch(1, [2], 0, eye1)
    with pytest.raises(ValueError, match="depths must not be empty"):
        rb.simulate_unitarity_acquisition_batch(1, [], 1, eye1)
    with pytest.raises(ValueError, match=r"flips must be \[2, 2\] or \[E, 2, 2\]"):
        rb.simulate_rb_acquisition_batch(2, [2], 1, eye2, flips=np.zeros((1, 2)))
    with pytest.raises(ValueError, match="prep must be a Pauli vector of 4 components"):
        rb.simulate_rb_acquisition_batch(1, [2], 1, eye1, prep=np.ones(3))
    with pytest.raises(ValueError, match="shots must be in"):
        rb.simulate_rb_acquisition_batch(1, [2], 1, eye1, shots=2 ** 31)
    with pytest.raises(ValueError, match="first_item must not be negative"):
        rb.simulate_rb_acquisition_batch(1, [2], 1, eye1, first_item=-1)
    with pytest.raises(ValueError, match="points must be 'depth' or 'sequence'"):
        rb.simulate_and_fit_rb_batch(1, [2, 3], 2, eye1, points="all")
    with pytest.raises(ValueError, match="a fit takes 2..256 points"):
        rb.simulate_and_fit_unitarity_batch(1, [2, 3, 4], 100, eye1, points="sequence")


def test_predictions():
    p = 0.93
    for n in (1, 2):
        assert rb.predicted_rb_decay(cases.depolarizing(n, p)) == pytest.approx(p, rel=1e-15)
        assert rb.predicted_unitarity(cases.depolarizing(n, p)) == pytest.approx(p * p, rel=1e-15)
        assert rb.predicted_unitarity(cases.over_rotation(n, 0.3)) == pytest.approx(1.0, rel=1e-14)
        assert rb.predicted_unitarity(cases.amplitude_damping(n, 0.1)) < 1.0
    assert rb.predicted_rb_decay(cases.channels(2)).shape == (3, 1)


def test_the_statistical_seed_passes_on_the_host():
    """GPU test 7 with the distributions written down analytically: under depolarizing noise the final vector of a depth-m
    sequence is (1, 0, 0, p^m), so the all-Z outcome distribution with symmetric flips f is ((1 + (1 - 2 f) p^m) / 2, ...).  The
    device counts equal ``restate_rb_counts`` of the device's distributions (GPU test 3), which differ from these in the last
    bits at most: this is the check that the committed seed passes."""
    s = cases.STAT
    pz = s["p"] ** np.repeat(np.array(s["depths"], dtype=np.float64), s["K"])
    vectors = np.zeros((s["E"], pz.size, 4))
    vectors[..., 0], vectors[..., 3] = 1.0, pz
    probs = synthetic.rb_outcome_distributions(vectors, 1, "standard", np.full((1, 2), s["flip"]))
    hist, _, _ = synthetic.restate_rb_counts(probs, s["shots"], "standard", s["seed"])
    z = (hist[..., 0] - hist[..., 1]).reshape(s["E"], len(s["depths"]), s["K"]).sum(axis=(0, 2)) / (s["E"] * s["K"] * s["shots"])
    mu, bound = cases.stat_bounds()
    print("mean Z per depth, in units of the five-sigma bound:", np.abs(z - mu) / bound)
    assert (np.abs(z - mu) <= bound).all()
