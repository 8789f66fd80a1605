"""Readout / adder / GHZ analysis on the host (no GPU): the numpy model of tests/readout_cases.py pinned to the reference's outputs in
tests/golden/readout_cases.npz (tests/golden/make_readout_goldens.py), so that the GPU tests on other shapes do not compare the
device with itself; the host tables and generators; the argument errors of the new entry points; the loud failure without a device.

Bound against the reference: it adds 1 / n_shots into a matrix entry once per shot, n_shots rounded additions into a sum of at most
1, so an entry is within n_shots 2^-52 of counts / n_shots."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import readout_cases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "readout_cases.npz")
U8 = C.POINTER(C.c_uint8)
I64 = C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def gold():
    assert os.path.getsize(GOLDEN) < 300 * 1024
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_model_reproduces_the_confusion_goldens(gold):
    zero, one = gold["single_should_be_0"], gold["single_should_be_1"]
    n = zero.shape[1]
    f0, f1 = rc.histogram(zero) / n, rc.histogram(one) / n
    assert np.abs(np.stack([f0, f1], axis=1) - gold["single_confusion"]).max() <= n * rc.EPS
    for g in rc.GOLDEN_GROUP_SIZES:
        assert gold[f"joint{g}_groups"].tolist() == [list(c) for c in itertools.combinations(rc.GOLDEN_QUBITS, g)]
        for name in ("joint", "reset"):
            shots = gold[f"{name}{g}_shots"]
            G, rows, n, _ = shots.shape
            counts = rc.histogram(shots.reshape(G * rows, n, g)).reshape(G, rows, rows)
            assert (counts.sum(axis=2) == n).all()
            assert np.abs(counts / n - gold[f"{name}{g}_confusion"]).max() <= n * rc.EPS, (name, g)


def test_model_reproduces_the_marginal_goldens(gold):
    for n in (2, 3):
        mat = gold[f"marginal{n}_matrix"][None]
        seen = 0
        for all_q, subset, keep, want in rc.marginal_cases(gold, n):
            assert np.all(np.abs(rc.marginal(mat, n, keep)[0] - want) <= rc.marginal_bound(mat, n, keep)[0]), (all_q, subset)
            seen += 1
        assert seen == {2: 2 * 4, 3: 6 * 15}[n]


def test_model_reproduces_the_adder_and_ghz_goldens(gold):
    from fbx.classical_logic import adder_expected_bits
    for n in rc.GOLDEN_ADDER_BITS:
        res = gold[f"adder{n}_results"]
        assert np.array_equal(adder_expected_bits(n), rc.adder_expected(n))
        counts = rc.histogram(res, expected=rc.adder_expected(n), kind=rc.WEIGHT)
        shots = res.shape[1]
        assert counts.shape == (4 ** n, n + 2)
        assert np.abs(counts / shots - gold[f"adder{n}_hamming"]).max() <= shots * rc.EPS
        assert np.abs(counts[:, 0] / shots - gold[f"adder{n}_success"]).max() <= shots * rc.EPS
        assert counts[0, 0] == shots
    for n in rc.GOLDEN_GHZ_WIDTHS:
        counts = rc.histogram(gold[f"ghz{n}_bits"][None], kind=rc.WEIGHT)[0]
        assert [counts[0] + counts[n], counts.sum()] == gold[f"ghz{n}_stats"].tolist()


def test_bit_helpers_follow_the_reference():
    from fbx import utils
    for n in (1, 3, 6):
        table = utils.all_bitstrings(n)
        assert table.dtype == np.uint8 and table.shape == (1 << n, n)
        assert table.tolist() == [list(b) for b in itertools.product((0, 1), repeat=n)]
        for r, row in enumerate(table):
            assert utils.bit_array_to_int(row) == r and utils.int_to_bit_array(r, n) == row.tolist()
    assert utils.int_to_bit_array(5, 2) == [0, 1] and utils.bit_array_to_int([]) == 0


def test_generators_are_seeded_and_shaped():
    from fbx import synthetic
    conf = rc.random_confusion(np.random.default_rng(1), 3, 2)
    shots = synthetic.readout_shots(conf, 400, seed=5)
    assert shots.shape == (3, 4, 400, 2) and shots.dtype == np.uint8 and shots.max() <= 1
    assert np.array_equal(shots, synthetic.readout_shots(conf, 400, seed=5))
    assert not np.array_equal(shots, synthetic.readout_shots(conf, 400, seed=6))
    assert synthetic.readout_shots(conf[0], 10).shape == (4, 10, 2)
    freq = rc.histogram(shots.reshape(12, 400, 2)).reshape(3, 4, 4) / 400.0
    assert np.abs(freq - conf).max() < 0.1                                       # 5 sigma of a frequency near 0.9 is 0.075
    add = synthetic.adder_shots(2, 0.0, 7)
    assert add.shape == (16, 7, 3) and np.array_equal(add, np.repeat(rc.adder_expected(2)[:, None], 7, axis=1))
    assert np.array_equal(synthetic.adder_shots(2, 1.0, 7), 1 - add)
    ghz = synthetic.ghz_shots(4, 0.0, 50)
    assert ghz.shape == (50, 4) and (ghz == ghz[:, :1]).all() and 0 < ghz[:, 0].sum() < 50
    with pytest.raises(ValueError):
        synthetic.readout_shots(np.ones((3, 3)) / 3, 5)


def histogram_rc(lib, n_cols=2, B=1, n_shots=4, bits=True, k=2, cols=None, shared=1, kind=0, counts=True, dev=False):
    b = np.zeros(max(1, B * max(n_shots, 1) * max(n_cols, 1)), dtype=np.uint8)
    out = np.zeros(4096, dtype=np.int64)
    c = None if cols is None else np.asarray(cols, dtype=np.uint8)
    if dev:
        return lib.fbx_bit_histogram_dev(n_cols, B, n_shots, b.ctypes.data if bits else None, k, None if c is None else c.ctypes.data,
                                         shared, None, kind, out.ctypes.data if counts else None)
    return lib.fbx_bit_histogram(n_cols, B, n_shots, b.ctypes.data_as(U8) if bits else None, k,
                                 None if c is None else c.ctypes.data_as(U8), shared, None, kind,
                                 out.ctypes.data_as(I64) if counts else None)


@pytest.mark.parametrize("dev", [False, True])
def test_histogram_argument_errors(dev):
    from fbx import _lib
    lib = _lib.lib()
    bad = [(dict(n_cols=0), b"n_cols"), (dict(n_cols=65), b"n_cols"),
           (dict(k=0), b"k must"), (dict(k=11, n_cols=11), b"k must"), (dict(kind=1, k=65, n_cols=64), b"k must"), (dict(kind=1, k=0), b"k must"),
           (dict(kind=2), b"kind"),
           (dict(k=3, n_cols=2), b"cols is NULL"),
           (dict(n_shots=0), b"n_shots"), (dict(n_shots=2 ** 31, bits=True, B=0), b"n_shots"),
           (dict(bits=False), b"NULL"), (dict(counts=False), b"NULL"), (dict(B=-1), b"B must")]
    if not dev:
        bad += [(dict(cols=[0, 2]), b"cols entry"), (dict(cols=[[0, 1], [1, 2]], shared=0, B=2), b"cols entry")]
    for kwargs, word in bad:
        assert histogram_rc(lib, dev=dev, **kwargs) == _lib.FBX_ERR_BAD_ARG, kwargs
        assert word in lib.fbx_last_error(), (kwargs, lib.fbx_last_error())
        with pytest.raises(ValueError):
            _lib.check(_lib.FBX_ERR_BAD_ARG)
    assert histogram_rc(lib, dev=dev, B=0, bits=False, counts=False) == _lib.FBX_OK
    assert histogram_rc(lib, dev=dev, B=0, kind=1, k=64, n_cols=64, bits=False, counts=False) == _lib.FBX_OK


@pytest.mark.parametrize("dev", [False, True])
def test_marginalize_argument_errors(dev):
    from fbx import _lib
    lib = _lib.lib()
    fn = lib.fbx_marginalize_confusion_dev if dev else lib.fbx_marginalize_confusion
    buf = np.zeros(16)
    ptr = buf.ctypes.data if dev else _lib.dptr(buf)

    def rc_of(n=2, B=1, keep=(0,), k=None, a=ptr, o=ptr):
        kp = np.asarray(keep, dtype=np.uint8)
        return fn(n, B, len(keep) if k is None else k, kp.ctypes.data_as(U8) if keep is not None else None, a, o)

    for kwargs, word in [(dict(n=0), b"n_qubits"), (dict(n=11), b"n_qubits"), (dict(keep=(), k=0), b"k must"),
                         (dict(keep=(0, 1, 1), k=3), b"k must"), (dict(keep=(1, 0)), b"ascending"), (dict(keep=(1, 1)), b"ascending"),
                         (dict(keep=(0, 2)), b"keep entry"), (dict(keep=(2,)), b"keep entry"), (dict(a=None), b"NULL"),
                         (dict(o=None), b"NULL"), (dict(B=-1), b"B must")]:
        assert rc_of(**kwargs) == _lib.FBX_ERR_BAD_ARG, kwargs
        assert word in lib.fbx_last_error(), (kwargs, lib.fbx_last_error())
    assert fn(2, 1, 1, None, ptr, ptr) == _lib.FBX_ERR_BAD_ARG and b"keep" in lib.fbx_last_error()
    assert rc_of(B=0, a=None, o=None) == _lib.FBX_OK


def test_frequencies_argument_errors():
    from fbx import _lib
    lib = _lib.lib()
    c, o = np.zeros(4, dtype=np.int64), np.zeros(4)
    assert lib.fbx_counts_to_frequencies(4, c.ctypes.data_as(I64), 0, _lib.dptr(o)) == _lib.FBX_ERR_BAD_ARG
    assert b"denom" in lib.fbx_last_error()
    assert lib.fbx_counts_to_frequencies(4, None, 5, _lib.dptr(o)) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_counts_to_frequencies(-1, c.ctypes.data_as(I64), 5, _lib.dptr(o)) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_counts_to_frequencies(0, None, 5, None) == _lib.FBX_OK


def test_python_front_ends_reject_bad_input_before_the_library():
    from fbx import entangled_states, readout, utils
    from fbx.classical_logic import get_success_probabilities_from_results_batch
    bits = np.zeros((2, 5, 3), dtype=np.uint8)
    for kwargs in (dict(cols=[0, 3]), dict(cols=[[0, 1]]), dict(expected=[0, 1]), dict(expected=[0, 1, 2]), dict(kind="parity")):
        with pytest.raises(ValueError):
            utils.bitstring_histogram_batch(bits, **kwargs)
    with pytest.raises(ValueError):
        utils.bitstring_histogram_batch(np.full((1, 2, 2), 2, dtype=np.int64))
    with pytest.raises(ValueError):
        utils.bitstring_histogram_batch(np.zeros((1, 4, 11), dtype=np.uint8))                 # a joint histogram of 11 columns
    with pytest.raises(ValueError):
        readout.joint_confusion_matrices_batch(np.zeros((1, 3, 5, 2), dtype=np.uint8))
    with pytest.raises(ValueError):
        readout.marginalize_confusion_matrix(np.eye(4), [0, 1], (2,))                            # the reference asserts here
    with pytest.raises(ValueError):
        readout.marginalize_confusion_matrix(np.eye(4), [0, 1, 2], (1,))
    with pytest.raises(ValueError):
        get_success_probabilities_from_results_batch(np.zeros((1, 5, 3, 2), dtype=np.uint8))
    with pytest.raises(ValueError):
        entangled_states.ghz_state_statistics_batch(np.zeros((4, 2), dtype=np.uint8))


def test_no_device_fails_loudly():
    """Without a GPU every compute call reports FBX_ERR_NO_DEVICE -- there is no host fallback; with one, the same calls answer."""
    import fbx
    from fbx import _lib, entangled_states, readout, utils
    from fbx.classical_logic import get_success_probabilities_from_results
    calls = [lambda: utils.bitstring_histogram_batch(np.zeros((1, 4, 2), dtype=np.uint8)),
             lambda: readout.marginalize_confusion_matrix(np.eye(4), [0, 1], (1,)),
             lambda: readout.estimate_confusion_matrix_from_shots(np.zeros(8, dtype=np.uint8), np.ones(8, dtype=np.uint8)),
             lambda: get_success_probabilities_from_results(np.zeros((4, 3, 2), dtype=np.uint8)),
             lambda: entangled_states.ghz_state_statistics(np.zeros((5, 3), dtype=np.uint8))]
    for call in calls:
        if fbx.device_count() > 0:
            call()
        else:
            with pytest.raises(fbx.FbxError) as ei:
                call()
            assert ei.value.code == _lib.FBX_ERR_NO_DEVICE
