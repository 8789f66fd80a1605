"""fbx.readout and fbx_marginalize_confusion on the GPU: the reference-named functions against the reference's own outputs
(tests/golden/readout_cases.npz), the dict form against the batch form, and the marginal kernel against the einsum model of
tests/readout_cases.py.

Bounds.  A confusion-matrix entry of the reference is n_shots rounded additions of 1 / n_shots into a sum of at most 1, so it lies
within n_shots 2^-52 of counts / n_shots, which the device returns correctly rounded.  A marginal is compared within
4^(n-k) 2^-52 S, S = the sum of the absolute values entering the element: two differently ordered float sums of 4^(n-k) terms."""
import ctypes as C
import os

import numpy as np
import pytest

import readout_cases as rc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "readout_cases.npz")
U8 = C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_single_qubit_confusion_matrices(gpu, gold):
    from fbx import readout
    zero, one = gold["single_should_be_0"], gold["single_should_be_1"]
    n = zero.shape[1]
    for i in range(zero.shape[0]):
        got = readout.estimate_confusion_matrix_from_shots(zero[i], one[i])
        assert got.shape == (2, 2) and np.abs(got - gold["single_confusion"][i]).max() <= n * rc.EPS
        assert np.array_equal(got, np.stack([rc.histogram(zero[i][None])[0], rc.histogram(one[i][None])[0]]) / n)
        assert np.array_equal(got, readout.estimate_confusion_matrix_from_shots(zero[i][:, 0], one[i][:, 0]))
    uneven = readout.estimate_confusion_matrix_from_shots(zero[0][:150], one[0])                 # two shot counts: two launches
    assert np.array_equal(uneven[0], rc.histogram(zero[0][None, :150])[0] / 150)
    assert np.array_equal(uneven[1], rc.histogram(one[0][None])[0] / n)


@pytest.mark.parametrize("g", rc.GOLDEN_GROUP_SIZES)
def test_joint_and_reset_confusion_against_the_reference(gpu, gold, g):
    from fbx import readout
    groups = [tuple(int(q) for q in grp) for grp in gold[f"joint{g}_groups"]]
    for name, fn in (("joint", readout.estimate_joint_confusion_in_set_from_shots),
                     ("reset", readout.estimate_joint_reset_confusion_from_shots)):
        shots, want = gold[f"{name}{g}_shots"], gold[f"{name}{g}_confusion"]
        n = shots.shape[2]
        batch = readout.joint_confusion_matrices_batch(shots)
        assert batch.shape == want.shape and np.abs(batch - want).max() <= n * rc.EPS
        counts = rc.histogram(shots.reshape(-1, n, g)).reshape(want.shape)
        assert np.array_equal(batch, counts / n)                                     # bit for bit numpy's division
        assert np.array_equal(batch.sum(axis=2).round(12), np.ones(want.shape[:2]))
        # the dict form: keys handed over unsorted and as lists' tuples, returned sorted; one value per group, equal to the batch row
        scrambled = {tuple(grp): shots[i] for i, grp in reversed(list(enumerate(groups)))}
        got = fn(scrambled)
        assert list(got) == groups
        for i, grp in enumerate(groups):
            assert np.array_equal(got[grp], batch[i]), (name, grp)
    assert np.array_equal(readout.estimate_joint_reset_confusion_from_shots({groups[0]: shots[0]}, num_trials=64)[groups[0]],
                          counts[0] / 64)


def test_groups_of_different_sizes_in_one_dict(gpu, gold):
    from fbx import readout
    mixed = {(3,): gold["joint1_shots"][3], (0, 2): gold["joint2_shots"][1], (0,): gold["joint1_shots"][0][:, :50],
             (1, 2, 3): gold["joint3_shots"][3]}
    got = readout.estimate_joint_confusion_in_set_from_shots(mixed)
    assert list(got) == sorted(mixed)
    for key, shots in mixed.items():
        n = shots.shape[1]
        assert np.array_equal(got[key], rc.histogram(shots) / n), key


def test_marginals_against_the_reference(gpu, gold):
    from fbx import readout
    for n in (2, 3):
        mat = gold[f"marginal{n}_matrix"]
        for all_q, subset, keep, want in rc.marginal_cases(gold, n):
            got = readout.marginalize_confusion_matrix(mat, all_q, tuple(subset))
            assert got.shape == want.shape
            assert np.all(np.abs(got - want) <= rc.marginal_bound(mat[None], n, keep)[0]), (all_q, subset)
    joint = gold["joint3_confusion"][0]                                  # a marginal of an estimated matrix stays row-stochastic
    assert np.allclose(readout.marginalize_confusion_matrix(joint, (0, 1, 2), (2, 0)).sum(axis=1), 1.0, atol=1e-14)


KEEPS = {1: [[0]], 2: [[0, 1], [0], [1]], 3: [[0, 1, 2], [0], [2], [0, 2]], 6: [[0, 1, 2, 3, 4, 5], [0], [5], [3], [0, 1, 2], [3, 4, 5], [1, 3, 4], [0, 2, 3, 5]],
         10: [list(range(10)), [0], [9], [1, 4, 6, 8, 9], [0, 1, 2, 3, 4, 5, 6, 8]]}


@pytest.mark.parametrize("n", [1, 2, 3, 6, 10])
def test_marginal_kernel(gpu, n):
    """k = n (the identity), k = 1 and middle k; the first, the last and scattered positions; B = 1 and B = 5; host and _dev forms;
    repeated runs bit-identical; an item does not depend on the batch around it."""
    rng = np.random.default_rng(300 + n)
    lib = gpu.lib()
    N = 1 << n
    for B in (1, 5):
        mats = rng.standard_normal((B, N, N))                            # signed: the bound is in terms of the absolute sum
        for keep in KEEPS[n]:
            k = len(keep)
            kp = np.asarray(keep, dtype=np.uint8)
            out = np.full((B, 1 << k, 1 << k), np.nan)
            gpu.check(lib.fbx_marginalize_confusion(n, B, k, kp.ctypes.data_as(U8), gpu.dptr(mats), gpu.dptr(out)))
            want = rc.marginal(mats, n, keep)
            assert np.all(np.abs(out - want) <= rc.marginal_bound(mats, n, keep)), (B, keep, np.abs(out - want).max())
            if k == n:
                assert np.array_equal(out, mats)
            again = np.full_like(out, np.nan)
            gpu.check(lib.fbx_marginalize_confusion(n, B, k, kp.ctypes.data_as(U8), gpu.dptr(mats), gpu.dptr(again)))
            assert np.array_equal(out, again)
            if B == 5:
                alone = np.full_like(out[:1], np.nan)
                gpu.check(lib.fbx_marginalize_confusion(n, 1, k, kp.ctypes.data_as(U8), gpu.dptr(mats[3:4].copy()), gpu.dptr(alone)))
                assert np.array_equal(alone[0], out[3])
                d_in, d_out = gpu.DeviceBuffer.from_array(mats), gpu.DeviceBuffer(out.nbytes)
                gpu.check(lib.fbx_marginalize_confusion_dev(n, B, k, kp.ctypes.data_as(U8), d_in.ptr, d_out.ptr))
                gpu.synchronize()
                assert np.array_equal(d_out.to_array(np.float64, out.shape), out)
                d_in.free(); d_out.free()


def test_marginal_batch_front_end(gpu):
    from fbx import readout
    rng = np.random.default_rng(12)
    mats = rc.random_confusion(rng, 5, 3)
    got = readout.marginalize_confusion_matrix_batch(mats, [4, 9, 1], [1, 4])
    want = rc.marginal(mats, 3, [0, 2])
    assert np.all(np.abs(got - want) <= rc.marginal_bound(mats, 3, [0, 2]))
    for b in range(5):
        assert np.array_equal(got[b], readout.marginalize_confusion_matrix(mats[b], [4, 9, 1], (4, 1)))
