"""Cases for tests/test_sampling_wide_cpu.py and tests/test_sampling_wide_gpu.py: the host restatement of the stream of
``fbx_sample_bitstrings_wide`` (include/fbx.h) for widths 14..26.  It is the restatement of tests/sampling_cases.py with the
Philox blocks t = 0 .. ceil((2 + n) / 4) - 1 of a shot (up to seven: words x_0 .. x_27) instead of four, and dyadic weights that
cross the 4096-entry blocks of the device's table.  Porter-Thomas weights, ``delta`` and the bit helpers are reused as they are.
"""
import numpy as np

import sampling_cases as sc

BLOCK = 4096                                                          # entries per block of the device's table


# ------------------------------------------------------------------------------------------------ the stream
def n_blocks(n):
    return (2 + n + 3) // 4


def words(seed, g, shots, n):
    """x_0 .. of shots 0 .. shots - 1 of item g at width n: [shots, 4 ceil((2 + n) / 4)] uint32"""
    s = np.arange(shots, dtype=np.uint64)
    return np.concatenate([sc.block(seed, g, s, t) for t in range(n_blocks(n))], axis=-1)


def restate(p, shots, lam=0.0, flip=None, seed=0, g=0):
    """the record [shots, n] of item g, the outcome indices that were drawn (before the flips), and the draws u"""
    n = int(np.asarray(p).size).bit_length() - 1
    x = words(seed, g, shots, n if flip is not None else 0)
    u = sc.uniforms(x)
    drawn = sc.outcomes_before_flips(p, lam, u)
    bits = sc.to_bits(drawn, n)
    if flip is not None:
        bits = sc.apply_flips(bits, np.asarray(flip, dtype=np.float64), x)
    return bits, drawn, u


def restate_batch(p, shots, lam=0.0, flip=None, seed=0, first_item=0):
    p = np.asarray(p)
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (p.shape[0],))
    n = p.shape[1].bit_length() - 1
    fl = None if flip is None else np.broadcast_to(np.asarray(flip, dtype=np.float64), (p.shape[0], n, 2))
    return np.stack([restate(p[b], shots, float(lam[b]), None if fl is None else fl[b], seed, first_item + b)[0]
                     for b in range(p.shape[0])])


# ------------------------------------------------------------------------------------------------ distributions
DYADIC_BITS = 30


def dyadic_weights_wide(n, batch, seed):
    """[batch, 2^n] weights k_i / 2^30 with integers k_i >= 0 summing to 2^30, n >= 14.  About a third of the entries are zero, among
    them index 0, index N - 1, both sides of the seam between blocks 0 and 1 (4095 and 4096) and of the last seam (N - 4097 and
    N - 4096); block 2 (8192 .. 12287) is zero as a whole.  Every partial sum in every order is a multiple of 2^-30 and at most 1,
    so no summation rounds; with depolarizing 0.25 the weights 3 k_i / 2^32 + 2^-(n + 2) are multiples of 2^-32 for n <= 26 and
    their sums stay below 2: 33 bits, nothing rounds either."""
    rng = np.random.default_rng([seed, n, 30])
    N = 1 << n
    assert N >= 4 * BLOCK
    out = np.zeros((batch, N))
    for b in range(batch):
        zero = rng.random(N) < 1.0 / 3.0
        zero[[0, N - 1, BLOCK - 1, BLOCK, N - BLOCK - 1, N - BLOCK]] = True
        zero[2 * BLOCK:3 * BLOCK] = True
        pos = np.flatnonzero(~zero)
        k = rng.multinomial((1 << DYADIC_BITS) - pos.size, np.full(pos.size, 1.0 / pos.size)) + 1
        out[b, pos] = k * 2.0 ** -DYADIC_BITS
    assert np.all(out.sum(axis=1) == 1.0)
    return out


def asymmetric_flips(n, batch, seed):
    """[batch, n, 2] flip probabilities from {0, 1/4, 1/32, 1} over n columns; the two directions of a column always differ"""
    return sc.asymmetric_flips(n, batch, seed)


def one_hot(n):
    """(outcomes, [6, 2^n]): all the weight on outcome 0, 1, 4095, 4096, N / 2 and N - 1"""
    N = 1 << n
    where = np.array([0, 1, BLOCK - 1, BLOCK, N // 2, N - 1])
    p = np.zeros((where.size, N))
    p[np.arange(where.size), where] = 1.0
    return where, p
