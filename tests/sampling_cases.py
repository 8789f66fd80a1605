"""Cases for tests/test_sampling_cpu.py and tests/test_sampling_gpu.py: a host restatement of the stream of
``fbx_sample_bitstrings`` (include/fbx.h) on ``fbx_oracle.acquisition.philox4x32_10`` -- itself pinned by the Random123 known
answers in tests/test_resample_cpu.py -- and the builders of the distributions the tests draw from.

The restatement sums the prefix sums left to right (``numpy.cumsum``).  The contract leaves the order of summation open, so it can
be compared bit for bit only where no order rounds: the dyadic cases below.  For any other distribution the tests check every shot
against the exact prefix sums with the bound ``delta``.
"""
import numpy as np

from fbx_oracle.acquisition import philox4x32_10

MASK32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ the stream
def block(seed, g, s, t):
    """the four words of the Philox block with counter (g low, g high, s, t) and key (seed low, seed high); s may be an array"""
    s = np.atleast_1d(np.asarray(s, dtype=np.uint64))
    ctr = np.empty(s.shape + (4,), dtype=np.uint32)
    ctr[..., 0], ctr[..., 1], ctr[..., 2], ctr[..., 3] = g & MASK32, (g >> 32) & MASK32, s, t
    key = np.broadcast_to(np.array([seed & MASK32, (seed >> 32) & MASK32], dtype=np.uint32), s.shape + (2,))
    return philox4x32_10(ctr, key)


def words(seed, g, shots):
    """x_0 .. x_15 of shots 0 .. shots - 1 of item g: [shots, 16] uint32"""
    s = np.arange(shots, dtype=np.uint64)
    return np.concatenate([block(seed, g, s, t) for t in range(4)], axis=-1)


def draw_integers(x):
    """k = ((x_0 >> 5) << 26) | (x_1 >> 6) of every shot (u = k 2^-53), as uint64"""
    x0, x1 = x[..., 0].astype(np.uint64), x[..., 1].astype(np.uint64)
    return ((x0 >> np.uint64(5)) << np.uint64(26)) | (x1 >> np.uint64(6))


def uniforms(x):
    return draw_integers(x).astype(np.float64) * 2.0 ** -53           # k < 2^53: the conversion and the product are exact


def weights(p, lam=0.0):
    p = np.asarray(p, dtype=np.float64)
    if lam == 0.0:
        return p.copy()
    return (1.0 - lam) * p + lam * p.sum() / p.size


def outcomes_before_flips(p, lam, u):
    """the smallest i with C_i > u C_{N-1}; if rounding leaves none, the last i of positive weight"""
    w = weights(p, lam)
    C = np.cumsum(w)
    idx = np.searchsorted(C, u * C[-1], side="right")
    return np.where(idx >= w.size, np.flatnonzero(w > 0.0)[-1], idx).astype(np.int64)


def to_bits(idx, n):
    """[shots] outcome indices -> [shots, n] uint8, first column = qubit 0 = the most significant bit"""
    return ((np.asarray(idx, dtype=np.int64)[:, None] >> np.arange(n - 1, -1, -1)) & 1).astype(np.uint8)


def from_bits(bits):
    bits = np.asarray(bits).astype(np.int64)
    return (bits << np.arange(bits.shape[-1] - 1, -1, -1)).sum(axis=-1)


def apply_flips(bits, flip, x):
    """column j, drawn bit d, flips iff (double) x_{2 + j} 2^-32 < flip[j][d]"""
    n = bits.shape[1]
    r = x[:, 2:2 + n].astype(np.float64) * 2.0 ** -32
    thr = np.where(bits == 1, flip[None, :, 1], flip[None, :, 0])
    return (bits ^ (r < thr)).astype(np.uint8)


def restate(p, shots, lam=0.0, flip=None, seed=0, g=0):
    """the record [shots, n] of item g, and the outcome indices that were drawn (before the flips)"""
    n = int(np.asarray(p).size).bit_length() - 1
    x = words(seed, g, shots)
    drawn = outcomes_before_flips(p, lam, uniforms(x))
    bits = to_bits(drawn, n)
    if flip is not None:
        bits = apply_flips(bits, np.asarray(flip, dtype=np.float64), x)
    return bits, drawn


def restate_batch(p, shots, lam=0.0, flip=None, seed=0, first_item=0):
    p = np.asarray(p)
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (p.shape[0],))
    n = p.shape[1].bit_length() - 1
    fl = None if flip is None else np.broadcast_to(np.asarray(flip, dtype=np.float64), (p.shape[0], n, 2))
    return np.stack([restate(p[b], shots, float(lam[b]), None if fl is None else fl[b], seed, first_item + b)[0]
                     for b in range(p.shape[0])])


# ------------------------------------------------------------------------------------------------ distributions
DYADIC_BITS = 20


def dyadic_weights(n, batch, seed):
    """[batch, 2^n] weights k_i / 2^20 with integers k_i >= 0 summing to 2^20, about a third of them zero -- among them index 0
    and index N - 1 (N = 2 cannot have both: there the items alternate between a zero at 0, a zero at 1 and none).  Every partial
    sum in every order is a multiple of 2^-20 below 2, so no summation rounds; the same holds with depolarizing 0.25 (multiples of
    2^-22 for n <= 13)."""
    rng = np.random.default_rng([seed, n])
    N = 1 << n
    out = np.zeros((batch, N))
    for b in range(batch):
        zero = rng.random(N) < 1.0 / 3.0
        if N >= 4:
            zero[0] = zero[N - 1] = True
            if zero.all():
                zero[1] = False
        else:
            zero[:] = False
            if b % 3 < 2:
                zero[b % 3] = True
        pos = np.flatnonzero(~zero)
        k = rng.multinomial((1 << DYADIC_BITS) - pos.size, np.full(pos.size, 1.0 / pos.size)) + 1
        out[b, pos] = k * 2.0 ** -DYADIC_BITS
    assert np.all(out.sum(axis=1) == 1.0)
    return out


FLIP_VALUES = (0.0, 2.0 ** -2, 2.0 ** -5, 1.0)


def asymmetric_flips(n, batch, seed):
    """[batch, n, 2] flip probabilities from {0, 1/4, 1/32, 1}; the two directions of a column always differ"""
    rng = np.random.default_rng([seed, n, 77])
    a = rng.integers(0, 4, size=(batch, n))
    b = (a + rng.integers(1, 4, size=(batch, n))) % 4
    return np.stack([np.take(FLIP_VALUES, a), np.take(FLIP_VALUES, b)], axis=-1)


def one_hot(n):
    """(outcomes, [4, 2^n]): all the weight on outcome 0, 1, N / 2 and N - 1"""
    N = 1 << n
    where = np.array([0, 1, N // 2, N - 1])
    p = np.zeros((4, N))
    p[np.arange(4), where] = 1.0
    return where, p


def porter_thomas(n, batch, seed):
    """[batch, 2^n] squared moduli of a complex normal vector, not normalised, a random half of them set to exactly 0"""
    rng = np.random.default_rng([seed, n, 1811])
    N = 1 << n
    z = rng.standard_normal((batch, N)) + 1j * rng.standard_normal((batch, N))
    p = np.abs(z) ** 2
    for b in range(batch):
        p[b, rng.permutation(N)[:N // 2]] = 0.0
    return p


def exact_prefix_sums(p):
    """the inclusive prefix sums in numpy.longdouble (64 bits of mantissa where the test machines run: N 2^-64 relative, far
    below delta)"""
    return np.cumsum(np.asarray(p, dtype=np.longdouble))


def delta(p):
    """N 2^-51 T: four times the worst-case rounding N 2^-53 T of an N-term sum of non-negative terms in any order, which also
    covers the one product u C_{N-1}"""
    p = np.asarray(p, dtype=np.longdouble)
    return p.size * np.longdouble(2.0 ** -51) * p.sum()
