"""Shapes, data and the exact reference for fbx_shots_to_moments[_dev] (csrc/fbx_shots.hip), shared by tests/test_shots_cases_cpu.py
(which proves that the table reaches every branch of the launcher) and tests/test_shots_dispatch_gpu.py (which runs it).

route() restates the launcher's choice in Python; CASES lists the smallest shapes that reach each of its branches; make() draws the data
(bytes 0..255 of which only bit 0 is the outcome, a bias per setting that saturates the counts, mask bytes from {0, 1, 2, 255});
exact() counts with integer numpy and forms the four moments with fractions.Fraction, rounded to double once.  Nothing here is the
kernel's algorithm: no vectors, no packed runs, no popcounts."""
import zlib
from fractions import Fraction
from typing import NamedTuple

import numpy as np

# ---------------------------------------------------------------------------------------------------------------------------------
# the launcher, fbx_shots_to_moments_dev (csrc/fbx_shots.hip); every constant once, beside the line it restates
# ---------------------------------------------------------------------------------------------------------------------------------
WAVE_BYTES = 16384          # :447  per_wave = n_shots * n_qubits < FBX_RECORD_WAVE_BYTES (csrc/fbx_common.hpp) && n_settings >= 4
WAVE_MIN_SETTINGS = 4       # :447
WAVES_PER_GROUP = 4         # :448  units = per_wave ? (n_settings + 3) / 4 : n_settings   (and :163, :176, :247: blockIdx.x * 4 + wave)
GRID_CAP = 256 * 16         # :449  grid = min(units, 256 * 16) = 4096 workgroups
PIPE_BYTES = 8192           # :453  bytes <= 8192: at most eight 16-byte vectors per lane
VEC_BYTES = 16              # :452  (bytes & 15) == 0 && (d_bits & 15) == 0
LANES = 64                  # :455  vpl = (bytes / 16 + 63) / 64
PACKED_ALIGN = 8            # :464-465  (bytes & 7) == 0 && (d_bits & 7) == 0
PACKED_RUN = 16             # :465  n_shots / 16: runs of 16 shots
PACKED_RUNS_ONE = 64        # :466  one = n_shots / 16 <= 64    -> RPL = 1
PACKED_RUNS_MAX = 128       # :465  n_shots / 16 <= 128         -> RPL = 2
VEC_N = (1, 2, 4, 8)        # :452, :258
PACKED_PIPE_N = (3, 5)      # :464
PACKED_N = (3, 5, 6, 7)     # :264
SECOND_TRIP_WAVE = WAVES_PER_GROUP * GRID_CAP + 5           # 16389 settings: five wavefronts make a second trip
SECOND_TRIP_GROUP = GRID_CAP + 5                            # 4101 settings: five workgroups make a second trip


class Route(NamedTuple):
    name: str               # "pipe<NQB,VPL>", "packed<NQ,RPL>", "wave" or "workgroup"
    paths: frozenset        # wave / workgroup: the per-record count paths reached, of {"vec", "packed", "generic"}; else empty
    second_trip: bool       # the grid-stride loop runs again for some wavefront / workgroup

    @property
    def label(self):
        return self.name + ("[" + "+".join(sorted(self.paths)) + "]" if self.paths else "") + ("-trip2" if self.second_trip else "")


def record_paths(n, S, shots, base_offset=0):
    """the count path of every record in shots_kernel (:256-271), by the record's own alignment"""
    out = []
    for s in range(S):
        addr = base_offset + s * shots * n
        if n in VEC_N and addr % VEC_BYTES == 0:                                       # :256, :258
            out.append("vec")
        elif n in PACKED_N and addr % PACKED_ALIGN == 0:                               # :264
            out.append("packed")
        else:                                                                          # :269
            out.append("generic")
    return out


def route(n, S, shots, base_offset=0):
    nbytes = shots * n                                                                 # :451
    per_wave = nbytes < WAVE_BYTES and S >= WAVE_MIN_SETTINGS                          # :447
    units = -(-S // WAVES_PER_GROUP) if per_wave else S                                # :448
    second = units > GRID_CAP                                                          # :449 with the loops at :140, :198, :249
    if per_wave and n in VEC_N and nbytes % VEC_BYTES == 0 and nbytes <= PIPE_BYTES and base_offset % VEC_BYTES == 0:   # :452-453
        vpl = -(-(nbytes // VEC_BYTES) // LANES)                                       # :455
        cls = 1 if vpl <= 1 else 2 if vpl == 2 else 4 if vpl <= 4 else 8               # :458-459
        return Route(f"pipe<{n},{cls}>", frozenset(), second)
    runs = shots // PACKED_RUN
    if (per_wave and n in PACKED_PIPE_N and nbytes % PACKED_ALIGN == 0 and base_offset % PACKED_ALIGN == 0
            and 1 <= runs <= PACKED_RUNS_MAX):                                         # :464-465
        return Route(f"packed<{n},{1 if runs <= PACKED_RUNS_ONE else 2}>", frozenset(), second)                         # :466
    return Route("wave" if per_wave else "workgroup", frozenset(record_paths(n, S, shots, base_offset)), second)       # :473-478


# ---------------------------------------------------------------------------------------------------------------------------------
# the table: (n, S, shots, base_offset)
# ---------------------------------------------------------------------------------------------------------------------------------
PIPE_VECTORS = (1, 63, 64, 65, 128, 129, 256, 257, 512)     # both sides of every VPL class boundary
PACKED_SHOTS = (16, 24, 1016, 1024, 1032, 1040, 2048, 2056)  # runs of 1, 63, 64, 65, 128 with a tail of 0 or 8 shots
BLOCKS = {
    "pipe_first_trip": [(n, 9, VEC_BYTES * v // n, 0) for n in VEC_N for v in PIPE_VECTORS],
    "pipe_past_8192_bytes": [(n, 9, VEC_BYTES * 513 // n, 0) for n in VEC_N],
    "pipe_second_trip": [(n, SECOND_TRIP_WAVE, VEC_BYTES // n, 0) for n in VEC_N]
                        + [(2, SECOND_TRIP_WAVE, VEC_BYTES * 65 // 2, 0), (4, SECOND_TRIP_WAVE, VEC_BYTES * 129 // 4, 0),
                           (8, SECOND_TRIP_WAVE, VEC_BYTES * 257 // 8, 0)],
    "packed_first_trip": [(n, 9, shots, 0) for n in PACKED_PIPE_N for shots in PACKED_SHOTS],
    "packed_past_128_runs": [(n, 9, 2064, 0) for n in PACKED_PIPE_N],
    "packed_second_trip": [(5, SECOND_TRIP_WAVE, 16, 0), (3, SECOND_TRIP_WAVE, 1040, 0)],
    "wave_vector_counts": [(n, 9, shots, 0) for n in VEC_N for shots in (1, 7, 17, 1000)],
    "wave_packed_counts": [(n, 9, shots, 0) for n in PACKED_N for shots in (1, 15, 16, 17, 1003)],
    "wave_wide": [(n, 9, shots, 0) for n in (9, 16, 33, 64) for shots in (1, 100)],
    "wave_second_trip": [(9, SECOND_TRIP_WAVE, 3, 0)],
    "workgroup_few_settings": [(n, S, 1000, 0) for n in (2, 3, 9) for S in (1, 2, 3)],
    "workgroup_switch": [(1, 9, 16383, 0), (1, 9, 16384, 0), (3, 9, 5461, 0), (3, 9, 5462, 0), (9, 9, 1820, 0), (9, 9, 1821, 0)],
    "workgroup_second_trip": [(2, SECOND_TRIP_GROUP, 8192, 0)],
    "misaligned_base": [(n, 9, shots, off) for off in (1, 8) for n, shots in ((2, 1000), (8, 40), (3, 1000), (5, 1000))],
}
CASES = list(dict.fromkeys(case for block in BLOCKS.values() for case in block))     # (3 | 5, 9, 16, 0) is in two blocks
MAX_CASE_BYTES = 70_000_000


def case_bytes(case):
    n, S, shots, _ = case
    return n * S * shots


def case_id(case):
    n, S, shots, off = case
    return f"{route(*case).label}-n{n}-S{S}-shots{shots}" + (f"-off{off}" if off else "")


def case_seed(case):
    return zlib.crc32(repr(tuple(case)).encode())


# ---------------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------------
BIASES = (0.0, 0.03, 0.5, 0.97, 1.0)                        # P(bit 0 = 1) of setting s is BIASES[s % 5]
MASK_BYTES = np.array([0, 1, 2, 255], dtype=np.uint8)
MASK_ROWS = ("all", "random", "first", "zero", "last", "random", "random")      # the row of setting s is MASK_ROWS[s % 7]


def make(case, seed=None):
    """bits [S, shots, n] uint8, masks [S, n] uint8, coefs [S] float64 for one case.

    bits: every byte carries seven random high bits; bit 0 is 1 with the setting's bias, drawn independently for every record (no
    tiling, so a record never equals the one a grid's width before it).  Settings 0 and 4 (mod 35) have a mask that makes the count
    saturate: all columns at bias 0 (n_minus = 0), the last column alone at bias 1 (n_minus = shots).
    masks: all non-zero / random / first column only / all zero / last column only, by s mod 7; non-zero bytes are 1, 2 or 255.  The
    zero row is the fourth so that, a grid's width later (16384 = 4 and 4096 = 1 mod 7, 4 and 1 mod 5), a one-column record at bias
    0.5 has a non-zero mask where the setting it would inherit a stale mask from has none.
    coefs: uniform in [-2, 2] with an exact 1 at setting 1 and an exact 0 at setting 2 (where there are that many settings)."""
    n, S, shots, _ = case
    rng = np.random.default_rng(case_seed(case) if seed is None else seed)
    thr = np.array([round(p * 65536) for p in BIASES], dtype=np.int64)[np.arange(S) % len(BIASES)]
    bits = np.empty((S, shots, n), dtype=np.uint8)
    step = max(1, (1 << 22) // (shots * n))                 # settings per piece: bounded scratch for the 67 MB cases
    for s0 in range(0, S, step):
        s1 = min(S, s0 + step)
        shape = (s1 - s0, shots, n)
        t = thr[s0:s1, None, None]
        low = (rng.integers(0, 65536, size=shape, dtype=np.uint16) < np.minimum(t, 65535).astype(np.uint16)) | (t == 65536)
        bits[s0:s1] = (rng.integers(0, 256, size=shape, dtype=np.uint8) & 0xFE) | low
    nonzero = MASK_BYTES[1:]
    masks = MASK_BYTES[rng.integers(0, 4, size=(S, n))]
    kind = np.arange(S) % len(MASK_ROWS)
    for k, name in enumerate(MASK_ROWS):
        rows = np.flatnonzero(kind == k)
        if name == "all":
            masks[rows] = nonzero[rng.integers(0, 3, size=(rows.size, n))]
        elif name == "zero":
            masks[rows] = 0
        elif name in ("first", "last"):
            masks[rows] = 0
            masks[rows, 0 if name == "first" else n - 1] = nonzero[rng.integers(0, 3, size=rows.size)]
    coefs = rng.uniform(-2.0, 2.0, size=S)
    if S > 1:
        coefs[1] = 1.0
    if S > 2:
        coefs[2] = 0.0
    return bits, masks, coefs


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def count_minus(bits, masks):
    """int64 [S]: the shots whose masked bits have odd parity, ((bits & 1) & (masks != 0)).sum(axis=2) & 1 summed over the shots
    (column by column: the sum over a last axis of 1..8 entries is numpy's slowest loop)"""
    bits, masks = np.asarray(bits), np.asarray(masks)
    S, shots, n = bits.shape
    ones = np.zeros((S, shots), dtype=np.uint8)             # at most 64 ones per shot
    for q in range(n):
        ones += (bits[:, :, q] & 1) & (masks[:, q] != 0)[:, None]
    return (ones & 1).sum(axis=1, dtype=np.int64)


def moments_of_count(n_minus, shots, prior):
    """exact (m, v) for coefficient 1: ((n+ - n-) / shots, (1 - m^2) / shots), or 2 E - 1 and 4 Var of Beta(n+ + 1, n- + 1)"""
    n_plus = shots - n_minus
    if prior:
        a, b = n_plus + 1, n_minus + 1
        return 2 * Fraction(a, a + b) - 1, 4 * Fraction(a * b, (a + b) ** 2 * (a + b + 1))
    m = Fraction(n_plus - n_minus, shots)
    return m, (1 - m * m) / shots


def exact(bits, masks, coefs=None, prior=False, n_minus=None):
    """(mean [S], var [S], n_minus [S]): integer counts, moments in exact rationals of the double coefficients, one rounding each
    (n_minus: the counts of an earlier call on the same bits and masks, to spare the pass over the bytes)"""
    bits, masks = np.asarray(bits), np.asarray(masks)
    S, shots, _ = bits.shape
    n_minus = count_minus(bits, masks) if n_minus is None else n_minus
    identity = ~(masks != 0).any(axis=1)
    table = {int(k): moments_of_count(int(k), shots, prior) for k in np.unique(n_minus)}
    mean, var = np.empty(S), np.empty(S)
    for s in range(S):
        c = Fraction(1) if coefs is None else Fraction(float(coefs[s]))
        m, v = (Fraction(1), Fraction(0)) if identity[s] else table[int(n_minus[s])]
        mean[s], var[s] = float(c * m), float(c * c * v)
    return mean, var, n_minus
