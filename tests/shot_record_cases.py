"""The edges of the record walk of qv_count_record (csrc/fbx_qvolume.hip) and rpe_count_record (csrc/fbx_rpe.hip) as a table of
shapes, shared by the readers of shot records that have no table of their own: fbx_qv_count_heavy[_dev] and
fbx_rpe_from_shots[_dev] (tests/test_shot_records_gpu.py runs it, tests/test_shot_record_cases_cpu.py checks that it reaches what
it names).  tests/shots_cases.py and tests/test_bit_histogram_gpu.py cover the same edges for fbx_shots_to_moments and
fbx_bit_histogram.

A record is [n_shots][width] bytes of which only bit 0 counts.  Both readers take runs of S shots as 16-byte vectors from the
first shot on a 16-byte boundary and read the shots around the runs byte-wise; a wavefront owns a record below WAVE_BYTES when
there are at least four records, else a workgroup; the grid is capped, so past GRID_WAVEFRONTS records a wavefront takes a second.
Nothing here is the kernels' algorithm: the expected counts come from qv_cases.count_heavy_direct and rpe_cases.moments_from_shots."""
import math

import numpy as np

WAVE_BYTES = 16384                      # FBX_RECORD_WAVE_BYTES (csrc/fbx_common.hpp)
WAVES_PER_GROUP = 4
GRID_CAP = 256 * 16
GRID_WAVEFRONTS = WAVES_PER_GROUP * GRID_CAP
SECOND_TRIP = GRID_WAVEFRONTS + 5       # five wavefronts take a second record

SHOTS = (1, 15, 16, 17, 33)             # no run; a head only; one run and no tail; a run and a one-shot tail; (S = 16 at an aligned base)
BATCHES = (1, 3, 4, 5)                  # a workgroup per record (fewer than four), a wavefront per record, a workgroup's fifth record
QV_WIDTHS = (2, 3, 8, 9, 13)
RPE_WIDTHS = (1, 2, 3, 4, 5, 6, 8)      # every class of gcd(width, 16), so every run length S = 16 / gcd of the RPE reader
QV_SWITCH = (2, (8191, 8192), 4)        # width, shots on either side of WAVE_BYTES, records
QV_SECOND_TRIP = (2, 16, SECOND_TRIP)   # width, shots, records: 0.5 MB
RPE_SECOND_TRIP = (1, 16, SECOND_TRIP)  # K = 1


def run_shots(width, reader):
    """shots per run: 16 for the readers that take 16 shots whatever the width, the shortest whole-vector run for RPE"""
    return 16 // math.gcd(width, 16) if reader == "rpe" else 16


def edge_cases(widths):
    """(width, n_shots, B) over SHOTS x BATCHES for every width"""
    return [(n, shots, B) for n in widths for shots in SHOTS for B in BATCHES]


def record_starts(width, n_shots, B, base_offset=0):
    """the byte address of every record, relative to a 16-byte aligned allocation"""
    return [base_offset + b * n_shots * width for b in range(B)]


def head_of(start, width, n_shots):
    """the shots a reader takes byte-wise in front of the runs of a record at byte address `start`"""
    for s in range(16):
        if (start + s * width) % 16 == 0:
            return min(s, n_shots)
    return n_shots


def random_bytes(rng, shape):
    """uint8 with seven random high bits in every byte: only bit 0 is the outcome"""
    return rng.integers(0, 256, size=shape, dtype=np.uint8)


def heavy_tables(rng, B, width):
    """boolean [B, 2^width]: random membership; record 0 has an empty heavy set, record 1 (if any) everything but output 0"""
    heavy = rng.integers(0, 2, size=(B, 1 << width)).astype(bool)
    heavy[0] = False
    if B > 1:
        heavy[1] = True
        heavy[1, 0] = False
    return heavy
