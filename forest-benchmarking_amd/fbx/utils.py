"""Small host-side helpers under the reference's names (forest/benchmarking/utils.py), and the histogram of measured bitstrings
that the readout, adder and GHZ analyses share (``fbx_bit_histogram``; the counting runs on the device)."""
import ctypes as C
import itertools
from typing import Sequence

import numpy as np


def transform_pauli_moments_to_bit(mean_p, var_p):
    """Mean and variance of a Pauli observable (on [-1, 1]) -> those of the bit it is read from (on [0, 1]); utils.py:431-443."""
    return (np.asarray(mean_p) + 1) / 2, np.asarray(var_p) / 4


def transform_bit_moments_to_pauli(mean_c, var_c):
    """Mean and variance of a bit (on [0, 1]) -> those of the Pauli observable (on [-1, 1]); utils.py:446-458."""
    return 2 * np.asarray(mean_c) - 1, 4 * np.asarray(var_c)


def bit_array_to_int(bit_array: Sequence[int]) -> int:
    """A bit array -> the integer it spells, the right-most bit least significant; utils.py:32-42."""
    output = 0
    for bit in bit_array:
        output = (output << 1) | int(bit)
    return output


def int_to_bit_array(num: int, n_bits: int) -> Sequence[int]:
    """An integer -> its ``n_bits`` bits, the right-most bit least significant; utils.py:45-53."""
    return [num >> bit & 1 for bit in range(n_bits - 1, -1, -1)]


def all_bitstrings(n: int) -> np.ndarray:
    """``[2^n, n]`` uint8: every bitstring of length n in ``itertools.product([0, 1], repeat=n)`` order (row r spells r)."""
    if n < 0:
        raise ValueError("n must not be negative")
    return np.array(list(itertools.product((0, 1), repeat=n)), dtype=np.uint8).reshape(1 << n, n)


_KINDS = {"joint": 0, "weight": 1}


def _u8(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))


def _as_bits(bitarrays):
    bits = np.asarray(bitarrays)
    if bits.ndim != 3:
        raise ValueError("bitarrays must be [B, n_shots, n_cols]")
    if bits.dtype != np.uint8:
        if bits.size and (bits.min() < 0 or bits.max() > 1):
            raise ValueError("bitarrays must hold 0 / 1")
        bits = bits.astype(np.uint8)
    return np.ascontiguousarray(bits)


def bitstring_histogram_batch(bitarrays, cols=None, expected=None, kind: str = "joint", frequencies: bool = False):
    """``bitarrays [B, n_shots, n_cols]`` (0/1 as ``qc.run`` returns them; of a uint8 array only bit 0 of every byte is read)
    -> ``counts [B, bins]`` int64, one launch for the batch.

    ``cols``: the k columns that form the bitstring, in any order -- ``[k]`` for the whole batch or ``[B, k]`` per record; ``None``
    = all columns in order.  ``expected``: ``[B, k]`` (or ``[k]``, repeated) of 0/1 XORed onto the selected bits.  ``kind="joint"``:
    ``2^k`` bins, k <= 10, bin = the integer the selected bits spell with the first selected column most significant
    (``bit_array_to_int``); ``kind="weight"``: ``k + 1`` bins, k <= 64, bin = the Hamming weight of the selected bits after the XOR.
    With ``frequencies=True`` returns ``(counts, counts / n_shots)``, the division on the device too."""
    from . import _lib
    if kind not in _KINDS:
        raise ValueError("kind must be 'joint' or 'weight'")
    bits = _as_bits(bitarrays)
    B, n_shots, n_cols = bits.shape
    shared, c = 1, None
    if cols is not None:
        c = np.ascontiguousarray(np.asarray(cols), dtype=np.int64)
        if c.ndim not in (1, 2) or (c.ndim == 2 and c.shape[0] != B) or c.shape[-1] < 1:
            raise ValueError("cols must be [k] or [B, k]")
        if c.size and (c.min() < 0 or c.max() >= n_cols):
            raise ValueError("cols holds a column that is not in 0..n_cols - 1")
        shared = int(c.ndim == 1)
        c = np.ascontiguousarray(c, dtype=np.uint8)
    k = n_cols if c is None else c.shape[-1]
    e = None
    if expected is not None:
        e = np.asarray(expected)
        if e.shape not in ((k,), (B, k)):
            raise ValueError("expected must be [k] or [B, k]")
        if e.size and (e.min() < 0 or e.max() > 1):
            raise ValueError("expected must hold 0 / 1")
        e = np.ascontiguousarray(np.broadcast_to(e, (B, k)), dtype=np.uint8)
    bins = (1 << k) if kind == "joint" and 1 <= k <= _lib.HIST_MAX_JOINT_K else k + 1
    counts = np.zeros((B, bins), dtype=np.int64)
    lib = _lib.lib()
    _lib.check(lib.fbx_bit_histogram(n_cols, B, n_shots, _u8(bits), k, _u8(c), shared, _u8(e), _KINDS[kind],
                                     counts.ctypes.data_as(C.POINTER(C.c_int64))))
    if not frequencies:
        return counts
    return counts, counts_to_frequencies(counts, n_shots)


def counts_to_frequencies(counts, denom: int) -> np.ndarray:
    """``counts / denom`` element by element on the device (``fbx_counts_to_frequencies``): int64 in, float64 out."""
    from . import _lib
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    out = np.zeros(counts.shape, dtype=np.float64)
    _lib.check(_lib.lib().fbx_counts_to_frequencies(counts.size, counts.ctypes.data_as(C.POINTER(C.c_int64)), int(denom),
                                                    _lib.dptr(out)))
    return out
