"""``ghz_state_statistics`` (forest/benchmarking/entangled_states.py:36-51) from measured bitstrings: the number of shots that are
all zeros or all ones.  Those are bins 0 and n of the weight-kind histogram of ``fbx_bit_histogram``, counted on the device.  The
program builders (``create_ghz_program``, the graph-state functions) are not mirrored."""
import numpy as np

from .utils import bitstring_histogram_batch

__all__ = ["ghz_state_statistics", "ghz_state_statistics_batch"]


def ghz_state_statistics_batch(bitstrings) -> dict:
    """``bitstrings [B, n_shots, n]`` -> ``{'bell': [B] int64, 'total': [B] int64}``; one launch."""
    bits = np.asarray(bitstrings)
    if bits.ndim != 3:
        raise ValueError("bitstrings must be [B, n_shots, n]")
    counts = bitstring_histogram_batch(bits, kind="weight")
    bell = counts[:, 0] + (counts[:, -1] if bits.shape[2] > 0 else 0)
    return {"bell": bell, "total": np.full(bits.shape[0], bits.shape[1], dtype=np.int64)}


def ghz_state_statistics(bitstrings) -> dict:
    """entangled_states.py:36-51: ``{'bell': shots consistent with a Bell / GHZ state, 'total': shots}`` as ints."""
    res = ghz_state_statistics_batch(np.asarray(bitstrings)[None])
    return {"bell": int(res["bell"][0]), "total": int(res["total"][0])}
