"""Quantum volume (forest/benchmarking/quantum_volume.py) without the acquisition: model circuits, their ideal heavy outputs, the
heavy-hitter counts of measured bitstrings and the statistics that turn the counts into a quantum volume.

What runs where:
  * ``collect_heavy_outputs[_batch]`` / ``ideal_heavy_output_probability_batch`` -- ``fbx_qv_heavy_outputs``: a state-vector
    simulation of B circuits of one width in one launch, the state in LDS, widths 2..13 (wider: ``FbxError(FBX_ERR_UNSUPPORTED)``;
    there is no host fallback);
  * ``heavy_outputs_flat_wide`` / ``collect_heavy_outputs_wide_batch`` / ``ideal_heavy_output_probability_wide_batch`` /
    ``count_heavy_hitters_sampled_wide_batch`` -- the same results for widths 2..26 through one call: widths up to 13 go to the
    entry points above unchanged, widths 14..26 to ``fbx_qv_heavy_outputs_wide`` / ``fbx_qv_count_heavy_wide`` (the state in device
    memory, a tile of ``2^tile_bits`` amplitudes at a time in LDS).  ``plan_wide_passes`` is the numpy mirror
    of the device planner that cuts a circuit into passes (``fbx_qv_wide_plan`` returns the device's decisions);
  * ``count_heavy_hitters_sampled[_batch]`` -- ``fbx_qv_count_heavy``: a streaming reduction of the ``qc.run`` bit arrays;
  * ``simulate_heavy_output_counts_batch`` -- a simulated run resident on the device: ``fbx_qv_heavy_outputs_dev`` ->
    ``fbx_sample_bitstrings_dev`` (noisy measured bitstrings from the ideal distributions) -> ``fbx_qv_count_heavy_dev``;
  * ``simulate_heavy_output_counts_wide_batch`` -- the same run for widths 2..26: up to 13 it IS the function above, from 14 on
    ``fbx_qv_heavy_outputs_wide_dev`` -> ``fbx_sample_bitstrings_wide_dev`` -> ``fbx_qv_count_heavy_wide_dev`` on slices of circuits
    that keep the resident probabilities and shots under a cap;
  * ``noisy_trajectories_flat`` / ``noisy_heavy_output_probability_batch`` -- ``fbx_qv_noisy_trajectories``: the same circuits
    under gate noise, as stochastic Pauli-error trajectories (after every gate, with that gate's error probability, one of the 15
    two-qubit Paulis on its pair), widths 2..13, the Pauli folded into the gate's own pass over the state.
    ``simulate_noisy_heavy_output_counts_batch`` is the resident run under that noise.  ``fold_gate_errors`` multiplies the Paulis
    of one trajectory (``synthetic.restate_qv_gate_errors`` restates the device's draws) into the gates: the trajectory is then an
    ordinary circuit for every entry point above, the ``_wide`` ones included -- noisy trajectories of widths 14..26 exist by
    composition, one circuit per trajectory, without a kernel of their own;
  * ``generate_abstract_qv_circuit`` -- host numpy with the reference's draw order (a run seeded with ``np.random.seed`` reproduces
    the reference's circuit); ``generate_abstract_qv_circuits_batch`` -- gates from the device generator;
  * ``calculate_prob_est_and_err``, ``get_prob_sample_heavy_by_depth``, ``extract_quantum_volume_from_results`` -- host arithmetic.

``measure_quantum_volume``, ``sample_rand_circuits_for_heavy_out`` and the program generator need a pyquil ``QuantumComputer`` and
a compiler and are not mirrored.

Conventions (quantum_volume.py:113-115): output index i has qubit 0 as its most significant bit; a gate on ``(q0, q1)`` has q0 as
the more significant bit of its 4 x 4 matrix index.  ``pairing="reference"`` is the reference's rule: gate g of a layer acts on
``(perm[g], perm[g + 1])`` -- consecutive gates of a layer overlap on one qubit, so their order matters and is kept.
``pairing="disjoint"`` is the layout of the paper (arXiv:1811.12926), ``(perm[2 g], perm[2 g + 1])``; a deviation from the
reference, offered because it is what the protocol describes.  For odd widths the last position is idle in both.
"""
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from .operator_tools.random_operators import _stream_seed, haar_rand_unitary

__all__ = ["generate_abstract_qv_circuit", "generate_abstract_qv_circuits_batch", "collect_heavy_outputs",
           "collect_heavy_outputs_batch", "ideal_heavy_output_probability_batch", "count_heavy_hitters_sampled",
           "count_heavy_hitters_sampled_batch", "calculate_prob_est_and_err", "get_prob_sample_heavy_by_depth",
           "extract_quantum_volume_from_results", "layer_pairs", "pack_heavy_mask", "unpack_heavy_mask", "heavy_outputs_flat",
           "simulate_heavy_output_counts_batch", "heavy_outputs_flat_wide", "collect_heavy_outputs_wide_batch",
           "ideal_heavy_output_probability_wide_batch", "count_heavy_hitters_sampled_wide_batch", "plan_wide_passes",
           "simulate_heavy_output_counts_wide_batch", "noisy_trajectories_flat", "noisy_heavy_output_probability_batch",
           "fold_gate_errors", "simulate_noisy_heavy_output_counts_batch"]

MIN_WIDTH, MAX_WIDTH = 2, 13
MIN_WIDE_WIDTH, MAX_WIDE_WIDTH = 14, 26                  # fbx_qv_*_wide
WIDE_DEFAULT_TILE_BITS, WIDE_LOW_BITS = 13, 3


# ------------------------------------------------------------------------------------------------ circuits
def generate_abstract_qv_circuit(depth: int) -> Tuple[List[np.ndarray], np.ndarray]:
    """quantum_volume.py:126-151: depth permutations of range(depth), then depth x depth // 2 Haar 4 x 4 gates, drawn from numpy's
    global stream in the reference's order (all permutations first, then the gates layer by layer)."""
    permutations = [np.random.permutation(range(depth)) for _ in range(depth)]
    gates = np.asarray([[haar_rand_unitary(4) for _ in range(depth // 2)] for _ in range(depth)])
    return permutations, gates


def generate_abstract_qv_circuits_batch(depth: int, batch: int, seed: Optional[int] = None, first_item: int = 0):
    """``batch`` model circuits of one depth: ``permutations [B, depth, depth]`` (int64, from ``np.random.default_rng`` keyed by
    the stream seed and the circuit's global id ``first_item + b``) and ``gates [B, depth, depth // 2, 4, 4]`` from
    ``fbx_random_operators`` (Haar unitaries; gate j of circuit b is device item ``(first_item + b) * depth * (depth // 2) + j``).
    A circuit depends on (seed, its id) only, not on the batch.  Parity with the reference is distributional."""
    depth, batch, first_item = int(depth), int(batch), int(first_item)
    if depth < 2 or batch < 0 or first_item < 0:
        raise ValueError("generate_abstract_qv_circuits_batch: need depth >= 2, batch >= 0 and first_item >= 0")
    from . import _lib
    key = _stream_seed(seed)
    per = depth * (depth // 2)
    perms = np.empty((batch, depth, depth), dtype=np.int64)
    for b in range(batch):
        rng = np.random.default_rng([key & 0xFFFFFFFF, key >> 32, first_item + b])
        for layer in range(depth):
            perms[b, layer] = rng.permutation(depth)
    gates = np.empty((batch, depth, depth // 2, 4, 4), dtype=np.complex128)
    if batch:
        _lib.check(_lib.lib().fbx_random_operators(_lib.RAND_UNITARY, 4, 0, batch * per, key, first_item * per,
                                                   _lib.dptr(gates.view(np.float64))))
    return perms, gates


def layer_pairs(permutations, pairing: str = "reference") -> np.ndarray:
    """``[..., depth, width]`` permutations -> ``[..., depth, width // 2, 2]`` qubit pairs (uint8) of every gate, in the order of
    application.  ``reference``: ``(perm[g], perm[g + 1])`` (quantum_volume.py:55, :113); ``disjoint``: ``(perm[2 g], perm[2 g + 1])``."""
    perms = np.asarray(permutations)
    if perms.ndim < 2 or not np.issubdtype(perms.dtype, np.integer):
        raise ValueError("permutations must be an integer array [..., depth, width]")
    width = perms.shape[-1]
    g = np.arange(width // 2)
    if pairing == "reference":
        first, second = g, g + 1
    elif pairing == "disjoint":
        first, second = 2 * g, 2 * g + 1
    else:
        raise ValueError(f"pairing must be 'reference' or 'disjoint', not {pairing!r}")
    if perms.size and (perms.min() < 0 or perms.max() >= width or np.any(np.sort(perms, axis=-1) != np.arange(width))):
        raise ValueError("every row of permutations must be a permutation of range(width)")
    return np.stack([perms[..., first], perms[..., second]], axis=-1).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ masks
def _mask_words(n_qubits: int) -> int:
    return max(1, (1 << n_qubits) // 64)


def pack_heavy_mask(heavy) -> np.ndarray:
    """boolean table ``[B, 2^n]`` -> ``[B, W]`` uint64, W = max(1, 2^n / 64): output i is bit i % 64 of word i // 64"""
    heavy = np.asarray(heavy, dtype=bool)
    if heavy.ndim != 2 or heavy.shape[1] < 4 or heavy.shape[1] & (heavy.shape[1] - 1):
        raise ValueError("heavy must be a boolean table [B, 2^n] with n >= 2")
    B, N = heavy.shape
    padded = np.zeros((B, max(N, 64)), dtype=np.uint8)
    padded[:, :N] = heavy
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").astype(np.uint64).reshape(B, max(N, 64) // 64)


def unpack_heavy_mask(mask, n_qubits: int) -> np.ndarray:
    """the inverse of ``pack_heavy_mask``: ``[B, W]`` uint64 -> boolean ``[B, 2^n]``"""
    mask = np.ascontiguousarray(mask, dtype=np.uint64)
    if mask.ndim != 2 or mask.shape[1] != _mask_words(n_qubits):
        raise ValueError(f"mask must be [B, {_mask_words(n_qubits)}] for {n_qubits} qubits")
    bits = np.unpackbits(mask.astype("<u8").view(np.uint8).reshape(mask.shape[0], 8 * mask.shape[1]), axis=1, bitorder="little")
    return bits[:, :1 << n_qubits].astype(bool)


# ------------------------------------------------------------------------------------------------ heavy outputs
def _heavy_outputs(entry, n, pairs, gates, probabilities, median, mask, heavy_prob, heavy_count, tile_bits=None):
    """Validation and marshalling of ``heavy_outputs_flat`` (``entry`` = "fbx_qv_heavy_outputs") and of ``heavy_outputs_flat_wide``
    past 13 qubits ("fbx_qv_heavy_outputs_wide", which takes ``tile_bits`` after the gates)."""
    wide = tile_bits is not None
    pairs = np.asarray(pairs)
    gates = np.asarray(gates)
    if pairs.ndim != 3 or pairs.shape[2] != 2:
        raise ValueError("pairs must be [B, L, 2]")
    B, L = pairs.shape[:2]
    if gates.shape != (B, L, 4, 4):
        raise ValueError(f"gates must be [B, L, 4, 4] = {(B, L, 4, 4)}, not {gates.shape}")
    if not (probabilities or median or mask or heavy_prob or heavy_count):
        raise ValueError("no output asked for")
    if not wide:                                         # the narrow path casts first: its checks see what the library will
        if pairs.size and (pairs.min() < 0 or pairs.max() > 255):
            raise ValueError("qubit indices must be 0..255")
        pairs = np.ascontiguousarray(pairs, dtype=np.uint8)
    if n >= 1 and pairs.size:
        if pairs.min() < 0 or pairs.max() >= n:
            raise ValueError(f"a qubit index is out of range for {n} qubits")
        if np.any(pairs[..., 0] == pairs[..., 1]):
            raise ValueError("a gate needs two different qubits")
    pairs = np.ascontiguousarray(pairs, dtype=np.uint8)
    from . import _lib
    import ctypes as C
    gates = _lib.c128(gates)
    N, W = 1 << max(n, 0), _mask_words(max(n, 0))
    ok = wide or MIN_WIDTH <= n <= MAX_WIDTH             # (outside, the library refuses before it touches a buffer)
    out = {}
    if probabilities:
        out["probabilities"] = np.empty((B, N if ok else 0))
    if median:
        out["median"] = np.empty(B)
    if mask:
        out["mask"] = np.zeros((B, W if ok else 0), dtype=np.uint64)
    if heavy_prob:
        out["heavy_prob"] = np.empty(B)
    if heavy_count:
        out["heavy_count"] = np.empty(B, dtype=np.int32)
    _lib.check(getattr(_lib.lib(), entry)(
        n, B, L, pairs.ctypes.data_as(C.POINTER(C.c_uint8)), _lib.dptr(gates.view(np.float64)), *((tile_bits,) if wide else ()),
        _lib.dptr(out.get("probabilities")), _lib.dptr(out.get("median")),
        out["mask"].ctypes.data_as(C.POINTER(C.c_uint64)) if mask else None,
        _lib.dptr(out.get("heavy_prob")), _lib.iptr(out.get("heavy_count"))))
    return out


def heavy_outputs_flat(n_qubits: int, pairs, gates, probabilities=True, median=True, mask=True, heavy_prob=True, heavy_count=True):
    """``fbx_qv_heavy_outputs`` on flat gate lists: ``pairs [B, L, 2]`` (q0, q1) and ``gates [B, L, 4, 4]``, applied in order.
    Returns a dict with the outputs asked for: ``probabilities [B, 2^n]``, ``median [B]``, ``mask [B, W]`` (uint64), ``heavy_prob [B]``,
    ``heavy_count [B]`` (int32)."""
    return _heavy_outputs("fbx_qv_heavy_outputs", int(n_qubits), pairs, gates, probabilities, median, mask, heavy_prob, heavy_count)


def _flatten_circuits(permutations, gates, pairing):
    perms = np.asarray(permutations)
    gates = np.asarray(gates)
    if perms.ndim != 3:
        raise ValueError("permutations must be [B, depth, width]")
    B, depth, width = perms.shape
    if gates.shape != (B, depth, width // 2, 4, 4):
        raise ValueError(f"gates must be [B, depth, width // 2, 4, 4] = {(B, depth, width // 2, 4, 4)}, not {gates.shape}")
    pairs = layer_pairs(perms, pairing)
    return width, pairs.reshape(B, depth * (width // 2), 2), gates.reshape(B, depth * (width // 2), 4, 4)


def _collected(r, width, return_probabilities, return_stats):
    """What ``collect_heavy_outputs_batch`` returns, from the dict ``r`` of ``heavy_outputs_flat``."""
    res = [unpack_heavy_mask(r["mask"], width)]
    if return_probabilities:
        res.append(r["probabilities"])
    if return_stats:
        res.append({k: r[k] for k in ("median", "heavy_prob", "heavy_count")})
    return res[0] if len(res) == 1 else tuple(res)


def collect_heavy_outputs_batch(permutations, gates, pairing: str = "reference", return_probabilities: bool = False,
                                return_stats: bool = False):
    """The heavy outputs of B model circuits of one width in one launch: ``permutations [B, depth, width]``,
    ``gates [B, depth, width // 2, 4, 4]`` -> the boolean heavy table ``[B, 2^width]``; with ``return_probabilities`` also the ideal
    output distribution ``[B, 2^width]``; with ``return_stats`` also a dict of ``median``, ``heavy_prob`` and ``heavy_count`` ([B] each)."""
    width, pairs, flat = _flatten_circuits(permutations, gates, pairing)
    r = heavy_outputs_flat(width, pairs, flat, probabilities=return_probabilities, median=return_stats, mask=True,
                           heavy_prob=return_stats, heavy_count=return_stats)
    return _collected(r, width, return_probabilities, return_stats)


def ideal_heavy_output_probability_batch(permutations, gates, pairing: str = "reference") -> np.ndarray:
    """``[B]``: the probability that an ideal device outputs a heavy bitstring of each circuit (the number a measured heavy
    fraction is compared with; (1 + ln 2) / 2 on average for wide random circuits)."""
    width, pairs, flat = _flatten_circuits(permutations, gates, pairing)
    return heavy_outputs_flat(width, pairs, flat, probabilities=False, median=False, mask=False, heavy_prob=True,
                              heavy_count=False)["heavy_prob"]


def collect_heavy_outputs(wfn_sim, permutations, gates) -> List[int]:
    """quantum_volume.py:94-123 with the reference's signature; ``wfn_sim`` is accepted and ignored (may be ``None``): the
    simulation runs on the device.  Returns the sorted list of heavy outputs as ints."""
    perms = np.asarray([np.asarray(p) for p in permutations])
    heavy = collect_heavy_outputs_batch(perms[None], np.asarray(gates)[None])
    return [int(i) for i in np.flatnonzero(heavy[0])]


# ------------------------------------------------------------------------------------------------ counts
def _count_heavy_hitters(entry, bitarrays, heavy) -> np.ndarray:
    """Validation and marshalling of the heavy-hitter count: ``entry`` = "fbx_qv_count_heavy" or "fbx_qv_count_heavy_wide"."""
    bits = np.asarray(bitarrays)
    if bits.ndim != 3:
        raise ValueError("bitarrays must be [B, shots, n_qubits]")
    B, shots, n = bits.shape
    mask = _heavy_masks(heavy, B, n)
    if bits.size and (bits.min() < 0 or bits.max() > 1):
        raise ValueError("bitarrays must hold 0 / 1")
    bits = np.ascontiguousarray(bits, dtype=np.uint8)
    from . import _lib
    import ctypes as C
    counts = np.zeros(B, dtype=np.int64)
    _lib.check(getattr(_lib.lib(), entry)(n, B, shots, bits.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          mask.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          counts.ctypes.data_as(C.POINTER(C.c_int64))))
    return counts


def count_heavy_hitters_sampled_batch(bitarrays, heavy) -> np.ndarray:
    """``bitarrays [B, shots, n]`` (0/1, first column = qubit 0, as ``qc.run`` returns them) and ``heavy`` -- the boolean table
    ``[B, 2^n]`` or the packed masks ``[B, W]`` (uint64) -- -> the number of heavy shots of every circuit, ``[B]`` int64."""
    return _count_heavy_hitters("fbx_qv_count_heavy", bitarrays, heavy)


def count_heavy_hitters_sampled(qc_results: Iterator[np.ndarray], heavy_hitters: Iterator[List[int]]) -> Iterator[int]:
    """quantum_volume.py:322-341 with the reference's signature: per circuit the measured bit array and the list of heavy outputs;
    yields the number of heavy shots of each.  Circuits of one (width, shot count) go to the device as one batch."""
    results = [np.asarray(r) for r in qc_results]
    lists = [list(h) for h in heavy_hitters]
    m = min(len(results), len(lists))                        # zip semantics
    results, lists = results[:m], lists[:m]
    counts = [0] * m
    by_shape: Dict[Tuple[int, int], List[int]] = {}
    for i, r in enumerate(results):
        if r.ndim != 2:
            raise ValueError("every result must be a [shots, n_qubits] bit array")
        by_shape.setdefault(r.shape, []).append(i)
    for (shots, n), idx in by_shape.items():
        table = np.zeros((len(idx), 1 << n), dtype=bool)
        for row, i in enumerate(idx):
            table[row, np.asarray(lists[i], dtype=np.int64)] = True
        got = count_heavy_hitters_sampled_batch(np.stack([results[i] for i in idx]), table)
        for row, i in enumerate(idx):
            counts[i] = int(got[row])
    yield from counts


# ------------------------------------------------------------------------------------------------ widths 14..26
def _check_wide(n: int, tile_bits: int, who: str) -> int:
    from . import _lib
    if not MIN_WIDTH <= n <= MAX_WIDE_WIDTH:
        raise _lib.FbxError(_lib.FBX_ERR_UNSUPPORTED, f"{who}: width must be {MIN_WIDTH}..{MAX_WIDE_WIDTH} (got {n}); there is no "
                                                      f"host fallback")
    tile_bits = int(tile_bits)
    if tile_bits != 0 and not 8 <= tile_bits <= 13:
        raise ValueError(f"{who}: tile_bits must be 0 (the default) or 8..13")
    return tile_bits


def plan_wide_passes(n_qubits: int, pairs, tile_bits: int = 0):
    """The pass plan of ``fbx_qv_heavy_outputs_wide``, restated in numpy (``fbx_qv_wide_plan`` must agree integer for integer).
    ``pairs [L, 2]`` or ``[B, L, 2]`` -> ``(n_passes, first_gate, local_mask)``: int32 ``[B]``, int32 ``[B, L + 1]`` and uint32
    ``[B, L]`` (without the leading axis for one circuit).  Pass k applies gates ``first_gate[k] .. first_gate[k + 1] - 1`` with the
    index bits of ``local_mask[k]`` local (bit p = index bit p = qubit ``n - 1 - p``); entries past the last pass are L and 0.

    The rule: index bits 0..2 are always local (8 amplitudes = 128 B contiguous in device memory).  A pass takes gates in order
    while their targets that are not yet local still fit into the ``tile_bits - 3`` free places, and stops at the first gate
    that does not (no reordering).  Places still free are filled with the lowest index bits not yet local."""
    n = int(n_qubits)
    T = int(tile_bits) or WIDE_DEFAULT_TILE_BITS
    if not MIN_WIDE_WIDTH <= n <= MAX_WIDE_WIDTH:
        raise ValueError(f"plan_wide_passes: n_qubits must be {MIN_WIDE_WIDTH}..{MAX_WIDE_WIDTH}")
    if not 8 <= T <= 13:
        raise ValueError("plan_wide_passes: tile_bits must be 0 (the default) or 8..13")
    pairs = np.asarray(pairs, dtype=np.int64)
    single = pairs.ndim == 2
    if single:
        pairs = pairs[None]
    if pairs.ndim != 3 or pairs.shape[2] != 2:
        raise ValueError("pairs must be [L, 2] or [B, L, 2]")
    if pairs.size and (pairs.min() < 0 or pairs.max() >= n or np.any(pairs[..., 0] == pairs[..., 1])):
        raise ValueError("a gate needs two different qubits below n_qubits")
    B, L = pairs.shape[:2]
    n_passes = np.zeros(B, dtype=np.int32)
    first = np.full((B, L + 1), L, dtype=np.int32)
    masks = np.zeros((B, L), dtype=np.uint32)
    low = (1 << WIDE_LOW_BITS) - 1
    for b in range(B):
        bits = [(1 << (n - 1 - int(q0)), 1 << (n - 1 - int(q1))) for q0, q1 in pairs[b]]
        k = l = 0
        while l < L:
            m, first[b, k] = low, l
            while l < L:
                grown = m | bits[l][0] | bits[l][1]
                if bin(grown).count("1") > T:
                    break
                m, l = grown, l + 1
            p = WIDE_LOW_BITS
            while bin(m).count("1") < T:
                m, p = m | (1 << p), p + 1
            masks[b, k] = m
            k += 1
        n_passes[b] = k
    return (n_passes[0], first[0], masks[0]) if single else (n_passes, first, masks)


def heavy_outputs_flat_wide(n_qubits: int, pairs, gates, probabilities=True, median=True, mask=True, heavy_prob=True,
                            heavy_count=True, tile_bits: int = 0):
    """``heavy_outputs_flat`` for widths 2..26: up to 13 it IS ``heavy_outputs_flat`` (``tile_bits`` is checked and unused); from 14
    on ``fbx_qv_heavy_outputs_wide`` with ``tile_bits`` (0 = the library's default, else 8..13; no result depends on it)."""
    n = int(n_qubits)
    tile_bits = _check_wide(n, tile_bits, "heavy_outputs_flat_wide")
    if n <= MAX_WIDTH:
        return heavy_outputs_flat(n, pairs, gates, probabilities, median, mask, heavy_prob, heavy_count)
    return _heavy_outputs("fbx_qv_heavy_outputs_wide", n, pairs, gates, probabilities, median, mask, heavy_prob, heavy_count, tile_bits)


def collect_heavy_outputs_wide_batch(permutations, gates, pairing: str = "reference", return_probabilities: bool = False,
                                     return_stats: bool = False, tile_bits: int = 0):
    """``collect_heavy_outputs_batch`` for widths 2..26 (``heavy_outputs_flat_wide``): the same arguments and return values."""
    width, pairs, flat = _flatten_circuits(permutations, gates, pairing)
    r = heavy_outputs_flat_wide(width, pairs, flat, probabilities=return_probabilities, median=return_stats, mask=True,
                                heavy_prob=return_stats, heavy_count=return_stats, tile_bits=tile_bits)
    return _collected(r, width, return_probabilities, return_stats)


def ideal_heavy_output_probability_wide_batch(permutations, gates, pairing: str = "reference", tile_bits: int = 0) -> np.ndarray:
    """``ideal_heavy_output_probability_batch`` for widths 2..26; from 14 on the probabilities stay in the device workspace."""
    width, pairs, flat = _flatten_circuits(permutations, gates, pairing)
    return heavy_outputs_flat_wide(width, pairs, flat, probabilities=False, median=False, mask=False, heavy_prob=True,
                                   heavy_count=False, tile_bits=tile_bits)["heavy_prob"]


def count_heavy_hitters_sampled_wide_batch(bitarrays, heavy, tile_bits: int = 0) -> np.ndarray:
    """``count_heavy_hitters_sampled_batch`` for widths 2..26 (from 14 on ``fbx_qv_count_heavy_wide``; ``tile_bits`` is accepted
    for symmetry with the other ``_wide`` functions and does not enter the count)."""
    bits = np.asarray(bitarrays)
    if bits.ndim != 3:
        raise ValueError("bitarrays must be [B, shots, n_qubits]")
    n = bits.shape[2]
    _check_wide(n, tile_bits, "count_heavy_hitters_sampled_wide_batch")
    if n <= MAX_WIDTH:
        return count_heavy_hitters_sampled_batch(bits, heavy)
    return _count_heavy_hitters("fbx_qv_count_heavy_wide", bits, heavy)


# ------------------------------------------------------------------------------------------------ simulated runs
def _simulate_counts_resident(wide, width, pairs, flat, shots, depolarizing, readout_flip, seed, tile_bits=0, max_resident_mib=None):
    """The resident chain of ``simulate_heavy_output_counts_batch`` and, with ``wide``, of its wide twin past 13 qubits: heavy
    outputs -> shots -> counts in slices of circuits whose probabilities (8 B x 2^n per circuit) and shot bytes stay under
    ``max_resident_mib`` (None: one slice, the narrow chain).  The slice that starts at circuit k is sampled with
    ``first_item = k``.  Only the wide heavy-outputs entry point takes ``tile_bits``; an item that cannot be sampled is reported
    under the wide function's name there and as the sampler reports it (the default of ``sampling._raise_poisoned``) here."""
    from . import _lib
    from .sampling import _noise, _raise_poisoned
    lib = _lib.lib()
    if wide:
        heavy_outputs, sample = lib.fbx_qv_heavy_outputs_wide_dev, lib.fbx_sample_bitstrings_wide_dev
        count = lib.fbx_qv_count_heavy_wide_dev
        tile, who = (tile_bits,), ("simulate_heavy_output_counts_wide_batch",)
    else:
        heavy_outputs, sample = lib.fbx_qv_heavy_outputs_dev, lib.fbx_sample_bitstrings_dev
        count = lib.fbx_qv_count_heavy_dev
        tile, who = (), ()
    B, L = pairs.shape[:2]
    N, W = 1 << width, _mask_words(width)
    shots, lam, flips, _ = _noise(B, width, shots, depolarizing, readout_flip)
    key = _stream_seed(seed)
    if B == 0:
        return np.zeros(0, dtype=np.int64), {"heavy_prob": np.zeros(0), "heavy_count": np.zeros(0, dtype=np.int32)}
    cut = B if max_resident_mib is None else int(max(1, min(B, max_resident_mib * 1048576.0 // (8 * N + shots * width))))
    with _lib.DeviceScope() as dev:
        d_pairs, d_gates = dev.upload(pairs), dev.upload(_lib.c128(flat))
        d_lam, d_flips = dev.upload(lam), dev.upload(flips)
        d_probs, d_mask = dev.alloc(8 * cut * N), dev.alloc(8 * cut * W)
        d_bits = dev.alloc(cut * shots * width)
        d_hp, d_hc, d_status, d_counts = dev.alloc(8 * B), dev.alloc(4 * B), dev.alloc(4 * B), dev.alloc(8 * B)
        for k in range(0, B, cut):
            cb = min(cut, B - k)
            _lib.check(heavy_outputs(width, cb, L, d_pairs.at(2 * L * k), d_gates.at(256 * L * k), *tile, d_probs.ptr, None,
                                     d_mask.ptr, d_hp.at(8 * k), d_hc.at(4 * k)))
            _lib.check(sample(width, cb, shots, d_probs.ptr, _lib.devptr(d_lam, 8 * k), _lib.devptr(d_flips, 16 * width * k), key, k,
                              d_bits.ptr, d_status.at(4 * k)))
            _lib.check(count(width, cb, shots, d_bits.ptr, d_mask.ptr, d_counts.at(8 * k)))
        counts = d_counts.to_array(np.int64, (B,))
        stats = {"heavy_prob": d_hp.to_array(np.float64, (B,)), "heavy_count": d_hc.to_array(np.int32, (B,))}
        if shots:
            _raise_poisoned(d_status.to_array(np.int32, (B,)), 0, *who)
    return counts, stats


def simulate_heavy_output_counts_batch(permutations, gates, shots: int, depolarizing=0.0, readout_flip=None,
                                       seed: Optional[int] = None, pairing: str = "reference"):
    """A simulated quantum-volume run of B model circuits of one width, resident on the device: ideal output distributions
    (``fbx_qv_heavy_outputs_dev``) -> ``shots`` noisy measured bitstrings per circuit (``fbx_sample_bitstrings_dev``: global
    depolarizing of strength ``depolarizing``, a scalar or ``[B]``, then readout flips ``[n, 2]`` or ``[B, n, 2]``, see
    ``sampling.sample_bitstrings_batch``) -> heavy-hitter counts (``fbx_qv_count_heavy_dev``).  The distributions and the
    ``B * shots * n`` bytes of shots never leave the device.

    Returns ``(counts [B] int64, stats)`` with ``stats["heavy_prob"]`` and ``stats["heavy_count"]`` of the ideal circuits: under
    depolarizing alone a shot of circuit b is heavy with probability ``(1 - lambda) heavy_prob_b + lambda heavy_count_b / 2^n``.
    Circuit b draws from item b of the Philox stream keyed by ``seed`` (``None``: a fresh key, the rule of ``random_operators``),
    so the counts equal those of the composed host calls on the same seed."""
    from . import _lib
    width, pairs, flat = _flatten_circuits(permutations, gates, pairing)
    if not MIN_WIDTH <= width <= MAX_WIDTH:
        raise _lib.FbxError(_lib.FBX_ERR_UNSUPPORTED, f"simulate_heavy_output_counts_batch: width must be {MIN_WIDTH}..{MAX_WIDTH} "
                                                      f"(got {width}); there is no host fallback")
    return _simulate_counts_resident(False, width, pairs, flat, shots, depolarizing, readout_flip, seed)


def simulate_heavy_output_counts_wide_batch(permutations, gates, shots: int, depolarizing=0.0, readout_flip=None,
                                            seed: Optional[int] = None, pairing: str = "reference", tile_bits: int = 0,
                                            max_resident_mib: float = 1024):
    """``simulate_heavy_output_counts_batch`` for widths 2..26: up to 13 it IS that function (``tile_bits`` and ``max_resident_mib``
    are checked and unused); from 14 on ``fbx_qv_heavy_outputs_wide_dev`` -> ``fbx_sample_bitstrings_wide_dev`` ->
    ``fbx_qv_count_heavy_wide_dev`` on device buffers.  The circuits run in slices, so that the probabilities (8 B x 2^n per
    circuit) plus the shot bytes of a slice stay under ``max_resident_mib`` (a slice holds at least one circuit); the slice that
    starts at circuit k is sampled with ``first_item = k``, so circuit b is item b of the stream whatever the cap, and the counts
    depend neither on the cap nor on ``tile_bits``: they equal the composed host calls (``heavy_outputs_flat_wide`` ->
    ``sampling.sample_bitstrings_wide_batch`` -> ``count_heavy_hitters_sampled_wide_batch``) on the same seed.

    Returns ``(counts [B] int64, stats)`` as the narrow function does."""
    width, pairs, flat = _flatten_circuits(permutations, gates, pairing)
    tile_bits = _check_wide(width, tile_bits, "simulate_heavy_output_counts_wide_batch")
    if not float(max_resident_mib) > 0.0:
        raise ValueError("simulate_heavy_output_counts_wide_batch: max_resident_mib must be positive")
    if width <= MAX_WIDTH:
        return simulate_heavy_output_counts_batch(permutations, gates, shots, depolarizing, readout_flip, seed, pairing)
    return _simulate_counts_resident(True, width, pairs, flat, shots, depolarizing, readout_flip, seed, tile_bits,
                                     float(max_resident_mib))


# ------------------------------------------------------------------------------------------------ gate noise
# P[k] = (X^xa Z^za) (x) (X^xc Z^zc) for the Pauli index k = 4 a + c (0 = I, 1 = X, 2 = Y, 3 = Z; a on q0, c on q1), with Y
# written as X Z = -i Y: the form the device applies (only probabilities leave it, so the phase is immaterial).
_PAULI_1Q = np.array([[[1, 0], [0, 1]], [[0, 1], [1, 0]], [[0, -1], [1, 0]], [[1, 0], [0, -1]]], dtype=np.float64)
_PAULI_2Q = np.stack([np.kron(_PAULI_1Q[k >> 2], _PAULI_1Q[k & 3]) for k in range(16)])


def fold_gate_errors(gates_flat, paulis) -> np.ndarray:
    """The gates of a trajectory with its Pauli errors folded in: ``gates_flat [..., L, 4, 4]`` and ``paulis [..., L]`` (the index
    ``k = 4 a + c`` of the Pauli after each gate, 0 = none; what ``synthetic.restate_qv_gate_errors`` returns) ->
    ``(P_a (x) P_c) U`` for every gate, with Y taken as X Z (a global phase, immaterial to every probability).  The leading axes
    broadcast; ``gates_flat [B, L, 4, 4]`` with ``paulis [B, T, L]`` gives ``[B, T, L, 4, 4]``.  Folding only permutes and negates
    rows, so it is exact: a folded trajectory is an ordinary circuit, for ``heavy_outputs_flat`` as for ``heavy_outputs_flat_wide``
    (widths 14..26), and on widths 2..13 it reproduces the device's trajectory arithmetic term for term."""
    gates = np.asarray(gates_flat, dtype=np.complex128)
    k = np.asarray(paulis)
    if gates.ndim < 3 or gates.shape[-2:] != (4, 4):
        raise ValueError("gates_flat must be [..., L, 4, 4]")
    if not np.issubdtype(k.dtype, np.integer) or k.ndim < 1 or k.shape[-1] != gates.shape[-3]:
        raise ValueError("paulis must be an integer array [..., L] with the L of gates_flat")
    if k.size and (k.min() < 0 or k.max() > 15):
        raise ValueError("a Pauli index must be 0..15")
    if k.ndim == gates.ndim - 1 and k.ndim >= 3:                          # [B, T, L] against [B, L, 4, 4]
        gates = gates[..., None, :, :, :]
    return np.matmul(_PAULI_2Q[k], gates)


def _gate_error_array(gate_error, B: int, L: int) -> np.ndarray:
    ge = np.asarray(gate_error, dtype=np.float64)
    if ge.shape == (B,):
        ge = ge[:, None]
    elif ge.shape not in ((), (B, L)):
        raise ValueError(f"gate_error must be a scalar, [B] = {(B,)} or [B, L] = {(B, L)}, not {ge.shape}")
    return np.ascontiguousarray(np.broadcast_to(ge, (B, L)))


def _heavy_masks(heavy, B: int, n: int) -> np.ndarray:
    heavy = np.asarray(heavy)
    if heavy.dtype == np.uint64:
        if heavy.shape != (B, _mask_words(n)):
            raise ValueError(f"masks must be [B, W] = {(B, _mask_words(n))}, not {heavy.shape}")
        return np.ascontiguousarray(heavy)
    if heavy.shape != (B, 1 << n):
        raise ValueError(f"heavy must be a boolean table [B, 2^n] = {(B, 1 << n)}, not {heavy.shape}")
    return pack_heavy_mask(heavy)


def noisy_trajectories_flat(n_qubits: int, pairs, gates, gate_error, trajectories: int, heavy=None, seed: Optional[int] = None,
                            first_item: int = 0, probs_mean: bool = True, hprob_traj: Optional[bool] = None, n_errors: bool = True):
    """``fbx_qv_noisy_trajectories`` on flat gate lists: ``trajectories`` = T stochastic Pauli-error trajectories of each of the B
    circuits ``pairs [B, L, 2]``, ``gates [B, L, 4, 4]`` (as ``heavy_outputs_flat`` takes them).  ``gate_error`` -- a scalar, ``[B]``
    or ``[B, L]`` -- is the probability that a gate is followed by one of the 15 non-identity Paulis on its pair, chosen uniformly.
    ``heavy``: the heavy sets of the IDEAL circuits, the boolean table ``[B, 2^n]`` or the packed masks ``[B, W]`` (uint64) of
    ``heavy_outputs_flat``; needed for ``hprob_traj`` (asked for by default exactly when ``heavy`` is given).

    Returns a dict with the outputs asked for: ``probs_mean [B, 2^n]`` (the mean output distribution over the T trajectories),
    ``hprob_traj [B, T]`` (the weight of every trajectory on the heavy set), ``n_errors [B, T]`` (int32, the Paulis inserted), and
    always ``status [B]`` (int32): 1 for a poisoned circuit (a non-finite gate entry, a pair that is not two different qubits below
    ``n_qubits``, a gate error outside [0, 1]), whose float outputs are NaN.  Trajectory t of circuit b depends on
    ``(seed, first_item + b, t)`` and the circuit alone (``seed=None``: a fresh key, the rule of ``random_operators``); the draws are
    restated by ``synthetic.restate_qv_gate_errors``.  Widths 2..13; a wider trajectory is a circuit for ``heavy_outputs_flat_wide``
    after ``fold_gate_errors``."""
    n, T, first_item = int(n_qubits), int(trajectories), int(first_item)
    pairs = np.asarray(pairs)
    gates = np.asarray(gates)
    if pairs.ndim != 3 or pairs.shape[2] != 2:
        raise ValueError("pairs must be [B, L, 2]")
    B, L = pairs.shape[:2]
    if gates.shape != (B, L, 4, 4):
        raise ValueError(f"gates must be [B, L, 4, 4] = {(B, L, 4, 4)}, not {gates.shape}")
    if pairs.size and (pairs.min() < 0 or pairs.max() > 255):
        raise ValueError("qubit indices must be 0..255")
    if hprob_traj is None:
        hprob_traj = heavy is not None
    if hprob_traj and heavy is None:
        raise ValueError("hprob_traj needs the heavy sets of the ideal circuits")
    if not (probs_mean or hprob_traj or n_errors):
        raise ValueError("no output asked for")
    from . import _lib
    import ctypes as C
    pairs = np.ascontiguousarray(pairs, dtype=np.uint8)
    gates = _lib.c128(gates)
    ge = _gate_error_array(gate_error, B, L)
    ok = MIN_WIDTH <= n <= MAX_WIDTH and T >= 0          # (outside, the library refuses before it touches a buffer)
    mask = _heavy_masks(heavy, B, n) if heavy is not None and n >= 0 else None
    out = {"status": np.zeros(B, dtype=np.int32)}
    if probs_mean:
        out["probs_mean"] = np.empty((B, 1 << n if ok else 0))
    if hprob_traj:
        out["hprob_traj"] = np.empty((B, T if ok else 0))
    if n_errors:
        out["n_errors"] = np.zeros((B, T if ok else 0), dtype=np.int32)
    _lib.check(_lib.lib().fbx_qv_noisy_trajectories(
        n, B, L, T, pairs.ctypes.data_as(C.POINTER(C.c_uint8)), _lib.dptr(gates.view(np.float64)), _lib.dptr(ge),
        mask.ctypes.data_as(C.POINTER(C.c_uint64)) if mask is not None else None, _stream_seed(seed), first_item,
        _lib.dptr(out.get("probs_mean")), _lib.dptr(out.get("hprob_traj")), _lib.iptr(out.get("n_errors")), _lib.iptr(out["status"])))
    return out


def _raise_poisoned_circuit(status, first_item: int, who: str):
    bad = np.flatnonzero(status)
    if bad.size:
        b = int(bad[0])
        raise ValueError(f"{who}: circuit {b} (global id {first_item + b}) cannot be simulated: a gate entry that is not finite or a "
                         f"gate error outside [0, 1] ({bad.size} such circuit(s) in the batch)")


def noisy_heavy_output_probability_batch(permutations, gates, gate_error, trajectories: int, pairing: str = "reference",
                                         seed: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The heavy-output probability of B model circuits under gate noise, in two device calls: the heavy sets of the ideal
    circuits (``heavy_outputs_flat``), then ``trajectories`` Pauli-error trajectories of each (``noisy_trajectories_flat``).
    Returns ``(mean [B], std_err [B])``: the mean over the trajectories of the weight on the IDEAL heavy set -- what the measured
    heavy fraction of a device with that gate error estimates -- and its standard error, the sample deviation over
    ``sqrt(trajectories)`` (NaN for fewer than two trajectories)."""
    width, pairs, flat = _flatten_circuits(permutations, gates, pairing)
    T = int(trajectories)
    if T < 1:
        raise ValueError("noisy_heavy_output_probability_batch: need at least one trajectory")
    ideal = heavy_outputs_flat(width, pairs, flat, probabilities=False, median=False, mask=True, heavy_prob=False, heavy_count=False)
    r = noisy_trajectories_flat(width, pairs, flat, gate_error, T, heavy=ideal["mask"], seed=seed, probs_mean=False, n_errors=False)
    _raise_poisoned_circuit(r["status"], 0, "noisy_heavy_output_probability_batch")
    hp = r["hprob_traj"]
    err = hp.std(axis=1, ddof=1) / np.sqrt(T) if T >= 2 else np.full(hp.shape[0], np.nan)
    return hp.mean(axis=1), err


def simulate_noisy_heavy_output_counts_batch(permutations, gates, shots: int, gate_error, trajectories: int, readout_flip=None,
                                             seed: Optional[int] = None, pairing: str = "reference"):
    """A simulated quantum-volume run under GATE noise, resident on the device (the ``_dev`` entry points only): heavy sets of the
    ideal circuits (``fbx_qv_heavy_outputs_dev``) -> the mean output distribution of ``trajectories`` = T Pauli-error trajectories
    per circuit (``fbx_qv_noisy_trajectories_dev``, ``gate_error`` a scalar, ``[B]`` or ``[B, L]``) -> ``shots`` measured bitstrings
    per circuit drawn from that mean (``fbx_sample_bitstrings_dev``: no depolarizing, optionally readout flips ``[n, 2]`` or
    ``[B, n, 2]``) -> heavy-hitter counts against the IDEAL heavy sets (``fbx_qv_count_heavy_dev``).

    The shots are drawn from the MEAN of T trajectories, not each from a trajectory of its own: that is the noisy channel's
    output distribution only up to the sampling error of the mean, and exact only as T grows (the error of an outcome's
    probability falls like ``1 / sqrt(T)``; ``stats["noisy_heavy_prob_err"]`` is that error for the heavy set).

    Returns ``(counts [B] int64, stats)``: ``stats["heavy_prob"]`` and ``stats["heavy_count"]`` of the ideal circuits,
    ``stats["noisy_heavy_prob"]`` = the mean over the trajectories of the weight on the ideal heavy set and
    ``stats["noisy_heavy_prob_err"]`` its standard error.  The trajectories and the shots both take ``seed`` (their streams carry
    different key tags) with circuit b as item b, so the counts equal those of the composed host calls (``heavy_outputs_flat`` ->
    ``noisy_trajectories_flat`` -> ``sampling.sample_bitstrings_batch`` -> ``count_heavy_hitters_sampled_batch``) on the same seed."""
    from . import _lib
    from .sampling import _noise, _raise_poisoned
    width, pairs, flat = _flatten_circuits(permutations, gates, pairing)
    B, L = pairs.shape[:2]
    T = int(trajectories)
    if not MIN_WIDTH <= width <= MAX_WIDTH:
        raise _lib.FbxError(_lib.FBX_ERR_UNSUPPORTED, f"simulate_noisy_heavy_output_counts_batch: width must be {MIN_WIDTH}..{MAX_WIDTH} "
                                                      f"(got {width}); there is no host fallback")
    if not 1 <= T < 2 ** 32:
        raise ValueError("simulate_noisy_heavy_output_counts_batch: need 1 <= trajectories < 2^32")
    N, W = 1 << width, _mask_words(width)
    shots, _, flips, _ = _noise(B, width, shots, None, readout_flip)
    ge = _gate_error_array(gate_error, B, L)
    key = _stream_seed(seed)
    if B == 0:
        return np.zeros(0, dtype=np.int64), {"heavy_prob": np.zeros(0), "heavy_count": np.zeros(0, dtype=np.int32),
                                             "noisy_heavy_prob": np.zeros(0), "noisy_heavy_prob_err": np.zeros(0)}
    lib = _lib.lib()
    with _lib.DeviceScope() as dev:
        d_pairs, d_gates, d_ge = dev.upload(pairs), dev.upload(_lib.c128(flat)), dev.upload(ge)
        d_flips = dev.upload(flips)
        d_probs, d_mask, d_hp, d_hc = dev.alloc(8 * B * N), dev.alloc(8 * B * W), dev.alloc(8 * B), dev.alloc(4 * B)
        d_traj, d_tstatus = dev.alloc(8 * B * T), dev.alloc(4 * B)
        d_bits, d_status, d_counts = dev.alloc(B * shots * width), dev.alloc(4 * B), dev.alloc(8 * B)
        _lib.check(lib.fbx_qv_heavy_outputs_dev(width, B, L, d_pairs.ptr, d_gates.ptr, None, None, d_mask.ptr, d_hp.ptr, d_hc.ptr))
        _lib.check(lib.fbx_qv_noisy_trajectories_dev(width, B, L, T, d_pairs.ptr, d_gates.ptr, d_ge.ptr, d_mask.ptr, key, 0,
                                                     d_probs.ptr, d_traj.ptr, None, d_tstatus.ptr))
        _lib.check(lib.fbx_sample_bitstrings_dev(width, B, shots, d_probs.ptr, None, _lib.devptr(d_flips), key, 0,
                                                 d_bits.ptr, d_status.ptr))
        _lib.check(lib.fbx_qv_count_heavy_dev(width, B, shots, d_bits.ptr, d_mask.ptr, d_counts.ptr))
        counts = d_counts.to_array(np.int64, (B,))
        hp = d_traj.to_array(np.float64, (B, T))
        stats = {"heavy_prob": d_hp.to_array(np.float64, (B,)), "heavy_count": d_hc.to_array(np.int32, (B,)),
                 "noisy_heavy_prob": hp.mean(axis=1),
                 "noisy_heavy_prob_err": hp.std(axis=1, ddof=1) / np.sqrt(T) if T >= 2 else np.full(B, np.nan)}
        _raise_poisoned_circuit(d_tstatus.to_array(np.int32, (B,)), 0, "simulate_noisy_heavy_output_counts_batch")
        if shots:
            _raise_poisoned(d_status.to_array(np.int32, (B,)), 0, "simulate_noisy_heavy_output_counts_batch")
    return counts, stats


# ------------------------------------------------------------------------------------------------ statistics (host)
def calculate_prob_est_and_err(num_heavy: int, num_circuits: int, num_shots: int) -> Tuple[float, float]:
    """quantum_volume.py:211-231: the heavy-output frequency over all circuits of a depth and its 2-sigma one-sided lower bound
    (Eq. (C3) of arXiv:1811.12926: worst-case binomial in the number of circuits, Gaussian approximation)."""
    total = num_circuits * num_shots
    prob = num_heavy / total
    lower = prob - 2 * np.sqrt(num_heavy * (num_shots - num_heavy / num_circuits)) / total
    return prob, lower


def get_prob_sample_heavy_by_depth(depths: Iterator[int], num_hh_sampled: Iterator[int],
                                   num_shots: Iterator[int]) -> Dict[int, Tuple[float, float]]:
    """quantum_volume.py:344-376: per-circuit (depth, heavy count, shots) -> {depth: (estimate, lower bound)}"""
    grouped: Dict[int, Tuple[List[int], int]] = {}
    for depth, heavy, shots in zip(depths, num_hh_sampled, num_shots):
        if depth in grouped:
            assert shots == grouped[depth][1], 'The number of shots should be the same for each circuit of a given depth.'
            grouped[depth][0].append(heavy)
        else:
            grouped[depth] = ([heavy], shots)
    return {depth: calculate_prob_est_and_err(sum(heavy), len(heavy), shots) for depth, (heavy, shots) in grouped.items()}


def extract_quantum_volume_from_results(results: Dict[int, Tuple[float, float]]) -> int:
    """quantum_volume.py:379-397: 2^(largest depth reached before the first depth whose lower bound is <= 2/3), Eq. 7"""
    achieved = 1
    for depth in sorted(results):
        if results[depth][1] <= 2 / 3:
            break
        achieved = depth
    return 2 ** achieved
