"""fbx_qv_noisy_trajectories on the GPU: Pauli-error trajectories of quantum-volume circuits against their numpy restatement
(``synthetic.restate_qv_gate_errors`` + ``quantum_volume.fold_gate_errors`` + ``qv_cases.simulate``, themselves checked against the
exact channel in tests/test_quantum_volume_noisy_cpu.py), the end points p = 0 and p = 1, the independence of an item from its batch,
the poisoned-item rule, the argument errors, the resident pipeline and the composition with the wide entry points.

Tolerances (derived, not tuned).  The Pauli after a gate is exact on the device (a slot permutation and sign flips) and in
``fold_gate_errors`` (a row permutation and sign flips), so a trajectory is an L-gate circuit on both sides and its probabilities
obey ``qv_cases.prob_bound``: |p_dev[t, i] - p_ref[t, i]| <= 2 sqrt(p_ref[t, i]) delta_L + delta_L^2.  The mean over T trajectories
therefore lies within the mean of those bounds, plus the summation term: a sum of T non-negative doubles in any order, then one
division, has a relative error of at most T u / (1 - T u) on either side, 2 T u / (1 - T u) times the mean's magnitude for both.
The weight on the heavy set is a sum of at most 2^n non-negative terms whose total is at most 1 (plus the bound): two summation
orders differ by at most 2^n u, on top of the summed element bounds."""
import ctypes as C
import functools

import numpy as np
import pytest

import qv_cases as qc

pytestmark = pytest.mark.gpu
SEED = 77001
WIDTHS = [2, 3, 6, 8, 9, 13]


def shape_of(n):
    """(B, T): three circuits of 37 trajectories -- 37 is no multiple of a segment length -- and B = 2, T = 4 with the LDS full"""
    return (2, 4) if n == 13 else (3, 37)


@functools.lru_cache(maxsize=None)
def case(n):
    """inputs of width n: model circuits (reference pairing), a [B, L] gate error of distinct entries around p = 0.3"""
    B, T = shape_of(n)
    perms, gates = qc.random_circuits(n, B, seed=500 + n)
    pairs = np.stack([qc.pairs_of(perms[b]) for b in range(B)])
    flat = gates.reshape(B, -1, 4, 4)
    L = pairs.shape[1]
    assert L == n * (n // 2)
    ge = 0.3 + 0.1 * (np.random.default_rng(600 + n).random((B, L)) - 0.5)
    assert len(np.unique(ge)) == B * L
    return B, T, L, pairs, flat, ge


@functools.lru_cache(maxsize=None)
def restated(n):
    """(paulis [B, T, L], p_ref [B, T, 2^n]): computed once per width, read-only"""
    from fbx import quantum_volume as qv, synthetic
    B, T, L, pairs, flat, ge = case(n)
    paulis = synthetic.restate_qv_gate_errors(B, T, L, ge, SEED + n)
    folded = qv.fold_gate_errors(flat, paulis)
    p = np.stack([np.stack([qc.simulate(n, pairs[b], folded[b, t]) for t in range(T)]) for b in range(B)])
    paulis.setflags(write=False); p.setflags(write=False)
    return paulis, p


@functools.lru_cache(maxsize=None)
def device(n):
    """(ideal result dict, trajectories result dict) of the case of width n on the device"""
    from fbx import quantum_volume as qv
    B, T, L, pairs, flat, ge = case(n)
    ideal = qv.heavy_outputs_flat(n, pairs, flat)
    r = qv.noisy_trajectories_flat(n, pairs, flat, ge, T, heavy=ideal["mask"], seed=SEED + n)
    return ideal, r


def same(a, b):
    """bit for bit, NaN included"""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n", WIDTHS)
def test_against_the_restatement(gpu, n):
    from fbx import quantum_volume as qv
    B, T, L, pairs, flat, ge = case(n)
    paulis, p_ref = restated(n)
    ideal, r = device(n)
    N = 1 << n
    assert r["probs_mean"].shape == (B, N) and r["hprob_traj"].shape == (B, T) and r["n_errors"].dtype == np.int32
    assert not r["status"].any()
    assert np.array_equal(r["n_errors"], np.count_nonzero(paulis, axis=2))
    assert 0 < r["n_errors"].sum() < B * T * L
    heavy = qv.unpack_heavy_mask(ideal["mask"], n)
    tu = T * qc.U_ROUND
    for b in range(B):
        bound_t = qc.prob_bound(p_ref[b], L)                                                   # [T, N]
        mean_ref, mean_bound = p_ref[b].mean(axis=0), bound_t.mean(axis=0)
        bound = mean_bound + 2 * tu / (1 - tu) * (mean_ref + mean_bound)
        err = np.abs(r["probs_mean"][b] - mean_ref)
        hp_ref = (p_ref[b] * heavy[b]).sum(axis=1)
        hp_bound = (bound_t * heavy[b]).sum(axis=1) + N * qc.U_ROUND
        hp_err = np.abs(r["hprob_traj"][b] - hp_ref)
        print(f"width {n} item {b}: max |d mean| {err.max():.3e} (bound there {bound[err.argmax()]:.3e}), "
              f"max |d hprob| {hp_err.max():.3e} (bound there {hp_bound[hp_err.argmax()]:.3e}), "
              f"|sum(mean) - 1| {abs(r['probs_mean'][b].sum() - 1):.3e}")
        assert np.all(err <= bound), (n, b)
        assert np.all(hp_err <= hp_bound), (n, b)
        assert abs(r["probs_mean"][b].sum() - 1) <= 2 * qc.delta(L) + (N + 2 * T) * qc.U_ROUND


@pytest.mark.parametrize("n", WIDTHS)
def test_end_points(gpu, n):
    """p = 0: no Pauli, every trajectory is the ideal circuit; p = 1: one after every gate"""
    from fbx import quantum_volume as qv
    B, T, L, pairs, flat, _ = case(n)
    ideal, _ = device(n)
    r0 = qv.noisy_trajectories_flat(n, pairs, flat, 0.0, T, heavy=ideal["mask"], seed=SEED)
    assert not r0["n_errors"].any() and not r0["status"].any()
    d = np.abs(r0["hprob_traj"] - ideal["heavy_prob"][:, None])
    print(f"width {n}: p = 0, max |hprob_traj - heavy_prob| {d.max():.3e} (bound {(1 << n) * qc.U_ROUND:.3e})")
    assert np.all(d <= (1 << n) * qc.U_ROUND)
    tu = T * qc.U_ROUND
    assert np.all(np.abs(r0["probs_mean"] - ideal["probabilities"]) <= qc.prob_bound(ideal["probabilities"], L)
                  + 2 * tu / (1 - tu) * ideal["probabilities"])
    r1 = qv.noisy_trajectories_flat(n, pairs, flat, np.ones(B), T, seed=SEED, probs_mean=False)
    assert list(r1) == ["status", "n_errors"] and np.all(r1["n_errors"] == L)


def dev_form(n, pairs, flat, ge, T, mask, seed, first_item=0):
    """the _dev entry point on caller-owned device buffers: (probs_mean, hprob_traj, n_errors, status)"""
    from fbx import _lib
    B, L = pairs.shape[:2]
    N = 1 << n
    DB = _lib.DeviceBuffer
    bufs = [DB.from_array(np.ascontiguousarray(pairs, dtype=np.uint8)), DB.from_array(_lib.c128(flat)),
            DB.from_array(np.ascontiguousarray(ge, dtype=np.float64)), DB.from_array(np.ascontiguousarray(mask)),
            DB(8 * B * N), DB(8 * B * T), DB(4 * B * T), DB(4 * B)]
    try:
        _lib.check(_lib.lib().fbx_qv_noisy_trajectories_dev(n, B, L, T, *(b.ptr for b in bufs[:4]), seed, first_item,
                                                            *(b.ptr for b in bufs[4:])))
        _lib.synchronize()
        return (bufs[4].to_array(np.float64, (B, N)), bufs[5].to_array(np.float64, (B, T)), bufs[6].to_array(np.int32, (B, T)),
                bufs[7].to_array(np.int32, (B,)))
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("n", [6, 9])
def test_independence_of_batch_trajectory_count_option_and_form(gpu, n):
    from fbx import _lib, quantum_volume as qv
    B, T, L, pairs, flat, ge = case(n)
    ideal, r = device(n)
    mask, seed = ideal["mask"], SEED + n
    # items k.. alone, with first_item = k
    tail = qv.noisy_trajectories_flat(n, pairs[1:], flat[1:], ge[1:], T, heavy=mask[1:], seed=seed, first_item=1)
    for key in ("probs_mean", "hprob_traj", "n_errors", "status"):
        assert same(tail[key], r[key][1:]), key
    assert not same(qv.noisy_trajectories_flat(n, pairs[1:], flat[1:], ge[1:], T, heavy=mask[1:], seed=seed)["n_errors"], r["n_errors"][1:])
    # fewer trajectories: a prefix (with and without the mean, which changes the launch shape)
    for mean in (True, False):
        short = qv.noisy_trajectories_flat(n, pairs, flat, ge, 13, heavy=mask, seed=seed, probs_mean=mean)
        assert same(short["hprob_traj"], np.ascontiguousarray(r["hprob_traj"][:, :13]))
        assert same(short["n_errors"], np.ascontiguousarray(r["n_errors"][:, :13]))
    # the workspace option: enough copies of the batch that 1 MiB of partial sums cuts it into chunks
    per_item = 8 * (1 << n) * ((T + 3) // 4)
    reps = (2 * 1048576) // (3 * per_item) + 1
    big = [np.tile(a, (reps,) + (1,) * (a.ndim - 1)) for a in (pairs, flat, ge, mask)]
    assert 3 * reps * per_item > 2 * 1048576
    want = qv.noisy_trajectories_flat(n, big[0], big[1], big[2], T, heavy=big[3], seed=seed)
    with _lib.option("qv_noisy_workspace_mib", 1.0):
        got = qv.noisy_trajectories_flat(n, big[0], big[1], big[2], T, heavy=big[3], seed=seed)
    assert _lib.get_option("qv_noisy_workspace_mib") == 128.0
    for key in ("probs_mean", "hprob_traj", "n_errors", "status"):
        assert same(got[key], want[key]), key
        assert same(want[key][:3], r[key]), key                           # and the first items are the small batch's
    assert not same(want["n_errors"][3:6], r["n_errors"])                 # the copies are other items of the stream
    # host-pointer and _dev forms
    d = dev_form(n, pairs, flat, ge, T, mask, seed)
    for got_d, key in zip(d, ("probs_mean", "hprob_traj", "n_errors", "status")):
        assert same(got_d, r[key]), key


@pytest.mark.parametrize("n", [6, 9])
@pytest.mark.parametrize("kind", ["nan_gate", "equal_pair", "gate_error_1.5", "gate_error_nan"])
def test_poisoned_item(gpu, n, kind):
    from fbx import quantum_volume as qv
    B, T, L, pairs, flat, ge = case(n)
    ideal, r = device(n)
    pairs, flat, ge = pairs.copy(), flat.copy(), ge.copy()
    if kind == "nan_gate":
        flat[1, L // 2, 2, 1] = complex(np.nan, 0.0)
    elif kind == "equal_pair":
        pairs[1, L - 1] = (n - 1, n - 1)
    elif kind == "gate_error_1.5":
        ge[1, 0] = 1.5
    else:
        ge[1, L - 1] = np.nan
    got = qv.noisy_trajectories_flat(n, pairs, flat, ge, T, heavy=ideal["mask"], seed=SEED + n)
    assert list(got["status"]) == [0, 1, 0]
    assert np.all(np.isnan(got["probs_mean"][1])) and np.all(np.isnan(got["hprob_traj"][1])) and not got["n_errors"][1].any()
    for key in ("probs_mean", "hprob_traj", "n_errors"):
        assert same(got[key][0], r[key][0]) and same(got[key][2], r[key][2]), key


def test_argument_errors_leave_the_buffers_alone(gpu):
    from fbx import _lib
    lib = _lib.lib()
    n, B, L, T = 3, 2, 3, 5
    pairs = np.tile(np.asarray([(0, 1), (1, 2), (2, 0)], dtype=np.uint8), (B, 1, 1))
    gates = np.tile(np.eye(4, dtype=np.complex128), (B, L, 1, 1)).view(np.float64)
    ge = np.full((B, L), 0.5)
    mask = np.ones((B, 1), dtype=np.uint64)
    out = {"mean": np.full((B, 1 << n), -3.0), "hp": np.full((B, T), -3.0), "ne": np.full((B, T), -3, dtype=np.int32),
           "st": np.full(B, -3, dtype=np.int32)}
    u8, u64 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    good = dict(n=n, B=B, L=L, T=T, pairs=pairs, gates=gates, ge=ge, mask=mask, first=0, mean=out["mean"], hp=out["hp"], ne=out["ne"])

    def call(**kw):
        a = dict(good, **kw)
        return lib.fbx_qv_noisy_trajectories(
            a["n"], a["B"], a["L"], a["T"], None if a["pairs"] is None else a["pairs"].ctypes.data_as(u8), _lib.dptr(a["gates"]),
            _lib.dptr(a["ge"]), None if a["mask"] is None else a["mask"].ctypes.data_as(u64), 9, a["first"], _lib.dptr(a["mean"]),
            _lib.dptr(a["hp"]), _lib.iptr(a["ne"]), _lib.iptr(out["st"]))
    for width in (0, 1, 14, 27):
        assert call(n=width) == _lib.FBX_ERR_UNSUPPORTED, width
    bad = [dict(T=2 ** 32), dict(T=-1), dict(B=-1), dict(L=-1), dict(first=-1), dict(pairs=None), dict(gates=None), dict(ge=None),
           dict(mask=None), dict(mean=None, hp=None, ne=None)]
    for kw in bad:
        assert call(**kw) == _lib.FBX_ERR_BAD_ARG, kw
        assert _lib.lib().fbx_last_error()
    for a in out.values():
        assert np.all(a == -3)
    # nothing to do
    assert call(T=0) == 0 and call(B=0) == 0
    for a in out.values():
        assert np.all(a == -3)
    # and the good call works: identity gates, so every trajectory stays a basis state
    assert call() == 0
    assert np.all(out["st"] == 0) and np.all(out["ne"] >= 0) and np.all(out["ne"] <= L) and np.all(out["hp"] >= 0)
    assert np.all(np.abs(out["mean"].sum(axis=1) - 1) <= 8 * qc.U_ROUND)
    # the same refusals from the _dev form, before any pointer is followed
    dev = lib.fbx_qv_noisy_trajectories_dev
    assert dev(14, B, L, T, 1, 1, 1, 1, 9, 0, 1, 1, 1, 1) == _lib.FBX_ERR_UNSUPPORTED
    assert dev(n, B, L, T, 1, 1, 1, None, 9, 0, 1, 1, 1, 1) == _lib.FBX_ERR_BAD_ARG
    assert dev(n, B, L, T, 1, 1, 1, 1, 9, 0, None, None, None, 1) == _lib.FBX_ERR_BAD_ARG
    assert dev(n, B, L, 2 ** 32, 1, 1, 1, 1, 9, 0, 1, 1, 1, 1) == _lib.FBX_ERR_BAD_ARG


@pytest.mark.parametrize("n, flips", [(5, True), (9, False)])
def test_resident_pipeline_equals_the_composed_host_calls(gpu, n, flips):
    from fbx import quantum_volume as qv, sampling
    B, T, shots, seed = 4, 9, 300, 4242 + n
    perms, gates = qc.random_circuits(n, B, seed=700 + n)
    ge = 0.1 * (1 + np.arange(B))
    flip = np.random.default_rng(n).uniform(0.0, 0.1, size=(n, 2)) if flips else None
    counts, stats = qv.simulate_noisy_heavy_output_counts_batch(perms, gates, shots, ge, T, readout_flip=flip, seed=seed)
    width, pairs, flat = qv._flatten_circuits(perms, gates, "reference")
    ideal = qv.heavy_outputs_flat(n, pairs, flat)
    r = qv.noisy_trajectories_flat(n, pairs, flat, ge, T, heavy=ideal["mask"], seed=seed)
    bits = sampling.sample_bitstrings_batch(r["probs_mean"], shots, readout_flip=flip, seed=seed)
    assert np.array_equal(counts, qv.count_heavy_hitters_sampled_batch(bits, ideal["mask"]))
    assert counts.dtype == np.int64 and 0 < counts.min() and counts.max() < shots
    assert same(stats["heavy_prob"], ideal["heavy_prob"]) and same(stats["heavy_count"], ideal["heavy_count"])
    assert same(stats["noisy_heavy_prob"], r["hprob_traj"].mean(axis=1))
    assert np.all(stats["noisy_heavy_prob"] > 0) and np.all(stats["noisy_heavy_prob"] < 1)
    mean, err = qv.noisy_heavy_output_probability_batch(perms, gates, ge, T, seed=seed)
    assert same(mean, stats["noisy_heavy_prob"]) and same(err, stats["noisy_heavy_prob_err"]) and np.all(np.isfinite(err))


def test_wide_composition_one_folded_trajectory_at_width_14(gpu):
    """a folded trajectory is an ordinary circuit: widths 14..26 run it through the wide entry points"""
    from fbx import quantum_volume as qv, synthetic
    n = 14
    perms, gates = qc.random_circuits(n, 1, seed=914)
    pairs, flat = qc.pairs_of(perms[0]), gates[0].reshape(-1, 4, 4)
    L = len(pairs)
    paulis = synthetic.restate_qv_gate_errors(1, 1, L, 0.3, SEED)[0, 0]
    assert 0 < np.count_nonzero(paulis) < L
    folded = qv.fold_gate_errors(flat, paulis)
    r = qv.heavy_outputs_flat_wide(n, pairs[None], folded[None], median=False, mask=False, heavy_prob=False, heavy_count=False)
    p = r["probabilities"][0]
    print(f"width 14: |sum - 1| {abs(p.sum() - 1):.3e} (bound {2 * qc.delta(L):.3e})")
    assert abs(p.sum() - 1) <= 2 * qc.delta(L)
    want = qc.simulate(n, pairs, folded)
    assert np.all(np.abs(p - want) <= qc.prob_bound(want, L))
    assert np.abs(want - qc.simulate(n, pairs, flat)).max() > 1e-6                           # the errors did something
