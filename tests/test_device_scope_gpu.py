"""``_lib.DeviceScope`` / ``DeviceBuffer.at`` and the resident chains that allocate through them: every chain gives its device
buffers back on every exit path -- a ``_dev`` call the library refuses, an allocation that fails -- and, with nothing injected,
returns what the composed host-pointer calls return.

The failures are injected in Python, by patching attributes of ``fbx._lib`` (no touched module binds ``check`` or ``DeviceBuffer``
at import time): the k-th ``_lib.check`` raises after its library call has returned, the j-th ``DeviceBuffer`` raises before
anything is allocated.  Nothing is provoked on the device.

The control compares five chains (and the all-gather, the GHZ and the RPE chain) with values computed another way -- the
host-pointer calls composed, the host restatement of the shots, the input itself; for the others it asserts that two runs agree
bit for bit and that every buffer is freed: their values are pinned by the GPU tests of their own modules (test_diamond_gpu,
test_chernoff_gpu, test_state_measures_big_gpu, test_tomo_sim_symm_gpu, test_rpe_gpu, test_randomized_benchmarking_gpu,
test_quantum_volume_noisy_gpu, test_frames_gpu).

The first ``check`` of a chain sits inside ``DeviceBuffer.__init__``, after ``fbx_malloc`` has returned and before the pointer is
kept, so k = 1 can show no leak (and loses those 16 bytes for the process); the case "first call" therefore refuses the first
check made outside ``DeviceBuffer`` once the chain holds a buffer: its first ``_dev`` call.

The chains run at their smallest shapes: 1-qubit designs, B = 2, 2 resamples, 8 shots, quantum volume of width 2 (narrow) and of
width 14 with one circuit of depth 1 (wide), 3 depths for RB and RPE, a one-rank communicator for the all-gather."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 11


# ------------------------------------------------------------------------------------------------ 1. the scope itself
def test_scope_frees_on_normal_exit(gpu):
    with gpu.DeviceScope() as dev:
        a, b = dev.alloc(64), dev.alloc(0)
        c = dev.upload(np.arange(4.0))
        assert dev.upload(None) is None
        assert a.nbytes == 64 and b.nbytes >= 16 and c.nbytes == 32
        assert all(buf.ptr is not None for buf in (a, b, c))
        assert np.array_equal(c.to_array(np.float64, (4,)), np.arange(4.0))
    assert a.ptr is None and b.ptr is None and c.ptr is None
    a.free()                                                    # freeing again stays harmless
    assert a.ptr is None


def test_scope_frees_on_exception_and_lets_it_through(gpu):
    class Boom(Exception):
        pass
    boom = Boom("unchanged")
    with pytest.raises(Boom) as ei:
        with gpu.DeviceScope() as dev:
            a, b = dev.alloc(32), dev.alloc(48)
            c = dev.upload(np.zeros(3, dtype=np.int32))
            raise boom
    assert ei.value is boom
    assert a.ptr is None and b.ptr is None and c.ptr is None


def test_buffer_at_checks_the_offset(gpu):
    x = np.array([1.5, -2.25, 3.0])
    with gpu.DeviceScope() as dev:
        buf, one = dev.upload(x), dev.alloc(8)
        assert buf.at(0).value == buf.ptr.value and buf.at(buf.nbytes).value == buf.ptr.value + buf.nbytes
        for bad in (-1, buf.nbytes + 1):
            with pytest.raises(ValueError):
                buf.at(bad)
        host = np.empty(1)
        gpu.check(gpu.lib().fbx_memcpy_d2h(host.ctypes.data_as(gpu._vp), buf.at(8), 8))
        assert host[0] == x[1]                                  # 8 bytes in: element 1 of a float64 array
        assert one.at(one.nbytes).value == one.ptr.value + one.nbytes


# ------------------------------------------------------------------------------------------------ the chains
def _circuits(width, depth, count, seed):
    """permutations [count, depth, width] and Haar gates [count, depth, width // 2, 4, 4]"""
    from fbx import synthetic
    rs = np.random.RandomState(seed)
    perms = np.stack([np.stack([rs.permutation(width) for _ in range(depth)]) for _ in range(count)])
    gates = np.stack([synthetic.haar_unitary(4, rs) for _ in range(count * depth * (width // 2))])
    return perms, gates.reshape(count, depth, width // 2, 4, 4)


@functools.lru_cache(maxsize=None)
def _inputs():
    """The inputs of every chain, built once (designs and groupings are created here, outside the injected runs)."""
    from fbx import synthetic, tomography as t
    from fbx.operator_tools import convert_batch
    pdesign, us, pe, pc = synthetic.process_batch(1, "pauli", 2, shots=500)
    sdesign, rhos, se, sc = synthetic.state_batch(1, 2, shots=500, mixed=0.1)
    t.calibration_list(pdesign)
    depths = np.repeat([2.0, 4.0, 8.0], 2)
    rb_e, rb_se = synthetic.rb_data(1, depths, [0.96, 0.9], 500, 2, seed=SEED)
    rng = np.random.default_rng(SEED)
    un_e = 0.9 * 0.95 ** depths[None, :, None] * np.array([1.0, 0.0, 0.0]) + rng.normal(0, 0.01, (2, 6, 3))
    angles = np.array([0.7, 2.9])
    rz = np.zeros((2, 4, 4))
    rz[:, 0, 0] = rz[:, 3, 3] = 1.0
    rz[:, 1, 1] = rz[:, 2, 2] = np.cos(angles)
    rz[:, 2, 1] = np.sin(angles)
    rz[:, 1, 2] = -np.sin(angles)
    k = 2.0 ** np.arange(3)
    return dict(pdesign=pdesign, us=us, pe=pe, pc=pc, sdesign=sdesign, rhos=rhos, se=se, sc=sc,
                ptm=convert_batch("kraus", "pauli_liouville", us[:, None]), choi=convert_batch("kraus", "choi", us[:, None]),
                depths=depths, rb_e=rb_e, rb_se=rb_se, un_e=un_e, un_se=np.full(un_e.shape, 0.02), rz=rz,
                x=np.cos(angles[:, None] * k) * 0.9, y=np.sin(angles[:, None] * k) * 0.9, xy_err=np.full((2, 3), 0.1),
                qv2=_circuits(2, 2, 2, 5), qv14=_circuits(14, 1, 1, 6), flip2=np.full((2, 2), 0.05),
                confusion=np.array([[0.95, 0.05], [0.1, 0.9]]))


def _fit(batch):
    return batch.params, batch.covar, batch.chisqr, batch.y, batch.weights, batch.has_weights


def _process_fidelity(i):
    from fbx import tomography as t
    return t.process_fidelity_variance_batch(i["pdesign"], i["pe"], i["pc"], i["ptm"], n_resamples=2, seed=3, return_samples=True)


def _process_diamond(i):
    from fbx import tomography as t
    return t.process_diamond_distance_variance_batch(i["pdesign"], i["pe"], i["pc"], i["choi"], n_resamples=2, seed=3,
                                                     return_samples=True)


def _state_chernoff(i):
    from fbx import tomography as t
    return t.state_chernoff_variance_batch(i["sdesign"], i["se"], i["sc"], i["rhos"], n_resamples=2, seed=3, return_samples=True)


def _state_measure(i):
    from fbx import tomography as t
    return t.state_measure_variance_batch(i["sdesign"], i["se"], i["sc"], i["rhos"], "fidelity", n_resamples=2, seed=3,
                                          return_samples=True)


def _sim_estimate(i):
    from fbx import tomography as t
    return t.simulate_and_estimate_process_batch(i["pdesign"], i["us"], 8, rep="unitary", readout_flip=i["flip2"][:1], seed=SEED)


def _sim_estimate_calibrated(i):
    from fbx import tomography as t
    return t.simulate_and_estimate_process_batch(i["pdesign"], i["us"], 8, rep="unitary", seed=SEED, confusion=i["confusion"])


def _phase_variance(i):
    from fbx import robust_phase_estimation as rpe
    return rpe.phase_variance_batch(i["x"], i["y"], i["xy_err"], i["xy_err"], 8, n_resamples=2, seed=7, return_samples=True)


def _rpe_sim(i):
    from fbx import robust_phase_estimation as rpe
    return rpe.simulate_and_estimate_rpe_batch(i["rz"], num_depths=3, num_shots=8, seed=SEED)


def _rb_fit(i):
    from fbx import randomized_benchmarking as rb
    return _fit(rb.fit_rb_results_batch(i["depths"], i["rb_e"], i["rb_se"]))


def _unitarity_fit(i):
    from fbx import randomized_benchmarking as rb
    return _fit(rb.fit_unitarity_results_batch(i["depths"], i["un_e"], i["un_se"]))


def _qv_counts(out):
    return out[0], out[1]["heavy_prob"], out[1]["heavy_count"]


def _qv_narrow(i):
    from fbx import quantum_volume as qv
    return _qv_counts(qv.simulate_heavy_output_counts_batch(*i["qv2"], 8, depolarizing=0.1, readout_flip=i["flip2"], seed=SEED))


def _qv_wide(i):
    from fbx import quantum_volume as qv
    return _qv_counts(qv.simulate_heavy_output_counts_wide_batch(*i["qv14"], 8, depolarizing=0.1, seed=SEED))


def _qv_noisy(i):
    from fbx import quantum_volume as qv
    counts, stats = qv.simulate_noisy_heavy_output_counts_batch(*i["qv2"], 8, 0.1, 2, readout_flip=i["flip2"], seed=SEED)
    return counts, stats["heavy_prob"], stats["noisy_heavy_prob"]


def _bcsz(i):
    from fbx.operator_tools import random_operators as ro
    return (ro.rand_map_with_BCSZ_dist_batch(2, 2, 2, seed=SEED),)


def _ghz(i):
    from fbx import entangled_states as es
    out = es.simulate_ghz_statistics_batch([(0, 1)], 8, np.array([[0.0], [0.2]]), readout_flip=i["flip2"], seed=SEED)
    return out["bell"], out["total"]


def _graph_state(i):
    from fbx import entangled_states as es
    return (es.simulate_graph_state_parities_batch(([0, 1], [(0, 1)]), 8, np.array([[0.0], [0.2]]), readout_flip=i["flip2"],
                                                   seed=SEED),)


_ALLGATHER = (np.arange(6.0).reshape(2, 3) + 0.5j).astype(np.complex128)
_comm = None


@pytest.fixture(scope="module")
def comm(gpu):
    """A one-rank RCCL communicator for the all-gather chain, made outside the injected runs and closed when the module is done."""
    global _comm
    from fbx import parallel
    _comm = parallel.RcclComm(0, 1, parallel.RcclComm.new_unique_id())
    try:
        yield _comm
    finally:
        _comm.close()
        _comm = None


def _allgather(i):
    return (_comm.allgather(_ALLGATHER),)


CHAINS = {f.__name__.lstrip("_"): f for f in (
    _process_fidelity, _process_diamond, _state_chernoff, _state_measure, _sim_estimate, _sim_estimate_calibrated, _phase_variance,
    _rpe_sim, _rb_fit, _unitarity_fit, _qv_narrow, _qv_wide, _qv_noisy, _bcsz, _ghz, _graph_state, _allgather)}


class _Probe:
    """Records every ``DeviceBuffer`` made while it is installed and counts the ``check`` calls, and among them the ``calls``: those
    made outside ``DeviceBuffer`` (not an allocation or a copy) while the chain holds a buffer.  Raises ``FbxError`` in the place of
    the ``fail_check``-th check or of the ``fail_call``-th call (after the library call returned), or of the ``fail_alloc``-th
    construction (before it allocates)."""

    def __init__(self, monkeypatch, lib, fail_check=0, fail_call=0, fail_alloc=0):
        self.made, self.checks, self.calls, self.inside = [], 0, 0, 0
        DB, real_check = lib.DeviceBuffer, lib.check
        real_init, real_from, real_to = DB.__init__, DB.from_array.__func__, DB.to_array

        def within(fn):
            def wrapped(*a, **k):
                self.inside += 1
                try:
                    return fn(*a, **k)
                finally:
                    self.inside -= 1
            return wrapped

        @within
        def init(buf, nbytes):
            self.made.append(buf)
            if len(self.made) == fail_alloc:
                raise lib.FbxError(lib.FBX_ERR_NOMEM, "injected")
            real_init(buf, nbytes)

        def check(code):
            self.checks += 1
            call = self.inside == 0 and len(self.made) > 0
            self.calls += call
            if self.checks == fail_check or (call and self.calls == fail_call):
                raise lib.FbxError(lib.FBX_ERR_HIP, "injected")
            real_check(code)
        monkeypatch.setattr(DB, "__init__", init)
        monkeypatch.setattr(DB, "from_array", classmethod(within(real_from)))
        monkeypatch.setattr(DB, "to_array", within(real_to))
        monkeypatch.setattr(lib, "check", check)

    def leaked(self):
        return [k for k, buf in enumerate(self.made) if getattr(buf, "ptr", None) is not None]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind in "fc":                                   # NaNs count as equal: compare the bits
        a, b = np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)
    return a.shape == b.shape and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def _clean_run(name):
    """(outputs, number of checks, number of allocations, leaked buffers) of the chain with nothing injected, the outputs of
    a run before it (which also fills the design and grouping caches, so that every later run makes the same calls), and the
    number of checks outside ``DeviceBuffer``"""
    from fbx import _lib
    before = CHAINS[name](_inputs())
    with pytest.MonkeyPatch.context() as mp:
        probe = _Probe(mp, _lib)
        out = CHAINS[name](_inputs())
    return out, probe.checks, len(probe.made), probe.leaked(), before, probe.calls


# ------------------------------------------------------------------------------------------------ 4. control
@pytest.mark.parametrize("name", list(CHAINS))
def test_chain_runs_clean_and_frees_everything(gpu, comm, name):
    out, checks, allocs, leaked, before, _ = _clean_run(name)
    assert checks >= 2 and allocs >= 2 and leaked == []
    assert len(out) == len(before)                              # the same bits on the same seed
    for a, b in zip(out, before):
        assert (a is None and b is None) or _same(a, b)


def test_controls_equal_the_composed_host_calls(gpu, comm):
    """The values the resident chains are pinned to elsewhere, at these shapes: bit for bit the host-pointer calls composed."""
    from fbx import clifford_circuit as cc, distance_measures as dm, entangled_states as es, quantum_volume as qv
    from fbx import robust_phase_estimation as rpe, sampling, tomography as t
    from fbx.operator_tools import convert_batch, random_operators as ro
    i = _inputs()
    B, R = 2, 2
    mean, var, samples = _clean_run("process_fidelity")[0]
    e_rs = t.resample_expectations_with_beta_batch(i["pe"], i["pc"], R, seed=3)
    choi = t.pgdb_process_estimate_batch(i["pdesign"], e_rs.reshape(R * B, -1), np.tile(i["pc"], (R, 1)))
    want = dm.process_fidelity_batch(np.tile(i["ptm"], (R, 1, 1)), convert_batch("choi", "pauli_liouville", choi)).reshape(R, B)
    assert np.array_equal(samples, want) and np.array_equal(mean, want.mean(axis=0)) and np.array_equal(var, want.var(axis=0))

    choi, fid = _clean_run("sim_estimate")[0]
    e, c = t.simulate_process_tomography_batch(i["pdesign"], i["us"], 8, rep="unitary", readout_flip=i["flip2"][:1], seed=SEED)
    want = t.pgdb_process_estimate_batch(i["pdesign"], e, c)
    truth = i["ptm"].real.astype(np.complex128)
    assert np.array_equal(choi, want)
    assert np.array_equal(fid, dm.process_fidelity_batch(truth, convert_batch("choi", "pauli_liouville", want)))

    perms, gates = i["qv2"]
    counts, heavy_prob, heavy_count = _clean_run("qv_narrow")[0]
    heavy, probs, stats = qv.collect_heavy_outputs_batch(perms, gates, return_probabilities=True, return_stats=True)
    bits = sampling.sample_bitstrings_batch(probs, 8, 0.1, i["flip2"], seed=SEED)
    assert np.array_equal(counts, qv.count_heavy_hitters_sampled_batch(bits, heavy))
    assert np.array_equal(heavy_prob, stats["heavy_prob"]) and np.array_equal(heavy_count, stats["heavy_count"])

    perms, gates = i["qv14"]
    counts, heavy_prob, heavy_count = _clean_run("qv_wide")[0]
    heavy, probs, stats = qv.collect_heavy_outputs_wide_batch(perms, gates, return_probabilities=True, return_stats=True)
    bits = sampling.sample_bitstrings_wide_batch(probs, 8, 0.1, seed=SEED)
    assert np.array_equal(counts, qv.count_heavy_hitters_sampled_wide_batch(bits, heavy))
    assert np.array_equal(heavy_prob, stats["heavy_prob"]) and np.array_equal(heavy_count, stats["heavy_count"])

    kraus = ro.random_kraus_batch(2, 2, 2, seed=SEED)
    assert np.array_equal(_clean_run("bcsz")[0][0], convert_batch("kraus", "choi", kraus))

    gathered, = _clean_run("allgather")[0]
    assert gathered.shape == (1, 2, 3) and np.array_equal(gathered[0], _ALLGATHER)

    errors = np.array([[0.0], [0.2]])
    shots = cc.restate_frame_shots(es.create_ghz_program([(0, 1)]), 2, 8, errors, None, i["flip2"], seed=SEED)
    want = es.ghz_state_statistics_batch(cc.unpack_shots(shots, 2))
    bell, total = _clean_run("ghz")[0]
    assert np.array_equal(bell, want["bell"]) and np.array_equal(total, want["total"])

    m, _ = rpe.simulate_rpe_batch(i["rz"], num_depths=3, num_shots=8, seed=SEED)
    want, stats = rpe.estimate_phase_from_moments_batch(m[0], m[1], m[4], m[5], errors_are_variances=True, return_stats=True)
    phases, depth = _clean_run("rpe_sim")[0]
    assert _same(phases, want) and np.array_equal(depth, stats["depth_reached"])


# ------------------------------------------------------------------------------------------------ 2. a refused call
@pytest.mark.parametrize("which", ["first", "first call", "last"])
@pytest.mark.parametrize("name", list(CHAINS))
def test_no_chain_leaks_on_a_refused_call(gpu, comm, monkeypatch, name, which):
    checks = _clean_run(name)[1]
    assert _clean_run(name)[5] >= 1
    inject = {"first": dict(fail_check=1), "first call": dict(fail_call=1), "last": dict(fail_check=checks)}[which]
    probe = _Probe(monkeypatch, gpu, **inject)
    with pytest.raises(gpu.FbxError, match="injected"):
        CHAINS[name](_inputs())
    assert probe.leaked() == [], f"{name}: buffers {probe.leaked()} of {len(probe.made)} outlive the refused call"


# ------------------------------------------------------------------------------------------------ 3. a failed allocation
@pytest.mark.parametrize("which", ["second", "last"])
@pytest.mark.parametrize("name", list(CHAINS))
def test_no_chain_leaks_on_a_failed_allocation(gpu, comm, monkeypatch, name, which):
    allocs = _clean_run(name)[2]
    probe = _Probe(monkeypatch, gpu, fail_alloc=2 if which == "second" else allocs)
    with pytest.raises(gpu.FbxError, match="injected"):
        CHAINS[name](_inputs())
    assert probe.leaked() == [], f"{name}: buffers {probe.leaked()} of {len(probe.made)} outlive the failed allocation"
