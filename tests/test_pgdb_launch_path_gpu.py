"""The host code between fbx_pgdb_process* and the kernel launches (csrc/fbx_pgdb_call.hpp: the call record and its slice();
csrc/fbx_pgdb.hip: launch_pgdb, pgdb_process_host; csrc/fbx_pgdb1.hip / fbx_pgdb3.hip: their launchers), at the places where an
offset or an owner of memory can be wrong without any other test noticing: the launch chunks of the two launchers (65 536 and
512 items), the pipelined path with optional outputs absent, the page-locked counters of the binned single-qubit run across
fbx_release_workspace, and the workspace slot of the 3-qubit cost / gradient launcher across two unsynchronised calls.
tests/test_pgdb_call_host.py checks slice() and the stage plan themselves without a GPU."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATS = ("iterations", "dykstra", "backtracks", "cost", "jacobi_sweeps", "eig_terms", "cost_evals", "power_sum_passes", "trace")


def _wrapped(e0, c0, chunk):
    """`chunk` items of the tiled experiments, then the experiments again: item chunk + k is item k."""
    reps = -(-chunk // len(e0))
    return (np.ascontiguousarray(np.concatenate([np.tile(e0, (reps, 1))[:chunk], e0])),
            np.ascontiguousarray(np.concatenate([np.tile(c0, (reps, 1))[:chunk], c0])))


def _assert_wraps(got, st, chunk, n):
    assert got.shape[0] == chunk + n
    assert np.array_equal(got[chunk], got[0])                # the first item of the second launch
    assert np.array_equal(got[chunk:], got[:n])
    for k in STATS:
        a = np.asarray(st[k])
        assert a.shape[0] == chunk + n and np.array_equal(a[chunk:], a[:n]), k
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])      # (distinct experiments)
    assert (st["iterations"] > 0).all()                      # every item was written


def test_launch_chunk_of_the_one_and_two_qubit_launcher_is_crossed(gpu):
    """65 536 + 3 single-qubit items on the wavefront-per-item kernel: two launches of launch_pgdb.  The second one's items
    are the first three experiments again: every output of theirs -- Choi matrix, counters, cost, work counters, trace -- equals
    the first launch's bit for bit, so each of the nine arrays was advanced by its own stride."""
    from fbx import synthetic, tomography
    design, _, e0, c0 = synthetic.process_batch(1, "pauli", 3)
    e, c = _wrapped(e0, c0, 65536)
    with gpu.option("pgdb_packed_1q", 0.0):
        got, st = tomography.pgdb_process_estimate_batch(design, e, c, mode="converge", max_iters=2, return_stats=True, trace_iters=2)
    _assert_wraps(got, st, 65536, 3)


def test_launch_chunk_of_the_three_qubit_launcher_is_crossed(gpu):
    """512 + 3 three-qubit items: two launches of launch3, same assertion across its boundary."""
    from fbx import synthetic, tomography
    design, _, e0, c0 = synthetic.process_batch(3, "sic", 3)
    e, c = _wrapped(e0, c0, 512)
    got, st = tomography.pgdb_process_estimate_batch(design, e, c, mode="fixed", max_iters=1, return_stats=True, trace_iters=1)
    _assert_wraps(got, st, 512, 3)


TRACE = 8


@pytest.fixture(scope="module")
def staged_700(gpu):
    """The 700-item batch of tests/test_pgdb_gpu.py::test_pipelined_host_entry_point_equals_the_staged_one on pageable
    arrays (the staged path), every output requested."""
    from fbx import synthetic, tomography
    design, _, e, c = synthetic.process_batch(2, "sic", 700)
    want, st = tomography.pgdb_process_estimate_batch(design, e, c, return_stats=True, trace_iters=TRACE)
    work = np.stack([st[k] for k in ("jacobi_sweeps", "eig_terms", "cost_evals", "power_sum_passes")], axis=1)
    for a in (want, work, st["trace"]):
        a.setflags(write=False)
    return design, e, c, want, work, st["trace"]


@pytest.mark.parametrize("given", ["none", "work_and_trace"])
def test_pipelined_path_with_optional_outputs_absent(gpu, staged_700, given):
    """fbx_pgdb_process_ex on page-locked buffers, two stages on two streams (256 + 444), with NULL for the optional outputs:
    the Choi matrices equal the staged path's bit for bit, and so do the outputs that were asked for."""
    design, e, c, want, want_work, want_trace = staged_700
    B = 700
    pe, pc = gpu.pinned_copy(e), gpu.pinned_copy(c)
    out = gpu.pinned_empty((B, 16, 16), np.complex128)
    out[...] = np.nan
    work = np.full((B, 4), -1, dtype=np.int32) if given == "work_and_trace" else None
    trace = np.full((B, TRACE, 2), -1, dtype=np.int32) if given == "work_and_trace" else None
    with gpu.option("pgdb_host_chunk", 256.0):
        gpu.check(gpu.lib().fbx_pgdb_process_ex(design.handle, B, gpu.dptr(pe), gpu.dptr(pc), 1, gpu.MODE_CONVERGE, 0, -1.0,
                                                gpu.dptr(out.view(np.float64)), None, None, None, None, gpu.iptr(work),
                                                gpu.iptr(trace), TRACE if trace is not None else 0))
    assert np.array_equal(out, want)
    if given == "work_and_trace":
        assert np.array_equal(work, want_work) and np.array_equal(trace, want_trace)


def test_page_locked_counters_of_the_binned_run_go_with_the_workspace(gpu):
    """The binned relaunch of the lane-per-item kernel reads its counters back into page-locked scratch of the calling thread:
    released with fbx_release_workspace, there again for the next call, and the results are those of the persistent kernel."""
    from fbx import synthetic, tomography
    design, _, e, c = synthetic.process_batch(1, "sic", 3000 + 5)
    kw = dict(return_stats=True, trace_iters=4)
    with gpu.option("pgdb_packed_1q", 2.0):
        with gpu.option("pgdb1_binned", 2.0):
            first, fst = tomography.pgdb_process_estimate_batch(design, e, c, **kw)
            gpu.release_workspace()
            again, ast = tomography.pgdb_process_estimate_batch(design, e, c, **kw)
        with gpu.option("pgdb1_binned", 0.0):
            ref, rst = tomography.pgdb_process_estimate_batch(design, e, c, **kw)
    assert np.array_equal(first, again) and np.array_equal(first, ref)
    for k in STATS:
        assert np.array_equal(fst[k], ast[k]) and np.array_equal(fst[k], rst[k]), k


def test_three_qubit_cost_grad_twice_without_a_synchronisation(gpu):
    """fbx_pgdb_cost_grad_dev for 3 qubits keeps n / p of every setting in a workspace of the calling thread between its two
    passes.  Two calls queued back to back, the second larger (the workspace regrows while the first kernel may still run):
    both results equal those of the same calls with a synchronisation after each."""
    from fbx import synthetic, tomography
    design, _, e, c = synthetic.process_batch(3, "sic", 7)
    nv = tomography.normalised_counts(e, c)
    rng = np.random.default_rng(11)
    h = rng.standard_normal((7, 64, 64)) + 1j * rng.standard_normal((7, 64, 64))
    est = np.eye(64) / 8 + 0.002 * (h + h.conj().transpose(0, 2, 1))
    calls = [(nv[:2], est[:2]), (nv[2:], est[2:])]           # B = 2, then B = 5
    lib, DB = gpu.lib(), gpu.DeviceBuffer

    def run(synchronise):
        gpu.release_workspace()                               # the workspace starts empty: the second call has to grow it
        ins = [(DB.from_array(n), DB.from_array(np.ascontiguousarray(x).view(np.float64))) for n, x in calls]
        outs = [(DB(8 * len(n)), DB(16 * 64 * 64 * len(n))) for n, _ in calls]
        try:
            for (d_n, d_x), (d_c, d_g), (n, _) in zip(ins, outs, calls):
                gpu.check(lib.fbx_pgdb_cost_grad_dev(design.handle, len(n), d_n.ptr, d_x.ptr, 1e-6, d_c.ptr, d_g.ptr))
                if synchronise:
                    gpu.synchronize()
            return [(d_c.to_array(np.float64, (len(n),)), d_g.to_array(np.complex128, (len(n), 64, 64)))
                    for (d_c, d_g), (n, _) in zip(outs, calls)]
        finally:
            for pair in ins + outs:
                for b in pair:
                    b.free()

    want, got = run(True), run(False)
    for (wc, wg), (gc, gg) in zip(want, got):
        assert np.isfinite(wc).all() and np.abs(wg).max() > 0
        assert np.array_equal(wc, gc) and np.array_equal(wg, gg)
    # and they are what the host-pointer form computes
    hc, hg = tomography.cost_and_gradient_batch(design, nv, est)
    assert np.array_equal(np.concatenate([g[0] for g in got]), hc) and np.array_equal(np.concatenate([g[1] for g in got]), hg)
