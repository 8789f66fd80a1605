"""world_size-2 runs of the sharded batch path on CPU: contiguous partition, no data-path collective,
one all-gather of result slabs, the summary all-reduce.  On a GPU node the communicator is libfbx's
RCCL one (fbx.parallel.RcclComm); here the SAME partition / gather / summary code (fbx.parallel.
run_sharded, reduce_summary) runs over (a) a gloo-backed stand-in with the communicator interface
and (b) the file rendezvous that hands the RCCL id around (and is bench.py's barrier of last resort).
The per-shard compute is the CPU oracle (the HIP library needs a GPU)."""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


class GlooComm:
    """torch.distributed(gloo) behind the communicator interface of fbx.parallel (test stand-in for RcclComm)."""
    backend = "gloo"

    def __init__(self, dist, torch):
        self.dist, self.torch = dist, torch
        self.rank, self.world = dist.get_rank(), dist.get_world_size()

    def allgather(self, arr):
        a = np.ascontiguousarray(arr)
        t = self.torch.from_numpy(a.view(np.uint8).reshape(-1).copy())
        outs = [self.torch.empty_like(t) for _ in range(self.world)]
        self.dist.all_gather(outs, t)
        return np.stack([o.numpy().view(a.dtype).reshape(a.shape) for o in outs])

    def allreduce(self, vec, op="sum"):
        t = self.torch.from_numpy(np.array(vec, dtype=np.float64, copy=True))
        self.dist.all_reduce(t, op={"sum": self.dist.ReduceOp.SUM, "max": self.dist.ReduceOp.MAX,
                                    "min": self.dist.ReduceOp.MIN}[op])
        return t.numpy()

    def barrier(self):
        self.dist.barrier()


def _check_sharded(comm, out_dir):
    from fbx import synthetic
    from fbx.parallel import reduce_summary, run_sharded, shard_bounds
    from fbx_oracle import design as od, estimators as oe
    design, _, e, c = synthetic.process_batch(1, "sic", 7)          # 7 items: ragged split 4 + 3
    o = od.process_design(1, "sic")

    def estimate(eb, cb):
        return np.array([oe.linear_inv_process_estimate(o, eb[i]) for i in range(eb.shape[0])]).reshape(-1, 4, 4)

    full, (lo, hi) = run_sharded(estimate, [e, c], comm)
    assert (lo, hi) == shard_bounds(7, comm.rank, comm.world)
    # max-over-ranks timing reduction as in bench.py
    assert comm.allreduce([float(comm.rank + 1)], "max")[0] == comm.world
    # whole-job summary: sum of the local item counts and traces, max of the local block length
    local = full[lo:hi]
    sums, maxima = reduce_summary([hi - lo, float(np.trace(local, axis1=1, axis2=2).real.sum())], [hi - lo], comm)
    assert sums[0] == 7 and abs(sums[1] - np.trace(full, axis1=1, axis2=2).real.sum()) < 1e-12 and maxima[0] == -(-7 // comm.world)
    # without the gather every rank keeps its block only
    part, _ = run_sharded(estimate, [e, c], comm, gather=False)
    assert part.shape[0] == hi - lo and np.array_equal(part, local)
    np.save(os.path.join(out_dir, f"full_{comm.backend}_{comm.rank}.npy"), full)
    comm.barrier()


def _gloo_worker(rank, world, port, out_dir):
    for p in (os.path.join(ROOT, "forest-benchmarking_amd"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _check_sharded(GlooComm(dist, torch), out_dir)
    dist.destroy_process_group()


def _files_worker(rank, world, rdzv_dir, out_dir):
    for p in (os.path.join(ROOT, "forest-benchmarking_amd"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    from fbx.parallel import FileRendezvous, HostComm
    r = FileRendezvous(rank, world, directory=rdzv_dir, timeout=60, join_timeout=0.5)
    # the hand-off RcclComm needs: rank 0's 128-byte id reaches everybody
    ident = bytes(range(128)) if rank == 0 else b""
    assert r.allgather(ident, tag="rccl_id")[0] == bytes(range(128))
    comm = HostComm(r)
    comm.barrier = r.barrier                    # (HostComm.barrier also synchronises the GPU stream)
    _check_sharded(comm, out_dir)
    r.close()


def _expected():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from fbx import synthetic
    from fbx_oracle import design as od, estimators as oe
    _, _, e, _ = synthetic.process_batch(1, "sic", 7)
    o = od.process_design(1, "sic")
    return np.array([oe.linear_inv_process_estimate(o, e[i]) for i in range(7)])


def test_two_rank_sharding_gloo(tmp_path):
    # torch is imported by the workers only: in this process its own HIP runtime and RCCL would shadow the ones
    # libfbx.so loads for the GPU tests that run after this one
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    a = np.load(tmp_path / "full_gloo_0.npy"); b = np.load(tmp_path / "full_gloo_1.npy")
    assert a.shape == (7, 4, 4) and np.array_equal(a, b)
    assert np.allclose(a, _expected(), atol=1e-14)


def test_two_rank_sharding_file_rendezvous(tmp_path):
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    rd = str(tmp_path / "rdzv")
    procs = [ctx.Process(target=_files_worker, args=(r, 2, rd, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    a = np.load(tmp_path / "full_host-files_0.npy"); b = np.load(tmp_path / "full_host-files_1.npy")
    assert np.array_equal(a, b) and np.allclose(a, _expected(), atol=1e-14)
    assert not os.path.exists(rd)               # every rank removed what it published


def test_file_rendezvous_ignores_a_stale_directory(tmp_path):
    """A directory left behind by a failed attempt (same path: torchrun restarts, a reused FBX_RDZV_DIR) holds a
    generation marker, an RCCL id and join / ok files of ranks that no longer exist.  The new attempt must not
    read any of it: rank 0 opens a fresh generation, a rank that saw the stale marker first re-joins."""
    import multiprocessing as mp
    rd = tmp_path / "rdzv"
    rd.mkdir(mode=0o700)
    (rd / "gen").write_text("deadbeefdeadbeef")
    for name in ("deadbeefdeadbeef.join.0", "deadbeefdeadbeef.join.1", "deadbeefdeadbeef.rccl_ok.1", "close.0"):
        (rd / name).write_bytes(b"1")
    (rd / "deadbeefdeadbeef.ack.0").write_bytes(b"rank0,0123456789abcdef")       # a complete-looking dead generation
    (rd / "deadbeefdeadbeef.rccl_id.0").write_bytes(b"\xff" * 128 + b"|")
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_files_worker, args=(r, 2, str(rd), str(tmp_path))) for r in (1, 0)]
    procs[0].start()                            # rank 1 first: it finds only the stale generation
    import time
    time.sleep(1.0)
    procs[1].start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    a = np.load(tmp_path / "full_host-files_0.npy"); b = np.load(tmp_path / "full_host-files_1.npy")
    assert np.array_equal(a, b) and np.allclose(a, _expected(), atol=1e-14)
    assert not os.path.exists(rd)


def _late_worker(rank, world, rdzv_dir, out_dir, delay):
    import time
    time.sleep(delay)
    _files_worker(rank, world, rdzv_dir, out_dir)


def test_file_rendezvous_three_ranks_with_a_straggler(tmp_path):
    """Rank 0 acknowledges a generation only after EVERY rank has joined: with three ranks the early non-zero rank
    waits for the straggler well beyond ``join_timeout`` (0.5 s in _files_worker; the straggler comes 2 s late) and
    must keep its place in the live generation instead of writing it off as stale (round-3 regression: all three
    ranks then failed, 'gen never appeared' / 'rank 1 never published')."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    rd = str(tmp_path / "rdzv")
    procs = [ctx.Process(target=_late_worker, args=(r, 3, rd, str(tmp_path), 2.0 if r == 2 else 0.0)) for r in range(3)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    full = [np.load(tmp_path / f"full_host-files_{r}.npy") for r in range(3)]
    assert all(np.array_equal(full[0], f) for f in full[1:]) and np.allclose(full[0], _expected(), atol=1e-14)
    assert not os.path.exists(rd)


def test_shard_bounds_cover_the_batch_exactly():
    from fbx.parallel import shard_bounds
    for n in (0, 1, 7, 1024, 65536, 65537):
        for world in (1, 2, 3, 4, 8):
            blocks = [shard_bounds(n, r, world) for r in range(world)]
            assert blocks[0][0] == 0 and blocks[-1][1] == n
            assert all(b[1] == nb[0] for b, nb in zip(blocks, blocks[1:]))
            assert max(hi - lo for lo, hi in blocks) == -(-n // world)


def test_file_rendezvous_reports_a_persistent_file_system_error_at_the_deadline(tmp_path, monkeypatch):
    """Round-5 advisor finding: an OSError from the join / ack files (ENOSPC, EACCES, a stale NFS handle) sent a rank back to
    re-read ``gen`` without looking at the clock -- 100 % CPU for ever.  Now the loop backs off and re-raises the error once the
    deadline has passed."""
    import time
    from fbx import parallel
    d = str(tmp_path / "rdzv")
    os.makedirs(d, mode=0o700)
    with open(os.path.join(d, "gen"), "w") as f:             # a generation somebody opened: rank 1 will try to join it
        f.write("deadbeef")
    calls = {"n": 0}

    def broken_publish(self, payload, tag):
        calls["n"] += 1
        raise OSError(28, "No space left on device")

    monkeypatch.setattr(parallel.FileRendezvous, "_publish", broken_publish)
    t0 = time.monotonic()
    with pytest.raises(OSError) as err:
        parallel.FileRendezvous(1, 2, directory=d, timeout=1.5, join_timeout=0.2)
    dt = time.monotonic() - t0
    assert err.value.errno == 28 and 1.0 < dt < 10.0
    assert calls["n"] < 200                                   # backed off between attempts instead of spinning
