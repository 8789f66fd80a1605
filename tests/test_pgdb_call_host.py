"""The PGDB call record and the stage plan of the pipelined host-pointer entry point (csrc/fbx_pgdb_call.hpp), compiled for the
host by tests/host_harness (test infrastructure only -- the package never loads it).  `slice(b0, nb)` is the one place that
knows the per-item strides of a call's nine arrays; the plan decides which items run on which stream over which workspace
slots.  No GPU: tests/test_pgdb_launch_path_gpu.py checks the launch loops that use them."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "host_harness")
FIELDS = ["des", "B", "e", "c", "tp", "mode", "max_iters", "choi", "it", "dy", "bt", "cost", "sw", "trace", "trace_iters",
          "launch_stream", "ws_items", "ws_offset", "total_batch", "m", "DD"]
OPTIONAL = ["it", "dy", "bt", "cost", "sw"]
i64p = ctypes.POINTER(ctypes.c_int64)
# settings m and Choi dimension D of the 1-qubit Pauli, 2-qubit SIC and 3-qubit SIC process designs
DESIGNS = [(18, 4), (240, 16), (4032, 64)]
HOST_CHUNK, BULK = 4096, 65536             # defaults of the product: fbx_set_option("pgdb_host_chunk"), launch_pgdb's launch chunk


@pytest.fixture(scope="module")
def lib():
    so_path = os.path.join(HARNESS, "libpgdb_call_host.so")
    src = os.path.join(HARNESS, "pgdb_call_host.cpp")
    hdr = os.path.join(ROOT, "forest-benchmarking_amd", "csrc", "fbx_pgdb_call.hpp")
    if not os.path.exists(so_path) or os.path.getmtime(so_path) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", src, "-o", so_path])
    L = ctypes.CDLL(so_path)
    L.pgdb_call_host_slice.argtypes = [i64p, ctypes.c_double, ctypes.c_int, i64p, i64p, ctypes.POINTER(ctypes.c_double)]
    L.pgdb_call_host_slice.restype = None
    L.pgdb_call_host_plan.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, i64p, ctypes.c_int, i64p]
    assert L.pgdb_call_host_nfields() == len(FIELDS)
    return L


def _slice(lib, call, *cuts):
    """call: dict over FIELDS + 'eig_rel_tol'; cuts: (b0, nb) pairs applied one after the other."""
    fin = np.array([call[k] for k in FIELDS], dtype=np.int64)
    cut = np.array(cuts, dtype=np.int64).reshape(-1)
    out = np.zeros(len(FIELDS), dtype=np.int64)
    tol = ctypes.c_double(0.0)
    lib.pgdb_call_host_slice(fin.ctypes.data_as(i64p), call["eig_rel_tol"], len(cuts), cut.ctypes.data_as(i64p),
                             out.ctypes.data_as(i64p), ctypes.byref(tol))
    got = dict(zip(FIELDS, (int(v) for v in out)))
    got["eig_rel_tol"] = tol.value
    return got


def _call(B, m, D, absent=(), trace_iters=0):
    """A call on real buffers of B items (kept alive in the returned list); `absent` optional outputs are NULL."""
    bufs = {"e": np.zeros((B, m)), "c": np.zeros((B, m)), "choi": np.zeros((B, D, D, 2)), "it": np.zeros(B, np.int32),
            "dy": np.zeros(B, np.int32), "bt": np.zeros(B, np.int32), "cost": np.zeros(B), "sw": np.zeros((B, 4), np.int32),
            "trace": np.zeros((B, max(trace_iters, 1), 2), np.int32)}
    call = {k: (0 if k in absent or (k == "trace" and not trace_iters) else a.ctypes.data) for k, a in bufs.items()}
    call.update(des=0x1000, B=B, tp=1, mode=0x101, max_iters=7, trace_iters=trace_iters, launch_stream=0x2000, ws_items=11,
                ws_offset=5, total_batch=3 * B, m=m, DD=D * D, eig_rel_tol=1e-9)
    return call, bufs


def _expected(call, b0, nb):
    m, DD, ti = call["m"], call["DD"], call["trace_iters"]
    step = {"e": 8 * m, "c": 8 * m, "choi": 16 * DD, "it": 4, "dy": 4, "bt": 4, "cost": 8, "sw": 16, "trace": 8 * ti}
    want = dict(call)
    want["B"] = nb
    for k, bytes_per_item in step.items():
        want[k] = call[k] + b0 * bytes_per_item if call[k] else 0
    return want


@pytest.mark.parametrize("m,D", DESIGNS)
@pytest.mark.parametrize("trace_iters", [0, 3])
def test_slice_moves_every_array_by_its_own_stride(lib, m, D, trace_iters):
    B = 7
    for absent in [()] + [(k,) for k in OPTIONAL] + [tuple(OPTIONAL)]:
        call, bufs = _call(B, m, D, absent, trace_iters)
        for b0, nb in [(0, B), (0, 2), (3, 2), (6, 1), (4, 0), (B, 0)]:
            got = _slice(lib, call, (b0, nb))
            assert got == _expected(call, b0, nb), (absent, b0, nb)
            for k in absent:
                assert got[k] == 0
            if not trace_iters:
                assert got["trace"] == 0
        del bufs


@pytest.mark.parametrize("m,D", DESIGNS)
def test_slices_compose(lib, m, D):
    B = 9
    call, bufs = _call(B, m, D, absent=("dy",), trace_iters=2)
    for a, n in [(0, 9), (2, 6), (8, 1)]:
        for b, k in itertools.product(range(n + 1), range(3)):
            if b + k <= n:
                assert _slice(lib, call, (a, n), (b, k)) == _slice(lib, call, (a + b, k)) == _expected(call, a + b, k)
    del bufs


def _plan(lib, B, chunk, two_streams, bulk=0):
    st = np.zeros((64, 4), dtype=np.int64)
    ws = ctypes.c_int64(0)
    n = lib.pgdb_call_host_plan(B, chunk, int(two_streams), bulk, st.ctypes.data_as(i64p), 64, ctypes.byref(ws))
    assert 0 < n <= 64
    return [tuple(int(v) for v in row) for row in st[:n]], ws.value


def _check_plan(stages, ws_total, B, two_streams):
    # the stages tile [0, B) exactly once, in order
    at = 0
    for b0, nb, second, off in stages:
        assert b0 == at and nb >= 0 and off >= 0
        at += nb
    assert at == B and not stages[0][2]                      # (the first stage runs on the calling thread's stream)
    # workspace slots: stages on different streams never share one, and ws_total covers every range
    for (b0, nb, s, off), (b0_, nb_, s_, off_) in itertools.combinations(stages, 2):
        if s != s_:
            assert off + nb <= off_ or off_ + nb_ <= off, (stages, ws_total)
    assert all(off + nb <= ws_total for _, nb, _, off in stages)
    if not two_streams:
        assert not any(s for _, _, s, _ in stages)


@pytest.mark.parametrize("two_streams", [True, False])
def test_stage_plan_tiles_the_batch_on_disjoint_workspace_ranges(lib, two_streams):
    for B in range(1, 41):                                   # chunk 4, bulk launches of 8: every shape of plan
        stages, ws_total = _plan(lib, B, 4, two_streams, bulk=8)
        _check_plan(stages, ws_total, B, two_streams)
        assert all(nb <= 8 for _, nb, _, _ in stages)
    CH = HOST_CHUNK
    for B in (2 * CH - 1, 2 * CH, 4 * CH - 1, 4 * CH, CH + BULK + 1):
        stages, ws_total = _plan(lib, B, CH, two_streams)
        _check_plan(stages, ws_total, B, two_streams)
        assert stages[0][1] == min(CH, B // 2)
        assert all(nb <= BULK for _, nb, _, _ in stages)


def test_stage_plan_is_the_one_the_pipeline_tests_ran_with(lib):
    """Worked out by hand from the inline code this function replaced (first = min(chunk, B / 2); last = chunk when
    B >= 4 chunk, else none; the rest in launches of 65 536 on the second stream at workspace offset `first`), for the
    shapes of tests/test_pgdb_gpu.py::test_pipelined_host_entry_point_*: 700 items with chunk 256, 2700 with chunk 300
    (2 qubits: two compute streams)."""
    assert _plan(lib, 700, 256, True) == ([(0, 256, 0, 0), (256, 444, 1, 256)], 700)
    assert _plan(lib, 2700, 300, True) == ([(0, 300, 0, 0), (300, 2100, 1, 300), (2400, 300, 0, 0)], 2400)
    # one compute stream (3 qubits): every stage at workspace offset 0, as many slots as the largest stage
    assert _plan(lib, 1300, 300, False) == ([(0, 300, 0, 0), (300, 700, 0, 0), (1000, 300, 0, 0)], 700)
    # and a bulk of more than one launch: 4096 | 65536 | 30464 | 4096 of 104192 items
    assert _plan(lib, 104192, 4096, True) == ([(0, 4096, 0, 0), (4096, 65536, 1, 4096), (69632, 30464, 1, 4096),
                                               (100096, 4096, 0, 0)], 4096 + 65536)
