"""The host-pointer half of the C ABI: staging buffers, H2D, the `_dev` form, D2H, synchronise -- one helper (HostIO,
csrc/fbx_common.hpp) behind every entry point.  What such a helper can get wrong is checked here on the smallest shapes:
a host form against its `_dev` form bit for bit, every optional output alone and left out, optional inputs absent, a
zero-length input, an argument error met after the uploads followed by a good call, and page-locked caller buffers.

Every output array is filled with a sentinel byte before the call and carries GUARD sentinel elements behind its
last one: a result must overwrite the body exactly as the reference call does and never touch the tail (a download
with a neighbour's byte count or into a neighbour's slot would)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 8


class In:
    def __init__(self, a):
        self.a = None if a is None else np.ascontiguousarray(a)


class Out:
    def __init__(self, dtype, n, want=True):
        self.dtype, self.n, self.want = np.dtype(dtype), int(n), want


def _sentinel(n, dtype, pinned, lib):
    h = lib.pinned_empty((n,), dtype) if pinned else np.empty(n, dtype)
    h.view(np.uint8)[:] = SENTINEL
    return h


def _run(lib, name, args, dev=False, pinned=False):
    """(return code, [output incl. guard tail, or None where not asked for]) of the host form on numpy (or page-locked)
    arrays, or of the `_dev` form on fbx_malloc buffers filled through fbx_memcpy_h2d and read through fbx_memcpy_d2h."""
    name = name + "_dev" if dev else name
    fn, types = getattr(lib.lib(), name), lib.PROTOTYPES[name]
    assert len(types) == len(args), name
    call, outs, keep = [], [], []
    for t, a in zip(types, args):
        if isinstance(a, In):
            if a.a is None:
                call.append(None)
            elif dev:
                keep.append(lib.DeviceBuffer.from_array(a.a)); call.append(keep[-1].ptr)
            else:
                keep.append(lib.pinned_copy(a.a) if pinned else a.a); call.append(keep[-1].ctypes.data_as(t))
        elif isinstance(a, Out):
            if not a.want:
                call.append(None); outs.append(None); continue
            h = _sentinel(a.n + GUARD, a.dtype, pinned and not dev, lib)
            if dev:
                outs.append(lib.DeviceBuffer.from_array(h)); call.append(outs[-1].ptr)
            else:
                outs.append(h); call.append(h.ctypes.data_as(t))
        else:
            call.append(a)
    rc = fn(*call)
    if dev:
        lib.synchronize()
        outs = [None if o is None else o.to_array(a.dtype, (a.n + GUARD,))
                for o, a in zip(outs, [x for x in args if isinstance(x, Out)])]
    return rc, outs


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def _check_written(outs):
    for o in outs:
        if o is not None:
            assert (o[-GUARD:].view(np.uint8) == SENTINEL).all(), "guard tail overwritten"
            assert not (o[:-GUARD].view(np.uint8) == SENTINEL).all(), "output never written"


def _want(args, keep):
    """`args` with the k-th output kept only when keep(k)."""
    k, res = 0, []
    for a in args:
        if isinstance(a, Out):
            a = Out(a.dtype, a.n, keep(k)); k += 1
        res.append(a)
    return res


# ---------------------------------------------------------------------------------------------- the cases, built once
def _fit_args(weights="given"):
    B, K = 3, 5
    rng = np.random.default_rng(11)
    x = np.arange(1.0, K + 1)
    amp, dec, base = np.array([0.5, 0.4, 0.45]), np.array([0.9, 0.8, 0.95]), np.array([0.5, 0.25, 0.3])
    y = base[:, None] + amp[:, None] * dec[:, None] ** x[None, :] + 1e-3 * rng.standard_normal((B, K))
    guess = np.stack([amp * 1.1, dec * 0.97, base * 0.9], axis=1)
    w = {"given": 1.0 + rng.random((B, K)), "ones": np.ones((B, K)), None: None}[weights]
    return [0, B, K, In(x), 0, In(y), In(w), In(guess), 7, 1e-10, 1e-10, 200,
            Out("f8", B * 3), Out("f8", B * 9), Out("f8", B), Out("f8", B), Out("i4", B), Out("i4", B), Out("f8", B)]


def _rpe_moments():
    B, K = 2, 3
    k = 2.0 ** np.arange(K)
    phi = np.array([0.7, 4.1])
    x, y = 0.9 * np.cos(phi[:, None] * k), 0.9 * np.sin(phi[:, None] * k)
    err = np.full((B, K), 0.05)
    return [B, K, In(x), In(y), In(err), In(err), 0, In(None), In(None), In(None), In(None), 0,
            Out("f8", B), Out("i4", B), Out("f8", B * K * 2)]


def _rpe_shots():
    B, K, shots, nq = 2, 3, 16, 2
    rng = np.random.default_rng(12)
    xb = (rng.random((B, K, shots, nq)) < 0.25).astype(np.uint8)
    yb = (rng.random((B, K, shots, nq)) < 0.35).astype(np.uint8)
    return [nq, B, K, shots, In(xb), In(yb), 0, 1, 0, Out("f8", B), Out("i4", B), Out("f8", B * K * 2), Out("f8", B * K * 4)]


def _circular():
    R, B = 4, 3
    ang = np.random.default_rng(13).random((R, B)) * 6.0
    ang[1, 2] = np.nan
    return [R, B, In(ang), Out("f8", B), Out("f8", B), Out("i4", B)]


def _qv_circuits(n, B, L):
    rng = np.random.default_rng(14)
    pairs = np.array([[[l % n, (l + 1) % n] for l in range(L)] for _ in range(B)], dtype=np.uint8).reshape(B, L, 2)
    g = rng.standard_normal((B, L, 4, 4)) + 1j * rng.standard_normal((B, L, 4, 4))
    gates = np.linalg.qr(g)[0] if L else g
    return pairs, np.ascontiguousarray(gates, dtype=np.complex128)


def _qv_heavy(L=2):
    n, B = 3, 2
    pairs, gates = _qv_circuits(n, B, L)
    return [n, B, L, In(pairs if L else None), In(gates.view(np.float64) if L else None),
            Out("f8", B * 8), Out("f8", B), Out("u8", B), Out("f8", B), Out("i4", B)]


def _qv_count(mask):
    n, B, shots = 3, 2, 10
    bits = (np.random.default_rng(15).random((B, shots, n)) < 0.5).astype(np.uint8)
    return [n, B, shots, In(bits), In(mask), Out("i8", B)]


def _calibrate(index="given"):
    B, m = 2, 5
    rng = np.random.default_rng(16)
    e, se = rng.uniform(-1, 1, (B, m)), rng.uniform(0.01, 0.05, (B, m))
    if index == "given":
        idx, n_cal = np.array([0, 1, 0, 2, 1], dtype=np.int32), 3
    else:
        idx, n_cal = (np.arange(m, dtype=np.int32) if index == "identity" else None), m
    cm, cv = rng.uniform(0.8, 1.0, n_cal), rng.uniform(1e-4, 1e-3, n_cal)
    return [B, m, In(e), In(se), In(idx), n_cal, In(cm), In(cv), Out("f8", B * m), Out("f8", B * m)]


def _shots():
    nq, S, shots = 2, 5, 24
    rng = np.random.default_rng(17)
    bits = (rng.random((S, shots, nq)) < 0.4).astype(np.uint8)
    mask = np.array([[1, 0], [0, 1], [1, 1], [0, 0], [1, 1]], dtype=np.uint8)
    return [nq, S, shots, In(bits), In(mask), In(rng.uniform(0.5, 1.5, S)), 0, Out("f8", S), Out("f8", S)]


def _rb_survival():
    dim, S = 4, 3
    rng = np.random.default_rng(18)
    return [dim, S, In(rng.uniform(0.2, 0.9, (S, dim - 1))), In(rng.uniform(0.01, 0.03, (S, dim - 1))), 100, Out("f8", S), Out("f8", S)]


def _chernoff():
    B = 3
    rng = np.random.default_rng(19)
    g = rng.standard_normal((2, B, 2, 2)) + 1j * rng.standard_normal((2, B, 2, 2))
    rho = g @ g.conj().transpose(0, 1, 3, 2)
    rho /= np.trace(rho, axis1=2, axis2=3)[..., None, None]
    rho = np.ascontiguousarray(rho).view(np.float64)
    return [1, B, In(rho[0]), In(rho[1]), 0, 0.0, 50, 1e-12, Out("f8", B), Out("f8", B), Out("f8", B), Out("i4", B)]


_CASES = {}


def _cases(lib):
    """name -> argument list; built on first use (the heavy mask that fbx_qv_count_heavy reads comes from the device)."""
    if not _CASES:
        rc, outs = _run(lib, "fbx_qv_heavy_outputs", _qv_heavy())
        assert rc == lib.FBX_OK
        _CASES.update({
            "fbx_curve_fit": _fit_args(), "fbx_rpe_phase": _rpe_moments(), "fbx_rpe_from_shots": _rpe_shots(),
            "fbx_circular_stats": _circular(), "fbx_qv_heavy_outputs": _qv_heavy(), "fbx_qv_count_heavy": _qv_count(outs[2][:-GUARD]),
            "fbx_calibrate_expectations": _calibrate(), "fbx_shots_to_moments": _shots(), "fbx_rb_survival": _rb_survival(),
            "fbx_chernoff_bound": _chernoff()})
    return _CASES


NAMES = ["fbx_curve_fit", "fbx_rpe_phase", "fbx_rpe_from_shots", "fbx_circular_stats", "fbx_qv_heavy_outputs", "fbx_qv_count_heavy",
         "fbx_calibrate_expectations", "fbx_shots_to_moments", "fbx_rb_survival", "fbx_chernoff_bound"]


# ---------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("name", NAMES)
def test_host_form_equals_dev_form_bit_for_bit(gpu, name):
    args = _cases(gpu)[name]
    rc_h, host = _run(gpu, name, args)
    rc_d, dev = _run(gpu, name, args, dev=True)
    assert rc_h == gpu.FBX_OK and rc_d == gpu.FBX_OK, gpu.lib().fbx_last_error()
    _check_written(host)
    for k, (h, d) in enumerate(zip(host, dev)):
        assert _same(h, d), (name, k, h, d)


@pytest.mark.parametrize("name", ["fbx_curve_fit", "fbx_rpe_from_shots"])
def test_page_locked_caller_buffers(gpu, name):
    """Inputs and outputs from fbx_host_alloc: the copies are asynchronous to the host, the results are the same."""
    args = _cases(gpu)[name]
    rc, plain = _run(gpu, name, args)
    rc_p, pinned = _run(gpu, name, args, pinned=True)
    assert rc == gpu.FBX_OK and rc_p == gpu.FBX_OK, gpu.lib().fbx_last_error()
    _check_written(pinned)
    for k, (a, b) in enumerate(zip(plain, pinned)):
        assert _same(a, b), (name, k)


@pytest.mark.parametrize("name", ["fbx_curve_fit", "fbx_qv_heavy_outputs"])
def test_every_optional_output_alone_and_left_out(gpu, name):
    args = _cases(gpu)[name]
    rc, full = _run(gpu, name, args)
    assert rc == gpu.FBX_OK, gpu.lib().fbx_last_error()
    _check_written(full)
    for k in range(len(full)):
        for keep in (lambda j: j == k, lambda j: j != k):           # output k alone; every output but k
            rc, part = _run(gpu, name, _want(args, keep))
            assert rc == gpu.FBX_OK, gpu.lib().fbx_last_error()
            for j, (p, f) in enumerate(zip(part, full)):
                assert (p is None) == (not keep(j))
                if p is not None:
                    assert _same(p, f), (name, "asked for", k, "slot", j)      # body as in the full call, guard tail intact


def test_optional_inputs_absent(gpu):
    for name, absent, spelled_out in (("fbx_curve_fit", _fit_args(None), _fit_args("ones")),
                                      ("fbx_calibrate_expectations", _calibrate(None), _calibrate("identity"))):
        rc_a, a = _run(gpu, name, absent)
        rc_s, s = _run(gpu, name, spelled_out)
        assert rc_a == gpu.FBX_OK and rc_s == gpu.FBX_OK, gpu.lib().fbx_last_error()
        _check_written(a)
        for k, (p, q) in enumerate(zip(a, s)):
            assert _same(p, q), (name, k)


def test_zero_length_input(gpu):
    """L = 0, pairs = gates = NULL: the staging still hands the `_dev` form two (empty) device blocks."""
    rc, outs = _run(gpu, "fbx_qv_heavy_outputs", _want(_qv_heavy(L=0), lambda j: j == 0))
    assert rc == gpu.FBX_OK, gpu.lib().fbx_last_error()
    _check_written(outs)
    want = np.zeros((2, 8)); want[:, 0] = 1.0
    assert np.array_equal(outs[0][:-GUARD].reshape(2, 8), want)


def test_error_after_staging_then_reuse(gpu):
    """An argument error that only the `_dev` form sees, after the uploads were queued: the call waits for them before its staging
    blocks go back to the pool, writes nothing, and the next call is as good as the one before."""
    from fbx import synthetic, tomography
    design, _, e, c = synthetic.process_batch(1, "pauli", 2)
    nv = tomography.normalised_counts(e, c)
    choi = np.ascontiguousarray(np.broadcast_to(np.eye(4, dtype=np.complex128) / 2, (2, 4, 4))).view(np.float64)

    def cost_grad(eps):
        return _run(gpu, "fbx_pgdb_cost_grad", [design.handle, 2, In(nv), In(choi), eps, Out("f8", 2), Out("f8", 2 * 16 * 2)])

    rc, before = cost_grad(0.0)
    assert rc == gpu.FBX_OK, gpu.lib().fbx_last_error()
    _check_written(before)
    rc, bad = cost_grad(-1.0)
    assert rc == gpu.FBX_ERR_BAD_ARG
    assert all((o.view(np.uint8) == SENTINEL).all() for o in bad)
    rc, after = cost_grad(0.0)
    assert rc == gpu.FBX_OK and all(_same(a, b) for a, b in zip(before, after))

    def unitaries(kind):
        return _run(gpu, "fbx_random_operators", [kind, 2, 0, 2, 1234, 0, Out("f8", 2 * 2 * 2 * 2)])

    rc, before = unitaries(gpu.RAND_UNITARY)
    assert rc == gpu.FBX_OK, gpu.lib().fbx_last_error()
    _check_written(before)
    rc, bad = unitaries(9)
    assert rc == gpu.FBX_ERR_BAD_ARG and (bad[0].view(np.uint8) == SENTINEL).all()
    rc, after = unitaries(gpu.RAND_UNITARY)
    assert rc == gpu.FBX_OK and _same(before[0], after[0])
