"""fbx_native_trajectories and fbx_native_unitary on the GPU (csrc/fbx_native.hip) against the host mirror
fbx.native_circuit, which is written from the contract in include/fbx.h.

Error counts are compared exactly: they depend on the stream alone.  Probabilities are compared with the mirror run on the
restated Paulis, within tests/native_cases.py:TOL = 8 x 4.5e-16 -- the mirror's own largest deviation (4.44e-16) from a 50-digit
mpmath evaluation of the same trajectories on these circuits, measured on the CPU, times a factor of 8 (the device makes the same
roundings in another order, so about 2 x is expected; the rest is margin for the tail over the ~10^5 values compared).  The
compiled adders are 293-709 gates long instead of 8 and the mirror's deviation on them is 3.1e-15 to 1.13e-14 (the rounding of
cos and sin of pi/4 enters every RX(+-pi/2) with one sign): each adder circuit is held to 8 x the mirror's deviation on that
circuit, measured the same way (tests/native_cases.py:ADDER_MIRROR_DEVIATION; 2.1e-15 for the noisy statistics case).  Unitaries
are compared up to a global phase with the reference's own tolerance, atol = 1e-12 (its test_compilation.py:49-93)."""
import ctypes as C

import numpy as np
import pytest

import native_cases as cases

pytestmark = pytest.mark.gpu
_cache = {}


def run_case(case):
    """The device (host form, both outputs) and the restatement of one case, computed once per session."""
    key = cases.case_id(case)
    if key not in _cache:
        from fbx import native_circuit as nc
        words, angles, cls, want = cases.restated(case)
        got = nc.native_trajectories(words, angles, case["n"], cases.INPUTS, case["out"], case["T"], cases.CLASS_ERROR, cls, seed=11)
        _cache[key] = (got, want)
    return _cache[key]


# ------------------------------------------------------------------ 1. the stream, 2. the probabilities
@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_error_counts_equal_the_restated_stream(gpu, case):
    got, want = run_case(case)
    assert not got["status"].any()
    assert got["n_errors"].dtype == np.int32 and np.array_equal(got["n_errors"], want["n_errors"])
    # the items of CLASS_ERROR: nothing errs; every gate that exists errs, so every Pauli index is exercised; a mixture
    assert not got["n_errors"][0].any()
    if case["G"]:
        assert (got["n_errors"][1] == (want["paulis"][1] >= 0).sum(axis=2)).all() and got["n_errors"][1].min() >= case["G"] // 2


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_probabilities_equal_the_mirror_on_the_restated_paulis(gpu, case):
    got, want = run_case(case)
    diff = np.abs(got["probs_mean"] - want["probs_mean"])
    print(cases.case_id(case), "largest deviation from the mirror", diff.max(), "allowed", cases.TOL)
    assert got["probs_mean"].shape == (3, 2, 1 << len(case["out"]))
    assert diff.max() <= cases.TOL
    if case["G"] == 0:
        assert (got["probs_mean"][:, :, 0] == 1.0).all() and not got["probs_mean"][:, :, 1:].any()      # |0..0>


# ------------------------------------------------------------------ 3. the unitary
def test_unitary_of_compiled_random_programs(gpu):
    from fbx import compilation, native_circuit as nc
    for n, prog in cases.random_programs():
        words, angles = nc.encode_native(compilation.basic_compile(prog), n)
        cases.assert_close_up_to_global_phase(nc.native_unitary(words, angles, n), compilation.program_unitary(prog, n))


def test_unitary_of_the_compiled_two_bit_adder_and_the_device_argument(gpu):
    from fbx import compilation, native_circuit as nc
    from fbx.classical_logic import ripple_carry_adder as rca
    gates, _ = rca.adder(*rca.default_adder_registers(2))
    body = [g for g in gates if g[0] != "XIN"]                       # the summands are run-time input: not part of a unitary
    want = compilation.program_unitary(body, 6)
    words, angles = nc.encode_native(compilation.basic_compile(body), 6)
    got = nc.native_unitary(words, angles, 6)
    assert got.shape == (64, 64)
    cases.assert_close_up_to_global_phase(got, want)
    cases.assert_close_up_to_global_phase(compilation.program_unitary(body, 6, device=0), want)
    with gpu.DeviceScope() as dev:                                   # the device-pointer form gives the same bits
        d_u = nc.native_unitary_dev(dev, 6, words.size, dev.upload(words), dev.upload(angles))
        assert np.array_equal(d_u.to_array(np.complex128, (64, 64)), got)
    # both teams, on the bit order: CNOT(0, 1) against CNOT(1, 0) embedded in WAVE and WAVE + 1 qubits
    for n in (cases.WAVE, cases.WAVE + 1):
        for pair in ((0, 1), (1, 0), (n - 1, 0)):
            prog = [("CNOT", pair), ("RY", (pair[0],), 0.3)]
            w, a = nc.encode_native(compilation.basic_compile(prog), n)
            cases.assert_close_up_to_global_phase(nc.native_unitary(w, a, n), compilation.program_unitary(prog, n))


# ------------------------------------------------------------------ 4. the noiseless adder
@pytest.mark.parametrize("n_bits,in_x_basis", [(1, False), (1, True), (2, False), (2, True)])
def test_noiseless_compiled_adder(gpu, n_bits, in_x_basis):
    from fbx import native_circuit as nc
    from fbx.classical_logic import ripple_carry_adder as rca
    words, angles, n, out, cls = rca.compiled_adder_circuit(n_bits, in_x_basis=in_x_basis)
    inputs = np.arange(4 ** n_bits, dtype=np.uint64)
    res = nc.native_trajectories(words, angles, n, inputs, out, 1, None, cls, n_errors=False)
    expected = rca.adder_expected_bits(n_bits)
    answer = (expected.astype(np.int64) << np.arange(n_bits, -1, -1)).sum(axis=1)
    weight = res["probs_mean"][0, np.arange(4 ** n_bits), answer]
    tol = cases.adder_tol(n_bits, in_x_basis)                        # 8 x the mirror's own deviation on THIS circuit
    print("smallest weight on the expected answer: 1 -", 1.0 - weight.min(), "allowed", tol, "gates", words.size)
    assert words.size == cases.ADDER_MIRROR_DEVIATION[(n_bits, in_x_basis)][0]
    assert weight.min() >= 1.0 - tol and weight.max() <= 1.0 + tol
    records = rca.simulate_compiled_adder_results(n_bits, in_x_basis=in_x_basis, num_shots=65, seed=5)
    assert records.dtype == np.uint8 and np.array_equal(records, np.repeat(expected[:, None, :], 65, axis=1))


# ------------------------------------------------------------------ 5. repeatability, bit for bit
def _dev_call(gpu, n, words, angles, cls, inputs, out, T, ce, seed, first_item=0, first_input=0, probs=True, errors=True):
    from fbx import native_circuit as nc
    B, P, m = ce.shape[0], inputs.size, len(out)
    with gpu.DeviceScope() as dev:
        res = nc.native_trajectories_dev(dev, n, words.size, dev.upload(words), dev.upload(angles), dev.upload(cls), ce.shape[1], P,
                                         dev.upload(inputs), m, dev.upload(np.asarray(out, dtype=np.uint8)), B, T, dev.upload(ce),
                                         seed, first_item, first_input, probs_mean=probs, n_errors=errors)
        back = {"status": res["status"].to_array(np.int32, (B,))}
        if probs:
            back["probs_mean"] = res["probs_mean"].to_array(np.float64, (B, P, 1 << m))
        if errors:
            back["n_errors"] = res["n_errors"].to_array(np.int32, (B, P, T))
    return back


@pytest.mark.parametrize("n", [6, cases.WAVE + 1])
def test_an_item_repeats_bit_for_bit(gpu, n):
    from fbx import native_circuit as nc
    T, seed = 2 * cases.SEG + 1, 23
    words, angles = nc.encode_native(cases.circuit(n, 8), n)
    cls = nc.native_noise_classes(words)
    inputs = np.array([1, 32, 33, 0], dtype=np.uint64)
    out = [n - 2, 0, 3]
    ce = np.array([[0.2, 0.0, 0.3], [0.05, 0.4, 0.1], [0.5, 0.5, 0.5]])
    base = nc.native_trajectories(words, angles, n, inputs, out, T, ce, cls, seed)

    def same(other, b, r):
        return (np.array_equal(other["probs_mean"], base["probs_mean"][b, r]) and np.array_equal(other["n_errors"], base["n_errors"][b, r])
                and not other["status"].any())
    # another B and a first_item offset; another P and a first_input offset
    assert same(nc.native_trajectories(words, angles, n, inputs, out, T, ce[1:2], cls, seed, first_item=1), slice(1, 2), slice(None))
    assert same(nc.native_trajectories(words, angles, n, inputs[2:], out, T, ce, cls, seed, first_input=2), slice(None), slice(2, 4))
    # the smallest workspace: a chunk per (item, input) pair at width 9
    with gpu.option("native_workspace_mib", 1.0 / 64):
        assert same(nc.native_trajectories(words, angles, n, inputs, out, T, ce, cls, seed), slice(None), slice(None))
    # the device-pointer form, and each output alone
    assert same(_dev_call(gpu, n, words, angles, cls, inputs, out, T, ce, seed), slice(None), slice(None))
    alone = _dev_call(gpu, n, words, angles, cls, inputs, out, T, ce, seed, errors=False)
    assert np.array_equal(alone["probs_mean"], base["probs_mean"])
    alone = _dev_call(gpu, n, words, angles, cls, inputs, out, T, ce, seed, probs=False)
    assert np.array_equal(alone["n_errors"], base["n_errors"])
    assert not np.array_equal(nc.native_trajectories(words, angles, n, inputs, out, T, ce, cls, seed + 1)["n_errors"], base["n_errors"])


# ------------------------------------------------------------------ 6. poisoned items and arguments
def test_poisoned_items_leave_their_neighbours_alone(gpu):
    from fbx import native_circuit as nc
    n, T = 3, cases.SEG + 1
    words, angles = nc.encode_native(cases.circuit(n, 8), n)
    cls = nc.native_noise_classes(words)
    ce = np.array([[0.2, 0.0, 0.3], [0.05, 0.4, 0.1], [0.5, 0.5, 0.5]])
    clean = nc.native_trajectories(words, angles, n, cases.INPUTS, [2, 0], T, ce, cls, 3)
    for bad in (-0.1, 1.5, np.nan):
        dirty = ce.copy()
        dirty[1, 2] = bad
        res = nc.native_trajectories(words, angles, n, cases.INPUTS, [2, 0], T, dirty, cls, 3)
        assert res["status"].tolist() == [0, 1, 0]
        assert np.isnan(res["probs_mean"][1]).all() and not res["n_errors"][1].any()
        for b in (0, 2):
            assert np.array_equal(res["probs_mean"][b], clean["probs_mean"][b]) and np.array_equal(res["n_errors"][b], clean["n_errors"][b])
    # a non-finite angle: refused by the host form, every item poisoned by the device-pointer form
    for bad in (np.nan, np.inf):
        broken = angles.copy()
        broken[2] = bad
        with pytest.raises(ValueError):
            nc.native_trajectories(words, broken, n, cases.INPUTS, [2, 0], T, ce, cls, 3)
        res = _dev_call(gpu, n, words, broken, cls, cases.INPUTS, [2, 0], T, ce, 3)
        assert res["status"].tolist() == [1, 1, 1] and np.isnan(res["probs_mean"]).all() and not res["n_errors"].any()
    # the device-pointer form never leaves the state: a qubit that is not below the width poisons, an out qubit gives NaN
    wide = words.copy()
    wide[0] = (wide[0] & ~np.uint32(15 << 3)) | np.uint32(7 << 3)
    res = _dev_call(gpu, n, wide, angles, cls, cases.INPUTS, [2, 0], T, ce, 3)
    assert res["status"].tolist() == [1, 1, 1] and np.isnan(res["probs_mean"]).all() and not res["n_errors"].any()
    res = _dev_call(gpu, n, words, angles, cls, cases.INPUTS, [2, 5], T, ce, 3)
    assert np.isnan(res["probs_mean"]).all() and np.array_equal(res["n_errors"], clean["n_errors"])


def test_refused_arguments_leave_the_outputs_untouched(gpu):
    from fbx import native_circuit as nc
    lib = gpu.lib()
    n, T, B, P, m, K = 3, 4, 2, 2, 2, 3
    words, angles = nc.encode_native(cases.circuit(n, 8), n)
    cls = nc.native_noise_classes(words)
    ce = np.full((B, K), 0.1)
    out = np.array([2, 0], dtype=np.uint8)
    probs, errors, status = np.full((B, P, 1 << m), -7.0), np.full((B, P, T), -7, dtype=np.int32), np.full(B, -7, dtype=np.int32)
    good = dict(n=n, G=words.size, words=words, angles=angles, cls=cls, K=K, P=P, inputs=cases.INPUTS, m=m, out=out, B=B, T=T, ce=ce,
                seed=1, first_item=0, first_input=0, probs=probs, errors=errors, status=status)

    def call(**change):
        a = dict(good, **change)
        return lib.fbx_native_trajectories(
            a["n"], a["G"], gpu.ptr(a["words"], C.c_uint32), gpu.dptr(a["angles"]), gpu.ptr(a["cls"], C.c_uint8), a["K"], a["P"],
            gpu.ptr(a["inputs"], C.c_uint64), a["m"], gpu.ptr(a["out"], C.c_uint8), a["B"], a["T"], gpu.dptr(a["ce"]), a["seed"],
            a["first_item"], a["first_input"], gpu.dptr(a["probs"]), gpu.iptr(a["errors"]), gpu.iptr(a["status"]))

    def word(w, **fields):
        w = int(w)
        for name, (shift, width) in {"op": (0, 3), "q0": (3, 4), "q1": (7, 4), "cond": (11, 1), "bit": (12, 6), "rest": (18, 14)}.items():
            if name in fields:
                w = (w & ~(((1 << width) - 1) << shift)) | (fields[name] << shift)
        return w

    def with_word(l, **fields):
        w = words.copy()
        w[l] = word(w[l], **fields)
        return w

    bad_angles = angles.copy()
    bad_angles[0] = np.inf
    one_qubit = int(np.flatnonzero((words & 7) <= 2)[0])
    two_qubit = int(np.flatnonzero((words & 7) >= 3)[0])
    plain = int(np.flatnonzero(((words >> 11) & 1) == 0)[0])
    refused = {
        "n = 0": (dict(n=0), gpu.FBX_ERR_UNSUPPORTED), "n = 14": (dict(n=14), gpu.FBX_ERR_UNSUPPORTED),
        "m = 0": (dict(m=0), gpu.FBX_ERR_BAD_ARG), "m > n": (dict(m=4, out=np.array([0, 1, 2, 2], dtype=np.uint8)), gpu.FBX_ERR_BAD_ARG),
        "K = 0": (dict(K=0), gpu.FBX_ERR_BAD_ARG), "K = 17": (dict(K=17), gpu.FBX_ERR_BAD_ARG),
        "T = 2^32": (dict(T=2 ** 32), gpu.FBX_ERR_BAD_ARG), "T < 0": (dict(T=-1), gpu.FBX_ERR_BAD_ARG),
        "B < 0": (dict(B=-1), gpu.FBX_ERR_BAD_ARG), "P < 0": (dict(P=-1), gpu.FBX_ERR_BAD_ARG), "G < 0": (dict(G=-1), gpu.FBX_ERR_BAD_ARG),
        "first_item < 0": (dict(first_item=-1), gpu.FBX_ERR_BAD_ARG), "first_input < 0": (dict(first_input=-1), gpu.FBX_ERR_BAD_ARG),
        "items past 2^32": (dict(first_item=2 ** 32 - 1), gpu.FBX_ERR_BAD_ARG),
        "inputs past 2^32": (dict(first_input=2 ** 32 - 1), gpu.FBX_ERR_BAD_ARG),
        "NULL words": (dict(words=None), gpu.FBX_ERR_BAD_ARG), "NULL angles": (dict(angles=None), gpu.FBX_ERR_BAD_ARG),
        "NULL inputs": (dict(inputs=None), gpu.FBX_ERR_BAD_ARG), "NULL out_qubits": (dict(out=None), gpu.FBX_ERR_BAD_ARG),
        "no output": (dict(probs=None, errors=None), gpu.FBX_ERR_BAD_ARG),
        "unknown opcode": (dict(words=with_word(0, op=5)), gpu.FBX_ERR_BAD_ARG),
        "q0 not below n": (dict(words=with_word(0, q0=3)), gpu.FBX_ERR_BAD_ARG),
        "q1 of a one-qubit gate": (dict(words=with_word(one_qubit, q1=1)), gpu.FBX_ERR_BAD_ARG),
        "q1 == q0": (dict(words=with_word(two_qubit, q0=1, q1=1)), gpu.FBX_ERR_BAD_ARG),
        "q1 not below n": (dict(words=with_word(two_qubit, q0=0, q1=4)), gpu.FBX_ERR_BAD_ARG),
        "input bit without the flag": (dict(words=with_word(plain, bit=1)), gpu.FBX_ERR_BAD_ARG),
        "a bit above the fields": (dict(words=with_word(0, rest=1)), gpu.FBX_ERR_BAD_ARG),
        "non-finite angle": (dict(angles=bad_angles), gpu.FBX_ERR_BAD_ARG),
        "class not below K": (dict(K=2), gpu.FBX_ERR_BAD_ARG),
        "out qubit not below n": (dict(out=np.array([2, 3], dtype=np.uint8)), gpu.FBX_ERR_BAD_ARG),
        "out qubit repeats": (dict(out=np.array([2, 2], dtype=np.uint8)), gpu.FBX_ERR_BAD_ARG),
    }
    for name, (change, code) in refused.items():
        assert call(**change) == code, name
        assert lib.fbx_last_error(), name
        assert (probs == -7.0).all() and (errors == -7).all() and (status == -7).all(), name
    for change in (dict(B=0), dict(P=0), dict(T=0)):                 # nothing is done
        assert call(**change) == gpu.FBX_OK
        assert (probs == -7.0).all() and (errors == -7).all() and (status == -7).all()
    assert call() == gpu.FBX_OK and not status.any() and (probs >= 0.0).all() and (errors >= 0).all()
    # the unitary: widths, NULL, and a conditional gate in the host form
    u = np.full((8, 8), -7.0 + 0j)
    for n_bad in (0, 14):
        assert lib.fbx_native_unitary(n_bad, words.size, gpu.ptr(words, C.c_uint32), gpu.dptr(angles), gpu.dptr(u.view(np.float64))) == gpu.FBX_ERR_UNSUPPORTED
    assert lib.fbx_native_unitary(n, words.size, gpu.ptr(words, C.c_uint32), gpu.dptr(angles), None) == gpu.FBX_ERR_BAD_ARG
    assert ((words >> 11) & 1).any()
    assert lib.fbx_native_unitary(n, words.size, gpu.ptr(words, C.c_uint32), gpu.dptr(angles), gpu.dptr(u.view(np.float64))) == gpu.FBX_ERR_BAD_ARG
    assert (u == -7.0).all()


# ------------------------------------------------------------------ 7. the adder's statistics from the mean marginals
def test_compiled_adder_statistics_against_the_mirror(gpu):
    from fbx import native_circuit as nc
    from fbx.classical_logic import ripple_carry_adder as rca
    ce, T, seed, tol = cases.ADDER_STATS_CLASS_ERROR, cases.ADDER_STATS_T, cases.ADDER_STATS_SEED, cases.ADDER_STATS_TOL
    success, hamming = rca.compiled_adder_statistics_batch(1, ce, trajectories=T, seed=seed)
    assert success.shape == (2, 4) and hamming.shape == (2, 4, 3) and np.array_equal(success, hamming[:, :, 0])
    words, angles, n, out, cls = rca.compiled_adder_circuit(1)
    want = nc.restate_native_trajectories(words, angles, n, np.arange(4, dtype=np.uint64), out, T, ce, cls, seed)["probs_mean"]
    answer = np.array([0, 1, 1, 2])
    weight = np.array([[bin(o ^ a).count("1") for o in range(4)] for a in answer])
    mirror = np.stack([np.where(weight[None] == w, want, 0.0).sum(axis=2) for w in range(3)], axis=2)
    print("largest deviation from the mirror", np.abs(hamming - mirror).max(), "row sums off by", np.abs(hamming.sum(axis=2) - 1.0).max(),
          "allowed per probability", tol)
    assert np.abs(hamming - mirror).max() <= 2 * tol                 # an entry sums at most two probabilities
    assert np.abs(hamming.sum(axis=2) - 1.0).max() <= 4 * tol        # a row sums all four
    assert (hamming >= 0.0).all() and (success < 1.0).all()          # with several expected errors per trajectory at both settings
