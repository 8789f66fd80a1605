"""Gate noise for quantum volume on the host (no GPU): the numpy restatement of the Pauli-error stream of
``fbx_qv_noisy_trajectories`` (``synthetic.restate_qv_gate_errors``) and the folding of a trajectory's Paulis into its gates
(``quantum_volume.fold_gate_errors``), checked against the channel they are meant to sample BEFORE the device is compared with
them in tests/test_quantum_volume_noisy_gpu.py -- so that the GPU tests do not compare the device with an unchecked mirror.

The channel: after a gate on (q0, q1), with probability p one of the 15 non-identity Paulis on the pair, uniformly -- on average
rho -> (1 - 16 p / 15) rho + (16 p / 15) (I / 4 on the pair) (x) tr_pair(rho)."""
import ctypes as C

import numpy as np
import pytest

import qv_cases as qc

SEED = 2024                    # fixed; the statistical checks below are conditions on this input, met before any device run
PAULIS = [np.eye(2), np.array([[0, 1], [1, 0]]), np.array([[0, -1j], [1j, 0]]), np.array([[1, 0], [0, -1]])]   # I X Y Z


def haar_gates(rng, count):
    z = rng.standard_normal((count, 4, 4)) + 1j * rng.standard_normal((count, 4, 4))
    q, r = np.linalg.qr(z)
    d = np.diagonal(r, axis1=-2, axis2=-1)
    return q * (d / np.abs(d))[..., None, :]


def trajectory_distributions(n, pairs, gates, p, T, seed):
    """[T, 2^n]: the restated trajectories of one circuit, each simulated as an ordinary circuit after folding"""
    from fbx import quantum_volume as qv, synthetic
    L = len(pairs)
    paulis = synthetic.restate_qv_gate_errors(1, T, L, p, seed)[0]
    folded = qv.fold_gate_errors(gates[None], paulis[None])[0]
    assert folded.shape == (T, L, 4, 4)
    return np.stack([qc.simulate(n, pairs, folded[t]) for t in range(T)]), paulis


def within_six_standard_errors(dists, want):
    T = len(dists)
    mean, se = dists.mean(axis=0), dists.std(axis=0, ddof=1) / np.sqrt(T)
    print("mean", mean, "want", want, "deviation / standard error", np.abs(mean - want) / se)
    assert np.all(se > 0)
    assert np.all(np.abs(mean - want) <= 6 * se)


def test_channel_average_width_2_closed_form():
    """six gates on one pair: every error channel depolarizes the whole state, so mean = f p_ideal + (1 - f) / 4, f = (1 - 16p/15)^L"""
    rng = np.random.default_rng(SEED)
    L, p, T = 6, 0.1, 4096
    pairs = np.asarray([(0, 1), (1, 0)] * 3)
    gates = haar_gates(rng, L)
    dists, paulis = trajectory_distributions(2, pairs, gates, p, T, SEED)
    f = (1 - 16 * p / 15) ** L
    within_six_standard_errors(dists, f * qc.simulate(2, pairs, gates) + (1 - f) / 4)
    assert 0 < np.count_nonzero(paulis) < paulis.size


def embed(n, op, q0, q1):
    """the 2^n x 2^n matrix of the two-qubit operator op on (q0, q1), in the conventions of qv_cases.simulate"""
    N = 1 << n
    cols = []
    for j in range(N):
        wf = np.zeros(N, dtype=np.complex128)
        wf[j] = 1.0
        t = np.tensordot(np.asarray(op, dtype=np.complex128).reshape(2, 2, 2, 2), wf.reshape((2,) * n), axes=((2, 3), (q0, q1)))
        cols.append(np.moveaxis(t, (0, 1), (q0, q1)).reshape(-1))
    return np.stack(cols, axis=1)


def test_channel_average_width_3_density_matrix():
    """overlapping pairs on three qubits against a density-matrix evolution of the channel written as its Pauli sum"""
    rng = np.random.default_rng(SEED + 1)
    n, p, T = 3, 0.1, 4096
    pairs = np.asarray([(0, 1), (2, 1), (1, 0), (0, 2)])
    gates = haar_gates(rng, len(pairs))
    rho = np.zeros((8, 8), dtype=np.complex128)
    rho[0, 0] = 1.0
    for (q0, q1), u in zip(pairs, gates):
        U = embed(n, u, q0, q1)
        rho = U @ rho @ U.conj().T
        noisy = (1 - p) * rho
        for k in range(1, 16):
            P = embed(n, np.kron(PAULIS[k >> 2], PAULIS[k & 3]), q0, q1)
            noisy = noisy + (p / 15) * (P @ rho @ P.conj().T)
        rho = noisy
    want = np.real(np.diagonal(rho))
    assert abs(want.sum() - 1) < 1e-12
    dists, _ = trajectory_distributions(n, pairs, gates, p, T, SEED + 1)
    within_six_standard_errors(dists, want)


def test_fractions_of_errors_and_of_each_pauli():
    from fbx import synthetic
    p, T, L = 0.25, 1000, 100
    k = synthetic.restate_qv_gate_errors(1, T, L, p, SEED + 2)
    count = k.size
    assert count == 10 ** 5 and k.dtype == np.uint8 and k.max() <= 15
    frac = np.count_nonzero(k) / count
    assert abs(frac - p) <= 6 * np.sqrt(p * (1 - p) / count), frac
    q = p / 15
    for pauli in range(1, 16):
        fq = np.count_nonzero(k == pauli) / count
        assert abs(fq - q) <= 6 * np.sqrt(q * (1 - q) / count), (pauli, fq)


def test_prefix_properties_and_gate_error_shapes():
    from fbx import synthetic
    B, T, L = 3, 20, 7
    ge = np.random.default_rng(SEED + 3).uniform(0.2, 0.6, size=(B, L))
    full = synthetic.restate_qv_gate_errors(B, T, L, ge, SEED + 3)
    assert full.shape == (B, T, L)
    assert np.array_equal(synthetic.restate_qv_gate_errors(B, 8, L, ge, SEED + 3), full[:, :8])              # fewer trajectories: a prefix
    assert np.array_equal(synthetic.restate_qv_gate_errors(2, T, L, ge[1:], SEED + 3, first_item=1), full[1:])   # items from k on
    assert np.array_equal(synthetic.restate_qv_gate_errors(B, T, 4, ge[:, :4], SEED + 3), full[:, :, :4])    # block j serves gates 2j, 2j+1
    assert not np.array_equal(synthetic.restate_qv_gate_errors(B, T, L, ge, SEED + 4), full)
    # end points and broadcasting
    assert not synthetic.restate_qv_gate_errors(B, T, L, 0.0, SEED).any()
    assert synthetic.restate_qv_gate_errors(B, T, L, 1.0, SEED).all()
    per_item = synthetic.restate_qv_gate_errors(B, T, L, np.array([0.0, 1.0, 0.0]), SEED)
    assert not per_item[0].any() and per_item[1].all() and not per_item[2].any()
    assert synthetic.restate_qv_gate_errors(0, T, L, 0.5, SEED).shape == (0, T, L)
    with pytest.raises(ValueError):
        synthetic.restate_qv_gate_errors(B, T, L, np.zeros(L + 1), SEED)
    with pytest.raises(ValueError):
        synthetic.restate_qv_gate_errors(B, 2 ** 32, L, 0.5, SEED)
    # the tag is new
    assert synthetic.QV_GATE_ERROR_KEY_TAG not in (synthetic.TOMO_KEY_TAG, synthetic.DFE_KEY_TAG, synthetic.DFE_CALIBRATION_KEY_TAG,
                                                   0x44464553)


def test_fold_gate_errors_is_the_pauli_product_up_to_a_phase():
    from fbx import quantum_volume as qv
    rng = np.random.default_rng(SEED + 5)
    gates = haar_gates(rng, 16)
    folded = qv.fold_gate_errors(gates, np.arange(16))
    assert np.array_equal(folded[0], gates[0])                                     # no error: the gate itself, bit for bit
    for k in range(16):
        want = np.kron(PAULIS[k >> 2], PAULIS[k & 3]) @ gates[k]
        phase = (-1j) ** ((k >> 2 == 2) + (k & 3 == 2))                            # Y is applied as X Z = -i Y
        assert np.abs(folded[k] - phase * want).max() == 0.0
        assert np.array_equal(np.sort(np.abs(folded[k]).ravel()), np.sort(np.abs(gates[k]).ravel()))   # rows permuted and negated: exact
    # broadcasting: [B, L, 4, 4] with [B, T, L]
    g = gates.reshape(2, 8, 4, 4)
    k = rng.integers(0, 16, size=(2, 5, 8))
    out = qv.fold_gate_errors(g, k)
    assert out.shape == (2, 5, 8, 4, 4)
    assert np.array_equal(out[1, 3], qv.fold_gate_errors(g[1], k[1, 3]))
    with pytest.raises(ValueError):
        qv.fold_gate_errors(g, np.full((2, 8), 16))
    with pytest.raises(ValueError):
        qv.fold_gate_errors(g, np.zeros((2, 7), dtype=int))


def test_option_and_refusals_need_no_device():
    """the workspace option behaves like its neighbours, and the argument checks come before the device is asked for"""
    from fbx import _lib
    lib = _lib.lib()
    v = C.c_double(0.0)
    assert lib.fbx_get_option(b"qv_noisy_workspace_mib", C.byref(v)) == 0 and v.value == 128.0
    assert lib.fbx_set_option(b"qv_noisy_workspace_mib", C.c_double(0.5)) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_set_option(b"qv_noisy_workspace_mib", C.c_double(1e6)) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_get_option(b"qv_noisy_workspace_mib", C.byref(v)) == 0 and v.value == 128.0
    assert _lib.get_option("qv_wide_workspace_mib") == 128.0                       # its neighbour is another option
    pairs = np.zeros((1, 1, 2), dtype=np.uint8)
    pairs[0, 0, 1] = 1
    gates = np.eye(4, dtype=np.complex128).reshape(1, 1, 4, 4).view(np.float64)
    ge = np.zeros((1, 1))
    nerr = np.full((1, 4), -7, dtype=np.int32)

    def call(n, T, first_item=0):
        return lib.fbx_qv_noisy_trajectories(n, 1, 1, T, pairs.ctypes.data_as(C.POINTER(C.c_uint8)), _lib.dptr(gates), _lib.dptr(ge),
                                             None, 1, first_item, None, None, _lib.iptr(nerr), None)
    assert call(14, 4) == _lib.FBX_ERR_UNSUPPORTED and call(1, 4) == _lib.FBX_ERR_UNSUPPORTED
    assert call(3, 2 ** 32) == _lib.FBX_ERR_BAD_ARG and call(3, -1) == _lib.FBX_ERR_BAD_ARG and call(3, 4, -1) == _lib.FBX_ERR_BAD_ARG
    assert np.all(nerr == -7)
