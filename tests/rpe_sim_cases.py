"""Cases shared by tests/test_rpe_sim_cpu.py and tests/test_rpe_sim_gpu.py: the outcome distributions of fbx_rpe_simulate
(include/fbx.h, steps 1-2) evaluated with mpmath at 50 digits FROM THE float64 INPUTS -- so that what separates numpy or the device
from them is their own rounding, not that of the inputs -- the gates and noise channels of the cases, and the host restatement
of a whole experiment (distributions -> counts -> moments -> the recursion of tests/rpe_cases.py) that the seeds of the
end-to-end tests are confirmed with."""
import functools
import math

import mpmath
import numpy as np

import rpe_cases
from fbx import robust_phase_estimation as rpe
from fbx import synthetic

mpmath.mp.dps = 50
THETA = 0.7364129871              # no nice fraction of pi
FLIPS_1Q = np.array([[0.08, 0.13]])
FLIPS_2Q = np.array([[0.08, 0.13], [0.02, 0.05]])


# ------------------------------------------------------------------------------------------------ gates and channels (numpy)
def rz(theta):
    return np.diag([np.exp(-0.5j * theta), np.exp(0.5j * theta)])


def rotation(axis, angle):
    """exp(-i angle/2 n.sigma) about the unit vector along `axis`"""
    nx, ny, nz = np.asarray(axis, dtype=float) / np.linalg.norm(axis)
    sigma = nx * synthetic.PAULIS_1Q[1] + ny * synthetic.PAULIS_1Q[2] + nz * synthetic.PAULIS_1Q[3]
    return np.cos(angle / 2) * np.eye(2) - 1j * np.sin(angle / 2) * sigma


def amplitude_damping_kraus(p):
    return np.array([[[1, 0], [0, np.sqrt(1 - p)]], [[0, np.sqrt(p)], [0, 0]]], dtype=complex)


def dephasing_kraus(p):
    return np.array([np.sqrt(1 - p) * np.eye(2), np.sqrt(p) * np.diag([1.0, -1.0])], dtype=complex)


def noisy_rotation_ptm(axis, angle, damping, dephasing):
    """the rotation, then amplitude damping, then dephasing, as one Pauli transfer matrix"""
    return (synthetic.pauli_transfer_matrix(dephasing_kraus(dephasing)) @ synthetic.pauli_transfer_matrix(amplitude_damping_kraus(damping))
            @ synthetic.pauli_transfer_matrix(rotation(axis, angle)))


def diagonal_gate_ptm(a, b, c, depolarizing):
    """diag(1, e^{ia}, e^{ib}, e^{ic}) followed by two-qubit depolarizing of strength `depolarizing`"""
    R = synthetic.pauli_transfer_matrix(np.diag(np.exp(1j * np.array([0.0, a, b, c]))))
    dep = np.diag([1.0] + [1.0 - depolarizing] * 15)
    return dep @ R


def hadamard_like(n, seed):
    """a fixed, well-conditioned change of basis on n qubits: a Haar unitary from a seeded stream"""
    return synthetic.haar_unitary(1 << n, np.random.RandomState(seed))


# ------------------------------------------------------------------------------------------------ steps 1-2 in mpmath
def _mp_matrix(a):
    a = np.asarray(a, dtype=np.float64)
    return mpmath.matrix([[mpmath.mpf(float(x)) for x in row] for row in a])


def mp_distributions(gate, K, prep=None, meas=None, init=None, xy_qubit=0, z_qubit=None, flips=None):
    """prob [B, K, 2, M] as float64 roundings of the 50-digit values; arguments as synthetic.rpe_distributions"""
    gate = np.asarray(gate, dtype=np.float64)
    gate = gate[None] if gate.ndim == 2 else gate
    B, D = gate.shape[0], gate.shape[-1]
    n = {4: 1, 16: 2}[D]
    if init is None:
        init = synthetic.pauli_vector_of_state(np.full(1 << n, 2.0 ** (-n / 2)))
        init = np.round(init)                       # |+..+>: exactly 0 / 1
    iP, iZ = synthetic._rpe_sim_indices(n, xy_qubit, z_qubit)
    M = 2 if z_qubit is None else 4
    out = np.empty((B, K, 2, M))
    half, quarter = mpmath.mpf(1) / 2, mpmath.mpf(1) / 4
    for b in range(B):
        w = mpmath.matrix([mpmath.mpf(float(x)) for x in init])
        if prep is not None:
            w = _mp_matrix(np.broadcast_to(prep, (B, D, D))[b]) * w
        Mm = None if meas is None else _mp_matrix(np.broadcast_to(meas, (B, D, D))[b])
        G = _mp_matrix(gate[b])
        fl = None if flips is None else [[mpmath.mpf(float(x)) for x in row] for row in np.broadcast_to(flips, (B, n, 2))[b]]
        for j in range(K):
            v = G * w
            if Mm is not None:
                v = Mm * v
            for basis in range(2):
                vI, vP = v[0], v[iP[basis]]
                if z_qubit is None:
                    p = [[(vI + vP) * half], [(vI - vP) * half]]
                else:
                    vZ, vPZ = v[iZ], v[iP[basis] | iZ]
                    p = [[(vI + vP + vZ + vPZ) * quarter, (vI + vP - vZ - vPZ) * quarter],
                         [(vI - vP + vZ - vPZ) * quarter, (vI - vP - vZ + vPZ) * quarter]]
                if fl is not None:
                    f0, f1 = fl[xy_qubit]
                    p = [[(1 - f0) * p[0][t] + f1 * p[1][t] for t in range(len(p[0]))],
                         [f0 * p[0][t] + (1 - f1) * p[1][t] for t in range(len(p[0]))]]
                    if z_qubit is not None:
                        g0, g1 = fl[z_qubit]
                        p = [[(1 - g0) * row[0] + g1 * row[1], g0 * row[0] + (1 - g1) * row[1]] for row in p]
                out[b, j, basis] = [float(x) for row in p for x in row]
            if j + 1 < K:
                G = G * G
    return out


# ------------------------------------------------------------------------------------------------ the distribution cases
@functools.lru_cache(maxsize=None)
def distribution_cases():
    """name -> (kwargs of synthetic.rpe_distributions / mp_distributions with 'gate' and 'K', the mpmath values): one qubit with
    K = 20, two qubits with K = 10 and B = 3, shared and per-item changes of basis, with and without a partner, with and without
    flips"""
    cases = {}
    cases["1q_rz"] = dict(gate=synthetic.pauli_transfer_matrix(rz(THETA))[None], K=20)
    axis = (math.sin(0.4), 0.0, math.cos(0.4))
    cob1 = rpe.get_change_of_basis_from_eigvecs(rpe.bloch_rotation_to_eigenvectors(0.4, 0.0))
    noisy = np.stack([noisy_rotation_ptm(axis, THETA + 0.3 * b, 0.004 * (b + 1), 0.007) for b in range(3)])
    prep1 = synthetic.pauli_transfer_matrix(cob1)
    cases["1q_noisy_shared_basis"] = dict(gate=noisy, K=20, prep=prep1, meas=prep1.T.copy(), flips=FLIPS_1Q)
    per_item1 = np.stack([synthetic.pauli_transfer_matrix(hadamard_like(1, 40 + b)) for b in range(3)])
    cases["1q_noisy_per_item_basis"] = dict(gate=noisy, K=20, prep=per_item1, meas=np.ascontiguousarray(per_item1.transpose(0, 2, 1)))
    diag = np.stack([diagonal_gate_ptm(0.31 + 0.2 * b, 1.27 - 0.1 * b, 2.05 + 0.3 * b, 0.002 * (b + 1)) for b in range(3)])
    cases["2q_diag_partner"] = dict(gate=diag, K=10, xy_qubit=0, z_qubit=1)
    cases["2q_diag_no_partner"] = dict(gate=diag, K=10, xy_qubit=1, z_qubit=None, flips=FLIPS_2Q)
    shared2 = synthetic.pauli_transfer_matrix(hadamard_like(2, 50))
    cases["2q_shared_basis_partner_flips"] = dict(gate=diag, K=10, prep=shared2, meas=shared2.T.copy(), xy_qubit=1, z_qubit=0,
                                                   flips=np.stack([FLIPS_2Q, FLIPS_2Q[::-1], 0.5 * FLIPS_2Q]))
    per_item2 = np.stack([synthetic.pauli_transfer_matrix(hadamard_like(2, 60 + b)) for b in range(3)])
    cases["2q_per_item_basis_partner"] = dict(gate=diag, K=10, prep=per_item2, meas=np.ascontiguousarray(per_item2.transpose(0, 2, 1)),
                                              xy_qubit=0, z_qubit=1)
    out = {}
    for name, kw in cases.items():
        kw = dict(kw)
        gate, K = kw.pop("gate"), kw.pop("K")
        out[name] = (gate, K, kw, mp_distributions(gate, K, prep=kw.get("prep"), meas=kw.get("meas"), xy_qubit=kw.get("xy_qubit", 0),
                                                   z_qubit=kw.get("z_qubit"), flips=kw.get("flips")))
    return out


def mirror(gate, K, kw):
    return synthetic.rpe_distributions(gate, K, prep_ptm=kw.get("prep"), meas_ptm=kw.get("meas"), xy_qubit=kw.get("xy_qubit", 0),
                                       z_qubit=kw.get("z_qubit"), flips=kw.get("flips"))


# ------------------------------------------------------------------------------------------------ whole experiments on the host
def host_moments(gate, K, shots, seed, first_item=0, **kw):
    """(moments [8, B, K]) of the host restatement: rpe_distributions -> restate_rpe_counts"""
    probs = synthetic.rpe_distributions(gate, K, **kw)
    return synthetic.restate_rpe_counts(probs, shots, seed, first_item)[1]


def host_phases(moments, partner=False, post_select=0):
    """phases [B] by the recursion of tests/rpe_cases.py on the planes of `moments`, with the post-selection of robust_phase_estimate"""
    x, y, xz, yz, vx, vy, vxz, vyz = moments
    if partner:
        xe, ye = np.sqrt(np.sqrt(vxz) ** 2 + np.sqrt(vx) ** 2), np.sqrt(np.sqrt(vyz) ** 2 + np.sqrt(vy) ** 2)
        x, y = (x + xz, y + yz) if post_select == 0 else (x - xz, y - yz)
    else:
        xe, ye = np.sqrt(vx), np.sqrt(vy)
    return np.array([rpe_cases.estimate(*row)[0] for row in zip(x, y, xe, ye)])


# the end-to-end experiments of the GPU test; their seeds are confirmed on the host by tests/test_rpe_sim_cpu.py
ONE_QUBIT_ANGLE, ONE_QUBIT_K, ONE_QUBIT_FACTOR, ONE_QUBIT_SEED = math.pi / 4 - 0.5, 7, 10, 11
CPHASE_ANGLE, CPHASE_K, CPHASE_SEED = 1.1, 6, 5
STAT_B, STAT_K, STAT_SEED = 4096, 8, 2          # (rms 0.0091 on the host; one rare wrong branch among 4096 items -- seed 2024 has one -- lifts it to 0.015)


def stat_angles():
    return np.random.RandomState(77).uniform(0.0, 2 * math.pi, STAT_B)


def stat_gates():
    c, s = np.cos(stat_angles()), np.sin(stat_angles())
    G = np.zeros((STAT_B, 4, 4))
    G[:, 0, 0] = 1.0; G[:, 3, 3] = 1.0
    G[:, 1, 1] = c; G[:, 1, 2] = -s; G[:, 2, 1] = s; G[:, 2, 2] = c          # RZ(angle): <X> = cos, <Y> = sin from |+>
    return G
