"""Shared inputs of tests/test_dfe_cpu.py and tests/test_dfe_gpu.py: dense matrices of the gates and Paulis, random Clifford
circuits, the reference's experiment loops written out with itertools, a scalar Philox of the tests' own, and a density-matrix
simulation of a circuit with per-gate depolarizing noise.  Dense convention: qubit q is tensor factor q (qubit 0 leftmost)."""
import functools
import itertools

import numpy as np

from fbx import clifford_circuit as cc

I2 = np.eye(2, dtype=complex)
PAULI = {"I": I2, "X": np.array([[0, 1], [1, 0]], dtype=complex), "Y": np.array([[0, -1j], [1j, 0]]),
         "Z": np.array([[1, 0], [0, -1]], dtype=complex)}


def _rot(axis, theta):
    return np.cos(theta / 2) * I2 - 1j * np.sin(theta / 2) * PAULI[axis]


GATE = {"H": np.array([[1, 1], [1, -1]], dtype=complex) / np.sqrt(2), "S": np.diag([1, 1j]), "SDG": np.diag([1, -1j]),
        "X": PAULI["X"], "Y": PAULI["Y"], "Z": PAULI["Z"],
        "RX(pi/2)": _rot("X", np.pi / 2), "RX(-pi/2)": _rot("X", -np.pi / 2), "RY(pi/2)": _rot("Y", np.pi / 2),
        "RY(-pi/2)": _rot("Y", -np.pi / 2), "RZ(pi/2)": _rot("Z", np.pi / 2), "RZ(-pi/2)": _rot("Z", -np.pi / 2),
        "CNOT": np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]], dtype=complex),       # first qubit = control
        "CZ": np.diag([1, 1, 1, -1]).astype(complex),
        "SWAP": np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=complex)}
ONE_QUBIT = cc.GATE_NAMES[:12]
TWO_QUBIT = cc.GATE_NAMES[12:]


def embed(u, qubits, n):
    """The k-qubit matrix u acting on ``qubits`` of n."""
    k = len(qubits)
    full = np.eye(2 ** n, dtype=complex).reshape((2,) * n + (2 ** n,))
    out = np.tensordot(np.asarray(u).reshape((2,) * (2 * k)), full, axes=(list(range(k, 2 * k)), list(qubits)))
    return np.moveaxis(out, list(range(k)), list(qubits)).reshape(2 ** n, 2 ** n)


def dense_pauli(label, sign=0):
    return (1 - 2 * int(sign)) * functools.reduce(np.kron, [PAULI[c] for c in label])


def dense_circuit(gates, n):
    u = np.eye(2 ** n, dtype=complex)
    for name, qubits in gates:
        u = embed(GATE[name], qubits, n) @ u
    return u


def all_labels(n, alphabet="IXYZ"):
    return ["".join(t) for t in itertools.product(alphabet, repeat=n)]


def random_circuit(rng, n, n_gates, pairs=()):
    """``n_gates`` random gates on n qubits as (name, qubits) tuples; the two-qubit gates first visit ``pairs``."""
    gates, pairs = [], list(pairs)
    for _ in range(n_gates):
        if n >= 2 and (pairs or rng.random() < 0.4):
            a, b = pairs.pop() if pairs else rng.choice(n, size=2, replace=False)
            if rng.random() < 0.5:
                a, b = b, a
            gates.append((TWO_QUBIT[rng.integers(3)], (int(a), int(b))))
        else:
            gates.append((ONE_QUBIT[rng.integers(12)], (int(rng.integers(n)),)))
    return gates


def random_paulis(rng, n, count):
    v = int(cc.valid_mask(n))
    x = np.array([int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(2)) for _ in range(count)], dtype=np.uint64) & np.uint64(v)
    z = np.array([int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(2)) for _ in range(count)], dtype=np.uint64) & np.uint64(v)
    return x, z, rng.integers(0, 2, size=count).astype(np.uint8)


def ghz_circuit(n):
    return [("H", (0,))] + [("CNOT", (q, q + 1)) for q in range(n - 1)]


# ------------------------------------------------------------------ the reference's loops (direct_fidelity_estimation.py:46-66, 91-94)
def reference_settings(kind, n, gates, pauli_labels=None, eigenstates=None):
    """The settings of the reference's generators as (in_labels, in_minus tuple, observable label, sign bit) per setting:
    exhaustive when ``pauli_labels`` is None, otherwise for the given input Paulis (and eigenstates, for a process)."""
    from fbx.observable_estimation import PauliTerm
    out = []
    if kind == "state":
        labels = all_labels(n, "IZ")[1:] if pauli_labels is None else pauli_labels
        for lab in labels:
            obs = cc.apply_clifford_to_pauli(gates, PauliTerm({q: c for q, c in enumerate(lab)}), n)
            out.append(("Z" * n, (0,) * n, "".join(obs[q] for q in range(n)), 0 if obs.coefficient.real > 0 else 1))
        return out
    labels = all_labels(n)[1:] if pauli_labels is None else pauli_labels
    for i, lab in enumerate(labels):
        obs = cc.apply_clifford_to_pauli(gates, PauliTerm({q: c for q, c in enumerate(lab)}), n)
        non_identity = [0 if c == "I" else 1 for c in lab]
        state_labels = "".join("Z" if c == "I" else c for c in lab)
        eigs = itertools.product([0, 1], repeat=n) if eigenstates is None else [eigenstates[i]]
        for eig in eigs:
            sign = (-1) ** int(np.dot(eig, non_identity)) * obs.coefficient.real
            out.append((state_labels, tuple(eig), "".join(obs[q] for q in range(n)), 0 if sign > 0 else 1))
    return out


def settings_as_tuples(n, s):
    """The arrays of a DfeExperiment / restate_dfe_settings in the form of ``reference_settings``."""
    get = (lambda k: s[k]) if isinstance(s, dict) else (lambda k: getattr(s, k))
    ins = cc.labels_from_paulis(n, get("in_x"), get("in_z"))
    obs = cc.labels_from_paulis(n, get("obs_x"), get("obs_z"))
    return [(a, tuple((int(mn) >> q) & 1 for q in range(n)), o, int(sg))
            for a, mn, o, sg in zip(ins, get("in_minus").tolist(), obs, get("obs_sign").tolist())]


# ------------------------------------------------------------------ a scalar Philox4x32-10 of the tests' own (Salmon et al., SC'11)
def philox_block(counter, key):
    c, k = [int(v) & 0xFFFFFFFF for v in counter], [int(v) & 0xFFFFFFFF for v in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def monte_carlo_inputs(kind, n, n_terms, seed):
    """Setting by setting, the input Paulis (labels) and eigenstates of the documented Monte Carlo stream; also the number of
    rejected attempts in all."""
    valid, key = (1 << n) - 1, ((seed & 0xFFFFFFFF) ^ 0x44464553, seed >> 32)
    labels, eigs, rejected = [], [], 0
    for k in range(n_terms):
        a = 0
        while True:
            w = philox_block((k & 0xFFFFFFFF, k >> 32, a, 0), key)
            first, second = (w[0] | (w[1] << 32)) & valid, (w[2] | (w[3] << 32)) & valid
            x, z = (first, second) if kind == "process" else (0, first)
            if x | z:
                break
            a, rejected = a + 1, rejected + 1
        labels.append("".join("IXZY"[((x >> q) & 1) | (((z >> q) & 1) << 1)] for q in range(n)))
        w = philox_block((k & 0xFFFFFFFF, k >> 32, a, 1), key)
        e = (w[0] | (w[1] << 32)) & valid if kind == "process" else 0
        eigs.append(tuple((e >> q) & 1 for q in range(n)))
    return labels, eigs, rejected


# ------------------------------------------------------------------ density-matrix simulation with per-gate depolarizing noise
def depolarize(rho, qubits, n, p):
    """rho -> (1 - p) rho + p tr_g(rho) (x) I / d_g on ``qubits``, the partial trace as the uniform Pauli twirl."""
    mixed = np.zeros_like(rho)
    for lab in all_labels(len(qubits)):
        pm = embed(functools.reduce(np.kron, [PAULI[c] for c in lab]), qubits, n)
        mixed += pm @ rho @ pm.conj().T
    return (1 - p) * rho + p * mixed / 4 ** len(qubits)


def noisy_channel(rho, gates, n, noise_class, class_error):
    """The noisy circuit applied to any matrix rho (it is linear): every gate, then its class's depolarizing channel."""
    for g, (name, qubits) in enumerate(gates):
        u = embed(GATE[name], qubits, n)
        rho = u @ rho @ u.conj().T
        c = 0 if noise_class is None else int(noise_class[g])
        if c != 255:
            rho = depolarize(rho, qubits, n, class_error[c])
    return rho


_EIGENSTATE = {("X", 0): np.array([1, 1]) / np.sqrt(2), ("X", 1): np.array([1, -1]) / np.sqrt(2),
               ("Y", 0): np.array([1, 1j]) / np.sqrt(2), ("Y", 1): np.array([1, -1j]) / np.sqrt(2),
               ("Z", 0): np.array([1, 0]), ("Z", 1): np.array([0, 1])}


def product_state(in_labels, in_minus):
    v = functools.reduce(np.kron, [_EIGENSTATE[(c, int(s))] for c, s in zip(in_labels, in_minus)]).astype(complex)
    return np.outer(v, v.conj())


def dense_exact_means(n, tuples, gates, noise_class, class_error, flips):
    """c_k mu of every setting from the density matrix: tr[O rho_out] times the readout product over O's support."""
    out, cache = [], {}
    for in_labels, in_minus, obs, sign in tuples:
        key = (in_labels, in_minus)
        if key not in cache:
            cache[key] = noisy_channel(product_state(in_labels, in_minus), gates, n, noise_class, class_error)
        mu = np.trace(dense_pauli(obs) @ cache[key]).real
        for q, c in enumerate(obs):
            if c != "I" and flips is not None:
                mu *= 1 - 2 * flips[q]
        out.append((1 - 2 * sign) * mu)
    return np.array(out)


def pauli_transfer_matrix(channel, n):
    """R[i, j] = tr(P_i channel(P_j)) / d for a linear map on matrices."""
    labels = all_labels(n)
    mats = [dense_pauli(lab) for lab in labels]
    images = [channel(pm) for pm in mats]
    return np.array([[np.trace(a @ b).real / 2 ** n for b in images] for a in mats])


# ------------------------------------------------------------------ propagation against dense matrices
@functools.lru_cache(maxsize=None)
def propagation_case(n):
    """A circuit of 12 gates in 3 noise classes (every fifth gate noiseless), 40 Monte Carlo process settings of which every
    fourth has a wrong in-state label on qubit 0, and the dense answers: ``(gates, classes, settings dict, wrong mask, sigma,
    touches)``.  Dense touches: a gate is touched iff fully depolarizing its qubits changes the back-propagated matrix (the
    channel is self-adjoint, so it is applied to the observable); dense sigma: tr[O_0 rho_in]."""
    rng = np.random.default_rng(40 + n)
    gates = random_circuit(rng, n, 12)
    classes = rng.integers(0, 3, size=len(gates)).astype(np.uint8)
    classes[::5] = 255
    s = cc.restate_dfe_settings(n, "process", 40, 5, gates)
    wrong = np.arange(40) % 4 == 0
    one = np.uint64(1)
    was_z = wrong & ((s["in_x"] & one) == 0)                         # Z -> X, and X or Y -> Z
    s["in_x"][was_z] |= one
    s["in_z"][was_z] &= ~one
    s["in_x"][wrong & ~was_z] &= ~one
    s["in_z"][wrong & ~was_z] |= one
    sigma, touches = np.zeros(40), np.zeros((40, 3), dtype=int)
    for k, (in_labels, in_minus, obs, _) in enumerate(settings_as_tuples(n, s)):
        o = dense_pauli(obs)
        for g in range(len(gates) - 1, -1, -1):
            name, qubits = gates[g]
            if classes[g] != 255:
                touches[k, classes[g]] += np.abs(depolarize(o, qubits, n, 1.0) - o).max() > 1e-9
            u = embed(GATE[name], qubits, n)
            o = u.conj().T @ o @ u
        sigma[k] = np.trace(o @ product_state(in_labels, in_minus)).real
    return gates, classes, s, wrong, sigma, touches
