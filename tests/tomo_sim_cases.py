"""Cases for tests/test_tomo_sim_cpu.py and tests/test_tomo_sim_gpu.py: truths, designs and independent routes to the numbers
``fbx_tomo_simulate`` (include/fbx.h) must produce.

Three routes that share no code with the kernel or with ``synthetic.restate_tomography_counts``:
``kraus_means`` -- tr[P K rho K^+] summed over Kraus operators, dense numpy; ``flipped_means`` -- the outcome distribution of every
setting over the 2^n bit patterns of the measured product basis in ``numpy.longdouble``, pushed through the per-bit confusion
matrices, then the parity over the observable's support; ``count_loop`` -- the stream shot by shot in a Python loop on
``fbx_oracle.acquisition.philox4x32_10`` (pinned by the Random123 known answers in tests/test_resample_cpu.py).
"""
import functools
import itertools

import numpy as np

from fbx_oracle.acquisition import philox4x32_10

SEED = 0x5EED0123456789AB            # both key words in use
B, FIRST, SHOTS = 5, 3, 4099         # ids that do not start at 0; a shot count that spans many blocks and leaves a tail
# The last Philox block of a shot count that is no multiple of 4 is owned by one walker of sim_walk (csrc/fbx_sim_shared.hpp),
# lane (N // 4) % 64 of a wavefront: no full block (lane 0), every residue, N // 4 = 64 (back at lane 0) and N // 4 = 5 (lane 5).
# Every simulator that draws its shots this way is run at these counts on its wavefront split, and at 5 and 7 on its lane split,
# where one lane owns every block.
TAIL_SHOTS = (1, 2, 3, 4, 5, 6, 7, 256, 257, 258, 259, 22)
TAIL_SHOTS_LANE = (5, 7)
KEY_TAG = 0x544F4D4F
EPS = 2.0 ** -53
COEF_VALUES = (1.0, -1.0, 0.5, -2.0)  # powers of two: exact / coef is exact


# ------------------------------------------------------------------------------------------------ the stream, shot by shot
def count_loop(mu, shots, seed, g, k):
    """k_plus of setting k of global item g with mean mu: one Philox block per four shots, one comparison per shot"""
    q = min(max(0.5 * mu + 0.5, 0.0), 1.0)
    t = int(np.floor(q * 2.0 ** 32))
    key = np.array([(seed & 0xFFFFFFFF) ^ KEY_TAG, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    k_plus, words = 0, None
    for s in range(shots):
        if s & 3 == 0:
            ctr = np.array([g & 0xFFFFFFFF, (g >> 32) & 0xFFFFFFFF, k, s >> 2], dtype=np.uint32)
            words = philox4x32_10(ctr, key)
        k_plus += int(words[s & 3]) < t
    return k_plus


def moments(k_plus, shots, coefs):
    """(expectation, std_err) of the contract from integer counts, in Python integers and one rounding each"""
    k_plus = np.asarray(k_plus)
    coefs = np.broadcast_to(np.asarray(coefs, dtype=np.float64), k_plus.shape)
    e, s = np.empty(k_plus.shape), np.empty(k_plus.shape)
    for i in np.ndindex(k_plus.shape):
        kp = int(k_plus[i]); km = shots - kp
        e[i] = coefs[i] * (float(kp - km) / float(shots))
        s[i] = abs(coefs[i]) * np.sqrt(float(4 * kp * km) / float(shots)) / float(shots)
    return e, s


def z_score(k_plus, q, shots):
    """sum(k+ - N q) / sqrt(sum N q (1 - q)): standard normal for binomial counts"""
    q = np.asarray(q, dtype=np.float64)
    return float((np.asarray(k_plus) - shots * q).sum() / np.sqrt((shots * q * (1.0 - q)).sum()))


# ------------------------------------------------------------------------------------------------ truths
def haar_unitary(d, rng):
    z = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    q, r = np.linalg.qr(z)
    ph = np.diagonal(r) / np.abs(np.diagonal(r))
    return q * ph[None, :]


@functools.lru_cache(maxsize=None)
def damped_kraus(n, batch=B, seed=11):
    """[batch, 2^n, d, d]: a Haar unitary after amplitude damping of every qubit (gamma between 0.1 and 0.4) -- non-unital and
    non-unitary"""
    rng = np.random.default_rng([seed, n])
    d = 1 << n
    out = np.empty((batch, d, d, d), dtype=np.complex128)
    for b in range(batch):
        u = haar_unitary(d, rng)
        ops = [np.array([[1.0 + 0j]])]
        for _ in range(n):
            g = rng.uniform(0.1, 0.4)
            a0 = np.array([[1, 0], [0, np.sqrt(1 - g)]], dtype=complex)
            a1 = np.array([[0, np.sqrt(g)], [0, 0]], dtype=complex)
            ops = [np.kron(o, a) for o in ops for a in (a0, a1)]
        out[b] = np.array([u @ o for o in ops])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def unitaries(n, batch, seed=13):
    rng = np.random.default_rng([seed, n])
    out = np.array([haar_unitary(1 << n, rng) for _ in range(batch)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mixed_states(n, batch=B, seed=17):
    """[batch, d, d] full-rank density matrices G G^+ / tr with G a d x d Ginibre matrix"""
    rng = np.random.default_rng([seed, n])
    d = 1 << n
    g = rng.standard_normal((batch, d, d)) + 1j * rng.standard_normal((batch, d, d))
    rho = g @ np.conj(np.swapaxes(g, 1, 2))
    rho /= np.trace(rho, axis1=1, axis2=2)[:, None, None]
    rho.setflags(write=False)
    return rho


# ------------------------------------------------------------------------------------------------ designs
PROCESS_CASES = ("1q-pauli", "1q-sic", "2q-pauli", "2q-sic", "3q-shuffled")
STATE_CASES = (1, 2, 3, 4, 5)


@functools.lru_cache(maxsize=None)
def process_case_design(name):
    """the design of a process case; "3q-shuffled" = 300 settings drawn from the three-qubit Pauli design, shuffled, some
    repeated, with coefficients from COEF_VALUES"""
    from fbx.design import Design, process_design
    if name != "3q-shuffled":
        n, basis = int(name[0]), name[3:]
        return process_design(n, basis)
    full = process_design(3, "pauli")
    rng = np.random.default_rng(29)
    pick = rng.permutation(full.m)[:280]
    pick = rng.permutation(np.concatenate([pick, pick[:20]]))             # 20 settings twice
    coefs = np.take(COEF_VALUES, rng.integers(0, 4, size=pick.size))
    return Design(3, "process", full.in_labels[pick], full.paulis[pick], coefs)


@functools.lru_cache(maxsize=None)
def with_identity_observable(n):
    """the Pauli process design of n qubits with one all-identity observable of coefficient -0.5 put in the middle"""
    from fbx.design import Design, process_design
    full = process_design(n, "pauli")
    at = full.m // 2
    ins = np.insert(full.in_labels, at, full.in_labels[at], axis=0)
    outs = np.insert(full.paulis, at, 0, axis=0)
    return Design(n, "process", ins, outs, np.insert(full.coefs, at, -0.5)), at


def tolerance(design):
    """64 D 2^-53 |c| per setting: a mean is a sum of at most D products of factors of magnitude <= 1, with room for the
    conversion that made the transfer matrix"""
    return 64.0 * design.dim ** 2 * EPS * np.abs(design.coefs)


# ------------------------------------------------------------------------------------------------ means, independently
def _design_ops(design):
    from fbx import synthetic
    rhos = np.array([synthetic.product_state_matrix(c) for c in design.in_labels])
    ps = np.array([synthetic.pauli_matrix(c) for c in design.paulis])
    return rhos, ps


def kraus_means(design, kraus):
    """coef_k sum_i tr[P_k K_i rho_k K_i^+], [B, m]"""
    rhos, ps = _design_ops(design)
    out = np.einsum('bkij,sjl,bkml->bsim', kraus, rhos, np.conj(kraus))     # Lambda_b(rho_s)
    return np.real(np.einsum('sxy,bsyx->bs', ps, out)) * design.coefs[None, :]


def state_means(design, states):
    _, ps = _design_ops(design)
    return np.real(np.einsum('sxy,byx->bs', ps, states)) * design.coefs[None, :]


_LD, _CLD = np.longdouble, np.clongdouble
_PAULI = [np.array(p, dtype=_CLD) for p in ([[1, 0], [0, 1]], [[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]])]


def _kron_all(mats):
    out = np.array([[1]], dtype=_CLD)
    for m in mats:
        out = np.kron(out, m)
    return out


def flipped_means(design, outputs, flips):
    """coef_k times the parity expectation of the READ bits over the observable's support.  ``outputs [B, m, d, d]``: the state
    that setting k of item b measures; ``flips [B, n, 2]``.  Qubit j is measured in the eigenbasis of its Pauli factor (Z for
    I), bit 0 = eigenvalue +1; the 2^n-pattern distribution goes through the per-bit confusion matrices in longdouble."""
    n = design.n_qubits
    Bn, m = outputs.shape[:2]
    eye = _PAULI[0]
    out = np.empty((Bn, m))
    patterns = list(itertools.product((0, 1), repeat=n))
    for k in range(m):
        codes = [int(c) for c in design.paulis[k]]
        axes = [_PAULI[c] if c else _PAULI[3] for c in codes]
        projs = [_kron_all([(eye + (1 - 2 * bit) * ax) / 2 for bit, ax in zip(bits, axes)]) for bits in patterns]
        for b in range(Bn):
            rho = outputs[b, k].astype(_CLD)
            p = np.array([np.real(np.trace(pr @ rho)) for pr in projs], dtype=_LD)
            f = flips[b].astype(_LD)
            conf = [np.array([[1 - f[j, 0], f[j, 0]], [f[j, 1], 1 - f[j, 1]]], dtype=_LD) for j in range(n)]   # [drawn][read]
            val = _LD(0)
            for read in patterns:
                pr = _LD(0)
                for drawn, pd in zip(patterns, p):
                    w = pd
                    for j in range(n):
                        w = w * conf[j][drawn[j], read[j]]
                    pr += w
                sign = 1
                for j in range(n):
                    if codes[j] and read[j]:
                        sign = -sign
                val += sign * pr
            out[b, k] = float(val) * design.coefs[k]
    return out


def process_outputs(design, kraus):
    """[B, m, d, d]: Lambda_b(rho_{s_k}) for every setting"""
    rhos, _ = _design_ops(design)
    return np.einsum('bkij,sjl,bkml->bsim', kraus, rhos, np.conj(kraus))
