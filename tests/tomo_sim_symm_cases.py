"""Cases for tests/test_tomo_sim_symm_cpu.py and tests/test_tomo_sim_symm_gpu.py: confusion matrices, the dense longdouble
route to the per-pattern distributions of ``fbx_tomo_simulate_symmetrized`` (include/fbx.h) and the stream shot by shot.

Nothing here shares code with the kernel or with ``synthetic.restate_symmetrized_tomography_counts``: the ideal distributions
come from projectors on the truth in ``numpy.longdouble``, the patterns from a filter over all masks, and ``pattern_loop`` walks
the stream one shot at a time on ``fbx_oracle.acquisition.philox4x32_10``.
"""
import functools
import math

import numpy as np

import tomo_sim_cases as tc
from tomo_sim_cases import B

from fbx_oracle.acquisition import philox4x32_10

ALL_CASES = tc.PROCESS_CASES + tuple(f"state-{n}" for n in tc.STATE_CASES)
TAG_MEASUREMENT, TAG_CALIBRATION, TAG_GROUPED = 0x544F4D53, 0x544F4D43, 0x544F4D47
_LD, _CLD = np.longdouble, np.clongdouble


@functools.lru_cache(maxsize=None)
def design_of(case):
    from fbx.design import state_design
    return state_design(int(case[6:])) if case.startswith("state") else tc.process_case_design(case)


@functools.lru_cache(maxsize=None)
def grouping_of(case):
    from fbx.design import group_design
    return group_design(design_of(case))


def masks_of(paulis):
    """parity mask per setting: bit t = qubit n - 1 - t"""
    n = paulis.shape[1]
    return ((np.asarray(paulis)[:, ::-1] != 0) << np.arange(n)).sum(axis=1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def unions_of(case):
    """U_g of every group: the union of its members' masks"""
    z = masks_of(design_of(case).paulis)
    return tuple(int(np.bitwise_or.reduce(z[grp])) for grp in grouping_of(case).groups)


def patterns_of(mask, symm_type, n):
    """the flip masks of a unit, by filtering all 2^n masks (no submask enumeration trick)"""
    return [f for f in range(1 << n) if (f & ~mask) == 0] if symm_type == -1 else [0]


def truth_of(case):
    des = design_of(case)
    return tc.mixed_states(des.n_qubits) if case.startswith("state") else tc.damped_kraus(des.n_qubits)


# ------------------------------------------------------------------------------------------------ confusion matrices
def kron_flips(flips):
    """[2^n, 2^n] from [n, 2] flips, qubit 0 the most significant bit, [drawn][read], by np.kron"""
    out = np.ones((1, 1))
    for f0, f1 in flips:
        out = np.kron(out, np.array([[1.0 - f0, f0], [f1, 1.0 - f1]]))
    return out


@functools.lru_cache(maxsize=None)
def product_confusion(n, batch=B, seed=31):
    """[batch, 2^n, 2^n]: tensor products of asymmetric per-qubit matrices, flips between 2 % and 12 %, the two directions apart"""
    rng = np.random.default_rng([seed, n])
    out = np.array([kron_flips(np.stack([rng.uniform(0.02, 0.06, n), rng.uniform(0.08, 0.12, n)], axis=1)) for _ in range(batch)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def correlated_confusion(n, batch=B, seed=37, weight=0.125):
    """[batch, 2^n, 2^n]: (1 - weight) x a tensor product + weight x a random row-stochastic matrix -- asymmetric, correlated, rows
    summing to 1 up to rounding"""
    rng = np.random.default_rng([seed, n])
    d = 1 << n
    out = np.empty((batch, d, d))
    for b in range(batch):
        r = rng.random((d, d)) ** 3
        r /= r.sum(axis=1, keepdims=True)
        out[b] = (1.0 - weight) * product_confusion(n, batch)[b] + weight * r
    out.setflags(write=False)
    return out


def distance_from_products(c):
    """A lower bound on the Frobenius distance of ``c [2^n, 2^n]`` from every Kronecker product of n 2 x 2 matrices: such a product
    is also a product across (qubit 0 | the rest), i.e. rank one after the realignment [(a, a'), (rest, rest')], and the second
    singular value of the realigned matrix is the distance from the rank-one matrices (Eckart-Young)."""
    d = c.shape[0]
    r = c.reshape(2, d // 2, 2, d // 2).transpose(0, 2, 1, 3).reshape(4, -1)
    return float(np.linalg.svd(r, compute_uv=False)[1])


# ------------------------------------------------------------------------------------------------ distributions, densely
def dense_ideal(basis, rho):
    """p [2^n] in longdouble: tr[(x)_j (I +- P_j) / 2 rho] over the bit patterns (bit 0 = eigenvalue +1, qubit 0 the most significant
    bit of the outcome)"""
    n = len(basis)
    T = rho.astype(_CLD).reshape((2,) * (2 * n))
    eye = tc._PAULI[0]
    for q, code in enumerate(basis):
        ax = tc._PAULI[int(code)]
        P = np.stack([(eye + ax) / 2, (eye - ax) / 2])
        T = np.moveaxis(np.tensordot(P, T, axes=([2, 1], [q, n])), 0, q)
    return np.real(T).astype(_LD).reshape(-1)


@functools.lru_cache(maxsize=None)
def ideal(case):
    """[B, G, 2^n] longdouble, no readout error"""
    des, g = design_of(case), grouping_of(case)
    if case.startswith("state"):
        rho = tc.mixed_states(des.n_qubits)
        outputs = lambda b, k: rho[b]
    else:
        out = tc.process_outputs(des, tc.damped_kraus(des.n_qubits))
        outputs = lambda b, k: out[b, k]
    p = np.array([[dense_ideal(g.basis[i], outputs(b, grp[0])) for i, grp in enumerate(g.groups)] for b in range(B)])
    p.setflags(write=False)
    return p


def dense_patterns(p, conf, unions, symm_type):
    """[B, G, 2^n, 2^n] longdouble: q_f(r) = sum_o p(o) C[o ^ f][r ^ f]; zero rows where f is no pattern"""
    Bn, G, d = p.shape
    n = d.bit_length() - 1
    c = conf.astype(_LD)
    idx = np.arange(d)
    out = np.zeros((Bn, G, d, d), dtype=_LD)
    for g in range(G):
        for f in patterns_of(unions[g], symm_type, n):
            for b in range(Bn):
                out[b, g, f] = p[b, g] @ c[b][idx ^ f][:, idx ^ f]
    return out


def tolerance(design):
    """(2 x 64 dim^2 + 2 dim) 2^-53: the grouped test's bound for p plus dim fma roundings of a convex sum"""
    return (2 * 64.0 * design.dim ** 2 + 2 * design.dim) * tc.EPS


# ------------------------------------------------------------------------------------------------ the stream, shot by shot
def pattern_loop(q, f, s, seed, gid, unit, tag):
    """histogram [2^n] of the s shots of flip mask f of (global item gid, unit): thresholds from the clamped running sum of q,
    one Philox block per four shots with counter (gid low, gid high, unit, (f << 27) | block)"""
    d = len(q)
    c = np.cumsum(np.maximum(q, 0.0))
    thr = [int(np.floor(x / c[-1] * 2.0 ** 32)) for x in c[:-1]]
    key = np.array([(seed & 0xFFFFFFFF) ^ tag, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    hist, words = np.zeros(d, dtype=np.int64), None
    for t in range(s):
        if t & 3 == 0:
            ctr = np.array([gid & 0xFFFFFFFF, (gid >> 32) & 0xFFFFFFFF, unit, (f << 27) | (t >> 2)], dtype=np.uint32)
            words = philox4x32_10(ctr, key)
        hist[sum(1 for x in thr if x <= int(words[t & 3]))] += 1
    return hist


def z_bound(cells):
    """the smallest z* with cells x erfc(z* / sqrt 2) <= 1e-6, by bisection (the bound of the grouped test)"""
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if cells * math.erfc(mid / math.sqrt(2.0)) <= 1e-6 else (mid, hi)
    return hi


def cell_z_scores(hist, qbar, counts):
    """the z-score of every merged-histogram cell with N qbar >= 5 (N per cell: ``counts`` broadcast over the outcomes), and their number"""
    n = np.broadcast_to(counts, hist.shape).astype(np.float64)
    keep = n * qbar >= 5.0
    k, q, n = hist[keep].astype(np.float64), qbar[keep], n[keep]
    return (k - n * q) / np.sqrt(n * q * (1.0 - q)), int(keep.sum())


def guard_items(n):
    """how many of the B items the host restatement walks: all for 1..3 qubits, two above (its loop over patterns is slow)"""
    return B if n < 4 else 2
