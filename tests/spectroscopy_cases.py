"""Shared inputs of the qubit-spectroscopy acquisition tests (fbx_spec_acquire): the curve grid, the shapes at which the kernel can
go wrong, the 50-digit evaluation of the contract's formula, and a shot-by-shot restatement of the counting."""
import functools
import os
import re

import mpmath
import numpy as np

from fbx import _lib, synthetic

MP_DPS = 50
U_ROUND = 2.0 ** -53
FLOOR = 8 * U_ROUND                                # four roundings around two functions of 1-2 ulp, on values below 1
SEED = (0x5EED << 32) + 0x51C5                     # above 2^32: both key words are in use
FLIPS = np.array([0.03, 0.08])
SHOTS = (0, 1, 3, 4, 5, 257, 1000)                 # the tail block of sim_walk (1, 3, 5), whole blocks (4), a share no lane of a
                                                   # wavefront gets (1, 3, 4, 5: fewer than 64 blocks), past a wavefront's round (257, 1000)
FIRST_ITEMS = (0, 2 ** 32 + 5)                     # the second: the high counter word is in use
KS = (1, 3, 70)                                    # the wavefront form: one point, an odd few, more than a wavefront's lanes


def lane_min_units():
    """the switch between the wavefront and the lane form, read from the source and from the binding, which must agree"""
    src = os.path.join(os.path.dirname(_lib.__file__), "..", "csrc", "fbx_sim_shared.hpp")
    value = int(re.search(r"#define\s+FBX_TOMO_LANE_MIN_UNITS\s+(\d+)", open(src).read()).group(1))
    assert value == _lib.SPEC_LANE_MIN_UNITS
    return value


def grid(B, K, per_item_x=False, seed=1):
    """(x, params [B, 6]) on the test grid: |amplitude|, |baseline| <= 1, |omega x + offset| <= 64, x / decay_time <= 20.  Items
    cycle through four families: 0 a T1-like decay (no cosine, no Gaussian), 1 a Ramsey fringe under both envelopes, 2 a Rabi-like
    cosine without envelope, 3 all six parameters drawn, the probability leaving [0, 1] at some points."""
    rng = np.random.RandomState(seed)
    x = np.sort(rng.uniform(0.0, 8.0, (B, K) if per_item_x else (K,)), axis=-1)
    p = np.empty((B, 6))
    for b in range(B):
        family = b % 4
        amplitude, baseline = rng.uniform(0.2, 0.5), rng.uniform(0.45, 0.5)
        decay, gauss = rng.uniform(0.4, 30.0), rng.uniform(2.0, 40.0)
        omega, offset = rng.uniform(-7.0, 7.0), rng.uniform(-8.0, 8.0)
        if family == 0:
            p[b] = (1.0 - baseline / 10, decay, np.inf, 0.0, 0.0, baseline / 10)
        elif family == 1:
            p[b] = (amplitude, decay, gauss, omega, 0.0, 0.5)
        elif family == 2:
            p[b] = (-amplitude, np.inf, np.inf, omega / 7, offset, 0.5)
        else:
            p[b] = (rng.uniform(-1.0, 1.0), decay, gauss, omega, offset, rng.uniform(-1.0, 1.0))
    assert np.abs(p[:, 3:4] * np.atleast_2d(x) + p[:, 4:5]).max() <= 64 and (np.atleast_2d(x) / p[:, 1:2]).max() <= 20
    return x, p


# the grids on which the mirror's deviation u from the 50-digit values is measured and the device is held to max(4 u, FLOOR)
PROBABILITY_GRIDS = {"shared_x_flips": dict(B=24, K=70, per_item_x=False, flips=True, seed=11),
                     "per_item_x": dict(B=24, K=33, per_item_x=True, flips=False, seed=12)}


def probability_grid(name):
    g = PROBABILITY_GRIDS[name]
    x, p = grid(g["B"], g["K"], g["per_item_x"], g["seed"])
    flips = np.stack([FLIPS * (1 + 0.1 * b) for b in range(g["B"])]) if g["flips"] else None
    return x, p, flips


@functools.lru_cache(maxsize=None)
def mp_probabilities(name):
    """(p_read, mu) of a probability grid as [B][K] lists of 50-digit numbers: the contract's formula at the same fp64 inputs,
    the cosine at the same ROUNDED argument fp64(omega x + offset), everything else unrounded"""
    mpmath.mp.dps = MP_DPS
    x, params, flips = probability_grid(name)
    f = mpmath.mpf
    ps, mus = [], []
    for b in range(params.shape[0]):
        xs = x[b] if x.ndim == 2 else x
        amplitude, decay, gauss, omega, offset, baseline = (float(v) for v in params[b])
        row_p, row_mu = [], []
        for xv in xs:
            xv = float(xv)
            a = f(0) if np.isinf(decay) else f(xv) / f(decay)
            g = f(0) if np.isinf(gauss) else f(xv) / f(gauss)
            arg = float(np.float64(omega) * np.float64(xv) + np.float64(offset))
            p = f(baseline) + f(amplitude) * mpmath.exp(-a - g * g) * mpmath.cos(f(arg))
            if flips is not None:
                p = f(float(flips[b, 0])) * (1 - p) + (1 - f(float(flips[b, 1]))) * p
            row_p.append(p); row_mu.append(1 - 2 * p)
        ps.append(row_p); mus.append(row_mu)
    return ps, mus


def deviation(values, exact):
    """the largest |value - exact| of an fp64 array [B, K] from the 50-digit values, as a float"""
    mpmath.mp.dps = MP_DPS
    return float(max(abs(mpmath.mpf(float(v)) - e) for row_v, row_e in zip(values, exact) for v, e in zip(row_v, row_e)))


@functools.lru_cache(maxsize=None)
def mirror_deviation(name):
    """(u_p, u_mu): the deviation of synthetic.spectroscopy_probabilities, and of 1 - 2 p of it, from the 50-digit values"""
    x, params, flips = probability_grid(name)
    p = synthetic.spectroscopy_probabilities(x, params, flips)
    ps, mus = mp_probabilities(name)
    return deviation(p, ps), deviation(1 - 2 * p, mus)


def shape_cases():
    """name -> dict(B, K, shots, per_item_x, flips, first_item): every K of the wavefront form with every shot count, the three
    switches cycling so that each value meets each K, and all eight switch settings at K = 3 with 5 shots"""
    out = {}
    i = 0
    for K in KS:
        for shots in SHOTS:
            out[f"K{K}_shots{shots}"] = dict(B=5, K=K, shots=shots, per_item_x=bool(i & 1), flips=bool((i >> 1) & 1),
                                            first_item=FIRST_ITEMS[(i >> 2) & 1])
            i += 1
    for j in range(8):
        out[f"switches{j}"] = dict(B=5, K=3, shots=5, per_item_x=bool(j & 1), flips=bool(j & 2), first_item=FIRST_ITEMS[j >> 2])
    return out


def case_inputs(case):
    x, params = grid(case["B"], case["K"], case["per_item_x"], seed=3 + case["K"])
    flips = np.stack([FLIPS * (1 + 0.1 * b) for b in range(case["B"])]) if case["flips"] else None
    return x, params, flips


def count_shot_by_shot(probabilities, shots, seed, first_item=0):
    """k_plus [B, K] by a loop over the shots, one Philox block per shot: shot s of point k of item gid = first_item + b counts +1
    iff word s & 3 of the block with counter (gid low, gid high, k, s >> 2) under the key (seed low ^ "QSPC", seed high) is below
    floor(clamp(0.5 mu + 0.5, 0, 1) 2^32), mu = 1 - 2 p"""
    p = np.atleast_2d(np.asarray(probabilities, dtype=np.float64))
    k0, k1 = (int(seed) & 0xFFFFFFFF) ^ 0x51535043, (int(seed) >> 32) & 0xFFFFFFFF
    out = np.zeros(p.shape, dtype=np.int64)
    for b in range(p.shape[0]):
        gid = int(first_item) + b
        for k in range(p.shape[1]):
            q = min(max(0.5 * (1.0 - 2.0 * p[b, k]) + 0.5, 0.0), 1.0)
            t = int(np.floor(q * 2.0 ** 32))
            for s in range(int(shots)):
                words = synthetic._philox4x32_10(gid & 0xFFFFFFFF, gid >> 32, k, s >> 2, k0, k1)
                out[b, k] += int(words[s & 3]) < t
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


# ------------------------------------------------------------------------------------------------ the physics cases
TIMES = np.linspace(0.0, 60.0, 20)                 # microseconds
ANGLES = np.linspace(0.0, 2 * np.pi, 20)
T1_STAT = dict(B=64, shots=1000, flips=(0.02, 0.05), seed=SEED + 7)
T1_STAT_TIMES = np.linspace(0.0, 12.0, 20)         # short against every T1 below: the readout floor stays small beside the signal


def t1_stat_truth():
    return np.random.RandomState(5).uniform(20.0, 40.0, T1_STAT["B"])
