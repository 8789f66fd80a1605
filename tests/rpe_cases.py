"""Robust phase estimation cases shared by tests/test_rpe_cpu.py and tests/test_rpe_gpu.py: a numpy restatement of the recursion of
estimate_phase_from_moments (pinned to the reference's answers of tests/golden/rpe_cases.npz in the CPU test, so that GPU tests on
shapes the goldens do not hold do not compare the device with itself), the margins that keep a case away from the estimator's
discontinuities, moment and shot generators, and the encoding of the stored two-qubit `results` structures."""
import math

import numpy as np

U_ROUND = 2.0 ** -53
TWO_PI = 2 * math.pi
MARGIN = 1e-9
GOLDEN_DEPTHS = (1, 2, 5, 12)


def estimate(xs, ys, x_stds, y_stds):
    """(phase, depth_reached, bloch [K, 2] with NaN beyond the cut, margins): the recursion on numpy float64 scalars with numpy's
    arctan2 and %, as the reference runs it on the moments of an ExperimentResult (numpy's arctan2 and the C library's atan2 differ
    in the last bit on some inputs); margins = (smallest distance of an offset from its window's ends in units of the width, smallest |r - r_std| / r)
    over the iterations that were looked at."""
    K = len(xs)
    theta = 0
    used = 0
    bloch = np.full((K, 2), np.nan)
    edge, gap = math.inf, math.inf
    for j in range(K):
        x, y, xs_, ys_ = (np.float64(v[j]) for v in (xs, ys, x_stds, y_stds))
        k = 2 ** j
        with np.errstate(all="ignore"):
            r = np.sqrt(x ** 2 + y ** 2)
            r_std = np.sqrt(xs_ ** 2 + ys_ ** 2)
        gap = min(gap, abs(r - r_std) / r if r > 0 else math.inf)          # (r = 0: exact zeros, no rounding to fear)
        if r < r_std:
            break
        theta_j = np.arctan2(y, x) / k
        half = np.pi / k
        low = theta - half
        offset = (theta_j - low) % (2 * half)
        edge = min(edge, offset / (2 * half), 1 - offset / (2 * half))
        theta = offset + low
        used = j + 1
        bloch[j] = (r, theta * k)
    return float(theta % (2 * np.pi)), used, bloch, (float(edge), float(gap))


def safe(margins):
    return margins[0] >= MARGIN and margins[1] >= MARGIN


def estimate_batch(x, y, xe, ye):
    out = [estimate(*row) for row in zip(x, y, xe, ye)]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int32), np.stack([o[2] for o in out]),
            [o[3] for o in out])


def estimate_vec(x, y, xe, ye):
    """phases [B] of the same recursion as array operations over the batch (for statistics over many resamples; numpy's array
    arctan2 may differ from its scalar one in the last bit, so this form is pinned to `estimate` within 1e-12 only)"""
    x, y, xe, ye = (np.asarray(a, dtype=np.float64) for a in (x, y, xe, ye))
    theta = np.zeros(x.shape[0])
    live = np.ones(x.shape[0], dtype=bool)
    for j in range(x.shape[1]):
        k = 2.0 ** j
        live &= ~(np.sqrt(x[:, j] ** 2 + y[:, j] ** 2) < np.sqrt(xe[:, j] ** 2 + ye[:, j] ** 2))
        low = theta - np.pi / k
        new = (np.arctan2(y[:, j], x[:, j]) / k - low) % (2 * np.pi / k) + low
        theta = np.where(live, new, theta)
    return theta % (2 * np.pi)


def circ_dist(a, b):
    d = np.abs(np.asarray(a, dtype=float) - np.asarray(b, dtype=float)) % TWO_PI
    return np.minimum(d, TWO_PI - d)


def moment_sets(rng, n, K, shots=500, decay_range=(0.03, 2.0)):
    """n safe moment sets of K depths from known phases: visibility exp(-2^j / T) with T log-uniform in 2^K x decay_range (so some
    items are cut short), binomial sampling noise of `shots` shots, standard errors sqrt((1 - m^2) / shots).  Unsafe draws (an
    offset within 1e-9 of a window end, r within 1e-9 of r_std) are drawn again."""
    x, y, xe, ye, phi = [], [], [], [], []
    depth = 2.0 ** np.arange(K)
    while len(x) < n:
        p = rng.uniform(0, TWO_PI)
        T = 2.0 ** K * math.exp(rng.uniform(math.log(decay_range[0]), math.log(decay_range[1])))
        vis = np.exp(-depth / T)
        mx = 2 * rng.binomial(shots, (1 + vis * np.cos(depth * p)) / 2) / shots - 1
        my = 2 * rng.binomial(shots, (1 + vis * np.sin(depth * p)) / 2) / shots - 1
        sx, sy = np.sqrt((1 - mx * mx) / shots), np.sqrt((1 - my * my) / shots)
        if safe(estimate(mx, my, sx, sy)[3]):
            x.append(mx); y.append(my); xe.append(sx); ye.append(sy); phi.append(p)
    return np.array(x), np.array(y), np.array(xe), np.array(ye), np.array(phi)


def shot_records(rng, B, K, shots, n_qubits, col, zcol, phases, visibility=0.9):
    """x_bits, y_bits [B, K, shots, n_qubits] uint8: column `col` carries the rotated qubit (P(1) = (1 - v cos(2^j phi)) / 2 in the X
    basis, sin in the Y basis), column `zcol` a partner that is 1 with probability 0.3 and, when it is, shifts the phase by 0.7;
    the other columns are coin flips."""
    depth = 2.0 ** np.arange(K)
    out = []
    for fn in (np.cos, np.sin):
        bits = rng.integers(0, 2, size=(B, K, shots, n_qubits), dtype=np.uint8)
        z = (rng.random((B, K, shots)) < 0.3).astype(np.uint8)
        ang = depth[None, :, None] * (np.asarray(phases)[:, None, None] + 0.7 * (z if zcol is not None else 0))
        bits[..., col] = rng.random((B, K, shots)) < (1 - visibility * fn(ang)) / 2
        if zcol is not None:
            bits[..., zcol] = z
        out.append(bits)
    return out[0], out[1]


def moments_from_shots(x_bits, y_bits, col, zcol, post_select):
    """[B, K, 4] = (x, y, x_err, y_err) as fbx_rpe_from_shots documents them, by direct counting in numpy"""
    res = []
    n = x_bits.shape[2]
    for bits in (x_bits, y_bits):
        b = bits & 1
        m = ((n - b[..., col].sum(axis=2, dtype=np.int64)) - b[..., col].sum(axis=2, dtype=np.int64)) / n
        v = (1.0 - m * m) / n
        if zcol is None:
            res.append((m, np.sqrt(v)))
        else:
            nz = (b[..., col] ^ b[..., zcol]).sum(axis=2, dtype=np.int64)
            mz = ((n - nz) - nz) / n
            vz = (1.0 - mz * mz) / n
            sel = m + mz if post_select == 0 else m - mz
            sz, s = np.sqrt(vz), np.sqrt(v)
            res.append((sel, np.sqrt(sz * sz + s * s)))
    return np.stack([res[0][0], res[1][0], res[0][1], res[1][1]], axis=-1)


# ------------------------------------------------------------------------------------------------ stored `results` structures
PAULI_CODES = "IXYZ"
STATE_LABELS = ("X", "Y", "Z")


def build_results(gold, name, make_state, make_term, make_setting, make_result):
    """The list over depths of lists of results of structure `name`, built with the given constructors (fbx's or the reference's):
    make_state(label, index, qubit) -> a one-qubit TensorProductState, make_term({qubit: 'X' | 'Y' | 'Z'}) -> the observable."""
    qubits = [int(q) for q in gold[f"{name}_qubits"]]
    obs, states = gold[f"{name}_observables"], gold[f"{name}_in_states"]
    exps, errs = gold[f"{name}_expectations"], gold[f"{name}_std_errs"]
    settings = []
    for s in range(obs.shape[0]):
        state = None
        for qi, q in enumerate(qubits):
            one = make_state(STATE_LABELS[int(states[s, qi, 0])], int(states[s, qi, 1]), q)
            state = one if state is None else state * one
        term = make_term({q: PAULI_CODES[int(obs[s, qi])] for qi, q in enumerate(qubits) if obs[s, qi]})
        settings.append(make_setting(state, term))
    return [[make_result(settings[s], float(exps[d, s]), float(errs[d, s]), int(gold[f"{name}_shots"]))
             for s in range(len(settings))] for d in range(exps.shape[0])], qubits


def fbx_results(gold, name):
    from fbx import observable_estimation as oe
    return build_results(gold, name,
                         lambda label, index, q: oe.TensorProductState((oe._OneQState(label, index, q),)),
                         lambda ops: oe.PauliTerm(ops),
                         oe.ExperimentSetting,
                         lambda setting, e, s, n: oe.ExperimentResult(setting=setting, expectation=e, total_counts=n, std_err=s))


RESULT_STRUCTURES = ("all_eigvecs", "fixed_one", "fixed_zero")
