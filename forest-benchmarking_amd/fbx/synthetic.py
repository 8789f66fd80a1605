"""Synthetic tomography data (host-side input generation; no estimator arithmetic).

Recipe of SURVEY.md 8d, mirroring how the reference's tests build data
(tests/test_process_tomography.py:56,87: ``haar_rand_unitary(d, rs=RandomState(52))``):
item b has truth U_b = Haar unitary from ``RandomState(1000 + b)`` (QR with phase fix,
operator_tools/random_operators.py:49-72), exact expectations e_k = tr[P_k U rho_in U^+]
(optionally depolarised), and k_+ ~ Binomial(shots, (1 + e_k)/2) from
``RandomState(2000 + b)``; ``expectation = 2 k_+/shots - 1``, ``total_counts = shots``.
"""
import itertools

import numpy as np

from .design import Design, process_design, state_design

_s2, _s3 = np.sqrt(2), np.sqrt(3)
# pyquil.simulation.matrices.STATES (pyquil==4.5.0) in the code order of include/fbx.h
STATE_VECTORS = np.array([
    [1 / _s2, 1 / _s2], [1 / _s2, -1 / _s2], [1 / _s2, 1j / _s2], [1 / _s2, -1j / _s2],
    [1, 0], [0, 1], [1, 0], [1 / _s3, _s2 / _s3],
    [1 / _s3, np.exp(-2j * np.pi / 3) * _s2 / _s3], [1 / _s3, np.exp(2j * np.pi / 3) * _s2 / _s3],
], dtype=complex)
PAULIS_1Q = np.array([[[1, 0], [0, 1]], [[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]]],
                     dtype=complex)


def haar_unitary(dim, rs):
    """Haar-random unitary: Ginibre -> QR -> fix the phases of R's diagonal."""
    z = rs.randn(dim, dim) + 1j * rs.randn(dim, dim)
    q, r = np.linalg.qr(z)
    diag = np.diagonal(r)
    return q @ (np.diag(diag) / np.absolute(diag))


def product_state_matrix(codes):
    mat = np.array([[1.0 + 0j]])
    for c in codes:
        v = STATE_VECTORS[c][:, None]
        mat = np.kron(mat, v @ v.conj().T)
    return mat


def pauli_matrix(codes):
    mat = np.array([[1.0 + 0j]])
    for c in codes:
        mat = np.kron(mat, PAULIS_1Q[c])
    return mat


def exact_process_expectations(design: Design, unitaries, depolarizing=0.0):
    """e[b, k] = coef_k * tr[P_k E_b(rho_in,k)] for E_b = (1-lam) U.U^+ + lam tr(.) I/d."""
    d = design.dim
    u = np.asarray(unitaries).reshape(-1, d, d)
    keys = [tuple(r) for r in design.in_labels]
    uniq = list(dict.fromkeys(keys))
    sidx = np.array([uniq.index(k) for k in keys])
    rhos = np.array([product_state_matrix(k) for k in uniq])                  # [S, d, d]
    pkeys = [tuple(r) for r in design.paulis]
    puniq = list(dict.fromkeys(pkeys))
    pidx = np.array([puniq.index(k) for k in pkeys])
    ps = np.array([pauli_matrix(k) for k in puniq])                          # [P, d, d]
    out = np.einsum('bij,sjk,blk->bsil', u, rhos, u.conj())                   # U rho U^+
    if depolarizing:
        out = (1 - depolarizing) * out + depolarizing * np.eye(d)[None, None] / d
    t = np.real(np.einsum('pxy,bsyx->bsp', ps, out))                          # tr(P out)
    return t[:, sidx, pidx] * design.coefs[None, :]


def exact_state_expectations(design: Design, states):
    """e[b, k] = coef_k * tr[P_k rho_b]."""
    d = design.dim
    rho = np.asarray(states).reshape(-1, d, d)
    ps = np.array([pauli_matrix(k) for k in design.paulis])
    return np.real(np.einsum('kxy,byx->bk', ps, rho)) * design.coefs[None, :]


def sample_expectations(exact, shots, first_item=0, seed_base=2000):
    """Binomial sampling per item with RandomState(seed_base + item)."""
    exact = np.asarray(exact)
    e = np.empty_like(exact)
    for b in range(exact.shape[0]):
        rs = np.random.RandomState(seed_base + first_item + b)
        kp = rs.binomial(shots, np.clip((1 + exact[b]) / 2, 0, 1))
        e[b] = 2 * kp / shots - 1
    return e, np.full(exact.shape, float(shots))


def process_batch(n_qubits, in_basis="pauli", batch=1, shots=1000, first_item=0,
                  depolarizing=0.0):
    """(design, unitaries[B,d,d], expectations[B,m], counts[B,m]) for items
    first_item .. first_item + batch - 1 of the SURVEY 8d recipe."""
    design = process_design(n_qubits, in_basis)
    d = design.dim
    us = np.array([haar_unitary(d, np.random.RandomState(1000 + first_item + b))
                   for b in range(batch)])
    exact = exact_process_expectations(design, us, depolarizing)
    e, c = sample_expectations(exact, shots, first_item)
    return design, us, e, c


def state_batch(n_qubits, batch=1, shots=1000, first_item=0, mixed=0.0):
    """(design, states[B,d,d], expectations[B,m], counts[B,m]); truth = Haar pure state
    (first column of haar_unitary(d, RandomState(1000 + item))), optionally mixed with I/d."""
    design = state_design(n_qubits)
    d = design.dim
    rhos = []
    for b in range(batch):
        psi = haar_unitary(d, np.random.RandomState(1000 + first_item + b))[:, :1]
        rho = psi @ psi.conj().T
        rhos.append((1 - mixed) * rho + mixed * np.eye(d) / d)
    rhos = np.array(rhos)
    exact = exact_state_expectations(design, rhos)
    e, c = sample_expectations(exact, shots, first_item)
    return design, rhos, e, c


def kraus_batch(n_qubits, n_kraus, batch, seed=0):
    """Random CPTP Kraus sets [B, K, d, d]: G_j Ginibre, K_j = G_j S^{-1/2}, S = sum G_j^+ G_j."""
    d = 2 ** n_qubits
    rs = np.random.RandomState(seed)
    g = rs.randn(batch, n_kraus, d, d) + 1j * rs.randn(batch, n_kraus, d, d)
    s = np.einsum('bkji,bkjl->bil', g.conj(), g)
    w, v = np.linalg.eigh(s)
    s_inv_half = np.einsum('bij,bj,bkj->bik', v, 1 / np.sqrt(w), v.conj())
    return np.einsum('bkij,bjl->bkil', g, s_inv_half)


def qv_shots(probabilities, shots, depolarizing=0.0, seed=3000):
    """Measured bitstrings of quantum-volume circuits: ``probabilities [B, 2^n]`` (the ideal output distributions,
    ``quantum_volume.collect_heavy_outputs_batch(..., return_probabilities=True)``) -> ``[B, shots, n]`` uint8 bit arrays as
    ``qc.run`` returns them (first column = qubit 0 = the most significant bit of the output index), sampled from
    ``(1 - depolarizing) p + depolarizing / 2^n``; circuit b draws from ``np.random.default_rng([seed, b])``."""
    p = np.asarray(probabilities, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] < 2 or p.shape[1] & (p.shape[1] - 1):
        raise ValueError("probabilities must be [B, 2^n]")
    if not 0.0 <= depolarizing <= 1.0 or int(shots) < 0:
        raise ValueError("need 0 <= depolarizing <= 1 and shots >= 0")
    B, N = p.shape
    n = N.bit_length() - 1
    out = np.empty((B, int(shots), n), dtype=np.uint8)
    shifts = np.arange(n - 1, -1, -1)
    for b in range(B):
        total = p[b].sum()
        if not np.isfinite(total) or total <= 0.0 or p[b].min() < 0.0:
            raise ValueError(f"probabilities[{b}] is not a distribution (sum {total}): a poisoned or empty item cannot be sampled")
        q = (1.0 - depolarizing) * p[b] / total + depolarizing / N
        idx = np.random.default_rng([int(seed), b]).choice(N, size=int(shots), p=q / q.sum())
        out[b] = (idx[:, None] >> shifts) & 1
    return out


def qv_shots_batch(probabilities, shots, depolarizing=0.0, readout_flip=None, seed=3000):
    """``qv_shots`` drawn on the device (``sampling.sample_bitstrings_batch``): the same shapes and the same distribution, one launch
    for the batch instead of one ``choice`` per circuit; optionally with readout flips (``[n, 2]`` or ``[B, n, 2]``).  The stream is
    the device's (include/fbx.h), not numpy's: circuit b is item b of the Philox stream keyed by ``seed``, and the records differ
    from those of ``qv_shots`` shot by shot."""
    from .sampling import sample_bitstrings_batch
    return sample_bitstrings_batch(probabilities, shots, depolarizing=depolarizing, readout_flip=readout_flip, seed=int(seed))


def qv_shots_wide_batch(probabilities, shots, depolarizing=0.0, readout_flip=None, seed=3000):
    """``qv_shots_batch`` for widths 1..26 (``sampling.sample_bitstrings_wide_batch``): up to 13 qubits it IS ``qv_shots_batch``."""
    from .sampling import sample_bitstrings_wide_batch
    return sample_bitstrings_wide_batch(probabilities, shots, depolarizing=depolarizing, readout_flip=readout_flip, seed=int(seed))


def rb_data(n_qubits, depths, decay=0.97, shots=500, batch=1, seed=4000):
    """Synthetic randomized-benchmarking statistics in the shapes ``randomized_benchmarking.fit_rb_results_batch`` takes:
    ``(z_expectations, z_std_errs)``, both [batch, len(depths), 2^n - 1].  A sequence of depth m leaves the depolarised state
    decay^m |0..0><0..0| + (1 - decay^m) I / 2^n; its ``shots`` outcomes are drawn from ``np.random.default_rng([seed, b])``
    (multinomial), observable z (a non-zero bit mask, in increasing order) has the expectation of (-1)^popcount(outcome & z)
    and the standard error sqrt((1 - e^2) / shots) -- all from ONE set of shots, hence covariant.  ``decay`` may be [batch]."""
    depths = np.asarray(depths, dtype=np.float64)
    dim = 1 << int(n_qubits)
    decay = np.broadcast_to(np.asarray(decay, dtype=np.float64), (int(batch),))
    outcomes = np.arange(dim)
    masks = np.arange(1, dim)
    parity = np.array([[bin(int(x & z)).count("1") & 1 for x in outcomes] for z in masks])
    signs = 1.0 - 2.0 * parity                                                  # [dim - 1, dim]
    e = np.empty((int(batch), len(depths), dim - 1))
    for b in range(int(batch)):
        rng = np.random.default_rng([int(seed), b])
        f = decay[b] ** depths
        probs = np.outer(1.0 - f, np.full(dim, 1.0 / dim))
        probs[:, 0] += f
        counts = np.stack([rng.multinomial(int(shots), p / p.sum()) for p in probs])
        e[b] = counts @ signs.T / float(shots)
    return e, np.sqrt(np.clip(1.0 - e * e, 0.0, None) / float(shots))


def rb_sequence_data(n_qubits, depths, noise_ptms, num_sequences=32, interleaved_gate=None, shots=None, seed=4000):
    """Randomized-benchmarking statistics from actual sequences under actual noise, in the shapes of ``rb_data``: Clifford
    sequences are drawn and simulated on the device under the Pauli transfer matrices ``noise_ptms`` ([G, 4^n, 4^n], or
    [batch, G, 4^n, 4^n] for a batch of experiments) and averaged per depth -- no decay is assumed
    (``randomized_benchmarking.simulate_rb_experiment_batch``)."""
    from . import randomized_benchmarking as rb
    return rb.simulate_rb_experiment_batch(n_qubits, depths, num_sequences, noise_ptms, interleaved_gate=interleaved_gate, seed=seed,
                                           shots=shots)


def spectroscopy_data(kind, xs, shots=500, batch=1, seed=5000, **params):
    """Synthetic single-qubit spectroscopy statistics for ``qubit_spectroscopy.fit_*_results_batch``: ``(expectations, std_errs)``,
    both [batch, len(xs)].  ``kind``: 't1' (amplitude, decay_time, offset), 't2' (amplitude, decay_time, offset, baseline,
    frequency), 'rabi' or 'cz_ramsey' (amplitude, offset, baseline, frequency) -- the model of analysis/fitting.py for the
    probability p1 of measuring 1, with the parameters given by name (scalars or [batch]).  Every point is k ~ Binomial(shots, p1)
    from ``np.random.default_rng([seed, b])``; the Pauli expectation is 1 - 2 k / shots (the fit front ends negate it) and the
    standard error sqrt((1 - e^2) / shots), zero where k is 0 or ``shots``."""
    from .analysis import fitting
    models = {"t1": fitting.decay_time_param_decay, "t2": fitting.decaying_cosine, "rabi": fitting.shifted_cosine,
              "cz_ramsey": fitting.shifted_cosine}
    if kind not in models:
        raise ValueError(f"kind must be one of {sorted(models)}")
    xs = np.asarray(xs, dtype=np.float64)
    cols = {k: np.broadcast_to(np.asarray(v, dtype=np.float64), (int(batch),)) for k, v in params.items()}
    e = np.empty((int(batch), len(xs)))
    for b in range(int(batch)):
        rng = np.random.default_rng([int(seed), b])
        p1 = np.clip(models[kind](xs, **{k: v[b] for k, v in cols.items()}), 0.0, 1.0)
        e[b] = 1.0 - 2.0 * rng.binomial(int(shots), p1) / float(shots)
    return e, np.sqrt(np.clip(1.0 - e * e, 0.0, None) / float(shots))


def readout_shots(confusion, shots, seed=6000):
    """Measured bitstrings of a joint readout characterisation: ``confusion [G, 2^g, 2^g]`` (or one ``[2^g, 2^g]`` matrix), row =
    the prepared bitstring, column = the observed one, rows summing to 1 -> ``[G, 2^g, shots, g]`` uint8 (``[2^g, shots, g]`` for
    one matrix) as ``readout.joint_confusion_matrices_batch`` takes them: the observed strings of row r of group G are drawn from
    that row by ``np.random.default_rng([seed, G, r])``, first column = most significant bit."""
    c = np.asarray(confusion, dtype=np.float64)
    single = c.ndim == 2
    c = c[None] if single else c
    if c.ndim != 3 or c.shape[1] != c.shape[2] or c.shape[1] < 2 or c.shape[1] & (c.shape[1] - 1):
        raise ValueError("confusion must be [G, 2^g, 2^g]")
    if int(shots) < 0 or c.min() < 0.0 or not np.allclose(c.sum(axis=2), 1.0):
        raise ValueError("need shots >= 0 and rows that are probability distributions")
    G, N = c.shape[:2]
    g = N.bit_length() - 1
    shifts = np.arange(g - 1, -1, -1)
    out = np.empty((G, N, int(shots), g), dtype=np.uint8)
    for grp in range(G):
        for r in range(N):
            idx = np.random.default_rng([int(seed), grp, r]).choice(N, size=int(shots), p=c[grp, r] / c[grp, r].sum())
            out[grp, r] = (idx[:, None] >> shifts) & 1
    return out[0] if single else out


def readout_shots_batch(confusion, shots, seed=6000):
    """``readout_shots`` drawn on the device: every row of every confusion matrix is one item of ``sample_bitstrings_batch`` (row r
    of group G is item ``G 2^g + r`` of the Philox stream keyed by ``seed``); the output has the shape of ``readout_shots``."""
    from .sampling import sample_bitstrings_batch
    c = np.asarray(confusion, dtype=np.float64)
    single = c.ndim == 2
    c = c[None] if single else c
    if c.ndim != 3 or c.shape[1] != c.shape[2] or c.shape[1] < 2 or c.shape[1] & (c.shape[1] - 1):
        raise ValueError("confusion must be [G, 2^g, 2^g]")
    if int(shots) < 0 or c.min() < 0.0 or not np.allclose(c.sum(axis=2), 1.0):
        raise ValueError("need shots >= 0 and rows that are probability distributions")
    G, N = c.shape[:2]
    out = sample_bitstrings_batch(c.reshape(G * N, N), shots, seed=int(seed)).reshape(G, N, int(shots), N.bit_length() - 1)
    return out[0] if single else out


def adder_shots(n_bits, flip_probability, shots, seed=7000):
    """Results of an n-bit ripple-carry adder run in the layout of the reference's ``get_n_bit_adder_results``: ``[4^n, shots,
    n + 1]`` uint8, row r = the addition a + b that the 2n-bit number r spells; every answer bit of every shot is flipped
    independently with ``flip_probability``; addition r draws from ``np.random.default_rng([seed, r])``."""
    from .classical_logic.ripple_carry_adder import adder_expected_bits
    if not 0.0 <= flip_probability <= 1.0 or int(shots) < 0:
        raise ValueError("need 0 <= flip_probability <= 1 and shots >= 0")
    ans = adder_expected_bits(int(n_bits))
    out = np.empty((ans.shape[0], int(shots), ans.shape[1]), dtype=np.uint8)
    for r in range(ans.shape[0]):
        flips = np.random.default_rng([int(seed), r]).random((int(shots), ans.shape[1])) < flip_probability
        out[r] = ans[r] ^ flips
    return out


def ghz_shots(n, flip_probability, shots, seed=8000):
    """Bitstrings measured on an n-qubit GHZ state: ``[shots, n]`` uint8, every shot all zeros or all ones with equal probability,
    then every bit flipped independently with ``flip_probability``; drawn from ``np.random.default_rng(seed)``."""
    if int(n) < 1 or not 0.0 <= flip_probability <= 1.0 or int(shots) < 0:
        raise ValueError("need n >= 1, 0 <= flip_probability <= 1 and shots >= 0")
    rng = np.random.default_rng(int(seed))
    side = rng.integers(0, 2, size=(int(shots), 1), dtype=np.uint8)
    flips = rng.random((int(shots), int(n))) < flip_probability
    return (side ^ flips).astype(np.uint8)


# --------------------------------------------------------------------------------------------------
# The stream of fbx_tomo_simulate (include/fbx.h), restated in numpy from the contract: what a host program checks the
# device's simulated tomography counts against.
# --------------------------------------------------------------------------------------------------
TOMO_KEY_TAG = 0x544F4D4F


def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """One Philox4x32-10 block per element (Salmon et al., SC'11): counter words and key words as uint64 arrays or scalars
    holding 32-bit values -> the four output words (uint64 arrays holding 32-bit values)."""
    mask = np.uint64(0xFFFFFFFF)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return c0, c1, c2, c3


DFE_KEY_TAG = 0x44464530                 # the shots of fbx_dfe_simulate
DFE_CALIBRATION_KEY_TAG = 0x44464543     # ... of its calibration mode


def restate_tomography_counts(exact, coefs, shots, seed, first_item=0):
    """``restate_dfe_counts`` under the key tag of ``fbx_tomo_simulate``: the counts ``tomography.simulate_*_tomography_batch``
    draws, restated on the host (the stream is described there)."""
    return restate_dfe_counts(exact, coefs, shots, seed, first_item, key_tag=TOMO_KEY_TAG)


def restate_dfe_counts(exact, coefs, shots, seed, first_item=0, key_tag=DFE_KEY_TAG):
    """The counts a simulated experiment draws, restated on the host from the contract of ``fbx_tomo_simulate`` and
    ``fbx_dfe_simulate`` (include/fbx.h): ``exact [B, m]`` = coefficient times the mean of the measured product (the
    ``return_exact`` output), ``coefs [m]`` the non-zero observable coefficients, ``shots`` = N >= 1, ``seed`` the 64-bit key and
    item b the global item ``first_item + b``.  Per setting: mu = exact / coef, q = 0.5 mu + 0.5 clamped to [0, 1], t =
    floor(q 2^32); shot s counts +1 iff word ``s & 3`` of the Philox4x32-10 block with counter (g low, g high, k, s >> 2) and
    key (seed low ^ key_tag, seed high) is below t: ``key_tag`` is 0x544F4D4F for ``fbx_tomo_simulate``
    (``restate_tomography_counts``), 0x44464530 for ``fbx_dfe_simulate`` and 0x44464543 for its calibration mode, where
    ``coefs`` are the signs c_k.  Returns ``(expectations, total_counts, std_errs, k_plus)``, all [B, m],
    ``k_plus`` int64: expectation = coef (k+ - k-) / N, std_err = |coef| sqrt(4 k+ k- / N) / N."""
    exact = np.atleast_2d(np.asarray(exact, dtype=np.float64))
    B, m = exact.shape
    coefs = np.broadcast_to(np.asarray(coefs, dtype=np.float64), (m,))
    N, seed, first_item = int(shots), int(seed) & (2 ** 64 - 1), int(first_item)
    if not 1 <= N < 2 ** 32 or first_item < 0 or not np.all(coefs != 0.0):
        raise ValueError("need 1 <= shots < 2^32, first_item >= 0 and non-zero coefficients")
    mu = exact / coefs[None, :]
    q = np.clip(0.5 * mu + 0.5, 0.0, 1.0)
    t = np.floor(q * 2.0 ** 32).astype(np.uint64)                       # in [0, 2^32]
    k0, k1 = (seed & 0xFFFFFFFF) ^ (int(key_tag) & 0xFFFFFFFF), seed >> 32
    n_blocks = (N + 3) // 4
    blocks = np.arange(n_blocks, dtype=np.uint64)
    valid = [4 * blocks + np.uint64(w) < np.uint64(N) for w in range(4)]  # the last block of a count that is no multiple of 4
    k_plus = np.zeros((B, m), dtype=np.int64)
    rows = max(1, (1 << 21) // n_blocks)                                 # settings per pass: about 2^21 blocks at a time
    ks = np.arange(m, dtype=np.uint64)
    for b in range(B):
        g = first_item + b
        for lo in range(0, m, rows):
            k = ks[lo:lo + rows, None]
            words = _philox4x32_10(np.uint64(g & 0xFFFFFFFF), np.uint64(g >> 32), k, blocks[None, :], k0, k1)
            tt = t[b, lo:lo + rows, None]
            k_plus[b, lo:lo + rows] = sum(((w < tt) & v[None, :]).sum(axis=1) for w, v in zip(words, valid))
    k_minus = N - k_plus
    e = coefs[None, :] * ((k_plus - k_minus).astype(np.float64) / float(N))
    prod = np.array([[int(p) * int(q_) * 4 for p, q_ in zip(rp, rm)] for rp, rm in zip(k_plus, k_minus)], dtype=object)
    s = np.abs(coefs)[None, :] * np.sqrt(prod.astype(np.float64) / float(N)) / float(N)
    return e, np.full((B, m), float(N)), s, k_plus


TOMO_GROUPED_KEY_TAG = 0x544F4D47        # "TOMG": the shots of fbx_tomo_simulate_grouped


def restate_grouped_tomography_counts(probabilities, grouping_or_group_of, paulis, coefs, shots, seed, first_item=0):
    """Steps 3-5 of the contract of ``fbx_tomo_simulate_grouped`` (include/fbx.h) restated on the host from the distributions it
    reports: ``probabilities [B, G, 2^n]`` (the ``return_probabilities`` output), the grouping (a ``design.Grouping`` or its
    ``group_of [m]``), ``paulis [m, n]`` and ``coefs [m]`` of the design.  Per (item, group): c = cumsum(max(p, 0)) in outcome
    order, thr_o = floor(c_o / c_last 2^32) for every outcome but the last; shot s reads word ``s & 3`` of the Philox4x32-10 block
    with counter (gid low, gid high, group, s >> 2) and key (seed low ^ 0x544F4D47, seed high), gid = first_item + item; its
    outcome is the number of thresholds <= the word.  Member k counts k+ = the shots whose outcome has even parity on its support
    (bit t of an outcome = qubit n - 1 - t).  Returns ``(expectations [B, m], total_counts [B, m], std_errs [B, m], hist [B, G,
    2^n] int64)`` with the integer formulas of ``restate_tomography_counts``."""
    p = np.asarray(probabilities, dtype=np.float64)
    group_of = np.asarray(getattr(grouping_or_group_of, "group_of", grouping_or_group_of)).astype(np.int64)
    paulis = np.asarray(paulis)
    m, n = paulis.shape
    coefs = np.broadcast_to(np.asarray(coefs, dtype=np.float64), (m,))
    N, seed, first_item = int(shots), int(seed) & (2 ** 64 - 1), int(first_item)
    if p.ndim != 3 or p.shape[2] != 1 << n or group_of.shape != (m,) or group_of.min() < 0 or group_of.max() >= p.shape[1]:
        raise ValueError("need probabilities [B, G, 2^n], paulis [m, n] and group ids [m] in [0, G)")
    if not 1 <= N < 2 ** 32 or first_item < 0:
        raise ValueError("need 1 <= shots < 2^32 and first_item >= 0")
    B, G, d = p.shape
    c = np.cumsum(np.where(p < 0.0, 0.0, p), axis=2)                    # one addition per outcome, in outcome order
    if not np.all((c[:, :, -1] > 0.0) & np.isfinite(c[:, :, -1])):
        raise ValueError("a distribution whose clamped sum is not a positive finite number (a poisoned item) cannot be restated")
    thr = np.floor(c[:, :, :-1] / c[:, :, -1:] * 2.0 ** 32).astype(np.uint64)
    k0, k1 = (seed & 0xFFFFFFFF) ^ TOMO_GROUPED_KEY_TAG, seed >> 32
    blocks = np.arange((N + 3) // 4, dtype=np.uint64)
    hist = np.zeros((B, G, d), dtype=np.int64)
    for b in range(B):
        gid = first_item + b
        for g in range(G):
            words = _philox4x32_10(np.uint64(gid & 0xFFFFFFFF), np.uint64(gid >> 32), np.uint64(g), blocks, k0, k1)
            w = np.stack(np.broadcast_arrays(*words), axis=1).reshape(-1)[:N]                 # shot s = word s & 3 of block s >> 2
            hist[b, g] = np.bincount(np.searchsorted(thr[b, g], w, side="right"), minlength=d)
    z = ((paulis[:, ::-1] != 0) << np.arange(n)).sum(axis=1)             # bit t: the qubit n - 1 - t
    outcomes = np.arange(d)
    even = np.array([[bin(int(o) & int(zk)).count("1") % 2 == 0 for o in outcomes] for zk in z])       # [m, d]
    k_plus = np.einsum("bmo,mo->bm", hist[:, group_of, :], even.astype(np.int64))
    k_minus = N - k_plus
    e = coefs[None, :] * ((k_plus - k_minus).astype(np.float64) / float(N))
    prod = np.array([[int(a) * int(b_) * 4 for a, b_ in zip(rp, rm)] for rp, rm in zip(k_plus, k_minus)], dtype=object)
    s = np.abs(coefs)[None, :] * np.sqrt(prod.astype(np.float64) / float(N)) / float(N)
    return e, np.full((B, m), float(N)), s, hist


TOMO_SYMMETRIZED_KEY_TAG = 0x544F4D53    # "TOMS": the shots of fbx_tomo_simulate_symmetrized
TOMO_CALIBRATION_KEY_TAG = 0x544F4D43    # "TOMC": the shots of fbx_tomo_simulate_calibration


def symmetrization_patterns(mask, symm_type):
    """The flip masks of a unit whose members act on the qubits of ``mask`` (bit t = qubit n - 1 - t), in ascending order:
    every submask for ``symm_type = -1`` (exhaustive symmetrization), 0 alone for ``symm_type = 0``.  The orthogonal arrays
    (1, 2, 3) are not implemented: ``ValueError``."""
    if symm_type not in (-1, 0):
        raise ValueError("symm_type must be -1 (exhaustive) or 0 (none); the orthogonal arrays 1, 2, 3 are not implemented")
    mask = int(mask)
    if symm_type == 0:
        return [0]
    out, f = [], 0
    while True:
        out.append(f)
        f = (f - mask) & mask                                            # the next submask, ascending
        if f == 0:
            return out


def shots_per_pattern(shots, mask, symm_type):
    """``floor(shots / patterns)`` of a unit (this library's rule, include/fbx.h); 0 or 2^29 and more raise ``ValueError``"""
    s = int(shots) // len(symmetrization_patterns(mask, symm_type))
    if not 1 <= s < 2 ** 29:
        raise ValueError("need at least one and fewer than 2^29 shots per flip pattern: floor(shots / patterns) is out of range")
    return s


def symmetrized_pattern_distributions(ideal, confusion, masks, symm_type):
    """``q_f(r) = sum_o p(o) C[o ^ f][r ^ f]`` in dense float64 (not the device's summation order): ``ideal [B, G, 2^n]`` the
    distributions without readout error, ``confusion [B, 2^n, 2^n]`` or ``[2^n, 2^n]`` laid out [drawn][read], ``masks [G]`` the
    union of the members' parity masks per group -> ``[B, G, 2^n, 2^n]``, row f = pattern f, a zero row where f is no pattern."""
    p = np.asarray(ideal, dtype=np.float64)
    B, G, d = p.shape
    c = np.broadcast_to(np.asarray(confusion, dtype=np.float64), (B, d, d))
    idx = np.arange(d)
    out = np.zeros((B, G, d, d))
    for g in range(G):
        for f in symmetrization_patterns(masks[g], symm_type):
            out[:, g, f, :] = np.einsum("bo,bor->br", p[:, g, :], c[:, idx ^ f][:, :, idx ^ f])
    return out


def _restate_symmetrized_hist(q, patterns, s, k0, k1, gid, unit):
    """the merged histogram of one unit: ``q [2^n, 2^n]`` its rows by flip mask, ``s`` shots per pattern"""
    d = q.shape[1]
    blocks = np.arange((s + 3) // 4, dtype=np.uint64)
    hist = np.zeros(d, dtype=np.int64)
    for f in patterns:
        c = np.cumsum(np.where(q[f] < 0.0, 0.0, q[f]))
        if not (c[-1] > 0.0 and np.isfinite(c[-1])):
            raise ValueError("a pattern whose clamped sum is not a positive finite number (a poisoned item) cannot be restated")
        thr = np.floor(c[:-1] / c[-1] * 2.0 ** 32).astype(np.uint64)
        words = _philox4x32_10(np.uint64(gid & 0xFFFFFFFF), np.uint64(gid >> 32), np.uint64(unit),
                               np.uint64(f << 27) | blocks, k0, k1)
        w = np.stack(np.broadcast_arrays(*words), axis=1).reshape(-1)[:s]                     # shot t = word t & 3 of block t >> 2
        hist += np.bincount(np.searchsorted(thr, w, side="right"), minlength=d)
    return hist


def _parity_counts(hist, z):
    d = hist.shape[-1]
    even = np.array([bin(o & int(z)).count("1") % 2 == 0 for o in range(d)])
    return int(hist[even].sum())


def restate_symmetrized_tomography_counts(probabilities, grouping_or_group_of, paulis, coefs, shots, symm_type, seed, first_item=0):
    """Steps 4-5 of the contract of ``fbx_tomo_simulate_symmetrized`` (include/fbx.h) restated on the host from the per-pattern
    distributions it reports: ``probabilities [B, G, 2^n, 2^n]`` (row f = the un-flipped record's distribution under flip mask f;
    the ``return_probabilities`` output), the grouping (a ``design.Grouping`` or its ``group_of [m]``), ``paulis [m, n]`` and
    ``coefs [m]`` of the design, ``shots`` the total of a group.  Per (item, group): the patterns are the submasks of the union of
    the members' masks (``symm_type = -1``) or 0 alone (0); every pattern draws s = floor(shots / patterns) shots with the
    thresholds of ``restate_grouped_tomography_counts``; shot t of pattern f reads word ``t & 3`` of the Philox4x32-10 block with
    counter (gid low, gid high, group, (f << 27) | (t >> 2)) and key (seed low ^ 0x544F4D53, seed high).  The histograms of the
    patterns are added, and member k counts k+ on the sum with N = s x patterns.  Returns ``(expectations [B, m], total_counts
    [B, m], std_errs [B, m], hist [B, G, 2^n] int64)``; ``ValueError`` for the orthogonal arrays and for s == 0."""
    p = np.asarray(probabilities, dtype=np.float64)
    group_of = np.asarray(getattr(grouping_or_group_of, "group_of", grouping_or_group_of)).astype(np.int64)
    paulis = np.asarray(paulis)
    m, n = paulis.shape
    coefs = np.broadcast_to(np.asarray(coefs, dtype=np.float64), (m,))
    seed, first_item = int(seed) & (2 ** 64 - 1), int(first_item)
    if p.ndim != 4 or p.shape[2:] != (1 << n, 1 << n) or group_of.shape != (m,) or group_of.min() < 0 or group_of.max() >= p.shape[1]:
        raise ValueError("need probabilities [B, G, 2^n, 2^n], paulis [m, n] and group ids [m] in [0, G)")
    if not 1 <= int(shots) < 2 ** 32 or first_item < 0:
        raise ValueError("need 1 <= shots < 2^32 and first_item >= 0")
    B, G, d = p.shape[:3]
    z = ((paulis[:, ::-1] != 0) << np.arange(n)).sum(axis=1)             # bit t: the qubit n - 1 - t
    union = np.zeros(G, dtype=np.int64)
    np.bitwise_or.at(union, group_of, z)
    patterns = [symmetrization_patterns(u, symm_type) for u in union]
    per = [shots_per_pattern(shots, u, symm_type) for u in union]
    k0, k1 = (seed & 0xFFFFFFFF) ^ TOMO_SYMMETRIZED_KEY_TAG, seed >> 32
    hist = np.zeros((B, G, d), dtype=np.int64)
    for b in range(B):
        for g in range(G):
            hist[b, g] = _restate_symmetrized_hist(p[b, g], patterns[g], per[g], k0, k1, first_item + b, g)
    e, cnt, se = np.empty((B, m)), np.empty((B, m)), np.empty((B, m))
    for k in range(m):
        g = group_of[k]
        N = per[g] * len(patterns[g])
        for b in range(B):
            kp = _parity_counts(hist[b, g], z[k]); km = N - kp
            e[b, k] = coefs[k] * (float(kp - km) / float(N))
            se[b, k] = abs(coefs[k]) * np.sqrt(float(4 * kp * km) / float(N)) / float(N)
            cnt[b, k] = float(N)
    return e, cnt, se, hist


def restate_readout_calibration_counts(confusion, cal_paulis, shots, symm_type, seed, first_item=0):
    """The stream of ``fbx_tomo_simulate_calibration`` (include/fbx.h) restated on the host: ``confusion [B, 2^n, 2^n]`` (or one
    matrix) laid out [drawn][read], ``cal_paulis [n_cal, n]`` the Pauli codes of the calibrations.  Calibration c with parity mask
    z_c draws, per flip mask f (the submasks of z_c, or 0 alone for ``symm_type = 0``), s = floor(shots / patterns) un-flipped
    records from ``q_f(r) = C[f][r ^ f]``; shot t reads word ``t & 3`` of the block with counter (gid low, gid high, c, (f << 27) |
    (t >> 2)) and key (seed low ^ 0x544F4D43, seed high).  Returns ``(cal_means, cal_vars, cal_counts [B, n_cal], hist [B, n_cal,
    2^n] int64)``: mean = (k+ - k-) / N, var = 4 k+ k- / N^3 (the variance of the mean of the +-1 values), N = s x patterns."""
    c = np.asarray(confusion, dtype=np.float64)
    c = c[None] if c.ndim == 2 else c
    cal_paulis = np.asarray(cal_paulis)
    n_cal, n = cal_paulis.shape
    d = 1 << n
    seed, first_item = int(seed) & (2 ** 64 - 1), int(first_item)
    if c.ndim != 3 or c.shape[1:] != (d, d):
        raise ValueError("need confusion [B, 2^n, 2^n] and cal_paulis [n_cal, n]")
    if not 1 <= int(shots) < 2 ** 32 or first_item < 0:
        raise ValueError("need 1 <= shots < 2^32 and first_item >= 0")
    B = c.shape[0]
    z = ((cal_paulis[:, ::-1] != 0) << np.arange(n)).sum(axis=1)
    patterns = [symmetrization_patterns(zc, symm_type) for zc in z]
    per = [shots_per_pattern(shots, zc, symm_type) for zc in z]
    k0, k1 = (seed & 0xFFFFFFFF) ^ TOMO_CALIBRATION_KEY_TAG, seed >> 32
    idx = np.arange(d)
    mean, var, cnt = np.empty((B, n_cal)), np.empty((B, n_cal)), np.empty((B, n_cal))
    hist = np.zeros((B, n_cal, d), dtype=np.int64)
    for b in range(B):
        for k in range(n_cal):
            q = np.zeros((d, d))
            for f in patterns[k]:
                q[f] = c[b, f, idx ^ f]
            hist[b, k] = _restate_symmetrized_hist(q, patterns[k], per[k], k0, k1, first_item + b, k)
            N = per[k] * len(patterns[k])
            kp = _parity_counts(hist[b, k], z[k]); km = N - kp
            mean[b, k] = float(kp - km) / float(N)
            var[b, k] = float(4 * kp * km) / float(N) / float(N) / float(N)
            cnt[b, k] = float(N)
    return mean, var, cnt, hist


QV_GATE_ERROR_KEY_TAG = 0x51564745      # "QVGE": the Pauli errors of fbx_qv_noisy_trajectories


def restate_qv_gate_errors(B, trajectories, L, gate_error, seed, first_item=0):
    """The Pauli errors ``fbx_qv_noisy_trajectories`` inserts, restated on the host from its contract (include/fbx.h): ``uint8
    [B, T, L]``, entry ``[b, t, l]`` = the Pauli index ``k = 4 a + c`` in 1..15 (a on q0, c on q1 of the gate's pair; 0 = I, 1 = X,
    2 = Y, 3 = Z) that follows gate l of circuit b in trajectory t, or 0 for none.  ``gate_error``: a scalar, ``[B]`` or ``[B, L]``.
    Trajectory t of the global circuit ``g = first_item + b`` owns the Philox4x32-10 blocks with counter (g low, g high, t, j) and key
    (seed low ^ 0x51564745, seed high); block j serves gates 2 j (words x0, x1) and 2 j + 1 (words x2, x3); a gate errs iff
    ``float(x_first) * 2^-32 < gate_error`` and then ``k = 1 + ((x_second * 15) >> 32)``.  ``quantum_volume.fold_gate_errors``
    turns the indices of a trajectory into an ordinary circuit."""
    B, T, L = int(B), int(trajectories), int(L)
    seed, first_item = int(seed) & (2 ** 64 - 1), int(first_item)
    if B < 0 or L < 0 or not 0 <= T < 2 ** 32 or first_item < 0:
        raise ValueError("need B >= 0, L >= 0, 0 <= trajectories < 2^32 and first_item >= 0")
    ge = np.asarray(gate_error, dtype=np.float64)
    if ge.shape == (B,):
        ge = ge[:, None]
    elif ge.shape not in ((), (B, L)):
        raise ValueError(f"gate_error must be a scalar, [B] = {(B,)} or [B, L] = {(B, L)}, not {ge.shape}")
    ge = np.broadcast_to(ge, (B, L))
    k0, k1 = (seed & 0xFFFFFFFF) ^ QV_GATE_ERROR_KEY_TAG, seed >> 32
    out = np.zeros((B, T, L), dtype=np.uint8)
    n_blocks = (L + 1) // 2
    if not (B and T and L):
        return out
    ts = np.arange(T, dtype=np.uint64)[:, None]
    js = np.arange(n_blocks, dtype=np.uint64)[None, :]
    for b in range(B):
        g = first_item + b
        x0, x1, x2, x3 = (np.broadcast_to(w, (T, n_blocks)) for w in
                          _philox4x32_10(np.uint64(g & 0xFFFFFFFF), np.uint64(g >> 32), ts, js, k0, k1))
        first = np.stack([x0, x2], axis=-1).reshape(T, 2 * n_blocks)[:, :L]
        second = np.stack([x1, x3], axis=-1).reshape(T, 2 * n_blocks)[:, :L]
        errs = first.astype(np.float64) * 2.0 ** -32 < ge[b][None, :]
        k = np.uint64(1) + ((second * np.uint64(15)) >> np.uint64(32))
        out[b] = np.where(errs, k, np.uint64(0)).astype(np.uint8)
    return out


# --------------------------------------------------------------------------------------------------
# fbx_rpe_simulate (include/fbx.h) on the host: the distributions mirrored in numpy, the shots restated in integers.
# --------------------------------------------------------------------------------------------------
RPE_SIM_KEY_TAG = 0x52504553             # "RPES": the shots of fbx_rpe_simulate


def pauli_transfer_matrix(kraus_ops):
    """The real Pauli transfer matrix R[i, j] = sum_k tr[P_i K_k P_j K_k^+] / d of a channel given by its Kraus operators (one
    d x d matrix = a unitary), in numpy: Pauli indices in base 4 with qubit 0 most significant, the order of include/fbx.h."""
    ks = np.asarray(kraus_ops, dtype=complex)
    ks = ks[None] if ks.ndim == 2 else ks
    d = ks.shape[-1]
    n = int(round(np.log2(d)))
    ps = np.array([pauli_matrix(codes) for codes in itertools.product(range(4), repeat=n)])
    out = np.einsum('iab,kbc,jcd,kad->ij', ps, ks, ps, ks.conj()) / d
    return np.ascontiguousarray(out.real)


def pauli_vector_of_state(rho):
    """tr[P_k rho] for every Pauli index k (the ``init`` of fbx_rpe_simulate); ``rho`` a density matrix or a state vector."""
    rho = np.asarray(rho, dtype=complex)
    rho = np.outer(rho, rho.conj()) if rho.ndim == 1 else rho
    n = int(round(np.log2(rho.shape[0])))
    return np.array([np.trace(pauli_matrix(codes) @ rho).real for codes in itertools.product(range(4), repeat=n)])


def _rpe_sim_indices(n, xy_qubit, z_qubit):
    sh_xy = 2 * (n - 1 - xy_qubit)
    iz = 0 if z_qubit is None else 3 << (2 * (n - 1 - z_qubit))
    return [1 << sh_xy, 2 << sh_xy], iz


def rpe_distributions(gate_ptm, num_depths, prep_ptm=None, meas_ptm=None, init=None, xy_qubit=0, z_qubit=None, flips=None):
    """Steps 1-2 of the contract of ``fbx_rpe_simulate`` (include/fbx.h) in numpy float64: ``gate_ptm [B, D, D]``, ``prep_ptm`` /
    ``meas_ptm`` ``[D, D]``, ``[B, D, D]`` or None, ``init [D]`` (None: |+> on every qubit), ``flips [n, 2]``, ``[B, n, 2]`` or None.
    G^(2^j) is ``np.linalg.matrix_power``.  Returns ``prob [B, K, 2, M]``, M = 4 with a partner (outcome 2 s + t) and 2 without;
    the sums are numpy's, so the device agrees within rounding, not bit for bit."""
    G = np.asarray(gate_ptm, dtype=np.float64)
    G = G[None] if G.ndim == 2 else G
    B, D = G.shape[0], G.shape[-1]
    n = {4: 1, 16: 2}[D]
    K = int(num_depths)
    if init is None:
        init = pauli_vector_of_state(np.full(1 << n, 2.0 ** (-n / 2)))
    eye = np.eye(D)
    prep = np.broadcast_to(eye if prep_ptm is None else np.asarray(prep_ptm, dtype=np.float64), (B, D, D))
    meas = np.broadcast_to(eye if meas_ptm is None else np.asarray(meas_ptm, dtype=np.float64), (B, D, D))
    fl = None if flips is None else np.broadcast_to(np.asarray(flips, dtype=np.float64), (B, n, 2))
    iP, iZ = _rpe_sim_indices(n, xy_qubit, z_qubit)
    M = 2 if z_qubit is None else 4
    out = np.empty((B, K, 2, M))
    for b in range(B):
        w = prep[b] @ np.asarray(init, dtype=np.float64)
        for j in range(K):
            v = meas[b] @ (np.linalg.matrix_power(G[b], 2 ** j) @ w)
            for basis in range(2):
                vP = v[iP[basis]]
                if z_qubit is None:
                    p = np.array([(v[0] + vP) * 0.5, (v[0] - vP) * 0.5])
                    if fl is not None:
                        f0, f1 = fl[b, xy_qubit]
                        p = np.array([(1 - f0) * p[0] + f1 * p[1], f0 * p[0] + (1 - f1) * p[1]])
                else:
                    vZ, vPZ = v[iZ], v[iP[basis] | iZ]
                    p = np.array([[v[0] + vP + vZ + vPZ, v[0] + vP - vZ - vPZ],
                                  [v[0] - vP + vZ - vPZ, v[0] - vP - vZ + vPZ]]) * 0.25             # [s, t]
                    if fl is not None:
                        (f0, f1), (g0, g1) = fl[b, xy_qubit], fl[b, z_qubit]
                        p = np.array([[1 - f0, f1], [f0, 1 - f1]]) @ p @ np.array([[1 - g0, g1], [g0, 1 - g1]]).T
                    p = p.reshape(4)
                out[b, j, basis] = p
    return out


def restate_rpe_counts(probs, n_shots, seed, first_item=0):
    """Steps 3-4 of the contract of ``fbx_rpe_simulate`` (include/fbx.h) restated on the host, in integers, from the distributions it
    reports: ``probs [B, K, 2, M]`` (M = 2 or 4), ``n_shots [K]`` (or one number).  Per (item, depth j, basis): c = cumsum(max(p,
    0)) in outcome order, thr_o = floor(c_o / c_last 2^32) for every outcome but the last; shot s reads word ``s & 3`` of the
    Philox4x32-10 block with counter (gid low, gid high, 2 j + basis, s >> 2) and key (seed low ^ 0x52504553, seed high), gid =
    first_item + item; its outcome is the number of thresholds <= the word.  Returns ``(hist [B, K, 2, M] int64, moments [8, B,
    K])``: the planes x, y, xz, yz and their variances, mean = (n_plus - n_minus) / N and (1 - mean^2) / N with n_minus the
    shots of odd parity (s for x / y, s ^ t for xz / yz; outcome = 2 s + t); without a partner (M = 2) the xz / yz planes are NaN."""
    p = np.asarray(probs, dtype=np.float64)
    if p.ndim != 4 or p.shape[2] != 2 or p.shape[3] not in (2, 4):
        raise ValueError("need probs [B, K, 2, M] with M = 2 or 4")
    B, K, _, M = p.shape
    shots = np.broadcast_to(np.asarray(n_shots, dtype=np.int64), (K,))
    seed, first_item = int(seed) & (2 ** 64 - 1), int(first_item)
    if shots.min() < 1 or shots.max() >= 2 ** 31 or first_item < 0:
        raise ValueError("need 1 <= n_shots < 2^31 and first_item >= 0")
    c = np.cumsum(np.where(p < 0.0, 0.0, p), axis=3)                    # one addition per outcome, in outcome order
    if not np.all((c[..., -1] > 0.0) & np.isfinite(c[..., -1])):
        raise ValueError("a distribution whose clamped sum is not a positive finite number (a poisoned item) cannot be restated")
    thr = np.floor(c[..., :-1] / c[..., -1:] * 2.0 ** 32).astype(np.uint64)
    k0, k1 = (seed & 0xFFFFFFFF) ^ RPE_SIM_KEY_TAG, seed >> 32
    gid = first_item + np.arange(B, dtype=np.uint64)
    g0, g1 = gid & np.uint64(0xFFFFFFFF), gid >> np.uint64(32)
    hist = np.zeros((B, K, 2, M), dtype=np.int64)
    for j in range(K):
        N = int(shots[j])
        blocks = np.arange((N + 3) // 4, dtype=np.uint64)
        rows = max(1, (1 << 20) // len(blocks))                          # items per pass: about 2^20 blocks at a time
        for basis in range(2):
            for lo in range(0, B, rows):
                sl = slice(lo, lo + rows)
                words = _philox4x32_10(g0[sl, None], g1[sl, None], np.uint64(2 * j + basis), blocks[None, :], k0, k1)
                w = np.stack(np.broadcast_arrays(*words), axis=2).reshape(len(g0[sl]), -1)[:, :N]    # shot s = word s & 3 of block s >> 2
                outcome = (thr[sl, j, basis, None, :] <= w[:, :, None]).sum(axis=2)
                for o in range(M):
                    hist[sl, j, basis, o] = (outcome == o).sum(axis=1)
    Nf = shots.astype(np.float64)[None, :]
    moments = np.full((8, B, K), np.nan)
    for basis in range(2):
        h = hist[:, :, basis, :]
        odd = [h[..., 1] if M == 2 else h[..., 2] + h[..., 3]] + ([h[..., 1] + h[..., 2]] if M == 4 else [])
        for which, n_minus in enumerate(odd):
            n_plus = shots[None, :] - n_minus
            mean = (n_plus.astype(np.float64) - n_minus.astype(np.float64)) / Nf
            moments[2 * which + basis] = mean
            moments[4 + 2 * which + basis] = (1.0 - mean * mean) / Nf
    return hist, moments


# --------------------------------------------------------------------------------------------------
# fbx_rb_acquire (include/fbx.h) on the host: the distributions mirrored in numpy, the shots restated in integers.
# --------------------------------------------------------------------------------------------------
RB_ACQUIRE_KEY_TAG = 0x52424151          # "RBAQ": the shots of fbx_rb_acquire


def rb_measured_bases(n_qubits, mode):
    """The measured bases of ``fbx_rb_acquire`` in basis-index order, each a tuple of Pauli digits (1, 2, 3 = X, Y, Z), one per
    qubit: ``mode`` "standard" (Z on every qubit) or "unitarity" (all 3^n products, qubit 0 most significant)."""
    if mode not in ("standard", "unitarity"):
        raise ValueError("mode must be 'standard' or 'unitarity'")
    n = int(n_qubits)
    return [(3,) * n] if mode == "standard" else list(itertools.product((1, 2, 3), repeat=n))


def rb_pauli_assignment(n_qubits, mode):
    """``[(pauli index, basis index, outcome mask)]`` for the columns of ``expect_out`` in order: column c is read from the
    histogram of that ONE basis as the parity of the outcome bits in the mask (bit n - 1 - q of an outcome belongs to qubit q).
    Standard: the I/Z products in the order of ``randomized_benchmarking.z_product_indices``, all from basis 0.  Unitarity: Pauli
    indices 1 .. 4^n - 1; a Pauli is read from the basis with its own non-identity factors and Z on every idle qubit."""
    n = int(n_qubits)
    bases = rb_measured_bases(n, mode)
    if mode == "standard":
        paulis = [sum(3 << (2 * t) for t in range(n) if (z >> t) & 1) for z in range(1, 1 << n)]
    else:
        paulis = list(range(1, 4 ** n))
    out = []
    for k in paulis:
        digits = [(k >> (2 * (n - 1 - q))) & 3 for q in range(n)]
        mask = sum(1 << (n - 1 - q) for q in range(n) if digits[q])
        out.append((k, bases.index(tuple(d if d else 3 for d in digits)), mask))
    return out


def rb_outcome_distributions(vectors, n_qubits, mode, flips=None):
    """Step 3 of the contract of ``fbx_rb_acquire``: final Pauli vectors ``[..., 4^n]`` -> outcome distributions ``[..., NB, 2^n]``,
    p(o) = 2^-n sum_T (-1)^|o & T| v[P_T] per measured basis, then the confusion matrix of every qubit's ``flips`` (``[n, 2]``, or
    ``[E, n, 2]`` with E the first axis of ``vectors``; [q][0] = P(read 1 | 0), [q][1] = P(read 0 | 1)).  The arithmetic runs in the
    dtype of ``vectors`` when that is ``numpy.longdouble`` and in float64 otherwise; the sums are numpy's, so the device agrees
    within rounding, not bit for bit."""
    v = np.asarray(vectors)
    dt = np.longdouble if v.dtype == np.longdouble else np.float64
    v = v.astype(dt)
    n = int(n_qubits)
    D, M = 4 ** n, 2 ** n
    if v.shape[-1] != D:
        raise ValueError(f"vectors must be [..., {D}]")
    bases = rb_measured_bases(n, mode)
    out = np.empty(v.shape[:-1] + (len(bases), M), dtype=dt)
    for bi, digits in enumerate(bases):
        for o in range(M):
            acc = np.zeros(v.shape[:-1], dtype=dt)
            for T in range(M):
                idx = sum(digits[q] << (2 * (n - 1 - q)) for q in range(n) if (T >> (n - 1 - q)) & 1)
                term = v[..., idx]
                acc = acc - term if bin(o & T).count("1") & 1 else acc + term
            out[..., bi, o] = acc / dt(M)
    if flips is not None:
        f = np.asarray(flips).astype(dt)
        if f.ndim == 3:
            f = f.reshape((f.shape[0],) + (1,) * (out.ndim - 2) + f.shape[1:])          # [E, 1.., n, 2] against [E, .., NB, M]
        p = out.reshape(out.shape[:-1] + (2,) * n)
        for q in range(n):
            f0, f1 = f[..., q, 0], f[..., q, 1]
            f0, f1 = f0.reshape(f0.shape + (1,) * (n - 1)), f1.reshape(f1.shape + (1,) * (n - 1))      # over the other qubits' bits
            ax = p.ndim - n + q
            p0, p1 = np.take(p, 0, axis=ax), np.take(p, 1, axis=ax)
            p = np.stack([(1 - f0) * p0 + f1 * p1, f0 * p0 + (1 - f1) * p1], axis=ax)
        out = p.reshape(out.shape)
    return out


def restate_rb_counts(probs, shots, mode, seed, first_item=0):
    """Steps 4-5 of the contract of ``fbx_rb_acquire`` (include/fbx.h) restated on the host, in integers, from the distributions it
    reports: ``probs [E, Q, NB, M]`` (Q = S K sequences, M = 2 or 4).  Per (experiment, sequence q, basis): c = cumsum(max(p, 0)) in
    outcome order, thr_o = floor(c_o / c_last 2^32) for every outcome but the last; shot s reads word ``s & 3`` of the
    Philox4x32-10 block with counter (gid low, gid high, q NB + basis, s >> 2) and key (seed low ^ 0x52424151, seed high), gid =
    first_item + experiment; its outcome is the number of thresholds <= the word.  Returns ``(hist [E, Q, NB, M] int64,
    expectations [E, Q, C], std_errs [E, Q, C])``: column c from the basis and parity mask of ``rb_pauli_assignment``, mean =
    ((N - n_odd) - n_odd) / N and sqrt((1 - mean^2) / N)."""
    p = np.asarray(probs, dtype=np.float64)
    if p.ndim != 4 or p.shape[3] not in (2, 4):
        raise ValueError("need probs [E, Q, NB, M] with M = 2 or 4")
    E, Q, NB, M = p.shape
    n = {2: 1, 4: 2}[M]
    if NB != len(rb_measured_bases(n, mode)):
        raise ValueError("the number of bases does not match the mode")
    N, seed, first_item = int(shots), int(seed) & (2 ** 64 - 1), int(first_item)
    if not 1 <= N < 2 ** 31 or first_item < 0 or Q * NB >= 2 ** 32:
        raise ValueError("need 1 <= shots < 2^31, first_item >= 0 and Q NB < 2^32")
    c = np.cumsum(np.where(p < 0.0, 0.0, p), axis=3)                    # one addition per outcome, in outcome order
    if not np.all((c[..., -1] > 0.0) & np.isfinite(c[..., -1])):
        raise ValueError("a distribution whose clamped sum is not a positive finite number (a poisoned experiment) cannot be restated")
    thr = np.floor(c[..., :-1] / c[..., -1:] * 2.0 ** 32).astype(np.uint64).reshape(E, Q * NB, M - 1)
    k0, k1 = (seed & 0xFFFFFFFF) ^ RB_ACQUIRE_KEY_TAG, seed >> 32
    blocks = np.arange((N + 3) // 4, dtype=np.uint64)
    units = np.arange(Q * NB, dtype=np.uint64)
    rows = max(1, (1 << 20) // len(blocks))                              # units per pass: about 2^20 blocks at a time
    hist = np.zeros((E, Q * NB, M), dtype=np.int64)
    for e in range(E):
        gid = first_item + e
        for lo in range(0, Q * NB, rows):
            sl = slice(lo, lo + rows)
            words = _philox4x32_10(np.uint64(gid & 0xFFFFFFFF), np.uint64(gid >> 32), units[sl, None], blocks[None, :], k0, k1)
            w = np.stack(np.broadcast_arrays(*words), axis=2).reshape(len(units[sl]), -1)[:, :N]     # shot s = word s & 3 of block s >> 2
            outcome = (thr[e, sl, None, :] <= w[:, :, None]).sum(axis=2)
            for o in range(M):
                hist[e, sl, o] = (outcome == o).sum(axis=1)
    hist = hist.reshape(E, Q, NB, M)
    assign = rb_pauli_assignment(n, mode)
    expect, std_err = np.empty((E, Q, len(assign))), np.empty((E, Q, len(assign)))
    for col, (_, basis, mask) in enumerate(assign):
        n_odd = sum(hist[:, :, basis, o] for o in range(M) if bin(o & mask).count("1") & 1)
        mean = ((N - n_odd).astype(np.float64) - n_odd.astype(np.float64)) / float(N)
        expect[:, :, col] = mean
        std_err[:, :, col] = np.sqrt((1.0 - mean * mean) / float(N))
    return hist, expect, std_err


# --------------------------------------------------------------------------------------------------
# fbx_spec_acquire (include/fbx.h) on the host: the curve mirrored in numpy, the shots restated in integers.
# --------------------------------------------------------------------------------------------------
SPECTROSCOPY_KEY_TAG = 0x51535043        # "QSPC": the shots of fbx_spec_acquire


def spectroscopy_probabilities(x, params, flips=None):
    """Steps 1-3 of the contract of ``fbx_spec_acquire`` in numpy, operation for operation: ``x`` [K] (shared) or [B, K],
    ``params`` [B, 6] = (amplitude, decay_time, gauss_time, omega, offset, baseline), ``flips`` None, [2] or [B, 2] -> the
    probabilities of reading 1, [B, K], unclamped: env = exp(-(x / decay_time) - (x / gauss_time) (x / gauss_time)), p_true =
    baseline + (amplitude env) cos(omega x + offset), p_read = f0 (1 - p_true) + (1 - f1) p_true.  The exact expectation of the
    measured Pauli is ``1 - 2 * p_read``.  numpy rounds every operation on its own, as the device does; the two differ through
    their exp and cos only."""
    x = np.asarray(x, dtype=np.float64)
    params = np.atleast_2d(np.asarray(params, dtype=np.float64))
    if params.ndim != 2 or params.shape[1] != 6 or x.ndim not in (1, 2) or (x.ndim == 2 and x.shape[0] != params.shape[0]):
        raise ValueError("need params [B, 6] and x [K] or [B, K]")
    xs = x if x.ndim == 2 else x[None, :]
    amplitude, decay_time, gauss_time, omega, offset, baseline = (params[:, j:j + 1] for j in range(6))
    with np.errstate(all="ignore"):
        env = np.exp(-(xs / decay_time) - (xs / gauss_time) * (xs / gauss_time))
        arg = omega * xs + offset
        p = baseline + (amplitude * env) * np.cos(arg)
        if flips is not None:
            f = np.broadcast_to(np.asarray(flips, dtype=np.float64), (params.shape[0], 2))
            f0, f1 = f[:, 0:1], f[:, 1:2]
            p = f0 * (1 - p) + (1 - f1) * p
    return p


def restate_spectroscopy_counts(probabilities, shots, seed, first_item=0):
    """Steps 4-5 of the contract of ``fbx_spec_acquire`` restated on the host, in integers, from the probabilities it reports
    (``prob_out`` [B, K]): mu = 1 - 2 p, t = floor(clamp(0.5 mu + 0.5, 0, 1) 2^32), and shot s of point k counts +1 iff word
    ``s & 3`` of the Philox4x32-10 block with counter (gid low, gid high, k, s >> 2) and key (seed low ^ 0x51535043, seed high) is
    below t, gid = first_item + item -- ``restate_dfe_counts`` under this simulator's key tag.  Returns ``(expectations, std_errs,
    counts, k_plus)``, all [B, K]; ``shots`` None or 0: (mu, 0, 0, 0), nothing drawn."""
    mu = 1 - 2 * np.atleast_2d(np.asarray(probabilities, dtype=np.float64))
    if shots is None or int(shots) == 0:
        return mu, np.zeros_like(mu), np.zeros_like(mu), np.zeros(mu.shape, dtype=np.int64)
    e, counts, s, k_plus = restate_dfe_counts(mu, 1.0, shots, seed, first_item, key_tag=SPECTROSCOPY_KEY_TAG)
    return e, s, counts, k_plus
