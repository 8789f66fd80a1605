"""numpy model of fbx_bit_histogram / fbx_marginalize_confusion and the case builders shared by tests/test_readout_cpu.py (which
pins the model to the reference's outputs in tests/golden/readout_cases.npz) and the GPU tests (which compare the device with the
model on shapes of their own).  The model is np.bincount on the packed index and np.einsum for the marginal -- not the kernel's
algorithm."""
import itertools

import numpy as np

JOINT, WEIGHT = "joint", "weight"
GOLDEN_QUBITS = (0, 1, 2, 3)          # the 4 qubits of the readout goldens
GOLDEN_GROUP_SIZES = (1, 2, 3)
GOLDEN_ADDER_BITS = (1, 2, 3)
GOLDEN_GHZ_WIDTHS = (2, 3, 5)
EPS = 2.0 ** -52


def selected_bits(bits, cols=None, expected=None):
    """[B, n_shots, k] of 0/1: bit 0 of the selected columns, XORed with `expected`"""
    bits = np.asarray(bits)
    B, n_shots, n_cols = bits.shape
    if cols is None:
        sel = bits & 1
    else:
        c = np.asarray(cols)
        c = np.broadcast_to(c, (B, c.shape[-1]))
        sel = np.take_along_axis(bits, np.broadcast_to(c[:, None, :], (B, n_shots, c.shape[-1])).astype(np.int64), axis=2) & 1
    if expected is not None:
        e = np.asarray(expected)
        sel = sel ^ np.broadcast_to(e, (B, sel.shape[2]))[:, None, :].astype(sel.dtype)
    return sel.astype(np.int64)


def histogram(bits, cols=None, expected=None, kind=JOINT):
    """int64 [B, bins]: the model of fbx_bit_histogram"""
    sel = selected_bits(bits, cols, expected)
    B, _, k = sel.shape
    if kind == JOINT:
        idx = (sel << np.arange(k - 1, -1, -1)).sum(axis=2)
        bins = 1 << k
    else:
        idx = sel.sum(axis=2)
        bins = k + 1
    return np.stack([np.bincount(idx[b], minlength=bins) for b in range(B)]).astype(np.int64)


def marginal(mats, n, keep):
    """[B, 2^k, 2^k]: the model of fbx_marginalize_confusion (keep = ascending positions, 0 = most significant)"""
    mats = np.asarray(mats, dtype=np.float64)
    B = mats.shape[0]
    t = mats.reshape([B] + [2] * (2 * n))
    keep = [int(p) for p in keep]
    out = np.einsum(t, [0] + list(range(1, 2 * n + 1)), [0] + [1 + p for p in keep] + [1 + n + p for p in keep])
    return out.reshape(B, 1 << len(keep), 1 << len(keep)) / float(1 << (n - len(keep)))


def marginal_bound(mats, n, keep):
    """4^(n-k) 2^-52 S per output element, S = the sum of the absolute values entering it: two differently ordered sums"""
    return 4.0 ** (n - len(keep)) * EPS * marginal(np.abs(mats), n, keep) * float(1 << (n - len(keep)))


def adder_expected(n_bits):
    """[4^n, n + 1]: the answers in the order of the reference's loops, built the slow way"""
    rows = []
    for bits in itertools.product((0, 1), repeat=2 * n_bits):
        a = int("".join(map(str, bits[:n_bits])), 2)
        b = int("".join(map(str, bits[n_bits:])), 2)
        rows.append([int(ch) for ch in format(a + b, "0%db" % (n_bits + 1))])
    return np.asarray(rows, dtype=np.uint8)


def random_confusion(rng, G, g, fidelity=0.9):
    """[G, 2^g, 2^g] row-stochastic matrices with a heavy diagonal"""
    N = 1 << g
    c = rng.random((G, N, N)) * (1.0 - fidelity) / N
    c[:, np.arange(N), np.arange(N)] += fidelity
    return c / c.sum(axis=2, keepdims=True)


def sample_rows(rng, confusion, shots):
    """[G, 2^g, shots, g] uint8 drawn from the rows of `confusion`"""
    G, N, _ = confusion.shape
    g = N.bit_length() - 1
    out = np.empty((G, N, shots, g), dtype=np.uint8)
    for grp in range(G):
        for r in range(N):
            idx = rng.choice(N, size=shots, p=confusion[grp, r])
            out[grp, r] = (idx[:, None] >> np.arange(g - 1, -1, -1)) & 1
    return out


def random_bits(rng, B, n_shots, n_cols, high_bits=False):
    """[B, n_shots, n_cols] uint8; with high_bits the bytes hold 0..3, of which only bit 0 counts"""
    return rng.integers(0, 4 if high_bits else 2, size=(B, n_shots, n_cols), dtype=np.uint8)


def marginal_cases(gold, n):
    """(all_qubits, subset, keep positions, the reference's result) of every stored marginal of the n-qubit matrix"""
    for all_q, padded, flat in zip(gold[f"marginal{n}_all_qubits"], gold[f"marginal{n}_subsets"], gold[f"marginal{n}_results"]):
        subset = [int(q) for q in padded if q >= 0]
        keep = sorted(list(all_q).index(q) for q in subset)
        yield list(all_q), subset, keep, flat[:4 ** len(subset)].reshape(1 << len(subset), 1 << len(subset))
