"""fbx_clifford_from_index / fbx_rb_sequences / fbx_rb_simulate on the GPU, and the Python surface above them.

The reference delegates all of this to quilc, so there are no fixtures: the truth is the host mirror fbx.clifford (pinned to dense
unitaries by tests/test_clifford_cpu.py), group theory, and the dense d^2 x d^2 numpy products written here.

Rounding bounds (u = 2^-53).  A signed permutation is exact.  A noise step computes every component as ONE chain of D = d^2 fused
multiply-adds; by the standard dot-product bound (Higham, Accuracy and Stability, 3.1) |fl(a.x) - a.x| <= gamma_D |a|.|x| with
gamma_D = D u / (1 - D u) <= (D + 1) u, in any summation order, so it also covers numpy's products.  ``dense_reference`` therefore
carries, next to the numpy result v_k, the componentwise bound  E_(k+1) = (1 + gamma_D) |L| E_k + gamma_D |L| |P v_k|,  E_0 = 0 --
K steps give at most K (D + 1) u times the norms involved -- and a test allows 2 E_K: one E for the device, one for numpy.
For depolarising noise diag(1, p, .., p) every product but one of a chain is an exact zero, so a step is one rounded multiplication:
after K steps the result is within ((1 + u)^K - 1) <= K (1 + K u) u of the exact p^K prep_k, which is evaluated in rationals."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from fbx import clifford as cl
from fbx import randomized_benchmarking as rb

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
U32, U8P, I64P, F64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.POINTER(C.c_double)
NONE = 0xFFFFFFFF
BATCHES = (1, 63, 64, 65, 257)              # simulator
SEQUENCE_BATCHES = (1, 3, 64, 65, 257)     # generator: sequence b must not depend on B


def offsets_of(lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    return off


def sequences_host(gpu, n, lengths, seed, interleaved=NONE, self_inverting=True):
    off = offsets_of(lengths)
    elems = np.full(int(off[-1]), 0xDEADBEEF, dtype=np.uint32)
    ids = np.full(int(off[-1]), 77, dtype=np.uint8)
    gpu.check(gpu.lib().fbx_rb_sequences(n, len(lengths), off.ctypes.data_as(I64P), seed, interleaved, int(self_inverting),
                                         elems.ctypes.data_as(U32), ids.ctypes.data_as(U8P)))
    return off, elems, ids


def sequences_dev(gpu, n, lengths, seed, interleaved=NONE, self_inverting=True):
    off = offsets_of(lengths)
    total = int(off[-1])
    d_off, d_e, d_i = gpu.DeviceBuffer.from_array(off), gpu.DeviceBuffer(4 * total + 16), gpu.DeviceBuffer(total + 16)
    gpu.check(gpu.lib().fbx_rb_sequences_dev(n, len(lengths), d_off.ptr, seed, interleaved, int(self_inverting), d_e.ptr, d_i.ptr))
    gpu.synchronize()
    out = off, d_e.to_array(np.uint32, (total,)), d_i.to_array(np.uint8, (total,))
    for b in (d_off, d_e, d_i):
        b.free()
    return out


def simulate_dev(gpu, n, off, elems, ids, ptms, prep):
    D = 4 ** n
    B = len(off) - 1
    bufs = [gpu.DeviceBuffer.from_array(off), gpu.DeviceBuffer.from_array(np.append(elems, np.uint32(0))),
            None if ids is None else gpu.DeviceBuffer.from_array(np.append(ids, np.uint8(0))),
            gpu.DeviceBuffer.from_array(np.ascontiguousarray(ptms, dtype=np.float64)),
            None if prep is None else gpu.DeviceBuffer.from_array(np.ascontiguousarray(prep, dtype=np.float64)), gpu.DeviceBuffer(8 * B * D + 16)]
    p = [None if b is None else b.ptr for b in bufs]
    gpu.check(gpu.lib().fbx_rb_simulate_dev(n, B, p[0], p[1], p[2], len(ptms), p[3], p[4], p[5]))
    gpu.synchronize()
    out = bufs[5].to_array(np.float64, (B, D))
    for b in bufs:
        if b is not None:
            b.free()
    return out


def compose_all(n, seq):
    total = cl.identity(n)
    for e in seq:
        total = cl._compose(n, int(e), total)
    return total


def default_prep(n):
    p = np.zeros(4 ** n)
    p[[0] + rb.z_product_indices(n).tolist()] = 1.0
    return p


def some_prep(n):
    """a non-trivial Pauli vector: every component different, none zero, signs mixed"""
    k = np.arange(4 ** n)
    p = (0.9 - 0.05 * k) * np.where(k % 3 == 1, -1.0, 1.0) / (1.0 + k)
    p[0] = 1.0
    return p


_PTM_CACHE = {}


def ptm_of(n, e):
    key = (n, int(e))
    if key not in _PTM_CACHE:
        _PTM_CACHE[key] = cl.to_ptm(int(e), n)
    return _PTM_CACHE[key]


def dense_reference(n, off, elems, ids, ptms, prep):
    """(out[B, D], E[B, D]): the dense numpy products and the componentwise rounding bound of the module docstring"""
    D = 4 ** n
    gam = D * U / (1 - D * U)
    absl = np.abs(ptms)
    out, err = np.empty((len(off) - 1, D)), np.empty((len(off) - 1, D))
    for b in range(len(off) - 1):
        v, e = np.array(prep, dtype=np.float64), np.zeros(D)
        for i in range(off[b], off[b + 1]):
            g = 0 if ids is None else int(ids[i])
            pv = ptm_of(n, elems[i]) @ v
            pe = np.abs(ptm_of(n, elems[i])) @ e
            e = (1 + gam) * (absl[g] @ pe) + gam * (absl[g] @ np.abs(pv))
            v = ptms[g] @ pv
        out[b], err[b] = v, e
    return out, err


def random_cptp_ptms(n, count, seed):
    from fbx.operator_tools import random_operators as ro, superoperator_transformations as st
    kraus = ro.random_kraus_batch(2 ** n, 3, count, seed=seed)
    ptms = np.array([np.real(st.kraus2pauli_liouville(list(k))) for k in kraus])
    assert np.abs(ptms[:, 0, 0] - 1).max() < 1e-12 and np.abs(ptms[:, 0, 1:]).max() < 1e-12       # trace preserving ...
    assert np.abs(ptms[:, 1:, 0]).max() > 1e-3                                                     # ... and not unital
    return ptms


def chi2_quantile(dof, tail):
    try:
        from scipy import stats
        return float(stats.chi2.ppf(1.0 - tail, dof))
    except ImportError:                                    # Wilson-Hilferty, z = the normal quantile of 1 - 1e-6
        assert tail == 1e-6
        z = 4.753424308822899
        return dof * (1 - 2 / (9 * dof) + z * np.sqrt(2 / (9 * dof))) ** 3


# ------------------------------------------------------------------------------------------------ 8. from_index
@pytest.mark.parametrize("n", [1, 2])
def test_from_index_matches_the_host_mirror(gpu, n):
    idx = np.arange(cl.ORDER[n], dtype=np.uint32)
    out = np.zeros_like(idx)
    gpu.check(gpu.lib().fbx_clifford_from_index(n, idx.size, idx.ctypes.data_as(U32), out.ctypes.data_as(U32)))
    assert (out == cl.group(n)).all()
    d_i, d_o = gpu.DeviceBuffer.from_array(np.append(idx, np.uint32(cl.ORDER[n]))), gpu.DeviceBuffer(4 * idx.size + 4)
    gpu.check(gpu.lib().fbx_clifford_from_index_dev(n, idx.size + 1, d_i.ptr, d_o.ptr))
    gpu.synchronize()
    dev = d_o.to_array(np.uint32, (idx.size + 1,))
    assert (dev[:-1] == out).all() and dev[-1] == NONE           # the _dev form marks an index past the group
    with pytest.raises(ValueError, match="not below the group's order"):
        bad = np.array([cl.ORDER[n]], dtype=np.uint32)
        gpu.check(gpu.lib().fbx_clifford_from_index(n, 1, bad.ctypes.data_as(U32), out.ctypes.data_as(U32)))


def test_native_gates_agree_with_kraus2pauli_liouville(gpu):
    from fbx.operator_tools import superoperator_transformations as st
    cz = np.diag([1, 1, 1, -1]).astype(complex)
    rx = (np.eye(2) - 1j * np.array([[0, 1], [1, 0]])) / np.sqrt(2)
    rx_on_1 = np.kron(np.eye(2), rx)
    for key, unitary in ((("CZ", (0, 1)), cz), (("RX(pi/2)", (1,)), rx_on_1)):
        word = cl.gate_word(*key, n=2)
        want = np.real(st.kraus2pauli_liouville([unitary]))
        assert np.abs(want - np.round(want)).max() < 1e-12
        assert (np.round(want) == cl.to_ptm(word, 2)).all()
    one = cl.gate_word("RX(pi/2)", (0,))
    assert (np.round(np.real(st.kraus2pauli_liouville([rx]))) == cl.to_ptm(one, 1)).all()


# ------------------------------------------------------------------------------------------------ 9. sequences
def ragged(B):
    return [(2, 3, 8)[b % 3] for b in range(B)]


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("interleaved", [False, True])
def test_self_inverting_sequences_compose_to_the_identity(gpu, n, interleaved):
    g = int(cl.group(n)[17]) if interleaved else NONE
    # interleaved: even lengths too, where the inverse directly follows a random element
    lengths = ragged(70) if not interleaved else [(2, 3, 8, 5, 9, 1)[b % 6] for b in range(72)]
    off, elems, ids = sequences_host(gpu, n, lengths, 1234, g, True)
    assert all(cl.is_valid(e, n) for e in elems)
    for b, L in enumerate(lengths):
        seq = elems[off[b]:off[b + 1]]
        assert compose_all(n, seq) == cl.identity(n)
        want_ids = [1 if interleaved and i % 2 == 1 and i < L - 1 else 0 for i in range(L)]
        assert ids[off[b]:off[b + 1]].tolist() == want_ids
        if interleaved:
            assert (seq[1:L - 1:2] == g).all()
    # the draws at the even positions of an interleaved sequence are those of the plain sequence of the same (seed, b)
    if interleaved:
        _, plain, _ = sequences_host(gpu, n, [L // 2 for L in lengths], 1234, NONE, False)
        assert (plain == np.concatenate([elems[off[b]:off[b + 1] - 1:2] for b in range(len(lengths))])).all()
    # not all sequences are the same, and their elements vary
    assert len(set(elems.tolist())) > (10 if n == 1 else 100)


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("interleaved", [False, True])
def test_non_self_inverting_is_the_longer_sequence_without_its_inverse(gpu, n, interleaved):
    g = int(cl.group(n)[5]) if interleaved else NONE
    lengths = ragged(65)
    off, elems, ids = sequences_host(gpu, n, lengths, 99, g, False)
    off1, elems1, ids1 = sequences_host(gpu, n, [L + 1 for L in lengths], 99, g, True)
    for b in range(len(lengths)):
        assert (elems[off[b]:off[b + 1]] == elems1[off1[b]:off1[b + 1] - 1]).all()
        assert (ids[off[b]:off[b + 1]] == ids1[off1[b]:off1[b + 1] - 1]).all()


@pytest.mark.parametrize("n", [1, 2])
def test_a_sequence_depends_on_seed_and_index_only(gpu, n):
    runs = {B: sequences_host(gpu, n, ragged(B), 4242) for B in SEQUENCE_BATCHES}
    big_off, big, _ = runs[257]
    for B in SEQUENCE_BATCHES:
        off, elems, _ = runs[B]
        assert (elems == big[:off[-1]]).all() and (off == big_off[:B + 1]).all()
    _, other, _ = sequences_host(gpu, n, ragged(257), 4243)
    assert (other != big).mean() > 0.5
    # the _dev form is the host form
    for g, inv in ((NONE, True), (int(cl.group(n)[3]), True), (NONE, False)):
        want, got = sequences_host(gpu, n, ragged(257), 7, g, inv), sequences_dev(gpu, n, ragged(257), 7, g, inv)
        assert (want[1] == got[1]).all() and (want[2] == got[2]).all()


def test_first_elements_are_uniform(gpu):
    B = 24 * 4096
    _, elems, _ = sequences_host(gpu, 1, [1] * B, 20260101, NONE, False)
    index_of = {int(e): i for i, e in enumerate(cl.group(1))}
    counts = np.bincount([index_of[int(e)] for e in elems], minlength=24)
    chi2 = float(((counts - 4096.0) ** 2 / 4096.0).sum())
    bound = chi2_quantile(23, 1e-6)
    print(f"chi2 = {chi2:.3f}, 1 - 1e-6 quantile of chi2_23 = {bound:.3f}")
    assert 60.0 < bound < 75.0
    assert chi2 < bound


# ------------------------------------------------------------------------------------------------ 10. noiseless
def mixed_lengths(B):
    return [(0, 1, 2, 7, 3, 12)[b % 6] for b in range(B)]


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("own_prep", [False, True])
def test_noiseless_self_inverting_sequences_return_prep_exactly(gpu, n, own_prep):
    prep = some_prep(n) if own_prep else None
    want = some_prep(n) if own_prep else default_prep(n)
    ident = np.eye(4 ** n)[None]
    for B in BATCHES:
        for lengths in ([0] * B, [1] * B, [2] * B, mixed_lengths(B)):
            off, elems, _ = sequences_host(gpu, n, lengths, 31 + B)
            out = rb.simulate_rb_sequences_batch(n, off, elems, ident, prep=prep)
            assert out.shape == (B, 4 ** n) and (out == want[None, :]).all()
    # without the inverse the vector is a signed permutation of prep, and not prep for most sequences
    off, elems, _ = sequences_host(gpu, n, mixed_lengths(257), 5, NONE, False)
    out = rb.simulate_rb_sequences_batch(n, off, elems, ident, prep=prep)
    ref, _ = dense_reference(n, off, elems, None, ident, want)
    assert (out == ref).all() and (out != want[None, :]).any(axis=1).sum() > 100


# ------------------------------------------------------------------------------------------------ 11. depolarising
def depolarising(n, p):
    return np.diag([1.0] + [p] * (4 ** n - 1))


def assert_power_law(out, prep, factors_of_length, lengths):
    for b, L in enumerate(lengths):
        K, exact = factors_of_length(L)
        assert out[b, 0] == prep[0]
        rel = Fraction(K) * Fraction(U) * (1 + Fraction(K) * Fraction(U))               # (1 + u)^K - 1 <= K u (1 + K u)
        for k in range(1, out.shape[1]):
            want = exact * Fraction(float(prep[k]))
            assert abs(Fraction(float(out[b, k])) - want) <= rel * abs(want), (b, k, L)


@pytest.mark.parametrize("n", [1, 2])
def test_depolarising_noise_gives_the_power_law(gpu, n):
    p, pg = 0.97, 0.91
    prep = some_prep(n)
    lengths = [(1, 2, 3, 8, 0)[b % 5] for b in range(65)]
    off, elems, _ = sequences_host(gpu, n, lengths, 77)
    out = rb.simulate_rb_sequences_batch(n, off, elems, depolarising(n, p), prep=prep)
    assert_power_law(out, prep, lambda L: (L, Fraction(p) ** L), lengths)
    # interleaved: L = 2 m + 1 elements see (p p_g)^m p, 2 m + 1 rounded multiplications
    lengths = [(1, 3, 5, 9)[b % 4] for b in range(65)]
    off, elems, ids = sequences_host(gpu, n, lengths, 78, int(cl.group(n)[9]), True)
    out = rb.simulate_rb_sequences_batch(n, off, elems, np.array([depolarising(n, p), depolarising(n, pg)]), ids, prep)
    assert_power_law(out, prep, lambda L: (L, Fraction(p) ** ((L + 1) // 2) * Fraction(pg) ** (L // 2)), lengths)


# ------------------------------------------------------------------------------------------------ 12. exhaustive twirl
def test_exhaustive_one_qubit_twirl(gpu):
    g = [int(e) for e in cl.group(1)]
    lam = random_cptp_ptms(1, 1, seed=2024)[0]
    seqs = np.array([[a, b, cl.inverse(cl.compose(b, a, 1), 1)] for a in g for b in g], dtype=np.uint32)
    off = offsets_of([3] * len(seqs))
    prep = np.array([1.0, 0.3, -0.5, 0.6])
    out = rb.simulate_rb_sequences_batch(1, off, seqs.ravel(), lam, prep=prep)
    assert len(seqs) == 576 and len(np.unique(out.round(12), axis=0)) > 50            # the elements matter
    p = (np.trace(lam) - 1) / 3
    r0 = prep.copy()
    r0[0] = 0.0
    want = lam @ (np.array([1.0, 0, 0, 0]) + p * p * r0)
    _, err = dense_reference(1, off, seqs.ravel(), None, lam[None], prep)
    norm = np.abs(lam).sum(axis=1).max() * np.abs(prep).max()
    # device rounding (mean of E), numpy's mean of 576 terms (gamma_577 max|out|), and the ~10 operations of the formula above
    bound = err.mean(axis=0).max() + 577 * U * np.abs(out).max() + 16 * U * norm
    got = np.abs(out.mean(axis=0) - want).max()
    print(f"twirl mean: deviation {got:.3e}, bound {bound:.3e}")
    assert got <= bound


# ------------------------------------------------------------------------------------------------ 13. dense restatement
@pytest.fixture(scope="module")
def dense_case(gpu):
    n, B = 2, 257
    rs = np.random.RandomState(8)
    lengths = [b % 8 for b in range(B)]
    off, elems, _ = sequences_host(gpu, n, lengths, 555, NONE, False)
    ids = rs.randint(0, 3, size=elems.size).astype(np.uint8)
    ptms = random_cptp_ptms(n, 3, seed=99)
    prep = some_prep(n)
    ref, err = dense_reference(n, off, elems, ids, ptms, prep)
    return n, off, elems, ids, ptms, prep, ref, err


def test_dense_restatement_two_qubits(gpu, dense_case):
    n, off, elems, ids, ptms, prep, ref, err = dense_case
    out = rb.simulate_rb_sequences_batch(n, off, elems, ptms, ids, prep)
    dev = np.abs(out - ref)
    print(f"dense n = 2: max deviation {dev.max():.3e}, max bound 2 E = {2 * err.max():.3e}, "
          f"max ratio {np.max(dev[err > 0] / (2 * err[err > 0])):.3f}")
    assert (dev <= 2 * err).all()
    assert (out[::8] == prep[None, :]).all()                       # length 0
    assert (simulate_dev(gpu, n, off, elems, ids, ptms, prep) == out).all()
    # each sequence alone gives the same bits as in the batch
    for b in (1, 7, 64, 200, 256):
        one = rb.simulate_rb_sequences_batch(n, off[b:b + 2] - off[b], elems[off[b]:off[b + 1]], ptms, ids[off[b]:off[b + 1]], prep)
        assert (one[0] == out[b]).all()


def test_sixteen_noise_ptms_two_qubits(gpu):
    """the largest launch there is: n = 2 with G = 16 is exactly 64 KB of dynamic LDS; id 15 is used"""
    n, B = 2, 65
    rs = np.random.RandomState(16)
    off, elems, _ = sequences_host(gpu, n, [b % 8 for b in range(B)], 1616, NONE, False)
    ids = rs.randint(0, 16, size=elems.size).astype(np.uint8)
    ids[::5] = 15
    ptms = random_cptp_ptms(n, 16, seed=1616)
    prep = some_prep(n)
    ref, err = dense_reference(n, off, elems, ids, ptms, prep)
    out = rb.simulate_rb_sequences_batch(n, off, elems, ptms, ids, prep)
    assert (ids == 15).sum() > 40 and len(set(ids.tolist())) == 16
    assert (np.abs(out - ref) <= 2 * err).all()
    assert np.abs(out[1::8] - ref[1::8]).max() < 1e-14 and np.abs(ref[1::8, 1:]).max() > 1e-3        # not trivially zero
    assert (simulate_dev(gpu, n, off, elems, ids, ptms, prep) == out).all()


# ------------------------------------------------------------------------------------------------ 14. isolation and errors
def test_a_nan_stays_in_the_sequences_that_use_its_ptm(gpu, dense_case):
    n, off, elems, ids, ptms, prep, _, _ = dense_case
    clean = rb.simulate_rb_sequences_batch(n, off, elems, ptms, ids, prep)
    dirty_ptms = ptms.copy()
    dirty_ptms[1, 5, 7] = np.nan
    dirty = rb.simulate_rb_sequences_batch(n, off, elems, dirty_ptms, ids, prep)
    uses = np.array([(ids[off[b]:off[b + 1]] == 1).any() for b in range(len(off) - 1)])
    assert 50 < uses.sum() < len(uses) - 50
    assert (np.isnan(dirty).any(axis=1) == uses).all()
    assert (dirty[~uses] == clean[~uses]).all()
    # a sequence that goes on after the damaged step is NaN in every component
    early = np.array([(ids[off[b]:max(off[b], off[b + 1] - 1)] == 1).any() for b in range(len(off) - 1)])
    assert early.sum() > 20 and np.isnan(dirty[early]).all()


def test_bad_elements_and_noise_ids(gpu, dense_case):
    n, off, elems, ids, ptms, prep, _, _ = dense_case
    clean = rb.simulate_rb_sequences_batch(n, off, elems, ptms, ids, prep)
    b_word, b_id = 100, 203                                       # lengths 4 and 3
    bad_elems, bad_ids = elems.copy(), ids.copy()
    bad_elems[off[b_word] + 1] = cl.identity(2) ^ (5 << 10)       # X_1 -> X_0: does not commute with the image of Z_0
    bad_ids[off[b_id] + 2] = 3
    assert not cl.is_valid(int(bad_elems[off[b_word] + 1]), 2)
    with pytest.raises(ValueError, match="not a valid Clifford element"):
        rb.simulate_rb_sequences_batch(n, off, bad_elems, ptms, ids, prep)
    with pytest.raises(ValueError, match="noise id is not below G"):
        rb.simulate_rb_sequences_batch(n, off, elems, ptms, bad_ids, prep)
    out = simulate_dev(gpu, n, off, bad_elems, bad_ids, ptms, prep)
    hit = np.zeros(len(off) - 1, dtype=bool)
    hit[[b_word, b_id]] = True
    assert np.isnan(out[hit]).all() and (out[~hit] == clean[~hit]).all()
    for w in (NONE, 0, 1 << 20):                                  # words with stray bits or identity images
        bad_elems[off[b_word] + 1] = w
        out = simulate_dev(gpu, n, off, bad_elems, ids, ptms, prep)
        assert np.isnan(out[b_word]).all() and (np.delete(out, b_word, 0) == np.delete(clean, b_word, 0)).all()


def test_argument_errors(gpu):
    lib = gpu.lib()
    off = offsets_of([2, 2])
    elems = np.full(4, cl.identity(1), dtype=np.uint32)
    ids = np.zeros(4, dtype=np.uint8)
    out = np.zeros((2, 4))
    ptms = np.ascontiguousarray(np.tile(np.eye(4), (17, 1, 1)))
    args = (off.ctypes.data_as(I64P), elems.ctypes.data_as(U32), ids.ctypes.data_as(U8P))

    def sim(n=1, G=1, p=ptms.ctypes.data_as(F64P), o=out.ctypes.data_as(F64P), a=args):
        gpu.check(lib.fbx_rb_simulate(n, 2, a[0], a[1], a[2], G, p, None, o))

    sim()
    assert (out == [1, 0, 0, 1]).all()
    for G in (0, 17):
        with pytest.raises(ValueError, match=r"G must be 1\.\.16"):
            sim(G=G)
    sim(G=16)
    with pytest.raises(gpu.FbxError, match="covers 1 and 2 qubits") as exc:
        sim(n=3)
    assert exc.value.code == gpu.FBX_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="n_qubits must be 1 or 2"):
        sim(n=0)
    with pytest.raises(ValueError, match="NULL offsets / out"):
        sim(o=None)
    with pytest.raises(ValueError, match="NULL noise_ptms"):
        sim(p=None)
    with pytest.raises(ValueError, match="NULL elems"):
        sim(a=(args[0], None, args[2]))
    d_off, d_ptm, d_out = gpu.DeviceBuffer.from_array(off), gpu.DeviceBuffer.from_array(ptms), gpu.DeviceBuffer(out.nbytes)
    with pytest.raises(ValueError, match="NULL elems"):          # the _dev form as well: nothing is launched
        gpu.check(lib.fbx_rb_simulate_dev(1, 2, d_off.ptr, None, None, 1, d_ptm.ptr, None, d_out.ptr))
    for b in (d_off, d_ptm, d_out):
        b.free()
    bad_off = np.array([0, 3, 2], dtype=np.int64)
    with pytest.raises(ValueError, match="offsets must start at 0 and never decrease"):
        sim(a=(bad_off.ctypes.data_as(I64P), args[1], args[2]))

    def seq(n=1, inter=NONE, e=elems.ctypes.data_as(U32), o=args[0]):
        gpu.check(lib.fbx_rb_sequences(n, 2, o, 1, inter, 1, e, None))

    seq()                                                         # noise_id_out may be NULL
    assert compose_all(1, elems[:2]) == cl.identity(1)
    with pytest.raises(gpu.FbxError, match="covers 1 and 2 qubits") as exc:
        seq(n=3)
    assert exc.value.code == gpu.FBX_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="NULL offsets / elems_out"):
        seq(e=None)
    with pytest.raises(ValueError, match="neither a valid element word"):
        seq(inter=0x21)                                           # X -> X, Z -> X
    with pytest.raises(ValueError, match="offsets must start at 0"):
        seq(o=bad_off.ctypes.data_as(I64P))
    with pytest.raises(gpu.FbxError) as exc:
        gpu.check(lib.fbx_clifford_from_index(3, 1, elems.ctypes.data_as(U32), elems.ctypes.data_as(U32)))
    assert exc.value.code == gpu.FBX_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="NULL idx / elems_out"):
        gpu.check(lib.fbx_clifford_from_index(1, 1, elems.ctypes.data_as(U32), None))
    # B = 0 is fine everywhere
    gpu.check(lib.fbx_rb_simulate(1, 0, None, None, None, 1, ptms.ctypes.data_as(F64P), None, None))
    gpu.check(lib.fbx_rb_sequences(1, 0, None, 1, NONE, 1, None, None))


# ------------------------------------------------------------------------------------------------ Python surface
def test_reference_named_generators(gpu):
    with pytest.raises(ValueError, match="Sequence depth must be at least 2 for rb sequences, or at least 1 for unitarity sequences."):
        rb.generate_rb_sequence(None, [0], 1)
    with pytest.raises(ValueError, match="No RB gateset for more than two qubits."):
        rb.generate_rb_sequence(None, [0, 1, 2], 3)
    for qubits in ([4], [7, 2]):
        n = len(qubits)
        seq = rb.generate_rb_sequence(None, qubits, 6, random_seed=3)
        assert seq.dtype == np.uint32 and seq.shape == (6,) and compose_all(n, seq) == cl.identity(n)
        assert (seq == rb.generate_rb_sequence("ignored", qubits, 6, random_seed=3)).all()
        g = int(cl.group(n)[7])
        irb = rb.generate_rb_sequence(None, qubits, 6, interleaved_gate=g, random_seed=3)
        assert irb.shape == (11,) and (irb[1:-1:2] == g).all() and (irb[0:-1:2] == seq[:-1]).all()
        assert compose_all(n, irb) == cl.identity(n)
        # the seed advances by one per depth; without self-inversion: depth + 1 Cliffords, no interleaved gate, inverse stripped
        depths = [2, 5, 5]
        expt = rb.generate_rb_experiment_sequences(None, qubits, depths, random_seed=10)
        for i, d in enumerate(depths):
            assert (expt[i] == rb.generate_rb_sequence(None, qubits, d, random_seed=11 + i)).all()
        assert (expt[1] != expt[2]).any()
        open_expt = rb.generate_rb_experiment_sequences(None, qubits, depths, interleaved_gate=g, random_seed=10, use_self_inv_seqs=False)
        for i, d in enumerate(depths):
            assert (open_expt[i] == rb.generate_rb_sequence(None, qubits, d + 1, random_seed=11 + i)[:-1]).all()
    assert len(rb.generate_rb_sequence(None, [0], 4)) == 4                       # no seed: fresh entropy
    with pytest.raises(ValueError, match="not a valid 1-qubit Clifford element word"):
        rb.generate_rb_sequence(None, [0], 4, interleaved_gate=0x21)


# ------------------------------------------------------------------------------------------------ 15. end to end
@pytest.mark.parametrize("n", [1, 2])
def test_sequences_to_fit_recovers_the_decay_of_the_noise(gpu, n):
    from fbx import synthetic
    from fbx.analysis import fitting
    p, dim = 0.96, 2 ** n
    lam = depolarising(n, p)
    assert abs(p - (np.trace(lam) - 1) / (dim * dim - 1)) <= dim * dim * U        # the decay the channel predicts (a sum of d^2 terms)
    depths = [2, 4, 8, 16, 32, 64, 128]
    e, se = rb.simulate_rb_experiment_batch(n, depths, 3, lam, seed=12)
    assert e.shape == se.shape == (1, len(depths), dim - 1)
    e2, _ = synthetic.rb_sequence_data(n, depths, lam, num_sequences=3, seed=12)
    assert (e == e2).all()
    assert np.abs(e - (p ** np.array(depths))[None, :, None]).max() < 200 * U      # every sequence of a depth gives p^depth
    # for dim > 2 the fit adds the covariance of the I/Z observables over num_shots; exact expectations are its limit of many shots
    batch = rb.fit_rb_results_batch(depths, e, se, num_shots=None if n == 1 else 10 ** 12)
    decay = float(batch.value("decay")[0])
    print(f"n = {n}: fitted decay - p = {decay - p:.3e} (xtol {fitting.DEFAULT_XTOL:g}), status {batch.status[0]}, iters {batch.iters[0]}")
    assert batch.success[0]
    assert abs(decay - p) <= fitting.DEFAULT_XTOL * p
    # the gate error of the fit is the average gate infidelity of the channel, 1 - (d F_pro + 1) / (d + 1), F_pro = tr(PTM) / d^2
    f_pro = np.trace(lam) / dim ** 2
    want = 1 - (dim * f_pro + 1) / (dim + 1)
    assert abs(rb.rb_decay_to_gate_error(decay, dim) - want) <= fitting.DEFAULT_XTOL * p * (dim - 1) / dim + 8 * U


def test_interleaved_experiment_and_shots(gpu):
    p, pg = 0.97, 0.9
    ptms = np.array([depolarising(1, p), depolarising(1, pg)])
    depths = [2, 3, 5, 9]
    g = int(cl.group(1)[13])
    e, se = rb.simulate_rb_experiment_batch(1, depths, 4, np.array([ptms, ptms]), interleaved_gate=g, seed=5)
    m = np.array(depths) - 1
    assert e.shape == (2, 4, 1) and np.abs(e[:, :, 0] - ((p * pg) ** m * p)[None, :]).max() < 100 * U
    assert np.abs(se).max() < 100 * U
    es, ses = rb.simulate_rb_experiment_batch(1, depths, 4, ptms, interleaved_gate=g, seed=5, shots=500)
    assert es.shape == (1, 4, 1) and (ses >= 0).all() and ses.max() > 0 and np.abs(es - e[:1]).max() < 0.2
    # depolarising noise gives every sequence the same exact expectation, so another seed differs through the shot noise alone
    es2, _ = rb.simulate_rb_experiment_batch(1, depths, 4, ptms, interleaved_gate=g, seed=6, shots=500)
    assert (es2 != es).any()
    assert (rb.simulate_rb_experiment_batch(1, depths, 4, ptms, interleaved_gate=g, seed=5, shots=500)[0] == es).all()
    with pytest.raises(ValueError, match="two noise PTMs"):
        rb.simulate_rb_experiment_batch(1, depths, 4, ptms[0], interleaved_gate=g)
