"""fbx_convert, fbx_convert_general and fbx_apply_choi on inputs with known answers (tests/convert_cases.py): gaussian integers,
on which every route without the |C| step is exact in float64 and is held to np.array_equal against the oracle; Choi matrices
with a prescribed spectrum (both signs, degenerate values, an exact zero, values on either side of the reference's cut at
1e-9) for the |C| step on the way into chi; batches past every grid cap and every host-side chunk; non-finite items.

Which test reaches which kernel of csrc/fbx_convert.hip (every one against the oracle or an exact answer):
  convert_kernel<1|2, false>    test_linear_routes_exact[1|2-*], test_kraus_routes_exact[1|2-*]
  convert_kernel<1|2, true>     test_abs_step_on_known_spectra[1|2-*], test_abs_step_batch_geometry, test_nonfinite_into_chi[1|2-*]
  convert3_kernel               test_linear_routes_exact[3-*] (chi ->), test_kraus_routes_exact[3-*] (-> superop; everything
                                under FBX_CONVERT3_V1=1), test_abs_step_on_known_spectra[3-*], test_nonfinite_into_chi[3-*]
  convert3_fast_kernel<1>, <4>  test_linear_routes_exact[3-*]; second trip of the grid-stride loop: test_second_trip_3q
  convert3_fast_kernel<0|2|3>   test_linear_routes_exact[3-*-v1]; second trip: test_second_trip_3q (superop -> PL, <2>)
  convert3_regs_kernel<0|2|3>   test_linear_routes_exact[3-*-default]
  convert_big_kernel<4>         test_linear_routes_exact[4-*], test_kraus_routes_exact[4-*]; second trip of launch_convert_big's
                                chunk loop: test_second_trip_4q
  convert_big_kernel<5>         test_five_qubit_routes_exact; second trip: test_second_trip_5q
  convert_into_chi_big          test_abs_step_on_known_spectra[4-*], test_nonfinite_into_chi[4-*]; second trip of its chunk
                                loop: test_second_trip_into_chi_4q
  convert_general_kernel        test_general_dimension_exact; as the Kraus-overflow fallback of fbx_convert_dev, second trip
                                of its chunk loop included: test_second_trip_4q (K = 41)
  fbx_apply_choi                test_apply_choi_on_non_hermitian_integers

Tolerances: none is new.  "Exact" follows from integer arithmetic; 1e-11 is the suite's figure for the routes into chi at 1-3
qubits (test_superops_gpu.py::test_pairwise_conversions), 1e-9 the one at 4 qubits
(test_four_qubit_conversions_match_the_oracle).

Measured on an MI355X (each test prints its figures):
  |C| step, worst max-abs error against the expected chi over the three sources
      qubits   Pauli-diagonal   Haar basis   bound
        1        1.11e-16        1.11e-16    1e-11
        2        1.39e-16        1.21e-16    1e-11
        3        6.25e-17        6.00e-16    1e-11
        4        2.43e-17        6.31e-16    1e-9
    the 257 diagonal four-qubit items: 0.0 on every item.
  non-finite items into chi: the bad item has 0 finite parts of 2 D^2 in all 36 cases (4 sizes x 3 sources x 3 kinds).  Before
    the guards in convert_kernel<NQ, true>, convert3_kernel and convert_into_chi_big all 2 D^2 parts were FINITE at 1-3 qubits in
    every case tried (the suspected silent answer: a NaN eigenvalue cut to 0, a NaN off the diagonal never rotated), and at 4
    qubits from a superoperator whose bad entry the reshuffle carries above the Choi matrix's diagonal; the neighbours kept
    their bits before and after.
"""
import contextlib
import os

import numpy as np
import pytest

import convert_cases as cc

pytestmark = pytest.mark.gpu
INTO_CHI_SOURCES = ("choi", "superop", "pauli_liouville")
TOL_INTO_CHI = {1: 1e-11, 2: 1e-11, 3: 1e-11, 4: 1e-9}


@contextlib.contextmanager
def convert3_form(v1):
    """the 3-qubit routes through the one-stage-per-pass kernels (FBX_CONVERT3_V1=1) or the default ones"""
    old = os.environ.pop("FBX_CONVERT3_V1", None)
    if v1:
        os.environ["FBX_CONVERT3_V1"] = "1"
    try:
        yield
    finally:
        os.environ.pop("FBX_CONVERT3_V1", None)
        if old is not None:
            os.environ["FBX_CONVERT3_V1"] = old


def convert(src, dst, x):
    from fbx.operator_tools import convert_batch
    return convert_batch(src, dst, np.ascontiguousarray(x))


def forms(n):
    return (False, True) if n == 3 else (False,)


def all_nan(z):
    return bool(np.isnan(z.real).all() and np.isnan(z.imag).all())


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ------------------------------------------------------------------ 1. every linear route, exactly
@pytest.mark.parametrize("n,B", [(1, 1), (1, 3), (1, 65), (2, 1), (2, 3), (2, 65), (3, 1), (3, 5), (4, 2)])
def test_linear_routes_exact(gpu, n, B):
    for src, dst in cc.LINEAR_ROUTES:
        x, want = cc.exact_case(src, dst, n, B)
        for v1 in forms(n):
            with convert3_form(v1):
                got = convert(src, dst, x)
            assert np.array_equal(got, want), (src, dst, "v1" if v1 else "default", float(np.abs(got - want).max()))


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n,B", [(1, 1), (1, 3), (1, 65), (2, 1), (2, 3), (2, 65), (3, 1), (3, 5), (4, 2)])
def test_kraus_routes_exact(gpu, n, B, K):
    for src, dst in cc.KRAUS_ROUTES:
        x, want = cc.exact_case(src, dst, n, B, K)
        for v1 in forms(n):
            with convert3_form(v1):
                got = convert(src, dst, x)
            assert np.array_equal(got, want), (dst, K, "v1" if v1 else "default", float(np.abs(got - want).max()))


def five_qubit_case(src, dst):
    """two items per route, shared by the B = 1 and the B = 17 test (the oracle's 1024^3 products run once)"""
    return cc.exact_case(src, dst, 5, 2, 2 if src == "kraus" else 0)


def test_five_qubit_routes_exact(gpu):
    """to_pauli_big (choi -> PL), from_pauli_big (PL -> superop, chi -> choi), the reshuffle and kraus_to at 1024 x 1024"""
    for src, dst in cc.FIVE_QUBIT_ROUTES + (("kraus", "chi"),):
        x, want = five_qubit_case(src, dst)
        got = convert(src, dst, x[:1])
        assert np.array_equal(got, want[:1]), (src, dst, float(np.abs(got - want[:1]).max()))


def test_general_dimension_exact(gpu):
    for d in (3, 5):
        ks = cc.int_kraus(d, 2, 3)
        choi = convert("kraus", "choi", ks)
        sup = convert("kraus", "superop", ks)
        assert np.array_equal(choi, cc.oracle_batch("kraus", "choi", ks)), d
        assert np.array_equal(sup, cc.oracle_batch("kraus", "superop", ks)), d
        x = cc.int_matrices(d * d, 3)
        assert np.array_equal(convert("choi", "superop", x), cc.oracle_batch("choi", "superop", x)), d
        assert np.array_equal(convert("superop", "choi", x), cc.oracle_batch("superop", "choi", x)), d


# ------------------------------------------------------------------ 2. second trips
def tiled(x2, B, cap):
    """B items alternating between the two of x2, the phase flipped from item `cap` on (the size of the first trip): item
    cap + k is not item k, so a trip that starts from the batch's beginning again, on either pointer, is seen"""
    tail_shape = (1,) * (x2.ndim - 1)
    head = np.tile(x2, (cap // 2,) + tail_shape)
    tail = np.tile(x2[::-1], ((B - cap) // 2 + 1,) + tail_shape)[:B - cap]
    pick = np.r_[np.arange(cap) % 2, 1 - np.arange(B - cap) % 2]
    return np.concatenate([head, tail]), pick


def assert_items_of_their_source(got, want2, pick, what):
    for k in (0, 1):
        assert np.array_equal(got[pick == k], np.broadcast_to(want2[k], got[pick == k].shape)), what


def test_second_trip_3q(gpu):
    """the grid of convert3_fast_kernel is min(B, 4096): 4099 items send three workgroups round their loop again"""
    B = 4096 + 3
    for src, dst, v1 in (("pauli_liouville", "choi", False), ("choi", "superop", False), ("superop", "pauli_liouville", True)):
        x2, want2 = cc.exact_case(src, dst, 3, 2, tag=1)
        assert not np.array_equal(want2[0], want2[1])
        with convert3_form(v1):
            x, pick = tiled(x2, B, 4096)
            got = convert(src, dst, x)
        assert_items_of_their_source(got, want2, pick, (src, dst))


@pytest.mark.parametrize("src,dst,K", [("pauli_liouville", "choi", 0), ("kraus", "pauli_liouville", 2), ("kraus", "pauli_liouville", 41)])
def test_second_trip_4q(gpu, src, dst, K):
    """257 four-qubit items: launch_convert_big's 512 MiB of work matrices hold 256, and so do the 256 MiB of Choi matrices of
    the fallback for more Kraus operators than the fused kernel stages (41 x 256 x 16 B is past its 160 KiB; 40 fit)"""
    x2, want2 = cc.exact_case(src, dst, 4, 2, K, tag=1)
    assert not np.array_equal(want2[0], want2[1])
    x, pick = tiled(x2, 257, 256)
    got = convert(src, dst, x)
    if K == 41:
        assert gpu.lib().fbx_last_error() == b""
    assert_items_of_their_source(got, want2, pick, (src, dst, K))


def test_second_trip_5q(gpu):
    """17 five-qubit items: the 512 MiB of work matrices hold 16"""
    x2, want2 = five_qubit_case("pauli_liouville", "superop")
    assert not np.array_equal(want2[0], want2[1])
    x, pick = tiled(x2, 17, 16)
    got = convert("pauli_liouville", "superop", x)
    assert_items_of_their_source(got, want2, pick, "5 qubits")


def test_second_trip_into_chi_4q(gpu):
    """257 diagonal four-qubit Choi matrices with signed integer diagonals, every item its own: convert_into_chi_big holds 256
    per chunk.  The Jacobi has nothing to rotate; an item read from or written to the wrong offset is off by integers / 256."""
    choi, chi = cc.diagonal_int_choi(4, 257)
    got = convert("choi", "chi", choi)
    err = np.abs(got - chi).reshape(257, -1).max(axis=1)
    print("into chi, 4 qubits, 257 diagonal items: worst", err.max(), "last item", err[-1])
    assert err.max() < TOL_INTO_CHI[4], int(err.argmax())


# ------------------------------------------------------------------ 3. the |C| step on known spectra
@pytest.mark.parametrize("family", ["diag", "basis"])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_abs_step_on_known_spectra(gpu, n, family):
    """chi of |C| for Choi matrices with a prescribed spectrum, entered as a Choi matrix, a superoperator and a Pauli-Liouville
    matrix.  At 1-3 qubits the eigenvalues +-5e-10 that the cut drops would contribute 5e-10 / d >= 6e-11, so a missing or
    misplaced cut fails the 1e-11.  At 4 qubits the bound is the suite's 1e-9 and the values near the cut are left out of the
    spectrum: at that tolerance the cut is NOT observable, and this case checks signs, degeneracy and the zero only."""
    choi, chi = cc.spectra_cases(n)[family]
    for src in INTO_CHI_SOURCES:
        got = convert(src, "chi", cc.as_source(src, choi))
        err = float(np.abs(got - chi).max())
        print(f"into chi from {src}, {n} qubits, {family}: {err:.3e}")
        assert err < TOL_INTO_CHI[n], (src, err)
    if n <= 3:
        # the reference's eigh reads the lower triangle: garbage above the diagonal changes no bit
        dirty = np.array(choi)
        iu = np.triu_indices(4 ** n, 1)
        dirty[:, iu[0], iu[1]] = 1e3 - 7e2j
        assert same_bits(convert("choi", "chi", dirty), convert("choi", "chi", choi))


@pytest.mark.parametrize("n,B", [(1, 1), (1, 63), (1, 64), (1, 65), (2, 1), (2, 63), (2, 64), (2, 65), (3, 1), (3, 3)])
def test_abs_step_batch_geometry(gpu, n, B):
    """every item of a batch has the bits it has when converted alone"""
    cases = cc.spectra_cases(n)
    pool = np.concatenate([cases["diag"][0], cases["basis"][0]])
    for src in INTO_CHI_SOURCES:
        xs = cc.as_source(src, pool)
        alone = np.concatenate([convert(src, "chi", xs[k:k + 1]) for k in range(len(xs))])
        pick = np.arange(B) % len(xs)
        assert same_bits(convert(src, "chi", xs[pick]), alone[pick]), src


# ------------------------------------------------------------------ 4. non-finite items
def bad_entry(src, kind, n):
    """(row, col, value) of the entry that makes an item non-finite.  For a Choi source it lies where the route reads (the
    diagonal's real part, the strict lower triangle); for a superoperator the off-diagonal ones are chosen so that the
    reshuffle carries them to where the Choi matrix is NOT read, [d, 0] -> [0, 1] above the diagonal and [d + 1, 0] -> the
    imaginary part of [1, 1]: the route reads every entry of such a source."""
    d = 2 ** n
    if kind == "nan_diagonal":
        return 2, 2, complex(np.nan, 0.0)
    if kind == "nan_lower":
        return d, 0, complex(np.nan, 0.0)
    return d + 1, 0, complex(0.0, np.inf)


@pytest.mark.parametrize("kind", ["nan_diagonal", "nan_lower", "inf_imaginary"])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_nonfinite_into_chi(gpu, n, kind):
    """include/fbx.h: a NaN or an Inf in an entry that a route into chi reads gives NaN in every entry of that item's output,
    FBX_OK, and every other item bit-identical to the clean call"""
    cases = cc.spectra_cases(n)
    pool = np.concatenate([cases["diag"][0], cases["basis"][0]])
    for src in INTO_CHI_SOURCES:
        x = cc.as_source(src, pool[np.arange(5) % len(pool)])
        clean = convert(src, "chi", x)
        assert np.isfinite(clean.real).all() and np.isfinite(clean.imag).all()
        r, c, v = bad_entry(src, kind, n)
        x[2, r, c] = v
        got = convert(src, "chi", x)                    # (returns: FBX_OK)
        finite = int(np.isfinite(got[2].real).sum() + np.isfinite(got[2].imag).sum())
        print(f"{src} -> chi, {n} qubits, {kind}: {finite} finite parts of {2 * got[2].size} in the bad item")
        assert all_nan(got[2]), (src, finite)
        keep = [0, 1, 3, 4]
        assert same_bits(got[keep], clean[keep]), src


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_nonfinite_on_the_linear_routes(gpu, n):
    """a non-finite item leaves its neighbours their bits on every linear route, and the reshuffle, a pure permutation,
    carries one NaN to exactly one entry"""
    d, D = 2 ** n, 4 ** n
    for src, dst in cc.LINEAR_ROUTES:
        x = np.array(cc.exact_case(src, dst, n, 5, tag=2)[0])
        for v1 in forms(n):
            with convert3_form(v1):
                clean = convert(src, dst, x)
                y = np.array(x)
                y[2, d, 0] = complex(np.nan, 0.0)
                got = convert(src, dst, y)
            keep = [0, 1, 3, 4]
            assert same_bits(got[keep], clean[keep]), (src, dst)
            assert np.isnan(got[2].real).any() or np.isnan(got[2].imag).any(), (src, dst)
            if {src, dst} == {"choi", "superop"}:
                nan = np.isnan(got[2].real) | np.isnan(got[2].imag)
                assert nan.sum() == 1 and nan[0, 1], (src, dst)         # [(1,0),(0,0)] <-> [(0,0),(0,1)]
                assert np.array_equal(got[2][~nan], clean[2][~nan])


# ------------------------------------------------------------------ 5. fbx_apply_choi
@pytest.mark.parametrize("n", [1, 2, 3])
def test_apply_choi_on_non_hermitian_integers(gpu, n):
    from fbx.operator_tools import apply_choi_matrix_2_state_batch
    d = 2 ** n
    choi, rho = cc.int_matrices(d * d, 5, tag=7), cc.int_states(d, 5, tag=7)
    assert not np.array_equal(choi, choi.conj().transpose(0, 2, 1)) and not np.array_equal(rho, rho.conj().transpose(0, 2, 1))
    got = apply_choi_matrix_2_state_batch(choi, rho)
    want = cc.apply_choi_exact(choi, rho)
    assert np.array_equal(got, want), float(np.abs(got - want).max())
