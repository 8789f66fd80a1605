"""fbx_proj_choi (CP, TP, TNI, Dykstra to the physical TP / TNI sets) on the structured inputs of tests/proj_cases.py -- rank-1,
degenerate and clustered spectra, partial traces that sit on the TNI clamp, exact integers -- against mpmath at 50 digits
(tests/golden/proj_cases.npz, from tests/golden/make_proj_goldens.py), long double, exact answers and properties that need no
reference; with the batch invariances, guard bytes around the outputs and the non-finite contract of include/fbx.h.

The bounds (tests/proj_cases.py, where they are derived; c_p and c_d are the float64 oracle's measured error against mpmath
with a factor 4 of margin):
  CP       ||got - ref||_F <= (1e-13 + c_p D eps) ||H||_F,  H the Hermitian part of the input
  TNI      ||got - ref||_F <= (1e-13 + c_p d eps) ||P||_F,  P = tr_out of the input
  TP       |got - ref| <= (D + 2) eps (|x| + kron((tr_out |x| + I) / d, I)) entrywise; bit for bit on integers
  Dykstra  the iteration count of the reference, and ||got - ref||_F <= iters (1e-13 + c_d D eps) (||x||_F + d)
Applying CP, TNI or TP a second time moves a result by no more than the bound of the first application.
Each test prints the ratio of what it saw to what it allows (pytest -s); every ratio is at most 1.
"""
import ctypes as C

import numpy as np
import pytest

import proj_cases as pc
from test_linalg_gpu import Guarded

pytestmark = pytest.mark.gpu
KIND = {"cp": 0, "tp": 1, "tni": 2, "ptp": 3, "ptni": 4}          # FBX_PROJ_*


@pytest.fixture(scope="module")
def gold():
    return pc.gold()


def proj(kind, xs):
    """(outputs, Dykstra counts) of one call; a second call on the reversed batch must be bit-identical per item"""
    from fbx.operator_tools.project_superoperators import proj_choi_batch
    xs = np.ascontiguousarray(xs)
    out, iters = proj_choi_batch(KIND[kind], xs, return_iters=True)
    out_r, iters_r = proj_choi_batch(KIND[kind], np.ascontiguousarray(xs[::-1]), return_iters=True)
    assert np.array_equal(out_r[::-1], out) and np.array_equal(iters_r[::-1], iters), (kind, "results depend on the item's place in the batch")
    return out, iters


def label(d):
    return {2: "wave1q", 4: "wave2q", 8: "block3q"}.get(d, f"host d={d}")


@pytest.mark.parametrize("D", pc.CP_SIZES)
def test_cp_structured(gpu, gold, D):
    """The cp and channel families of one size in one shuffled batch: proj_choi_kernel<1>, <2>, proj_choi3_kernel, and for the
    qutrit eigh + matmul driven by the host."""
    cases = pc.cp_inputs(D)
    pc.check_hashes(cases, gold)
    keys, xs = pc.shuffled(cases, D)
    got, _ = proj("cp", xs)
    assert pc.check_cp(label(pc.dim_of(D)), keys, xs, got, gold) <= 1.0
    assert pc.check_twice(label(pc.dim_of(D)), "cp", keys, xs, got, proj("cp", got)[0], gold) <= 1.0
    if D != 9:                                                  # exact powers of two: the relative bound is met above
        at = {pc.family_of(k): b for b, k in enumerate(keys)}
        for name, e in (("scale_up", 200), ("scale_down", -200)):
            same = np.array_equal(got[at[name]], np.ldexp(got[at["gaussian"]].real, e) + 1j * np.ldexp(got[at["gaussian"]].imag, e))
            print(f"{label(pc.dim_of(D)):8s} cp {name} is the gaussian result times 2^{e} bit for bit: {same}")


@pytest.mark.parametrize("d", pc.DIMS)
def test_tni_structured(gpu, gold, d):
    cases = pc.tni_inputs(d)
    pc.check_hashes(cases, gold)
    keys, xs = pc.shuffled(cases, d)
    got, _ = proj("tni", xs)
    assert pc.check_tni(label(d), keys, xs, got, gold) <= 1.0
    assert pc.check_twice(label(d), "tni", keys, xs, got, proj("tni", got)[0], gold) <= 1.0


@pytest.mark.parametrize("d", pc.DIMS)
def test_tp_structured(gpu, gold, d):
    """bit for bit on the integer family; the entrywise dot-product bound on the channel and tni families"""
    x = pc.tpx_cases(d)[f"tpx_d{d}"]
    pc.check_hashes(pc.tpx_cases(d), gold)
    got, _ = proj("tp", x)
    for b in range(len(x)):
        assert np.array_equal(got[b], pc.tp_projection(x[b], d)), (d, b, np.abs(got[b] - pc.tp_projection(x[b], d)).max())
    keys, xs = pc.shuffled(pc.tni_inputs(d), 100 + d)
    got, _ = proj("tp", xs)
    assert pc.check_tp(label(d), keys, xs, got) <= 1.0
    assert pc.check_twice(label(d), "tp", keys, xs, got, proj("tp", got)[0], gold) <= 1.0


@pytest.mark.parametrize("kind", ["ptp", "ptni"])
@pytest.mark.parametrize("d", pc.DIMS)
def test_dykstra_structured(gpu, gold, d, kind):
    """The channel family through Dykstra: 1 to 294 iterations, every CP projection from the second on warm-started from the
    previous basis -- of a rank-1 matrix for the unitary cases.  d = 2, 3, 4 against the mpmath iteration, d = 8 against the
    float64 oracle (run here, once per process)."""
    cases = pc.channel_cases(d)
    pc.check_hashes(cases, gold)
    keys, xs = pc.shuffled(cases, 200 + d)
    got, iters = proj(kind, xs)
    assert pc.check_dykstra(label(d), kind, keys, xs, got, iters, gold) <= 1.0


@pytest.mark.parametrize("kind", pc.KINDS)
def test_two_waves_kernel_is_bit_identical(gpu, kind):
    """n = 2: a batch of 2048 items or more goes to proj_choi_w2_kernel (two wavefronts per SIMD, at most 256 registers); the
    structured batch tiled past that size must give what the small batch gives, iteration counts included"""
    from fbx.operator_tools.project_superoperators import proj_choi_batch
    cases = pc.channel_cases(4) if kind in ("ptp", "ptni") else pc.cp_inputs(16) if kind == "cp" else pc.tni_inputs(4)
    _, xs = pc.shuffled(cases, 300)
    small, it_small = proj_choi_batch(KIND[kind], xs, return_iters=True)
    reps = -(-2049 // len(xs))
    big, it_big = proj_choi_batch(KIND[kind], np.ascontiguousarray(np.tile(xs, (reps, 1, 1))), return_iters=True)
    assert len(big) >= 2048
    assert np.array_equal(big.reshape(reps, *small.shape), np.broadcast_to(small, (reps,) + small.shape))
    assert np.array_equal(it_big.reshape(reps, -1), np.broadcast_to(it_small, (reps, len(xs))))


@pytest.mark.parametrize("kind", ["cp", "ptp"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_proj_choi_dev_writes_inside_its_outputs(gpu, n, kind):
    d = 2 ** n
    D, B = d * d, 4                                            # four int32 counts: two whole guard words
    xs = np.stack([pc.channel_cases(d)[f"ch_d{d}_{name}"] for name in ("unitary", "noisy_e1", "tpnotcp", "cp17")])
    d_x = gpu.DeviceBuffer.from_array(xs)
    out, its = Guarded(gpu, B * D * D * 2), Guarded(gpu, B // 2)
    gpu.check(gpu.lib().fbx_proj_choi_dev(KIND[kind], n, B, d_x.ptr, out.ptr, its.ptr))
    want, want_it = proj(kind, xs)
    assert np.array_equal(out.doubles().view(np.complex128).reshape(B, D, D), want)
    assert np.array_equal(its.read().view(np.int32), want_it if kind == "ptp" else np.zeros(B, dtype=np.int32))
    no_its = Guarded(gpu, B * D * D * 2)
    gpu.check(gpu.lib().fbx_proj_choi_dev(KIND[kind], n, B, d_x.ptr, no_its.ptr, C.c_void_p(None)))
    assert np.array_equal(no_its.doubles().view(np.complex128).reshape(B, D, D), want)


def _poisoned(x, how):
    a = np.array(x)
    D = a.shape[0]
    if how == "nan_off":                                       # off the diagonal: the eigensolver alone would not notice
        a[D - 1, 1] = complex(np.nan, 0.25)
    elif how == "nan_diag":
        a[D // 2, D // 2] = np.nan
    elif how == "inf_off_imag":
        a[1, D - 2] = complex(0.5, np.inf)
    elif how == "minus_inf_diag":                              # a clamp alone would turn it into a finite 0
        a[0, 0] = -np.inf
    return a


@pytest.mark.parametrize("kind", pc.KINDS)
@pytest.mark.parametrize("n", [1, 2, 3])
def test_nonfinite_item_gives_nan_for_itself_only(gpu, n, kind):
    """include/fbx.h: an item with a NaN or an Inf anywhere returns NaN in every entry and, for the Dykstra kinds, the count 1;
    the call returns FBX_OK and every other item is bit-identical to the same call with a finite matrix in that place.
    Termination: such an item is not projected at all (proj_choi_body in csrc/fbx_superop.hip and proj_choi3_kernel in
    csrc/fbx_pgdb3.hip test the entries they loaded and return)."""
    from fbx.operator_tools.project_superoperators import proj_choi_batch
    d = 2 ** n
    names = ("noisy_e3", "unitary", "noisy_e1", "tpnotcp", "mix")
    clean = np.stack([pc.channel_cases(d)[f"ch_d{d}_{name}"] for name in names])
    out0, it0 = proj_choi_batch(KIND[kind], clean, return_iters=True)
    assert np.isfinite(out0).all()
    for place, how in ((2, "nan_off"), (1, "nan_diag"), (3, "inf_off_imag"), (2, "minus_inf_diag")):
        dirty = clean.copy()
        dirty[place] = _poisoned(clean[place], how)
        out1, it1 = proj_choi_batch(KIND[kind], dirty, return_iters=True)          # raises unless FBX_OK
        keep = [b for b in range(len(names)) if b != place]
        assert np.isnan(out1[place].real).all() and np.isnan(out1[place].imag).all(), (n, kind, how)
        assert it1[place] == (1 if kind in ("ptp", "ptni") else 0), (n, kind, how, it1[place])
        assert np.array_equal(out1[keep], out0[keep]) and np.array_equal(it1[keep], it0[keep]), (n, kind, how)
