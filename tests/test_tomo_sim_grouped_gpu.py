"""fbx_tomo_simulate_grouped on the GPU (include/fbx.h): the outcome distribution of every group against a dense longdouble
computation, the exact means against those of fbx_tomo_simulate bit for bit, histograms / expectations / counts bit for bit
against the host restatement of the stream, known answers that only shared shots can give, the stream's dependence on (seed,
item, group) only, poisoned items, a guard on the sampler that does not use the restatement, and the consumers.

The kernel has ONE switch between work splits (csrc/fbx_tomo_sim_grouped.hip): for 1..3 qubits, from FBX_TOMOG_LANE_MIN_UNITS
(a compile-time macro; its default 131072 is assumed here) units = B x groups on a lane takes an (item, group), below a
wavefront does; 4 and 5 qubits have the wavefront form only.  B = 5 of every design is on the wavefront side;
test_both_sides_of_the_lane_switch crosses it.  Inside the wavefront form the number of qubits picks the counters (registers
for 1..3 qubits, LDS above): the cases cover both."""
import functools
import math

import numpy as np
import pytest

import sampling_cases as sc
import tomo_sim_cases as tc
from tomo_sim_cases import B, FIRST, SEED

pytestmark = pytest.mark.gpu

LANE_MIN_UNITS = 131072
SHOT_COUNTS = (1, 3, 4, 5, 257, 1000)       # the tail block, fewer blocks than lanes, the general case
ALL_CASES = tc.PROCESS_CASES + tuple(f"state-{n}" for n in tc.STATE_CASES)
_LD, _CLD = np.longdouble, np.clongdouble


@functools.lru_cache(maxsize=None)
def design_of(case):
    from fbx.design import state_design
    return state_design(int(case[6:])) if case.startswith("state") else tc.process_case_design(case)


@functools.lru_cache(maxsize=None)
def grouping_of(case):
    from fbx.design import group_design
    return group_design(design_of(case))


def flips_of(case, on):
    return sc.asymmetric_flips(design_of(case).n_qubits, B, seed=5) if on else None


def simulate(case, grouped, shots, **kw):
    from fbx import tomography as t
    des = design_of(case)
    if grouped:
        kw.setdefault("groups", grouping_of(case))
    if case.startswith("state"):
        f = t.simulate_grouped_state_tomography_batch if grouped else t.simulate_state_tomography_batch
        return f(des, kw.pop("truth", tc.mixed_states(des.n_qubits)), shots, **kw)
    f = t.simulate_grouped_process_tomography_batch if grouped else t.simulate_process_tomography_batch
    return f(des, kw.pop("truth", tc.damped_kraus(des.n_qubits)), shots, rep=kw.pop("rep", "kraus"), **kw)


@functools.lru_cache(maxsize=None)
def device(case, with_flips=False, shots=1000):
    """(expectations, counts, std_errs, exact, probabilities, histograms) of the B-item grouped call that the tests share"""
    out = simulate(case, True, shots, readout_flip=flips_of(case, with_flips), seed=SEED, first_item=FIRST, return_std_errs=True,
                   return_exact=True, return_probabilities=True, return_histograms=True)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def host(case, with_flips=False, shots=1000):
    """the restatement from the device's distributions"""
    from fbx import synthetic
    des = design_of(case)
    return synthetic.restate_grouped_tomography_counts(device(case, with_flips, shots)[4], grouping_of(case), des.paulis, des.coefs,
                                                       shots, SEED, FIRST)


def check_counts(got, want, shots):
    """histograms, expectations and counts bit for bit; std_err within 8 x 2^-53 relative of the integer formula, 0 at the ends"""
    e, c, s, _, _, hist = got
    we, wc, ws, whist = want
    assert hist.dtype == np.uint32 and np.array_equal(hist, whist)
    bad = np.argwhere(e != we)
    assert bad.size == 0, f"{len(bad)} expectations differ, first at (item, setting) {bad[0].tolist()}: {e[tuple(bad[0])]!r} != {we[tuple(bad[0])]!r}"
    assert np.array_equal(c, wc) and np.all(c == float(shots))
    rel = np.abs(s - ws) / np.where(ws > 0, ws, 1.0)
    print(f"std_err: worst relative excursion {rel.max() / 2.0 ** -53:.2f} x 2^-53")
    assert np.all(rel <= 8 * 2.0 ** -53)
    assert np.all(s[ws == 0.0] == 0.0)                    # (the integer formula is 0 exactly where k_plus is 0 or N)


# ------------------------------------------------------------------------------------------------ 1. the distribution
def dense_distribution(basis, rho, flips):
    """p [2^n] in longdouble: tr[(x)_j (I +- P_j) / 2 rho] over the bit patterns (bit 0 = eigenvalue +1, qubit 0 the most significant
    bit of the outcome), then the [drawn][read] confusion matrix of every qubit"""
    n = len(basis)
    T = rho.astype(_CLD).reshape((2,) * (2 * n))           # axes: row bits of the qubits, then column bits
    eye = tc._PAULI[0]
    for q, code in enumerate(basis):
        ax = tc._PAULI[int(code)]
        P = np.stack([(eye + ax) / 2, (eye - ax) / 2])     # [bit, row, column]
        T = np.moveaxis(np.tensordot(P, T, axes=([2, 1], [q, n])), 0, q)       # tr over qubit q: P[a, b] rho[b, a]
    p = np.real(T).astype(_LD)
    if flips is not None:
        f = flips.astype(_LD)
        for j in range(n):
            conf = np.array([[1 - f[j, 0], f[j, 0]], [f[j, 1], 1 - f[j, 1]]], dtype=_LD)          # [drawn][read]
            p = np.moveaxis(np.tensordot(conf, p, axes=([0], [j])), 0, j)
    return p.reshape(-1)


@functools.lru_cache(maxsize=None)
def dense(case, with_flips):
    """[B, G, 2^n] longdouble"""
    des, g = design_of(case), grouping_of(case)
    flips = flips_of(case, with_flips)
    if case.startswith("state"):
        rho = tc.mixed_states(des.n_qubits)
        outputs = lambda b, k: rho[b]
    else:
        out = tc.process_outputs(des, tc.damped_kraus(des.n_qubits))
        outputs = lambda b, k: out[b, k]
    return np.array([[dense_distribution(g.basis[i], outputs(b, grp[0]), None if flips is None else flips[b])
                      for i, grp in enumerate(g.groups)] for b in range(B)])


@pytest.mark.parametrize("with_flips", (False, True))
@pytest.mark.parametrize("case", ALL_CASES)
def test_distribution_against_dense_longdouble(gpu, case, with_flips):
    """tolerance 2 x 64 dim^2 2^-53 per probability: a probability is the mean of 2^n means, each within tc.tolerance (64 dim^2
    2^-53, conversion of the truth included); the transform and the n convex butterflies add a few ulps, which the 2 covers"""
    des = design_of(case)
    tol = 2 * 64.0 * des.dim ** 2 * tc.EPS
    got, want = device(case, with_flips)[4], dense(case, with_flips)
    assert got.shape == want.shape == (B, grouping_of(case).n_groups, des.dim)
    worst = float(np.abs(got - want).max()) / tol
    rows = float(np.abs(got.sum(axis=2) - 1.0).max()) / tol
    print(f"{case} flips={with_flips}: worst excursion {worst:.4f} of the tolerance, row sums {rows:.4f}")
    assert worst <= 1.0 and rows <= 1.0
    assert float(np.ptp(want)) > 0.25 / des.dim                            # (the distributions are not flat)
    if with_flips:
        assert np.abs(got - device(case, False)[4]).max() > 0.1 / des.dim  # (the flips matter)


# ------------------------------------------------------------------------------------------------ 2. exact means
@pytest.mark.parametrize("with_flips", (False, True))
@pytest.mark.parametrize("case", ALL_CASES)
def test_exact_means_are_those_of_the_ungrouped_call(gpu, case, with_flips):
    want = simulate(case, False, 1000, readout_flip=flips_of(case, with_flips), seed=SEED, first_item=FIRST, return_exact=True)[2]
    assert np.array_equal(device(case, with_flips)[3], want) and np.abs(want).max() > 0.0
    # n_shots == 0 through the C ABI: exact_out and prob_out only, the same values
    from fbx import _lib
    if case == "2q-sic":
        from fbx.operator_tools.superoperator_transformations import convert_batch
        des, g = design_of(case), grouping_of(case)
        ptm = np.ascontiguousarray(convert_batch("kraus", "pauli_liouville", tc.damped_kraus(2)).real)
        flips = flips_of(case, with_flips)
        ex, pr = np.empty((B, des.m)), np.empty((B, g.n_groups, 4))
        _lib.check(_lib.lib().fbx_tomo_simulate_grouped(des.handle, g.handle, B, _lib.dptr(ptm), 0, _lib.dptr(flips), SEED, FIRST,
                                                        None, None, None, _lib.dptr(ex), _lib.dptr(pr), None, None))
        assert np.array_equal(ex, want) and np.array_equal(pr, device(case, with_flips)[4])


# ------------------------------------------------------------------------------------------------ 3. counts bit for bit
@pytest.mark.parametrize("shots", SHOT_COUNTS)
@pytest.mark.parametrize("case", ALL_CASES)
def test_counts_bit_for_bit(gpu, case, shots):
    check_counts(device(case, True, shots), host(case, True, shots), shots)
    if shots == 1000:
        check_counts(device(case, False, shots), host(case, False, shots), shots)
        assert len(np.unique(host(case, False, shots)[3])) > 10           # (counts that vary: the comparison is not of constants)


# ------------------------------------------------------------------------------------------------ 4. known answers
def singletons_but(design, together):
    """a Grouping with the settings `together` in group 0 and every other setting alone"""
    from fbx.design import Grouping
    rest = [k for k in range(design.m) if k not in together]
    return Grouping.from_groups(design, [list(together)] + [[k] for k in rest])


@pytest.mark.parametrize("shots", (1, 37, 1000))
def test_bell_state_shares_shots_within_a_group(gpu, shots):
    """(|00> + |11>) / sqrt 2: in a ZZ group every shot reads 00 or 11, so IZ and ZI agree shot by shot and ZZ is +1 in all of
    them -- independent shots per setting (fbx_tomo_simulate) cannot give E[IZ] == E[ZI]"""
    from fbx import tomography as t
    from fbx.design import Grouping, state_design
    des = state_design(2)                                               # IX IY IZ XI XX XY XZ YI YX YY YZ ZI ZX ZY ZZ
    IZ, ZI, ZZ, IX, XI, XX = 2, 11, 14, 0, 3, 4
    g = Grouping.from_groups(des, [[IZ, ZI, ZZ], [IX, XI, XX]] + [[k] for k in range(15) if k not in (IZ, ZI, ZZ, IX, XI, XX)])
    bell = np.zeros((4, 4), dtype=complex); bell[np.ix_([0, 3], [0, 3])] = 0.5
    rho = np.broadcast_to(bell, (B, 4, 4))
    e, c, s, x, p, h = t.simulate_grouped_state_tomography_batch(des, rho, shots, groups=g, seed=SEED, first_item=FIRST,
                                                                 return_std_errs=True, return_exact=True,
                                                                 return_probabilities=True, return_histograms=True)
    assert np.array_equal(p[:, 0], np.broadcast_to([0.5, 0.0, 0.0, 0.5], (B, 4))) and np.all(h[:, 0, 1:3] == 0)
    assert np.array_equal(e[:, IZ], e[:, ZI]) and np.all(e[:, ZZ] == 1.0) and np.all(s[:, ZZ] == 0.0)
    assert np.all(e[:, XX] == 1.0) and np.all(s[:, XX] == 0.0) and np.array_equal(e[:, IX], e[:, XI])
    assert np.all(x[:, [IZ, ZI, IX, XI]] == 0.0) and np.all(x[:, [ZZ, XX]] == 1.0)
    if shots == 1000:
        assert len(np.unique(e[:, IZ])) > 1 and np.all(np.abs(e[:, IZ]) < 0.3) and np.all(s[:, IZ] > 0.0)
        ungrouped = t.simulate_state_tomography_batch(des, rho, shots, seed=SEED, first_item=FIRST)[0]
        assert not np.array_equal(ungrouped[:, IZ], ungrouped[:, ZI])


@pytest.mark.parametrize("n", (1, 2, 3, 4, 5))
def test_all_zeros_state_in_the_all_z_group(gpu, n):
    from fbx import tomography as t
    from fbx.design import state_design
    des = state_design(n)
    zs = [k for k in range(des.m) if np.all((des.paulis[k] == 0) | (des.paulis[k] == 3))]
    assert len(zs) == 2 ** n - 1
    g = singletons_but(des, zs)
    rho = np.zeros((B, 2 ** n, 2 ** n), dtype=complex); rho[:, 0, 0] = 1.0
    kw = dict(groups=g, seed=SEED, first_item=FIRST, return_std_errs=True, return_histograms=True)
    e, c, s, h = t.simulate_grouped_state_tomography_batch(des, rho, 37, **kw)
    assert np.all(e[:, zs] == 1.0) and np.all(s[:, zs] == 0.0) and np.all(h[:, 0, 0] == 37) and np.all(h[:, 0, 1:] == 0)
    flips = np.zeros((n, 2)); flips[:, 0] = 1.0                         # every drawn 0 is read as 1
    e, c, s, h = t.simulate_grouped_state_tomography_batch(des, rho, 37, readout_flip=flips, **kw)
    weight = (des.paulis[zs] != 0).sum(axis=1)
    assert np.array_equal(e[:, zs], np.broadcast_to((-1.0) ** weight, (B, len(zs)))) and np.all(s[:, zs] == 0.0)
    assert np.all(h[:, 0, -1] == 37)


# ------------------------------------------------------------------------------------------------ 5. the stream
def test_a_value_depends_on_seed_item_and_group_only(gpu):
    case = "2q-sic"
    flips, full = flips_of(case, True), device(case, True)
    kw = dict(seed=SEED, return_std_errs=True, return_exact=True, return_probabilities=True, return_histograms=True)
    kraus = tc.damped_kraus(2)
    head = simulate(case, True, 1000, truth=kraus[:2], readout_flip=flips[:2], first_item=FIRST, **kw)
    tail = simulate(case, True, 1000, truth=kraus[2:], readout_flip=flips[2:], first_item=FIRST + 2, **kw)
    one = simulate(case, True, 1000, truth=kraus[3:4], readout_flip=flips[3:4], first_item=FIRST + 3, **kw)
    for a, hd, tl, o in zip(full, head, tail, one):
        assert np.array_equal(a[:2], hd) and np.array_equal(a[2:], tl) and np.array_equal(a[3:4], o)
    other = simulate(case, True, 1000, readout_flip=flips, first_item=FIRST, **{**kw, "seed": SEED + 1})
    assert np.array_equal(other[3], full[3]) and np.array_equal(other[4], full[4])
    assert (other[5] != full[5]).mean() > 0.3 and (other[0] != full[0]).mean() > 0.5
    # the tag: the ungrouped call under the same seed draws other words -- compare on the singleton groups of the one-qubit
    # design, where group id == setting index and the two distributions are the same
    from fbx.design import Grouping
    des1 = design_of("1q-pauli")
    g1 = Grouping(des1, np.arange(des1.m))
    e_g = simulate("1q-pauli", True, 1000, groups=g1, seed=SEED, first_item=FIRST)[0]
    e_u = simulate("1q-pauli", False, 1000, seed=SEED, first_item=FIRST)[0]
    assert (e_g != e_u).mean() > 0.5
    # a group_of array and the method name give what the Grouping gives
    des = design_of(case)
    by_array = simulate(case, True, 1000, groups=grouping_of(case).group_of, readout_flip=flips, first_item=FIRST, **kw)
    by_name = simulate(case, True, 1000, groups="greedy", readout_flip=flips, first_item=FIRST, **kw)
    for a, x, y in zip(full, by_array, by_name):
        assert np.array_equal(a, x) and np.array_equal(a, y)
    assert des._groupings["greedy"] is not None


def test_dev_form_on_device_buffers(gpu):
    from fbx import _lib
    from fbx.operator_tools.superoperator_transformations import convert_batch
    case = "2q-sic"
    des, g, flips, full = design_of(case), grouping_of(case), flips_of(case, True), device(case, True)
    ptm = np.ascontiguousarray(convert_batch("kraus", "pauli_liouville", tc.damped_kraus(2)).real)
    DB, m, cells = _lib.DeviceBuffer, des.m, g.n_groups * 4
    d_t, d_f = DB.from_array(ptm), DB.from_array(flips)
    outs = [DB(B * m * 8) for _ in range(4)] + [DB(B * cells * 8), DB(B * cells * 4)]
    d_st = DB(B * 4)
    _lib.check(_lib.lib().fbx_tomo_simulate_grouped_dev(des.handle, g.handle, B, d_t.ptr, 1000, d_f.ptr, SEED, FIRST,
                                                        *[o.ptr for o in outs], d_st.ptr))
    _lib.synchronize()
    for a, buf in zip(full, outs):
        assert np.array_equal(a, buf.to_array(a.dtype, a.shape))
    assert not d_st.to_array(np.int32, (B,)).any()
    for buf in [d_t, d_f, d_st] + outs:
        buf.free()


# ------------------------------------------------------------------------------------------------ 6. work splits
@pytest.mark.parametrize("case", ("1q-sic", "2q-sic", "3q-shuffled"))
def test_both_sides_of_the_lane_switch(gpu, case):
    """LANE_MIN_UNITS = 131072 (the default of FBX_TOMOG_LANE_MIN_UNITS): the smallest design, 1q SIC with 12 groups, at 37 shots
    (nine blocks and a tail of one) -- 10923 x 12 units take a lane each, 5 x 12 a wavefront each; first_item puts the same
    global items into both calls, and they agree bit for bit and with the restatement.  The lane form is compiled once per
    number of qubits, so a two- and a three-qubit design cross the switch as well."""
    from fbx import synthetic
    des, g, shots = design_of(case), grouping_of(case), 37
    n = des.n_qubits
    assert case != "1q-sic" or g.n_groups == 12
    big = LANE_MIN_UNITS // g.n_groups + 1
    assert big * g.n_groups >= LANE_MIN_UNITS > 5 * g.n_groups
    us = tc.unitaries(n, big)
    flips = sc.asymmetric_flips(n, big, seed=7)
    kw = dict(rep="unitary", seed=SEED, return_std_errs=True, return_exact=True, return_probabilities=True, return_histograms=True)
    lane = simulate(case, True, shots, truth=us, readout_flip=flips, first_item=FIRST, **kw)
    wave = simulate(case, True, shots, truth=us[big - 5:], readout_flip=flips[big - 5:], first_item=FIRST + big - 5, **kw)
    for a, b in zip(lane, wave):
        assert np.array_equal(a[big - 5:], b)
    want = synthetic.restate_grouped_tomography_counts(wave[4], g, des.paulis, des.coefs, shots, SEED, FIRST + big - 5)
    check_counts(wave, want, shots)
    head = synthetic.restate_grouped_tomography_counts(lane[4][:3], g, des.paulis, des.coefs, shots, SEED, FIRST)
    check_counts([a[:3] for a in lane], head, shots)
    # a poisoned item on the lane side: status 1 and NaN for it alone
    from fbx import tomography as t
    bad = us.copy(); bad[7, 0, 0] = np.nan
    *got, status = t.simulate_grouped_process_tomography_batch(des, bad, shots, groups=g, readout_flip=flips, first_item=FIRST,
                                                               return_status=True, **kw)
    assert status[7] == 1 and status.sum() == 1
    assert all(np.all(np.isnan(a[7])) for a in (got[0], got[2], got[3], got[4])) and np.all(got[1][7] == 37.0) and np.all(got[5][7] == 0)
    for a, b in zip(got, lane):
        assert np.array_equal(np.delete(a, 7, axis=0), np.delete(b, 7, axis=0))


def _tail_call(case, batch, shots):
    """`batch` items of a case with flips: the device's outputs and the restatement of items [lo, hi)"""
    from fbx import synthetic
    des, g = design_of(case), grouping_of(case)
    n = des.n_qubits
    truth = dict(truth=tc.mixed_states(n, batch)) if case.startswith("state") else dict(truth=tc.unitaries(n, batch), rep="unitary")
    got = simulate(case, True, shots, readout_flip=sc.asymmetric_flips(n, batch, seed=7), seed=SEED, first_item=FIRST,
                   return_std_errs=True, return_exact=True, return_probabilities=True, return_histograms=True, **truth)
    return got, lambda lo, hi: synthetic.restate_grouped_tomography_counts(got[4][lo:hi], g, des.paulis, des.coefs, shots, SEED,
                                                                           FIRST + lo)


@pytest.mark.parametrize("shots", tc.TAIL_SHOTS)
@pytest.mark.parametrize("case", ("1q-sic", "state-4"))
def test_tail_block_on_the_wavefront_split(gpu, case, shots):
    """who owns the last, partial Philox block (tomo_sim_cases.TAIL_SHOTS), B = 3 and a wavefront per (item, group): the
    smallest design (one-qubit SIC, 12 groups) counts in registers, four qubits in LDS -- two calls of the walk"""
    got, restate = _tail_call(case, 3, shots)
    check_counts(got, restate(0, 3), shots)


@pytest.mark.parametrize("shots", tc.TAIL_SHOTS_LANE)
def test_tail_block_on_the_lane_split(gpu, shots):
    """... and 10923 x 12 >= LANE_MIN_UNITS units, a lane each: the first and the last items against the restatement"""
    big = LANE_MIN_UNITS // 12 + 1
    assert grouping_of("1q-sic").n_groups == 12 and big * 12 >= LANE_MIN_UNITS > (big - 1) * 12
    got, restate = _tail_call("1q-sic", big, shots)
    for lo, hi in ((0, 20), (big - 20, big)):
        check_counts([a[lo:hi] for a in got], restate(lo, hi), shots)


# ------------------------------------------------------------------------------------------------ 7. poison
@pytest.mark.parametrize("what", ("nan-truth", "flip-1.5", "overflowing-group"))
def test_poisoned_item(gpu, what):
    """A NaN truth entry, a flip of 1.5, and a FINITE truth with a group whose clamped probabilities do not sum to a positive
    finite number.  The probabilities of a group sum to t of the empty set = 1 whatever the truth is, so with finite
    probabilities the clamped sum is at least 1 -- it cannot be 0; the sum fails to be a positive finite number only by
    overflow, which this case provokes: diagonal entries of 1.5e308 pass the check of the truth entries, the ZZ-basis group adds
    two of the traces to infinity, and the groups without a Z stay finite.  One bad group poisons the item, all its groups."""
    from fbx import tomography as t
    des, bad, shots = design_of("state-2"), 3, 257
    g = grouping_of("state-2")
    rho = tc.mixed_states(2).copy()
    flips = flips_of("state-2", True).copy()
    kw = dict(groups=g, seed=SEED, first_item=FIRST, return_std_errs=True, return_exact=True, return_probabilities=True,
              return_histograms=True)
    clean = t.simulate_grouped_state_tomography_batch(des, rho, shots, readout_flip=flips, **kw)
    if what == "nan-truth":
        rho[bad, 1, 2] = complex(np.nan, 0.0)
    elif what == "flip-1.5":
        flips[bad, 1, 0] = 1.5
    else:
        rho[bad] = np.diag([1.5e308, 0.0, 0.0, 0.0])
        flips[bad] = 0.0
    *got, status = t.simulate_grouped_state_tomography_batch(des, rho, shots, readout_flip=flips, return_status=True, **kw)
    good = [b for b in range(B) if b != bad]
    assert status.tolist() == [int(b == bad) for b in range(B)]
    e, c, s, x, p, h = got
    assert np.all(np.isnan(e[bad])) and np.all(np.isnan(s[bad])) and np.all(np.isnan(x[bad])) and np.all(np.isnan(p[bad]))
    assert np.all(c[bad] == float(shots)) and np.all(h[bad] == 0)
    for a, b in zip(got, clean):
        assert np.array_equal(a[good], b[good])
    with pytest.raises(ValueError, match="item 3"):
        t.simulate_grouped_state_tomography_batch(des, rho, shots, readout_flip=flips, **kw)


def test_bad_arguments(gpu):
    import ctypes
    from fbx import _lib
    from fbx.design import state_design
    des, other = design_of("1q-pauli"), state_design(1)
    g = grouping_of("1q-pauli")
    lib, m = _lib.lib(), des.m
    ptm = np.ascontiguousarray(np.broadcast_to(np.eye(4), (B, 4, 4)))
    out = [np.full((B, m), -7.0) for _ in range(4)] + [np.full((B, g.n_groups, 2), -7.0)]
    hist = np.full((B, g.n_groups, 2), 7, dtype=np.uint32)
    st = np.full(B, -7, dtype=np.int32)

    def call(design=des.handle, grouping=g.handle, batch=B, truth=ptm, shots=37, first=FIRST, outs=(0, 1, 2, 3, 4, 5)):
        ptrs = [_lib.dptr(out[i]) if i in outs else None for i in range(5)] + [_lib.ptr(hist, ctypes.c_uint32) if 5 in outs else None]
        return lib.fbx_tomo_simulate_grouped(design, grouping, batch, _lib.dptr(truth), shots, None, SEED, first, *ptrs, _lib.iptr(st))
    for kw in (dict(batch=-1), dict(shots=-1), dict(shots=2 ** 32), dict(first=-1), dict(truth=None), dict(outs=()), dict(shots=0),
               dict(shots=0, outs=(3, 5)), dict(design=None), dict(grouping=None), dict(design=other.handle)):
        assert call(**kw) == _lib.FBX_ERR_BAD_ARG, kw
        assert lib.fbx_last_error()
    assert all(np.all(o == -7.0) for o in out) and np.all(hist == 7) and np.all(st == -7)     # refused before any buffer was touched
    assert call(batch=0) == _lib.FBX_OK and all(np.all(o == -7.0) for o in out)
    assert call(shots=0, outs=(3, 4)) == _lib.FBX_OK and np.all(out[0] == -7.0) and np.all(st == 0)
    assert set(np.unique(np.round(out[3], 12))) == {0.0, 1.0, -1.0} and np.allclose(out[4].sum(axis=2), 1.0)
    assert call(outs=(5,)) == _lib.FBX_OK and np.all(hist.sum(axis=2) == 37) and np.all(out[1] == -7.0)
    # fbx_grouping_create validates on its own (the Python class refuses the same groupings before it gets there)
    sdes = state_design(2)
    h = ctypes.c_void_p()

    def create(ids, n_groups):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        return lib.fbx_grouping_create(sdes.handle, n_groups, _lib.iptr(ids), ctypes.byref(h))
    ok = grouping_of("state-2").group_of
    clash = ok.copy(); clash[1] = clash[0]
    gap = np.arange(15); gap[gap >= 7] += 1
    for ids, n_groups in ((clash, 9), (gap, 16), (np.full(15, 9), 9), (np.full(15, -1), 9), (ok, 0)):
        assert create(ids, n_groups) == _lib.FBX_ERR_BAD_ARG and not h.value
    pdes = tc.process_case_design("2q-sic")
    mixed = np.arange(pdes.m, dtype=np.int32); mixed[15] = 0; mixed[mixed > 15] -= 1
    assert lib.fbx_grouping_create(pdes.handle, pdes.m - 1, _lib.iptr(mixed), ctypes.byref(h)) == _lib.FBX_ERR_BAD_ARG
    assert b"input state" in lib.fbx_last_error()
    assert create(ok, 9) == _lib.FBX_OK and h.value
    assert lib.fbx_grouping_destroy(h) == _lib.FBX_OK and lib.fbx_grouping_destroy(None) == _lib.FBX_OK


# ------------------------------------------------------------------------------------------------ 8. a guard without the restatement
def z_bound(cells):
    """the smallest z* with cells x erfc(z* / sqrt 2) <= 1e-6, by bisection"""
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if cells * math.erfc(mid / math.sqrt(2.0)) <= 1e-6 else (mid, hi)
    return hi


def cell_z_scores(hist, p, shots):
    """the z-score (tc.z_score) of every histogram cell with N p >= 5, and their number"""
    keep = shots * p >= 5.0
    z = np.array([tc.z_score(k, q, shots) for k, q in zip(hist[keep], p[keep])])
    return z, int(keep.sum())


@pytest.mark.parametrize("case", ALL_CASES)
def test_histogram_cells_follow_their_probabilities(gpu, case):
    """(confirmed on the CPU for this seed with the restatement on dense float64 distributions before the first GPU run)"""
    _, _, _, _, p, hist = device(case, False, 1000)
    z, cells = cell_z_scores(hist.astype(np.int64), p, 1000)
    bound = z_bound(cells)
    print(f"{case}: {cells} cells, worst |z| {np.abs(z).max():.3f}, bound {bound:.3f}")
    assert cells >= 30 and np.all(np.abs(z) <= bound)


# ------------------------------------------------------------------------------------------------ 9. consumers
def test_resident_loop_equals_the_composed_calls(gpu):
    from fbx import distance_measures as dm, tomography as t
    from fbx.operator_tools.superoperator_transformations import convert_batch
    des, us = design_of("2q-pauli"), tc.unitaries(2, 8)
    g = grouping_of("2q-pauli")
    flips = sc.asymmetric_flips(2, 8, seed=9) * 0.125
    kw = dict(rep="unitary", readout_flip=flips, seed=SEED, first_item=FIRST, groups=g)
    choi, fid = t.simulate_and_estimate_process_batch(des, us, 1000, **kw)
    e, c = t.simulate_grouped_process_tomography_batch(des, us, 1000, **kw)
    want = t.pgdb_process_estimate_batch(des, e, c)
    truth = convert_batch("kraus", "pauli_liouville", us[:, None]).real.astype(np.complex128)
    want_fid = dm.process_fidelity_batch(truth, convert_batch("choi", "pauli_liouville", want))
    assert np.array_equal(choi, want) and np.array_equal(fid, want_fid)
    assert np.all((fid > 0.5) & (fid <= 1.0 + 1e-9))
    ungrouped, _ = t.simulate_and_estimate_process_batch(des, us, 1000, **{**kw, "groups": None})
    assert not np.array_equal(ungrouped, choi)


@pytest.mark.parametrize("n", (1, 2))
def test_grouped_results_feed_the_reference_signature_estimators(gpu, n):
    from fbx import tomography as t
    qubits = list(range(n))
    u = tc.unitaries(n, 1)[0]
    flips = np.full((n, 2), 0.01)
    res = t.simulate_tomography_results(qubits, "process", u, 2000, rep="unitary", seed=SEED, readout_flip=flips,
                                        group_tpb_settings=True)
    settings = t.generate_process_tomography_settings(qubits)
    assert [r.setting for r in res] == settings and all(r.total_counts == 2000 for r in res)
    des = t.process_design(n)
    e, c, se = t.simulate_grouped_process_tomography_batch(des, u, 2000, rep="unitary", seed=SEED, readout_flip=flips,
                                                           return_std_errs=True)
    assert [r.expectation for r in res] == e[0].tolist() and [r.std_err for r in res] == se[0].tolist()
    plain = t.simulate_tomography_results(qubits, "process", u, 2000, rep="unitary", seed=SEED, readout_flip=flips)
    assert [r.expectation for r in plain] != [r.expectation for r in res]       # (the default is still the ungrouped stream)
    choi = t.pgdb_process_estimate(res, qubits)
    assert choi.shape == (4 ** n, 4 ** n) and np.all(np.isfinite(choi)) and np.allclose(choi, choi.conj().T)
    psi = u[:, :1]
    sres = t.simulate_tomography_results(qubits, "state", psi @ psi.conj().T, 2000, seed=SEED, group_tpb_settings=True)
    rho = t.linear_inv_state_estimate(sres, qubits)
    assert rho.shape == (2 ** n, 2 ** n) and np.real(psi.conj().T @ rho @ psi)[0, 0] > 0.9
