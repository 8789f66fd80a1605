"""fbx_tomo_simulate_symmetrized and fbx_tomo_simulate_calibration on the GPU (include/fbx.h): the per-pattern distributions
against a dense longdouble computation under a correlated confusion matrix, the link to fbx_tomo_simulate_grouped, histograms /
expectations / counts bit for bit against the host restatements, the calibration call, the identities that symmetrization plus
calibration do and do not satisfy, the stream's dependence on (seed, item, unit, pattern, shot) only, poisoned items, refusals
through the C ABI, a guard on the sampler that does not use the restatement, the consumers and the `_dev` forms.

The kernel has ONE form for every number of qubits (csrc/fbx_tomo_sim_symm.hip: a wavefront per unit, threshold search, private
LDS counters); what varies with the case is the number of patterns per pass (64 / 2^n), the number of passes and how (pattern,
block) pairs fall on the lanes, which the shot counts below spread over: per-pattern s = 1, 3, 4, 5 and 257 for the full-weight
groups of every case, with tail blocks, and s on both sides of 256."""
import ctypes
import functools

import numpy as np
import pytest

import sampling_cases as sc
import tomo_sim_cases as tc
import tomo_sim_symm_cases as ss
from tomo_sim_cases import B, FIRST, SEED
from tomo_sim_symm_cases import ALL_CASES, design_of, grouping_of

pytestmark = pytest.mark.gpu


def confusion_of(case, kind):
    n = design_of(case).n_qubits
    return ss.correlated_confusion(n) if kind == "correlated" else ss.product_confusion(n)


def simulate(case, shots, confusion, symm_type, **kw):
    from fbx import tomography as t
    des = design_of(case)
    kw.setdefault("groups", grouping_of(case))
    if case.startswith("state"):
        return t.simulate_symmetrized_state_tomography_batch(des, kw.pop("truth", tc.mixed_states(des.n_qubits)), shots, confusion,
                                                             symm_type, **kw)
    return t.simulate_symmetrized_process_tomography_batch(des, kw.pop("truth", tc.damped_kraus(des.n_qubits)), shots, confusion,
                                                           symm_type, rep=kw.pop("rep", "kraus"), **kw)


ALL_OUT = dict(return_std_errs=True, return_exact=True, return_probabilities=True, return_histograms=True)


@functools.lru_cache(maxsize=None)
def device(case, kind="correlated", symm_type=-1, shots=1000):
    """(expectations, counts, std_errs, exact, probabilities, histograms) of the B-item call that the tests share"""
    out = simulate(case, shots, confusion_of(case, kind), symm_type, seed=SEED, first_item=FIRST, **ALL_OUT)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def host(case, kind, symm_type, shots):
    """the restatement from the device's distributions, of the first guard_items items"""
    from fbx import synthetic
    des = design_of(case)
    nb = ss.guard_items(des.n_qubits)
    return synthetic.restate_symmetrized_tomography_counts(device(case, kind, symm_type, shots)[4][:nb], grouping_of(case), des.paulis,
                                                           des.coefs, shots, symm_type, SEED, FIRST)


def group_counts(case, symm_type, shots):
    """N of every setting: floor(shots / patterns) x patterns of its group"""
    g = grouping_of(case)
    pats = np.array([1 << bin(u).count("1") if symm_type == -1 else 1 for u in ss.unions_of(case)])
    return ((shots // pats) * pats)[g.group_of].astype(np.float64)


def check_counts(got, want, counts):
    """histograms, expectations and counts bit for bit; std_err within 8 x 2^-53 relative of the integer formula, 0 at the ends"""
    we, wc, ws, whist = want
    nb = we.shape[0]
    e, c, s, _, _, hist = [a[:nb] for a in got]
    assert hist.dtype == np.uint32 and np.array_equal(hist, whist)
    bad = np.argwhere(e != we)
    assert bad.size == 0, f"{len(bad)} expectations differ, first at (item, setting) {bad[0].tolist()}: {e[tuple(bad[0])]!r} != {we[tuple(bad[0])]!r}"
    assert np.array_equal(c, wc) and np.array_equal(got[1], np.broadcast_to(counts, got[1].shape))
    rel = np.abs(s - ws) / np.where(ws > 0, ws, 1.0)
    print(f"std_err: worst relative excursion {rel.max() / 2.0 ** -53:.2f} x 2^-53")
    assert np.all(rel <= 8 * 2.0 ** -53)
    assert np.all(s[ws == 0.0] == 0.0)


# ------------------------------------------------------------------------------------------------ 1. the distributions
@pytest.mark.parametrize("symm_type", (-1, 0))
@pytest.mark.parametrize("case", ALL_CASES)
def test_distributions_against_dense_longdouble(gpu, case, symm_type):
    """tolerance (2 x 64 dim^2 + 2 dim) 2^-53 per probability: the grouped test's bound for p (ss.tolerance) plus dim fma roundings
    of a convex sum of numbers <= 1"""
    des, unions = design_of(case), ss.unions_of(case)
    n, d = des.n_qubits, des.dim
    conf = confusion_of(case, "correlated")
    if n > 1:
        assert min(ss.distance_from_products(c) for c in conf) > 0.01          # no tensor product: the matrix is correlated
    assert np.abs(conf - np.swapaxes(conf, 1, 2)).max() > 0.01                 # ... and asymmetric
    tol = ss.tolerance(des)
    got, want = device(case, "correlated", symm_type)[4], ss.dense_patterns(ss.ideal(case), conf, unions, symm_type)
    assert got.shape == want.shape == (B, grouping_of(case).n_groups, d, d)
    worst = float(np.abs(got - want).max()) / tol
    print(f"{case} symm_type={symm_type}: worst excursion {worst:.4f} of the tolerance")
    assert worst <= 1.0
    for g, u in enumerate(unions):
        pats = ss.patterns_of(u, symm_type, n)
        rest = [f for f in range(d) if f not in pats]
        assert not got[:, g, rest].any()                                       # exact zeros for masks that are no pattern
        assert np.abs(got[:, g, pats].sum(axis=2) - 1.0).max() <= tol * d
    assert float(np.ptp(want[:, :, 0])) > 0.25 / d


# ------------------------------------------------------------------------------------------------ 2. the link to the grouped call
@pytest.mark.parametrize("case", ALL_CASES)
def test_product_matrix_without_symmetrization_is_the_grouped_call(gpu, case):
    from fbx import readout, synthetic, tomography as t
    des, g = design_of(case), grouping_of(case)
    flips = sc.asymmetric_flips(des.n_qubits, B, seed=5)
    conf = readout.confusion_from_flips(flips)
    prob = simulate(case, 1000, conf, 0, seed=SEED, first_item=FIRST, return_probabilities=True)[2]
    if case.startswith("state"):
        grouped = t.simulate_grouped_state_tomography_batch(des, tc.mixed_states(des.n_qubits), 1000, groups=g, readout_flip=flips,
                                                            seed=SEED, first_item=FIRST, **ALL_OUT)
        plain = t.simulate_state_tomography_batch(des, tc.mixed_states(des.n_qubits), 1000, readout_flip=flips, seed=SEED,
                                                  first_item=FIRST, return_exact=True)[2]
    else:
        grouped = t.simulate_grouped_process_tomography_batch(des, tc.damped_kraus(des.n_qubits), 1000, groups=g, rep="kraus",
                                                              readout_flip=flips, seed=SEED, first_item=FIRST, **ALL_OUT)
        plain = t.simulate_process_tomography_batch(des, tc.damped_kraus(des.n_qubits), 1000, rep="kraus", readout_flip=flips,
                                                    seed=SEED, first_item=FIRST, return_exact=True)[2]
    worst = float(np.abs(prob[:, :, 0, :] - grouped[4]).max()) / ss.tolerance(des)
    print(f"{case}: worst excursion {worst:.4f} of the tolerance")
    assert worst <= 1.0 and not prob[:, :, 1:, :].any()
    # the grouped call itself is what it was: its stream restated from its own distributions, its exact means those of the ungrouped call
    we, wc, ws, whist = synthetic.restate_grouped_tomography_counts(grouped[4], g, des.paulis, des.coefs, 1000, SEED, FIRST)
    assert np.array_equal(grouped[0], we) and np.array_equal(grouped[1], wc) and np.array_equal(grouped[5], whist)
    assert np.array_equal(grouped[3], plain)


# ------------------------------------------------------------------------------------------------ 3. counts bit for bit
def shot_counts(n):
    """total shots that give the full-weight groups (2^n patterns) s = 1, 3 (+ a remainder), 4, 5 (+ a remainder), 257 (+ a
    remainder) and, with 1000, s < 256 for n >= 2; lower-weight groups of the same call see other s"""
    P = 1 << n
    return (P, 3 * P + 1, 4 * P, 5 * P + 1, 257 * P + 1, 1000)


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("case", ALL_CASES)
def test_counts_bit_for_bit(gpu, case, which):
    n = design_of(case).n_qubits
    shots = shot_counts(n)[which]
    full = [shots // (1 << n) for u in ss.unions_of(case) if u == (1 << n) - 1]
    assert full and full[0] == (1, 3, 4, 5, 257, 1000 >> n)[which]            # (every case has a full-weight group)
    check_counts(device(case, "correlated", -1, shots), host(case, "correlated", -1, shots), group_counts(case, -1, shots))
    if which == 5:
        assert len(np.unique(host(case, "correlated", -1, shots)[3])) > 10      # (counts that vary: the comparison is not of constants)


@pytest.mark.parametrize("shots", (1, 5, 257, 1000))
@pytest.mark.parametrize("case", ALL_CASES)
def test_counts_bit_for_bit_without_symmetrization(gpu, case, shots):
    check_counts(device(case, "correlated", 0, shots), host(case, "correlated", 0, shots), group_counts(case, 0, shots))
    assert np.all(device(case, "correlated", 0, shots)[1] == float(shots))


def test_counts_differ_between_the_groups_of_one_call(gpu):
    """43 shots on three qubits: unions of weight 3 and 2 draw 5 x 8 = 10 x 4 = 40, unions of weight 1 draw 21 x 2 = 42"""
    counts = device("3q-shuffled", "correlated", -1, 43)[1]
    want = group_counts("3q-shuffled", -1, 43)
    assert np.array_equal(counts, np.broadcast_to(want, counts.shape)) and len(np.unique(want)) > 1 and want.max() <= 43


# ------------------------------------------------------------------------------------------------ 4. the calibration
def calibration(case, kind, symm_type, shots, **kw):
    from fbx import tomography as t
    return t.simulate_readout_calibration_batch(design_of(case), confusion_of(case, kind), shots, symm_type, seed=SEED,
                                                first_item=FIRST, **kw)


def first_appearance(paulis):
    seen, index = {}, []
    for row in paulis:
        key = tuple(int(x) for x in row)
        if key not in seen:
            seen[key] = len(seen)
        index.append(seen[key])
    return np.array(list(seen), dtype=np.uint8).reshape(len(seen), paulis.shape[1]), np.array(index, dtype=np.int32)


def dense_cal_exact(conf, cal_paulis, symm_type):
    """[B, n_cal] longdouble: the mean parity on z_c of r with q_f(r) = C[f][r ^ f], averaged over the patterns"""
    n = cal_paulis.shape[1]
    d = 1 << n
    idx = np.arange(d)
    c = conf.astype(np.longdouble)
    z = ss.masks_of(cal_paulis)
    out = np.zeros((conf.shape[0], len(z)), dtype=np.longdouble)
    for k, zc in enumerate(z):
        sign = np.array([1 - 2 * (bin(int(r) & int(zc)).count("1") & 1) for r in idx], dtype=np.longdouble)
        pats = ss.patterns_of(int(zc), symm_type, n)
        for f in pats:
            out[:, k] += c[:, f, idx ^ f] @ sign
        out[:, k] /= len(pats)
    return out


@pytest.mark.parametrize("symm_type", (-1, 0))
@pytest.mark.parametrize("case", ALL_CASES)
def test_calibration(gpu, case, symm_type):
    from fbx import synthetic, tomography as t
    des = design_of(case)
    n = des.n_qubits
    want_paulis, want_index = first_appearance(des.paulis)
    cal_paulis, cal_index = t.calibration_list(des)
    assert np.array_equal(cal_paulis, want_paulis) and np.array_equal(cal_index, want_index) and cal_index.dtype == np.int32
    conf = confusion_of(case, "correlated")
    nb = ss.guard_items(n) if n < 5 else 1
    for shots in ((1 << n) * 5 + 1, 1000):
        mean, var, cnt, index, exact = calibration(case, "correlated", symm_type, shots, return_exact=True)
        assert np.array_equal(index, want_index) and mean.shape == (B, len(want_paulis))
        wm, wv, wc, _ = synthetic.restate_readout_calibration_counts(conf[:nb], cal_paulis, shots, symm_type, SEED, FIRST)
        assert np.array_equal(mean[:nb], wm) and np.array_equal(var[:nb], wv) and np.array_equal(cnt[:nb], wc)
        pats = np.array([1 << bin(int(z)).count("1") if symm_type == -1 else 1 for z in ss.masks_of(cal_paulis)])
        assert np.array_equal(cnt, np.broadcast_to(((shots // pats) * pats).astype(float), cnt.shape))
    dense = dense_cal_exact(conf, cal_paulis, symm_type)
    worst = float(np.abs(exact - dense).max()) / ss.tolerance(des)
    print(f"{case} symm_type={symm_type}: cal_exact worst excursion {worst:.4f} of the tolerance")
    assert worst <= 1.0 and np.all(np.abs(mean - exact) < 0.25) and np.ptp(exact) > 1e-3


def test_calibration_of_an_identity_observable_has_no_run(gpu):
    from fbx import tomography as t
    des, at = tc.with_identity_observable(1)
    cal_paulis, cal_index = t.calibration_list(des)
    assert cal_index[at] == -1 and np.array_equal(np.delete(cal_index, at), first_appearance(np.delete(des.paulis, at, axis=0))[1])
    assert cal_paulis.shape == (3, 1) and np.all(cal_paulis != 0)


# ------------------------------------------------------------------------------------------------ 5. exact identities
def ideal_exact(case):
    """return_exact of the ungrouped call without flips: coef x tr[P .]"""
    from fbx import tomography as t
    des = design_of(case)
    if case.startswith("state"):
        return t.simulate_state_tomography_batch(des, tc.mixed_states(des.n_qubits), 1000, seed=SEED, first_item=FIRST, return_exact=True)[2]
    return t.simulate_process_tomography_batch(des, tc.damped_kraus(des.n_qubits), 1000, rep="kraus", seed=SEED, first_item=FIRST,
                                               return_exact=True)[2]


@pytest.mark.parametrize("case", ALL_CASES)
def test_what_symmetrization_and_calibration_undo(gpu, case):
    """exact == cal_exact[cal_index] x ideal, within 2^n x the tolerance of test 1 (x |coef|): for a tensor-product matrix under
    exhaustive symmetrization, for every member; for the correlated matrix, for the members that act on all n qubits (the group's
    flips and the calibration's are then the same set); NOT for some lower-weight member under the correlated matrix -- the
    calibration flips only the member's qubits while the group flips its union, and the crosstalk from the others stays: the bias
    the reference has too; and NOT without symmetrization under asymmetric flips, which is the bias symmetrization removes."""
    des = design_of(case)
    n = des.n_qubits
    tol = (1 << n) * ss.tolerance(des) * np.abs(des.coefs)[None, :]
    ideal = ideal_exact(case)
    weight = (des.paulis != 0).sum(axis=1)

    def excess(kind, symm_type):
        exact = device(case, kind, symm_type)[3]
        cal_exact, index = calibration(case, kind, symm_type, 1000, return_exact=True)[4], t_index
        return np.abs(exact - cal_exact[:, index] * ideal) / tol
    from fbx import tomography as t
    t_index = t.calibration_list(des)[1]
    product = excess("product", -1)
    print(f"{case}: product matrix, worst {product.max():.4f} of the tolerance")
    assert product.max() <= 1.0
    correlated = excess("correlated", -1)
    print(f"{case}: correlated matrix, full weight worst {correlated[:, weight == n].max():.4f}, "
          f"lower weight worst {correlated[:, weight < n].max() if n > 1 else 0.0:.1f} of the tolerance")
    assert correlated[:, weight == n].max() <= 1.0
    if n > 1:
        assert correlated[:, weight < n].max() > 100.0
    raw = excess("product", 0)
    assert raw.max() > 100.0


# ------------------------------------------------------------------------------------------------ 6. the stream
def test_a_value_depends_on_seed_item_unit_pattern_and_shot_only(gpu):
    case = "2q-sic"
    conf, full = confusion_of(case, "correlated"), device(case)
    kw = dict(seed=SEED, **ALL_OUT)
    kraus = tc.damped_kraus(2)
    head = simulate(case, 1000, conf[:2], -1, truth=kraus[:2], first_item=FIRST, **kw)
    tail = simulate(case, 1000, conf[2:], -1, truth=kraus[2:], first_item=FIRST + 2, **kw)
    one = simulate(case, 1000, conf[3], -1, truth=kraus[3:4], first_item=FIRST + 3, **kw)        # (one matrix for the batch)
    for a, hd, tl, o in zip(full, head, tail, one):
        assert np.array_equal(a[:2], hd) and np.array_equal(a[2:], tl) and np.array_equal(a[3:4], o)
    other = simulate(case, 1000, conf, -1, first_item=FIRST, **{**kw, "seed": SEED + 1})
    assert np.array_equal(other[3], full[3]) and np.array_equal(other[4], full[4])
    assert (other[5] != full[5]).mean() > 0.3 and (other[0] != full[0]).mean() > 0.5
    # the calibration likewise
    cal = calibration(case, "correlated", -1, 1000, return_exact=True)
    from fbx import tomography as t
    des = design_of(case)
    part = t.simulate_readout_calibration_batch(des, conf[2:], 1000, -1, seed=SEED, first_item=FIRST + 2, return_exact=True)
    single = t.simulate_readout_calibration_batch(des, conf[3], 1000, -1, seed=SEED, first_item=FIRST + 3, return_exact=True)
    reseeded = t.simulate_readout_calibration_batch(des, conf, 1000, -1, seed=SEED + 1, first_item=FIRST, return_exact=True)
    for a, p, o in zip((cal[0], cal[1], cal[2], cal[4]), (part[0], part[1], part[2], part[4]), (single[0], single[1], single[2], single[4])):
        assert np.array_equal(a[2:], p) and np.array_equal(a[3:4], o)
    assert np.array_equal(reseeded[4], cal[4]) and (reseeded[0] != cal[0]).mean() > 0.5
    # a group_of array and the method name give what the Grouping gives
    by_array = simulate(case, 1000, conf, -1, groups=grouping_of(case).group_of, first_item=FIRST, **kw)
    by_name = simulate(case, 1000, conf, -1, groups="greedy", first_item=FIRST, **kw)
    for a, x, y in zip(full, by_array, by_name):
        assert np.array_equal(a, x) and np.array_equal(a, y)


def test_deterministic_matrices_on_the_device(gpu):
    """the known answers of the CPU test, by the kernel: every bit read inverted on |0...0> in the all-Z group (n = 1..5), and
    the one-way flip that symmetrization turns into an exact 0"""
    from fbx import tomography as t
    from fbx.design import Grouping, state_design
    for n in (1, 2, 3, 4, 5):
        des, d = state_design(n), 1 << n
        zs = [k for k in range(des.m) if np.all((des.paulis[k] == 0) | (des.paulis[k] == 3))]
        rest = [k for k in range(des.m) if k not in zs]
        g = Grouping.from_groups(des, [zs] + [[k] for k in rest])
        rho = np.zeros((B, d, d), dtype=complex); rho[:, 0, 0] = 1.0
        for symm_type in (-1, 0):
            e, c, s, h = t.simulate_symmetrized_state_tomography_batch(des, rho, 37, np.eye(d)[::-1], symm_type, groups=g, seed=SEED,
                                                                       first_item=FIRST, return_std_errs=True, return_histograms=True)
            N = (37 // d) * d if symm_type == -1 else 37
            weight = (des.paulis[zs] != 0).sum(axis=1)
            assert np.array_equal(e[:, zs], np.broadcast_to((-1.0) ** weight, (B, len(zs)))) and np.all(s[:, zs] == 0.0)
            assert np.all(h[:, 0, -1] == N) and np.all(h[:, 0, :-1] == 0) and np.all(c[:, zs] == N)
    des = state_design(1)
    rho = np.zeros((B, 2, 2), dtype=complex); rho[:, 0, 0] = 1.0
    conf = np.array([[0.0, 1.0], [0.0, 1.0]])
    Z = 2
    e0 = t.simulate_symmetrized_state_tomography_batch(des, rho, 36, conf, 0, seed=SEED)[0]
    e1, _, h1 = t.simulate_symmetrized_state_tomography_batch(des, rho, 36, conf, -1, seed=SEED, return_histograms=True)
    assert np.all(e0[:, Z] == -1.0) and np.all(e1[:, Z] == 0.0) and np.all(h1[:, grouping_of("state-1").group_of[Z]] == 18)
    mean = t.simulate_readout_calibration_batch(des, conf, 36, -1, seed=SEED, batch=B)[0]
    assert mean.shape == (B, 3) and np.all(mean[:, Z] == 0.0)


# ------------------------------------------------------------------------------------------------ 7. poison
@pytest.mark.parametrize("what", ("nan-truth", "confusion-1.5", "nan-confusion", "overflowing-group"))
def test_poisoned_item(gpu, what):
    """the grouped test's cases, with the confusion matrix in the place of the flips.  The entry of 1.5 is balanced by one of -0.5
    so that the row still sums to 1 and the Python layer lets it through; the NaN row has no finite sum and goes through as well."""
    from fbx import tomography as t
    des, bad, shots = design_of("state-2"), 3, 257
    g = grouping_of("state-2")
    rho = tc.mixed_states(2).copy()
    conf = ss.correlated_confusion(2).copy()
    kw = dict(groups=g, seed=SEED, first_item=FIRST, **ALL_OUT)
    clean = t.simulate_symmetrized_state_tomography_batch(des, rho, shots, conf, -1, **kw)
    if what == "nan-truth":
        rho[bad, 1, 2] = complex(np.nan, 0.0)
    elif what == "confusion-1.5":
        conf[bad, 2] = [1.5, -0.5, 0.0, 0.0]
    elif what == "nan-confusion":
        conf[bad, 1, 3] = np.nan
    else:
        rho[bad] = np.diag([1.5e308, 0.0, 0.0, 0.0])
    *got, status = t.simulate_symmetrized_state_tomography_batch(des, rho, shots, conf, -1, return_status=True, **kw)
    good = [b for b in range(B) if b != bad]
    assert status.tolist() == [int(b == bad) for b in range(B)]
    e, c, s, x, p, h = got
    assert np.all(np.isnan(e[bad])) and np.all(np.isnan(s[bad])) and np.all(np.isnan(x[bad])) and np.all(np.isnan(p[bad]))
    assert np.array_equal(c[bad], group_counts("state-2", -1, shots)) and np.all(h[bad] == 0)
    for a, b in zip(got, clean):
        assert np.array_equal(a[good], b[good])
    with pytest.raises(ValueError, match="item 3"):
        t.simulate_symmetrized_state_tomography_batch(des, rho, shots, conf, -1, **kw)
    if "confusion" in what:
        cal_clean = t.simulate_readout_calibration_batch(des, ss.correlated_confusion(2), shots, -1, seed=SEED, first_item=FIRST,
                                                         return_exact=True)
        *cal, cal_status = t.simulate_readout_calibration_batch(des, conf, shots, -1, seed=SEED, first_item=FIRST, return_exact=True,
                                                                return_status=True)
        assert cal_status.tolist() == status.tolist()
        for i in (0, 1, 4):
            assert np.all(np.isnan(cal[i][bad])) and np.array_equal(cal[i][good], cal_clean[i][good])
        assert np.array_equal(cal[2], cal_clean[2])
        with pytest.raises(ValueError, match="item 3"):
            t.simulate_readout_calibration_batch(des, conf, shots, -1, seed=SEED, first_item=FIRST)


def test_rows_that_do_not_sum_to_one_are_refused_in_python(gpu):
    from fbx import tomography as t
    des = design_of("state-2")
    conf = ss.correlated_confusion(2).copy()
    conf[1, 2, 0] += 0.01
    with pytest.raises(ValueError, match="sum to 1"):
        t.simulate_symmetrized_state_tomography_batch(des, tc.mixed_states(2), 100, conf, -1, seed=SEED)
    with pytest.raises(ValueError, match="sum to 1"):
        t.simulate_readout_calibration_batch(des, conf, 100, -1, seed=SEED)
    with pytest.raises(ValueError, match="confusion must be"):
        t.simulate_symmetrized_state_tomography_batch(des, tc.mixed_states(2), 100, np.eye(8), -1, seed=SEED)
    for symm_type in (1, 2, 3):
        with pytest.raises(ValueError, match="orthogonal"):
            t.simulate_symmetrized_state_tomography_batch(des, tc.mixed_states(2), 100, np.eye(4), symm_type, seed=SEED)
    with pytest.raises(ValueError, match="flip patterns"):
        t.simulate_symmetrized_state_tomography_batch(des, tc.mixed_states(2), 3, np.eye(4), -1, seed=SEED)


# ------------------------------------------------------------------------------------------------ 8. bad arguments
def test_bad_arguments(gpu):
    from fbx import _lib
    from fbx.design import state_design
    des, other = design_of("1q-pauli"), state_design(1)
    g = grouping_of("1q-pauli")
    lib, m = _lib.lib(), des.m
    ptm = np.ascontiguousarray(np.broadcast_to(np.eye(4), (B, 4, 4)))
    conf = np.ascontiguousarray(np.broadcast_to(np.array([[0.9, 0.1], [0.2, 0.8]]), (B, 2, 2)))
    out = [np.full((B, m), -7.0) for _ in range(4)] + [np.full((B, g.n_groups, 2, 2), -7.0)]
    hist = np.full((B, g.n_groups, 2), 7, dtype=np.uint32)
    st = np.full(B, -7, dtype=np.int32)

    def call(design=des.handle, grouping=g.handle, batch=B, truth=ptm, confusion=conf, symm=-1, shots=37, first=FIRST,
             outs=(0, 1, 2, 3, 4, 5)):
        ptrs = [_lib.dptr(out[i]) if i in outs else None for i in range(5)] + [_lib.ptr(hist, ctypes.c_uint32) if 5 in outs else None]
        return lib.fbx_tomo_simulate_symmetrized(design, grouping, batch, _lib.dptr(truth), _lib.dptr(confusion), symm, shots, SEED,
                                                 first, *ptrs, _lib.iptr(st))
    for kw in (dict(batch=-1), dict(shots=-1), dict(shots=2 ** 32), dict(first=-1), dict(truth=None), dict(confusion=None),
               dict(outs=()), dict(shots=0), dict(shots=0, outs=(3, 5)), dict(design=None), dict(grouping=None),
               dict(design=other.handle), dict(symm=-2), dict(symm=4), dict(shots=1), dict(shots=2 ** 30), dict(shots=2 ** 29, symm=0)):
        assert call(**kw) == _lib.FBX_ERR_BAD_ARG, kw
        assert lib.fbx_last_error()
    for symm in (1, 2, 3):
        assert call(symm=symm) == _lib.FBX_ERR_UNSUPPORTED and b"orthogonal" in lib.fbx_last_error()
    assert all(np.all(o == -7.0) for o in out) and np.all(hist == 7) and np.all(st == -7)     # refused before any buffer was touched
    assert call(batch=0) == _lib.FBX_OK and all(np.all(o == -7.0) for o in out)
    assert call(shots=0, outs=(3, 4)) == _lib.FBX_OK and np.all(out[0] == -7.0) and np.all(st == 0)
    assert np.allclose(out[4].sum(axis=3), 1.0) and np.all(np.abs(out[3]) <= 1.0)
    assert call(outs=(5,)) == _lib.FBX_OK and np.all(hist.sum(axis=2) == 36) and np.all(out[1] == -7.0)
    assert call(outs=(5,), shots=2 ** 29 - 1, symm=0, batch=1) == _lib.FBX_OK and np.all(hist[0].sum(axis=1) == 2 ** 29 - 1)
    # the calibration call
    cal = [np.full((B, 3), -7.0) for _ in range(4)]
    st[:] = -7

    def ccall(design=des.handle, batch=B, confusion=conf, symm=-1, shots=37, first=FIRST, outs=(0, 1, 2, 3)):
        ptrs = [_lib.dptr(cal[i]) if i in outs else None for i in range(4)]
        return lib.fbx_tomo_simulate_calibration(design, batch, _lib.dptr(confusion), symm, shots, SEED, first, *ptrs, _lib.iptr(st))
    for kw in (dict(batch=-1), dict(shots=-1), dict(shots=2 ** 32), dict(first=-1), dict(confusion=None), dict(outs=()), dict(shots=0),
               dict(design=None), dict(symm=-2), dict(symm=4), dict(shots=1), dict(shots=2 ** 30)):
        assert ccall(**kw) == _lib.FBX_ERR_BAD_ARG, kw
    for symm in (1, 2, 3):
        assert ccall(symm=symm) == _lib.FBX_ERR_UNSUPPORTED
    assert all(np.all(o == -7.0) for o in cal) and np.all(st == -7)
    assert ccall(batch=0) == _lib.FBX_OK and all(np.all(o == -7.0) for o in cal)
    assert ccall(shots=0, outs=(2,)) == _lib.FBX_OK and np.allclose(cal[2], 0.7) and np.all(cal[0] == -7.0)      # 1 - 0.1 - 0.2, symmetrized
    assert ccall() == _lib.FBX_OK and np.all(cal[3] == 36.0) and np.all(st == 0)
    n_cal = ctypes.c_int32(-1)
    assert lib.fbx_tomo_calibration_list(None, ctypes.byref(n_cal), None, None) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_tomo_calibration_list(des.handle, None, None, None) == _lib.FBX_ERR_BAD_ARG
    assert lib.fbx_tomo_calibration_list(des.handle, ctypes.byref(n_cal), None, None) == _lib.FBX_OK and n_cal.value == 3


# ------------------------------------------------------------------------------------------------ 9. a guard without the restatement
@pytest.mark.parametrize("case", ALL_CASES)
def test_merged_cells_follow_their_probabilities(gpu, case):
    """z-scores of the merged histogram cells with N qbar >= 5 against the grouped test's bound, 1000 shots per pattern set at seed
    SEED.  The variance used, N qbar (1 - qbar), is that of N draws from the mean distribution and is at least the true one (the
    cell is a sum of binomials with different q_f), so the bound is no tighter than it should be.  (Confirmed on the CPU for this
    seed, these cases and these items with the restatement on dense float64 distributions before the first GPU run:
    tests/test_tomo_sim_symm_cpu.py::test_restatement_alone_stays_inside_the_z_bound.)"""
    nb = ss.guard_items(design_of(case).n_qubits)
    _, c, _, _, p, hist = device(case, "correlated", -1, 1000)
    unions = ss.unions_of(case)
    pats = np.array([1 << bin(u).count("1") for u in unions], dtype=np.float64)
    qbar = p[:nb].sum(axis=2) / pats[None, :, None]
    per_group = (1000 // pats) * pats
    z, cells = ss.cell_z_scores(hist[:nb].astype(np.int64), qbar, per_group[None, :, None])
    bound = ss.z_bound(cells)
    print(f"{case}: {cells} cells, worst |z| {np.abs(z).max():.3f}, bound {bound:.3f}")
    assert cells >= 30 and np.all(np.abs(z) <= bound)


# ------------------------------------------------------------------------------------------------ 10. consumers
def flips_5_10(n, batch):
    return np.broadcast_to(np.array([0.05, 0.10]), (batch, n, 2))


def test_resident_loop_equals_the_composed_calls(gpu):
    from fbx import distance_measures as dm, observable_estimation as oe, readout, tomography as t
    from fbx.operator_tools.superoperator_transformations import convert_batch
    des, us = design_of("2q-pauli"), tc.unitaries(2, 8)
    g = grouping_of("2q-pauli")
    truth = convert_batch("kraus", "pauli_liouville", us[:, None]).real.astype(np.complex128)
    for conf in (ss.correlated_confusion(2, 8), readout.confusion_from_flips(flips_5_10(2, 8))):
        kw = dict(rep="unitary", seed=SEED, first_item=FIRST, groups=g)
        choi, fid = t.simulate_and_estimate_process_batch(des, us, 1000, confusion=conf, **kw)
        e, c, se = t.simulate_symmetrized_process_tomography_batch(des, us, 1000, conf, -1, return_std_errs=True, **kw)
        cm, cv, cc, ci = t.simulate_readout_calibration_batch(des, conf, 1000, -1, seed=SEED, first_item=FIRST)
        flat = (np.arange(8)[:, None] * cm.shape[1] + ci[None, :]).reshape(-1)
        e2, se2 = oe.calibrate_expectations_batch(e.reshape(1, -1), se.reshape(1, -1), cm.reshape(-1), cv.reshape(-1), flat)
        want = t.pgdb_process_estimate_batch(des, e2.reshape(e.shape), c)
        want_fid = dm.process_fidelity_batch(truth, convert_batch("choi", "pauli_liouville", want))
        assert np.array_equal(choi, want) and np.array_equal(fid, want_fid)
        assert np.array_equal(e2.reshape(e.shape), e / cm[:, ci])
        # without the calibration, and without either: the composed calls again
        choi_s, fid_s = t.simulate_and_estimate_process_batch(des, us, 1000, confusion=conf, calibrate=False, **kw)
        assert np.array_equal(choi_s, t.pgdb_process_estimate_batch(des, e, c))
        choi_r, fid_r = t.simulate_and_estimate_process_batch(des, us, 1000, confusion=conf, symm_type=0, calibrate=False, **kw)
        e0, c0 = t.simulate_symmetrized_process_tomography_batch(des, us, 1000, conf, 0, **kw)
        assert np.array_equal(choi_r, t.pgdb_process_estimate_batch(des, e0, c0))
    # the tensor product of 5 % / 10 % flips: calibration recovers most of what the readout error costs
    print(f"fidelity to truth: raw {fid_r.mean():.4f}, symmetrized {fid_s.mean():.4f}, symmetrized and calibrated {fid.mean():.4f}")
    assert fid.mean() > fid_r.mean() and np.all((fid > 0.5) & (fid <= 1.0 + 1e-9))
    # without confusion nothing changed
    plain = t.simulate_and_estimate_process_batch(des, us, 1000, rep="unitary", seed=SEED, first_item=FIRST, groups=g)
    e, c = t.simulate_grouped_process_tomography_batch(des, us, 1000, rep="unitary", seed=SEED, first_item=FIRST, groups=g)
    assert np.array_equal(plain[0], t.pgdb_process_estimate_batch(des, e, c))


@pytest.mark.parametrize("n", (1, 2))
def test_calibrated_results_feed_the_reference_signature_estimators(gpu, n):
    from fbx import readout, tomography as t
    qubits = list(range(n))
    u = tc.unitaries(n, 1)[0]
    conf = readout.confusion_from_flips(flips_5_10(n, 1)[0])
    res = t.simulate_tomography_results(qubits, "process", u, 2000, rep="unitary", seed=SEED, confusion=conf, symm_type=-1,
                                        calibrate_observables=True, group_tpb_settings=True)
    settings = t.generate_process_tomography_settings(qubits)
    des = t.process_design(n)
    assert [r.setting for r in res] == settings
    e, c, se = t.simulate_symmetrized_process_tomography_batch(des, u, 2000, conf, -1, rep="unitary", seed=SEED, return_std_errs=True)
    cm, cv, cc, ci = t.simulate_readout_calibration_batch(des, conf, 2000, -1, seed=SEED)
    assert [r.raw_expectation for r in res] == e[0].tolist() and [r.raw_std_err for r in res] == se[0].tolist()
    assert [r.total_counts for r in res] == c[0].astype(int).tolist()
    assert [r.calibration_expectation for r in res] == cm[0, ci].tolist() and [r.calibration_counts for r in res] == cc[0, ci].astype(int).tolist()
    assert [r.calibration_std_err for r in res] == np.sqrt(cv[0, ci]).tolist()
    assert [r.expectation for r in res] == (e[0] / cm[0, ci]).tolist()
    assert all(0.6 < r.calibration_expectation < 0.9 for r in res)             # (1 - 0.15)^weight
    choi = t.pgdb_process_estimate(res, qubits)
    assert choi.shape == (4 ** n, 4 ** n) and np.all(np.isfinite(choi)) and np.allclose(choi, choi.conj().T)
    # the confusion matrix alone: the symmetrized stream, every setting a group of its own, no calibration fields
    alone = t.simulate_tomography_results(qubits, "process", u, 2000, rep="unitary", seed=SEED, confusion=conf)
    e0 = t.simulate_symmetrized_process_tomography_batch(des, u, 2000, conf, 0, groups=np.arange(des.m), rep="unitary", seed=SEED)[0]
    assert [r.expectation for r in alone] == e0[0].tolist() and all(r.raw_expectation is None for r in alone)
    # and the defaults are the streams of before
    plain = t.simulate_tomography_results(qubits, "process", u, 2000, rep="unitary", seed=SEED)
    assert [r.expectation for r in plain] == t.simulate_process_tomography_batch(des, u, 2000, rep="unitary", seed=SEED)[0][0].tolist()


# ------------------------------------------------------------------------------------------------ 11. the _dev forms
def test_dev_forms_on_device_buffers(gpu):
    from fbx import _lib
    from fbx.operator_tools.superoperator_transformations import convert_batch
    case = "2q-sic"
    des, g, conf, full = design_of(case), grouping_of(case), confusion_of(case, "correlated"), device(case)
    ptm = np.ascontiguousarray(convert_batch("kraus", "pauli_liouville", tc.damped_kraus(2)).real)
    DB, m, cells = _lib.DeviceBuffer, des.m, g.n_groups * 4
    d_t, d_c = DB.from_array(ptm), DB.from_array(conf)
    outs = [DB(B * m * 8) for _ in range(4)] + [DB(B * cells * 4 * 8), DB(B * cells * 4)]
    d_st = DB(B * 4)
    _lib.check(_lib.lib().fbx_tomo_simulate_symmetrized_dev(des.handle, g.handle, B, d_t.ptr, d_c.ptr, -1, 1000, SEED, FIRST,
                                                            *[o.ptr for o in outs], d_st.ptr))
    _lib.synchronize()
    for a, buf in zip(full, outs):
        assert np.array_equal(a, buf.to_array(a.dtype, a.shape))
    assert not d_st.to_array(np.int32, (B,)).any()
    mean, var, cnt, _, exact = calibration(case, "correlated", -1, 1000, return_exact=True)
    n_cal = mean.shape[1]
    couts = [DB(B * n_cal * 8) for _ in range(4)]
    _lib.check(_lib.lib().fbx_tomo_simulate_calibration_dev(des.handle, B, d_c.ptr, -1, 1000, SEED, FIRST, *[o.ptr for o in couts],
                                                            d_st.ptr))
    _lib.synchronize()
    for a, buf in zip((mean, var, exact, cnt), couts):
        assert np.array_equal(a, buf.to_array(np.float64, a.shape))
    for buf in [d_t, d_c, d_st] + outs + couts:
        buf.free()
