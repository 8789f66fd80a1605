"""Grouping of settings by a shared tensor-product basis on the host: ``observable_estimation.group_settings`` and its parts,
``design.group_design`` on the label arrays against it, known partitions (worked out on the CPU from the greedy rule, the
move of a grown bucket to the end of the order included), the checks of ``design.Grouping``, which refuse before the library is
touched, and ``synthetic.restate_grouped_tomography_counts`` against the stream stated shot by shot."""
import functools

import numpy as np
import pytest

import tomo_sim_cases as tc

GROUPED_KEY_TAG = 0x544F4D47                         # "TOMG" (include/fbx.h)
ALL_CASES = tc.PROCESS_CASES + tuple(f"state-{n}" for n in tc.STATE_CASES)


def design_of(case):
    from fbx.design import state_design
    return state_design(int(case[6:])) if case.startswith("state") else tc.process_case_design(case)


def basis_text(design, group):
    top = design.paulis[group].max(axis=0)
    return "".join("IXYZ"[c] for c in top)


@functools.lru_cache(maxsize=None)
def grouped_objects(case, method):
    """(settings of the design, its ObservablesExperiment grouped by `method`)"""
    from fbx import observable_estimation as oe, tomography as t
    if case == "state-2-repeats":
        settings = t.generate_state_tomography_settings([0, 1])
        settings = settings + settings[3:6] + settings[:1]
    else:
        des = design_of(case)
        settings = t._settings_of(des, range(des.n_qubits))
    return settings, oe.group_settings(oe.ObservablesExperiment(list(settings)), method)


# ------------------------------------------------------------------------------------------------ 1. known answers
def test_two_qubit_state_design_groups():
    from fbx.design import group_design, state_design
    des = state_design(2)
    g = group_design(des)
    assert g.groups == [[0, 3, 4], [1, 5], [2, 6], [7, 8], [9], [10], [11, 12], [13], [14]]
    assert [basis_text(des, grp) for grp in g.groups] == ["XX", "XY", "XZ", "YX", "YY", "YZ", "ZX", "ZY", "ZZ"]
    assert g.n_groups == 9 and g.group_of.dtype == np.int32
    assert g.group_of.tolist() == [0, 1, 2, 0, 0, 1, 2, 3, 3, 4, 5, 6, 6, 7, 8]


@pytest.mark.parametrize("n, largest", ((1, 1), (2, 3), (3, 6), (4, 11), (5, 21)))
def test_state_designs_have_3_to_the_n_full_weight_groups(n, largest):
    """(largest group: 7 at n = 3 if a grown bucket kept its place in the order)"""
    from fbx.design import group_design, state_design
    des = state_design(n)
    g = group_design(des)
    assert g.n_groups == 3 ** n and max(len(grp) for grp in g.groups) == largest
    assert all("I" not in basis_text(des, grp) for grp in g.groups)
    assert np.all(g.basis != 0)


@pytest.mark.parametrize("n, basis, count", ((1, "pauli", 18), (2, "pauli", 324), (2, "sic", 144), (3, "sic", 1728)))
def test_process_designs_have_states_times_3_to_the_n_groups(n, basis, count):
    from fbx.design import group_design, process_design
    des = process_design(n, basis)
    g = group_design(des)
    assert g.n_groups == count
    if n == 1:
        assert g.groups == [[k] for k in range(des.m)]            # grouping does nothing on one qubit


def test_shuffled_three_qubit_design():
    from fbx.design import group_design
    des = tc.process_case_design("3q-shuffled")
    g = group_design(des)
    assert des.m == 300 and g.n_groups == 247
    assert sum("I" not in basis_text(des, grp) for grp in g.groups) == 132
    rows = [r.tobytes() for r in np.concatenate([des.in_labels, des.paulis], axis=1)]
    twins = [k for k in range(des.m) if rows.index(rows[k]) != k]
    assert len(twins) == 20
    for k in twins:
        assert g.group_of[k] == g.group_of[rows.index(rows[k])]    # a repeated setting lands in the group of its twin


# ------------------------------------------------------------------------------------------------ 2. arrays against objects
@pytest.mark.parametrize("case", ALL_CASES)
def test_group_design_equals_the_greedy_grouping_of_the_objects(case):
    from fbx.design import Grouping, group_design
    des = design_of(case)
    settings, grouped = grouped_objects(case, "greedy")
    got = group_design(des)
    assert len(grouped) == got.n_groups
    # the same groups in the same order with the same member order: compare setting by setting ...
    for members, group in zip(got.groups, grouped):
        assert [settings[k] for k in members] == list(group)
    # ... and as indices (a repeated setting: the twins in ascending order, as the objects meet them)
    assert Grouping.from_experiment(des, grouped).groups == got.groups


# ------------------------------------------------------------------------------------------------ 3. both methods
@pytest.mark.parametrize("case, method", [(c, "greedy") for c in ("2q-pauli", "3q-shuffled", "state-3", "state-2-repeats")]
                         + [(c, "clique-removal") for c in ("1q-sic", "state-3", "state-2-repeats")])
def test_groups_are_valid_and_cover_every_setting(case, method):
    """(clique removal on small experiments: the graph takes a comparison per pair of settings, and networkx recurses per node)"""
    from fbx import observable_estimation as oe
    settings, grouped = grouped_objects(case, method)
    flat = [s for group in grouped for s in group]
    assert len(flat) == len(settings)                               # every setting once, repeats kept
    count = lambda xs: {s: xs.count(s) for s in set(xs)}
    assert count(flat) == count(list(settings))
    for group in grouped:
        assert len({s.in_state for s in group}) == 1
        assert oe._max_weight_state(s.in_state for s in group) is not None
        assert oe._max_weight_operator(s.observable for s in group) is not None


def test_max_weight_operator_and_state():
    from fbx import observable_estimation as oe
    P = oe.PauliTerm
    assert oe._max_weight_operator([P({0: "X"}), P({1: "Z"})]) == P({0: "X", 1: "Z"})           # XI, IZ -> XZ
    assert oe._max_weight_operator([P({0: "X"}), P({0: "Z"})]) is None                          # XI, ZI
    assert oe._max_weight_operator([P({0: "X"}, 0.5), P({0: "X", 1: "Y"}, -2.0)]) == P({0: "X", 1: "Y"})
    assert oe._max_weight_state([oe.plusX(0), oe.minusZ(1)]) == oe.plusX(0) * oe.minusZ(1)
    assert oe._max_weight_state([oe.plusX(0), oe.plusZ(0)]) is None


def test_tpb_graph_and_buckets():
    from fbx import observable_estimation as oe, tomography as t
    settings = t.generate_state_tomography_settings([0, 1])
    expt = oe.ObservablesExperiment(settings + settings[:2])
    graph = oe.construct_tpb_graph(expt)
    assert graph.number_of_nodes() == 15 and graph.nodes[settings[0]]["count"] == 2 and graph.nodes[settings[5]]["count"] == 1
    assert graph.has_edge(settings[0], settings[3]) and not graph.has_edge(settings[0], settings[1])      # IX-XI, IX-IY
    buckets = oe._max_tpb_overlap(oe.ObservablesExperiment(settings))
    assert [str(k.observable) for k in buckets][:3] == ["(1+0j)*X0X1", "(1+0j)*X0Y1", "(1+0j)*X0Z1"]
    with pytest.raises(AssertionError):
        oe.group_settings(oe.ObservablesExperiment(settings), "best")
    with pytest.raises(AssertionError):
        oe.group_settings_greedy(oe.group_settings_greedy(oe.ObservablesExperiment(settings)))           # already grouped


def test_observables_experiment_is_a_list_of_groups(tmp_path):
    from fbx import observable_estimation as oe, tomography as t
    settings = t.generate_process_tomography_settings([0, 1], "sic")[:30]
    flat = oe.ObservablesExperiment(settings, program="X 0\nCZ 0 1")
    assert len(flat) == 30 and flat[3] == [settings[3]] and [g for g in flat][29] == [settings[29]] and [settings[2]] in flat
    grouped = oe.group_settings(flat)
    assert grouped.program == "X 0\nCZ 0 1" and len(grouped) < 30 and sum(len(g) for g in grouped) == 30
    lines = grouped.settings_string().split("\n")
    assert len(lines) == len(grouped) and lines[0].startswith("0: ") and str(settings[0]) in lines[0]
    assert len(grouped.settings_string(abbrev_after=4).split("\n")) == 6
    assert str(grouped).startswith("X 0; CZ 0 1\n0: ")
    fn = oe.to_json(str(tmp_path / "expt.json"), grouped)
    back = oe.read_json(fn)
    assert isinstance(back, oe.ObservablesExperiment) and back == grouped and back != flat
    assert [list(g) for g in back] == [list(g) for g in grouped] and back.program == grouped.program
    none = oe.ObservablesExperiment(settings[:2])
    assert none.program is None and oe.read_json(oe.to_json(str(tmp_path / "none.json"), none)) == none
    none.append(settings[2]); none.append([settings[3], settings[4]])
    assert len(none) == 4 and none.pop() == [settings[3], settings[4]] and len(oe.ObservablesExperiment([])) == 0


# ------------------------------------------------------------------------------------------------ 4. Grouping refuses on the host
def test_grouping_validation_needs_no_library(monkeypatch):
    from fbx import _lib
    from fbx.design import Grouping, group_design, state_design, process_design

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    des = process_design(2, "sic")
    good = group_design(des).group_of
    assert Grouping(des, good).groups == group_design(des).groups         # an explicit group_of: members ascending
    mixed = good.copy(); mixed[15] = good[0]                              # setting 15 has another input state than setting 0
    with pytest.raises(ValueError, match="input state"):
        Grouping(des, mixed)
    sdes = state_design(2)
    clash = group_design(sdes).group_of.copy(); clash[1] = clash[0]       # IY into the XX group
    with pytest.raises(ValueError, match="tensor-product basis"):
        Grouping(sdes, clash)
    with pytest.raises(ValueError, match="no member"):
        Grouping(sdes, _ids_with_a_gap())
    with pytest.raises(ValueError, match="group ids"):
        Grouping(sdes, np.full(15, -1))
    with pytest.raises(ValueError, match="group ids"):
        Grouping(sdes, np.arange(15), groups=[[k] for k in range(14)])
    with pytest.raises(ValueError, match="one per setting"):
        Grouping(sdes, np.zeros(14, dtype=int))
    with pytest.raises(ValueError, match="exactly once"):
        Grouping.from_groups(sdes, [[k] for k in range(14)])
    assert Grouping(sdes, np.arange(15)).n_groups == 15                   # the ungrouped experiment is a grouping too


def _ids_with_a_gap():
    ids = np.arange(15)
    ids[ids >= 7] += 1                                                    # 16 ids, none of them 7
    return ids


# ------------------------------------------------------------------------------------------------ 5. the restatement
def test_restated_histograms_sum_to_the_shots_and_follow_a_point_distribution():
    from fbx import synthetic
    from fbx.design import group_design, state_design
    des = state_design(3)
    g = group_design(des)
    rng = np.random.default_rng(5)
    p = rng.dirichlet(np.ones(8), size=(2, g.n_groups))
    for shots in (1, 3, 4, 5, 257):
        e, c, s, hist = synthetic.restate_grouped_tomography_counts(p, g, des.paulis, des.coefs, shots, tc.SEED, tc.FIRST)
        assert hist.shape == (2, 27, 8) and np.all(hist.sum(axis=2) == shots) and np.all(c == float(shots))
        assert np.all(np.abs(e) <= 1.0) and np.all(s >= 0.0)
    # all the weight on one outcome: every shot gives it, and the members read (-1)^popcount(outcome & support) exactly
    point = np.zeros((2, g.n_groups, 8))
    where = rng.integers(0, 8, size=(2, g.n_groups))
    np.put_along_axis(point, where[:, :, None], 1.0, axis=2)
    e, c, s, hist = synthetic.restate_grouped_tomography_counts(point, g.group_of, des.paulis, des.coefs, 37, tc.SEED, tc.FIRST)
    assert np.array_equal(hist, (point * 37).astype(np.int64)) and np.all(s == 0.0)
    z = ((des.paulis[:, ::-1] != 0) << np.arange(3)).sum(axis=1)
    want = np.array([[(-1.0) ** bin(int(where[b, g.group_of[k]]) & int(z[k])).count("1") for k in range(des.m)] for b in range(2)])
    assert np.array_equal(e, want)
    # negative entries are clamped, and the result depends on the global item only
    tilted = p.copy(); tilted[:, :, 0] = -0.25
    h2 = synthetic.restate_grouped_tomography_counts(tilted, g, des.paulis, des.coefs, 257, tc.SEED, tc.FIRST)[3]
    assert np.all(h2[:, :, 0] == 0) and np.all(h2.sum(axis=2) == 257)
    h1 = synthetic.restate_grouped_tomography_counts(p, g, des.paulis, des.coefs, 257, tc.SEED, tc.FIRST)[3]
    again = synthetic.restate_grouped_tomography_counts(p[1:], g, des.paulis, des.coefs, 257, tc.SEED, tc.FIRST + 1)[3]
    assert np.array_equal(again, h1[1:])
    with pytest.raises(ValueError, match="poisoned"):
        synthetic.restate_grouped_tomography_counts(np.zeros((1, 27, 8)), g, des.paulis, des.coefs, 5, tc.SEED)


@pytest.mark.parametrize("shots", (1, 3, 4, 5, 203))
def test_restatement_equals_the_shot_by_shot_loop_under_the_grouped_tag(shots):
    """p = (1/2, 1/2) on one qubit: outcome 0 iff the word is below 2^31, which is count_loop at mu = 0 -- run under the tag
    "TOMG" (count_loop applies "TOMO" itself: the seed carries the difference) with the GROUP id as the third counter word"""
    from fbx import synthetic
    from fbx.design import Grouping, process_design
    des = process_design(1, "sic")
    g = Grouping(des, np.arange(des.m))
    p = np.full((2, des.m, 2), 0.5)
    e, c, s, hist = synthetic.restate_grouped_tomography_counts(p, g, des.paulis, des.coefs, shots, tc.SEED, tc.FIRST)
    retagged = tc.SEED ^ tc.KEY_TAG ^ GROUPED_KEY_TAG
    want = np.array([[tc.count_loop(0.0, shots, retagged, tc.FIRST + b, k) for k in range(des.m)] for b in range(2)])
    assert np.array_equal(hist[:, :, 0], want) and np.array_equal(hist[:, :, 1], shots - want)
    we, ws = tc.moments(want, shots, des.coefs[None, :])
    assert np.array_equal(e, we) and np.array_equal(s, ws)
    untagged = np.array([[tc.count_loop(0.0, shots, tc.SEED, tc.FIRST + b, k) for k in range(des.m)] for b in range(2)])
    assert shots < 5 or not np.array_equal(untagged, want)
