"""The shots -> moments case table (tests/shots_cases.py) reaches every branch of fbx_shots_to_moments_dev's launcher, and its exact
reference agrees with the oracle.  No GPU: route() is the launcher restated, so these assertions are about the table alone; the table
is run on the device by tests/test_shots_dispatch_gpu.py.  Every block of sc.BLOCKS is needed by at least one assertion here."""
import numpy as np
import pytest

import shots_cases as sc

ROUTES = {case: sc.route(*case) for case in sc.CASES}


def routed(pred=lambda case, r: True):
    return [(case, r) for case, r in ROUTES.items() if pred(case, r)]


def vectors(case):
    n, _, shots, _ = case
    return shots * n / sc.VEC_BYTES


def test_the_table_is_the_blocks_and_has_no_duplicates():
    listed = [case for block in sc.BLOCKS.values() for case in block]
    assert sc.CASES == list(dict.fromkeys(listed)) and len(sc.CASES) == len(set(sc.CASES)) >= len(listed) - 2
    assert len({sc.case_id(c) for c in sc.CASES}) == len(sc.CASES)
    assert all(1 <= n <= 64 and S >= 1 and shots >= 1 and 0 <= off < 16 for n, S, shots, off in sc.CASES)


def test_every_pipe_instantiation_runs_a_first_trip():
    first = {r.name for _, r in routed(lambda c, r: not r.second_trip and c[3] == 0)}
    want = {f"pipe<{n},{v}>" for n in sc.VEC_N for v in (1, 2, 4, 8)} | {f"packed<{n},{r}>" for n in sc.PACKED_PIPE_N for r in (1, 2)}
    assert want <= first, sorted(want - first)
    assert len(want) == 16 + 4


def test_every_size_class_runs_a_second_trip():
    second = {r.name for _, r in routed(lambda c, r: r.second_trip)}
    for n in sc.VEC_N:                                                  # every byte width hands a record over
        assert any(name.startswith(f"pipe<{n},") for name in second), n
    for v in (1, 2, 4, 8):                                              # and so does every register-buffer size
        assert any(name.endswith(f",{v}>") and name.startswith("pipe<") for name in second), v
    assert {"packed<5,1>", "packed<3,2>", "wave", "workgroup"} <= second
    for case, r in routed(lambda c, r: r.second_trip):
        cap = sc.GRID_CAP * (1 if r.name == "workgroup" else sc.WAVES_PER_GROUP)
        assert case[1] == cap + 5                                       # five units past the grid, no more


def test_second_trip_flag_sits_on_the_cap():
    assert not sc.route(2, sc.WAVES_PER_GROUP * sc.GRID_CAP, 8).second_trip and sc.route(2, sc.WAVES_PER_GROUP * sc.GRID_CAP + 1, 8).second_trip
    assert not sc.route(2, sc.GRID_CAP, 8192).second_trip and sc.route(2, sc.GRID_CAP + 1, 8192).second_trip


def test_both_sides_of_every_vector_class_boundary():
    for n in sc.VEC_N:
        by_vectors = {vectors(c): r.name for c, r in routed(lambda c, r: c[0] == n and c[1] == 9 and c[3] == 0 and vectors(c) in
                                                            (1, 63, 64, 65, 128, 129, 256, 257, 512, 513))}
        assert by_vectors == {1: f"pipe<{n},1>", 63: f"pipe<{n},1>", 64: f"pipe<{n},1>", 65: f"pipe<{n},2>", 128: f"pipe<{n},2>",
                              129: f"pipe<{n},4>", 256: f"pipe<{n},4>", 257: f"pipe<{n},8>", 512: f"pipe<{n},8>", 513: "wave"}, n
        past = [r for c, r in routed(lambda c, r: c[0] == n and vectors(c) == 513)]
        assert past and all(r.paths == {"vec"} for r in past)           # whole vectors from an aligned base: the vector path


def test_packed_runs_and_tails():
    for n in sc.PACKED_PIPE_N:
        got = {c[2]: r.name for c, r in routed(lambda c, r: c[0] == n and c[1] == 9 and c[3] == 0 and c[2] >= 16 and c[2] % 8 == 0)}
        one, two = f"packed<{n},1>", f"packed<{n},2>"
        assert got == {16: one, 24: one, 1016: one, 1024: one, 1032: one, 1040: two, 2048: two, 2056: two, 2064: "wave"}, n
        for name in (one, two):                                         # each with and without the byte-wise tail
            tails = {c[2] % sc.PACKED_RUN for c, r in routed(lambda c, r: r.name == name and not r.second_trip)}
            assert {0, 8} <= tails, (name, tails)
        assert {c[2] // sc.PACKED_RUN for c, r in routed(lambda c, r: r.name in (one, two))} >= {1, 63, 64, 65, 128}
    # the 8-byte size condition leaves tails of 0 and 8 shots only, for odd n
    assert all((shots * n) % 8 or shots % 16 in (0, 8) for n in sc.PACKED_PIPE_N for shots in range(16, 200))


def test_both_generic_forms_reach_each_count_path_under_a_non_zero_mask():
    for form in ("wave", "workgroup"):
        reached = set()
        for case, r in routed(lambda c, r: r.name == form):
            _, masks, _ = sc.make(case) if sc.case_bytes(case) < 1 << 20 else (None, None, None)
            if masks is None:
                continue
            paths = sc.record_paths(*case)
            assert set(paths) == r.paths
            reached |= {p for p, row in zip(paths, masks) if row.any()}
        assert reached == {"vec", "packed", "generic"}, (form, reached)


def test_wavefront_form_shapes():
    wave = routed(lambda c, r: r.name == "wave" and c[3] == 0 and not r.second_trip)
    for n in sc.VEC_N:                                                  # records that are no whole vectors: later records lose alignment
        cases = [(c, r) for c, r in wave if c[0] == n and (c[2] * n) % sc.VEC_BYTES]
        assert {c[2] for c, _ in cases} >= {s for s in (1, 7, 17, 1000) if (s * n) % sc.VEC_BYTES}, n
        assert any(r.paths == {"vec", "generic"} for _, r in cases), n
    for n in sc.PACKED_N:                                               # (16 shots of 3 or 5 columns go to the packed pipe)
        assert {c[2] for c in ROUTES if c[0] == n and c[1] == 9 and c[3] == 0} >= {1, 15, 16, 17, 1003}, n
        assert any(r.paths == {"packed", "generic"} for c, r in wave if c[0] == n), n
    for n in (9, 16, 33, 64):                                           # count-like sizes up to the contract's 64 columns
        cases = [(c, r) for c, r in wave if c[0] == n]
        assert {c[2] for c, _ in cases} >= {1, 100} and all(r.paths == {"generic"} for _, r in cases), n


def test_workgroup_form_shapes():
    few = routed(lambda c, r: r.name == "workgroup" and c[1] < sc.WAVE_MIN_SETTINGS)
    assert {c[1] for c, _ in few} == {1, 2, 3}
    for S in (1, 2, 3):                                                 # a short record still takes a workgroup when there are few
        assert {p for c, r in few if c[1] == S for p in r.paths} == {"vec", "packed", "generic"}, S
        assert all(c[2] * c[0] < sc.WAVE_BYTES for c, _ in few)
    for n in (1, 3, 9):                                                 # the longest record of a wavefront, the shortest of a workgroup
        below, above = (sc.WAVE_BYTES - 1) // n, -(-sc.WAVE_BYTES // n)
        assert ROUTES[(n, 9, below, 0)].name == "wave" and ROUTES[(n, 9, above, 0)].name == "workgroup", n
        assert below * n < sc.WAVE_BYTES <= above * n and above == below + 1


def test_misaligned_bases():
    got = {c: r for c, r in routed(lambda c, r: c[3] != 0)}
    assert {c[3] for c in got} == {1, 8}
    for n, shots in ((2, 1000), (8, 40), (3, 1000), (5, 1000)):
        aligned = sc.route(n, 9, shots, 0).name
        assert aligned.startswith("pipe<" if n in sc.VEC_N else "packed<")               # a pipe shape, were the base aligned
        assert got[(n, 9, shots, 1)] == sc.Route("wave", frozenset({"generic"}), False)  # offset 1 loses both
        at8 = got[(n, 9, shots, 8)]
        if n in sc.VEC_N:                                                                # offset 8 loses the vector kernels ...
            assert at8.name == "wave" and "vec" not in at8.paths
        else:                                                                            # ... and keeps the packed ones
            assert at8.name == aligned
    # offset 8 in the wavefront form: a packed count from a base that is 8- and not 16-byte aligned
    assert "packed" in sc.route(6, 9, 16, 8).paths and "packed" in sc.route(3, 9, 8, 8).paths


def test_no_case_is_large():
    assert max(sc.case_bytes(c) for c in sc.CASES) <= sc.MAX_CASE_BYTES
    assert max(sc.case_bytes(c) for c in sc.CASES) > 60_000_000         # the 257-vector second trip is there


SMALL = [c for c in sc.CASES if sc.case_bytes(c) <= 1 << 21]


def test_data_contract_of_make():
    kinds = set()
    for case in SMALL:
        n, S, shots, _ = case
        bits, masks, coefs = sc.make(case)
        assert bits.shape == (S, shots, n) and bits.dtype == np.uint8 and masks.shape == (S, n) and masks.dtype == np.uint8
        assert coefs.shape == (S,) and (np.abs(coefs) <= 2).all()
        assert set(np.unique(masks)) <= {0, 1, 2, 255}
        b2, m2, c2 = sc.make(case)
        assert np.array_equal(bits, b2) and np.array_equal(masks, m2) and np.array_equal(coefs, c2)
        if S >= 5:
            n_minus = sc.count_minus(bits, masks)
            live = masks.any(axis=1)
            assert (live & (n_minus == 0)).any() and (live & (n_minus == shots)).any(), case
            assert not masks[3].any() and masks[0].all()
            assert masks[2, 0] and not masks[2, 1:].any() and masks[4, -1] and not masks[4, :-1].any()
            assert coefs[1] == 1.0 and coefs[2] == 0.0
        if bits.size >= 4096:
            assert (bits > 1).any()                                    # high bits are set: only bit 0 is the outcome
            kinds |= set(np.unique(masks))
    assert kinds == {0, 1, 2, 255}


@pytest.mark.parametrize("case", [c for c in sc.CASES if ROUTES[c].second_trip], ids=sc.case_id)
def test_a_stale_record_or_mask_on_the_second_trip_changes_the_count(case):
    """what a second trip would count from the record, or with the mask, of the setting a grid's width before it: not the answer"""
    bits, masks, _ = sc.make(case)
    back = sc.GRID_CAP * (1 if ROUTES[case].name == "workgroup" else sc.WAVES_PER_GROUP)
    past = case[1] - back
    assert past == 5 and all(not np.array_equal(bits[back + i], bits[i]) for i in range(past))
    true = sc.count_minus(bits[back:], masks[back:])
    assert (sc.count_minus(bits[:past], masks[back:]) != true).any()
    assert (sc.count_minus(bits[back:], masks[:past]) != true).any()


@pytest.mark.parametrize("case", [(2, 9, 1000, 0), (1, 9, 7, 0), (3, 9, 1003, 0), (5, 9, 24, 0), (9, 9, 100, 0), (8, 9, 2, 0)], ids=sc.case_id)
def test_exact_agrees_with_the_oracle_on_zero_one_bits(case):
    from fbx_oracle import acquisition as oa
    assert case in sc.CASES
    bits, masks, coefs = sc.make(case)
    bits01, masks01 = bits & 1, (masks != 0).astype(np.uint8)
    for prior in (False, True):
        for cf in (None, coefs):
            mean, var, n_minus = sc.exact(bits, masks, cf, prior)
            m01, v01, k01 = sc.exact(bits01, masks01, cf, prior)        # the high bits and the mask's byte value change nothing
            assert np.array_equal(mean, m01) and np.array_equal(var, v01) and np.array_equal(n_minus, k01)
            for s in range(case[1]):
                wm, wv = oa.shots_to_obs_moments(bits01[s], masks01[s], 1.0 if cf is None else cf[s], prior)
                assert abs(mean[s] - wm) <= 1e-14 and abs(var[s] - wv) <= 1e-14, (case, s, prior)
            want = ((bits01 & masks01[:, None, :]).sum(axis=2) & 1).sum(axis=1)
            assert n_minus.dtype == np.int64 and np.array_equal(n_minus, want)
