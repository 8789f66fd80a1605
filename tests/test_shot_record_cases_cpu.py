"""tests/shot_record_cases.py reaches the edges it names (no GPU): every run length of each reader, records with no run / a head
only / a run without and with a tail, both teams, records off the 16-byte grid, both sides of the switch, a second grid trip."""
import shot_record_cases as sr
import shots_cases as sc


def walk(start, width, n_shots, S):
    head = sr.head_of(start, width, n_shots)
    runs = (n_shots - head) // S
    return head, runs, n_shots - head - runs * S


def test_constants_agree_with_the_other_tables():
    from fbx import _lib
    assert sr.WAVE_BYTES == sc.WAVE_BYTES == _lib.HIST_WAVE_BYTES == 16384
    assert sr.GRID_CAP == sc.GRID_CAP and sr.SECOND_TRIP == sc.SECOND_TRIP_WAVE


def test_every_run_length_and_every_part_of_a_record():
    assert {sr.run_shots(n, "rpe") for n in sr.RPE_WIDTHS} == {16, 8, 4, 2}        # gcd(width, 16) = 1, 2, 4, 8
    assert {sr.run_shots(n, "qv") for n in sr.QV_WIDTHS} == {16}
    for widths, reader in ((sr.QV_WIDTHS, "qv"), (sr.RPE_WIDTHS, "rpe")):
        for n in widths:
            S = sr.run_shots(n, reader)
            seen = set()
            for width, shots, B in sr.edge_cases((n,)):
                for offset in (0, 1):
                    for start in sr.record_starts(width, shots, B, offset):
                        head, runs, tail = walk(start, width, shots, S)
                        seen.add(("no run" if runs == 0 else "runs", "head" if head else "no head", "tail" if tail else "no tail"))
            assert ("no run", "no head", "tail") in seen and ("runs", "no head", "no tail") in seen, (n, seen)
            assert ("runs", "no head", "tail") in seen, (n, seen)
            if n % 16:                                                           # an offset base or an odd record: shots in front
                assert any(s[1] == "head" for s in seen), (n, seen)
                assert ("no run", "head", "no tail") in seen, (n, seen)           # the record ends before its first boundary


def test_teams_odd_records_switch_and_second_trip():
    assert {B >= sc.WAVE_MIN_SETTINGS for B in sr.BATCHES} == {False, True} and max(sr.BATCHES) > sr.WAVES_PER_GROUP
    for widths in (sr.QV_WIDTHS, sr.RPE_WIDTHS):
        odd = [(n, shots) for n, shots, _ in sr.edge_cases(widths) if (n * shots) % 2]
        assert len({n for n, _ in odd}) >= 2 and all(max(sr.BATCHES) * n * shots < sr.WAVE_BYTES for n, shots in odd)
    width, (below, above), B = sr.QV_SWITCH
    assert below * width < sr.WAVE_BYTES <= above * width and above == below + 1 and B >= sc.WAVE_MIN_SETTINGS
    for width, shots, B in (sr.QV_SECOND_TRIP, sr.RPE_SECOND_TRIP):
        assert -(-B // sr.WAVES_PER_GROUP) > sr.GRID_CAP and width * shots < sr.WAVE_BYTES and width * shots * B < 1 << 20
