"""The restatement of pg_asm_cns.py (tests/cnsjob_util.py) against what the real script printed (tests/golden/cnsjob_cases.npz): the layout
from its stderr and its stdout, case by case and chunk by chunk.  No GPU."""
import json

import numpy as np
import pytest

import cnsjob_util as J


def _chunks():
    return [(c.name, i) for c in J.load_cases() for i in range(len(c.chunks))]


def _lengths(case):
    rl, _ = case.ref_db.by_rid()
    return {int(r): int(rl[int(r)]) for r in case.ref_db.rid}


@pytest.mark.parametrize("name,i", _chunks())
def test_layout_equals_the_scripts(name, i):
    case = next(c for c in J.load_cases() if c.name == name)
    total, my, _, want, _ = case.chunks[i]
    got = J.layout(J.chunk_rows(J.parse_map(case.map_text), total, my), _lengths(case))
    assert [c["ctg"] for c in got] == [c["ctg"] for c in want]
    for a, b in zip(got, want):
        assert [(g["left"], g["right"], g["n_mapped"], g["offsets"]) for g in a["groups"]] == \
               [(g["left"], g["right"], g["n_mapped"], g["offsets"]) for g in b["groups"]], a["ctg"]


@pytest.mark.parametrize("name,i", _chunks())
def test_stdout_and_accepted_reads_equal_the_scripts(name, i):
    case = next(c for c in J.load_cases() if c.name == name)
    total, my, stdout, _, runs = case.chunks[i]
    det = []
    assert J.job(case.read_db, case.ref_db, case.map_text, total, my, details=det) == stdout
    lay = J.layout(J.chunk_rows(J.parse_map(case.map_text), total, my), _lengths(case))
    groups = [g for c in lay for g in c["groups"]]
    assert len(det) == len(runs) == len(groups)
    for (ctg, seg, said, n, base), run, g in zip(det, runs, groups):
        assert [e[0] for e, s in zip(g["entries"], said) if s] == run["accepted"], (ctg, seg)
        assert (n, base) == (run["aln_count"], run["aln_base"]), (ctg, seg)


def test_the_fixture_holds_what_it_was_made_for():
    cases = {c.name: c for c in J.load_cases()}
    prov = json.load(open(J.PROVENANCE))
    bio = prov["cases"]["bio"]["chunks"]["1_0"]
    assert bio["pieces"] == 5 and 4 * bio["called"] >= 3 * bio["pieces"]
    lay = {c["ctg"]: c["groups"] for ch in cases["edges"].chunks for c in ch[3]}
    lens = _lengths(cases["edges"])
    assert sorted(lens.values())[:7] == [1, 999, 1000, 1999, 2000, 2001, 2002]
    by_len = {lens[c]: g for c, g in lay.items()}
    assert [len(by_len[n]) for n in (1, 999, 1000, 1999, 2000, 2001, 2002)] == [1] * 7
    assert [by_len[n][0]["n_mapped"] > 0 for n in (1999, 2000, 2001, 2002)] == [False, False, True, True]
    assert (by_len[52_000][0]["left"], by_len[52_000][0]["right"]) == (1000, 52_000) and by_len[52_000][0]["n_mapped"] > 0        # merged, had rows
    assert [(g["left"], g["right"]) for g in by_len[105_000]] == [(1000, 51_005), (51_005, 101_010), (101_010, 105_000)]
    assert by_len[101_000][0]["n_mapped"] == 0 and by_len[100_999][0]["n_mapped"] > 0                                              # tails of 100,000 / 99,999
    shifts = [o[2] - (g["left"] - J.FLANK) for gs in lay.values() for g in gs for o in g["offsets"]]
    assert min(shifts) < 0 and any(s == 2002 for s in shifts) and any(s > 2002 for s in by_len[2002][0]["offsets"] for s in [s[2]])
    # the refusals of the rule
    with pytest.raises(J.Refused, match="line 2"):
        J.parse_map("1 2 3 4 5 6 7 8 9\n1 2 3 4 5 6 7 8\n")
    with pytest.raises(J.Refused, match="line 1"):
        J.parse_map("1 2 3 4 x 6 7 8 9\n")
    with pytest.raises(J.Refused, match="total_chunks"):
        J.chunk_rows([], 0, 0)
    with pytest.raises(J.Refused, match="contig 5"):
        J.layout([(5, 1, 2, 0, 0, 0, 0, 0, 0)], {4: 100})
    with pytest.raises(J.Refused, match="length 0"):
        J.layout([(4, 1, 2, 0, 0, 0, 0, 0, 0)], {4: 0})
    with pytest.raises(J.Refused, match="stitch"):
        J.stitch([b"A" * 999, b"A" * 2000])
    assert np.array_equal(J.tables(J.layout([], {}))[0], np.zeros(0, J.JOB_PIECE_DTYPE))
