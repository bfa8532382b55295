"""The consensus rule restated in integers (tests/cns_util.py) against the stored answers of the reference's own
get_align_tags and get_cns_from_align_tags (tests/golden/cns_cases.npz, written by tests/golden/make_golden_cns.py from falcon/falcon.c,
DW_banded.c and kalloc.c compiled with -DNDEBUG): tags field by field and consensus byte for byte on every case.  Runs on the CPU."""
import hashlib
import json
import os

import numpy as np
import pytest

import cns_util as CU


@pytest.fixture(scope="module")
def cases():
    return CU.load_cases()


def test_fixture_holds_the_cases_the_kernels_can_go_wrong_at(cases):
    by = {c.name: c for c in cases}
    rates = {n.split("_")[1] for n in by if n.startswith("real_")}
    assert rates == {"e00", "e01", "e05", "e15"}
    real = [c for n, c in by.items() if n.startswith("real_")]
    assert min(p[0] for c in real for p in c.pieces) == 60 and max(p[0] for c in real for p in c.pieces) == 3000
    assert {len(c.pieces[0][1]) - 1 for c in real} >= {1, 20}
    offs = [a[4] for c in real for a in c.pieces[0][1]]
    assert 0 in offs and max(offs) > 0                                            # both sort positions of the '.' predecessor
    assert any(len(set(c.pieces[0][1][0][0])) == 2 for c in real)                 # a two-letter template
    assert len(by["batch64"].pieces) == 64 and {60, 2000} <= {p[0] for p in by["batch64"].pieces}
    big = by["big8192"].pieces[0]
    assert big[0] >= 8192 and len(big[1]) == 13
    assert by["backbone"].cns[0] == by["backbone"].pieces[0][1][0][0].lower()
    for n in (254, 255, 300):                                                     # the cut: an insertion of 255 and more ends the alignment's tags
        c = by[f"hand_ins{n}"]
        assert (len(c.tags[2]) == len(c.pieces[0][1][2][0])) == (n == 254), n
        assert int(c.tags[2]["delta"].max()) == 254
    assert max(np.bincount(by["hand_wide_position"].tags[5]["t_pos"])) > 250
    assert by["hand_min_cov0"].cns[0] != by["hand_min_cov1"].cns[0] != by["hand_min_cov2"].cns[0]
    assert by["hand_min_cov0"].cns[0].upper() == by["hand_min_cov2"].cns[0].upper()
    # the windows of the scoring ring (1024) and of the back-track (2048) at their exact values: the index difference of two nodes
    for what, dist in (("ring", 1023), ("ring", 1024), ("ring", 1025), ("back", 2047), ("back", 2048), ("back", 2049)):
        c = by[f"edge_{what}_{dist}"]
        (t_len, alns), T = c.pieces[0], c.pieces[0][1][0][0]
        assert t_len == 120 and len(alns) == 22 and alns[:12] == [alns[0]] * 12 and c.cns[0] == T
        assert CU.node_distance(alns, (59, 0, T[59]), (60, 0, T[60])) == dist, c.name
    # the back-track's first window hangs from the end node: here the end node itself is the one that jumps 2047, 2048 and 2049 places
    for dist in (2047, 2048, 2049):
        c = by[f"edge_back_end_{dist}"]
        (t_len, alns), T = c.pieces[0], c.pieces[0][1][0][0]
        assert t_len == 120 and len(alns) == 22 and alns[:12] == [alns[0]] * 12 and c.cns[0] == T
        end = (119, 0, c.cns[0][-1])                                              # the consensus ends on the last node of the piece
        assert CU.tag_key(*end) == int(CU.distinct_keys(alns)[-1])
        assert CU.node_distance(alns, (118, 0, c.cns[0][-2]), end) == dist, c.name
    cuts = [len(tg) for c in cases if c.name.startswith(("edge_", "hand_")) for a, tg in zip([a for _, al in c.pieces for a in al], c.tags)
            if len(tg) < len(a[0]) and len(tg) and int(tg["delta"][-1]) == 254]
    assert {0, 63} <= {n % 64 for n in cuts}                                      # the column of the cut: a chunk's first and last lane
    assert sorted(len(tg) for tg in by["edge_cut_lanes"].tags if int(tg["delta"].max()) == 254) == [255, 255, 256, 256, 319, 319, 320, 320]
    strings = by["edge_strings"]
    assert any(len(a[0]) == 0 for a in strings.pieces[0][1]) and sum(len(tg) == 0 for tg in strings.tags) >= 3
    ties = by["edge_ties"]
    assert len(ties.pieces) == 65 and ties.min_cov == 0
    pairs = [(x, y) for i, x in enumerate(CU.LETTERS) for y in CU.LETTERS[i + 1:]]
    for (x, y), (_, alns), cns in zip(pairs, ties.pieces, ties.cns):
        assert {alns[0][0][50], alns[1][0][50]} == {x, y} and len(cns) == 100 and cns[50] == min(x, y), (chr(x), chr(y))
    for x, (_, alns), cns in zip(CU.LETTERS, ties.pieces[45:55], ties.cns[45:55]):   # a gap sorts before every letter
        assert {alns[0][0][50], alns[1][0][50]} == {x, 45} and len(cns) == 99
    for x, (_, alns), cns in zip(CU.LETTERS, ties.pieces[55:], ties.cns[55:]):
        assert len(cns) == 101 and cns[50] == x
    assert {c.min_cov for c in cases} >= {0, 1, 2, 3, 65535, 2**31 - 1}
    assert len(by["edge_full_count"].pieces[0][1]) == CU.MAX_ALNS and by["edge_full_count"].cns[0].isupper()
    assert by["edge_min_cov_max_lower"].cns[0].islower() and by["edge_min_cov_max_allN"].cns[0] == b"N" * 200


OLD_CASES = ["real_e00_t60_r1", "real_e00_t200_r3", "real_e00_t333_r7", "real_e00_t1000_r12", "real_e01_t60_r1", "real_e01_t200_r3",
             "real_e01_t333_r7", "real_e01_t1000_r12", "real_e05_t60_r1", "real_e05_t200_r3", "real_e05_t333_r7", "real_e05_t1000_r12",
             "real_e05_t3000_r20", "real_e15_t60_r1", "real_e15_t200_r3", "real_e15_t333_r7", "real_e15_t1000_r12", "real_e15_t3000_r20",
             "backbone", "hand_tie", "hand_tie3", "hand_ins254", "hand_ins255", "hand_ins300", "hand_long_deletion", "hand_rare_insertion",
             "hand_min_cov0", "hand_min_cov1", "hand_min_cov2", "hand_ends_mid_template", "hand_lower_case_reads", "hand_wide_position",
             "batch64", "big8192"]
OLD_SHA256 = "e8fe9e4610a2b7dd94c3c9ce5139f42eb4b3bb5a8770c553dd6a0fcfb1636b03"


def test_the_first_34_cases_are_the_ones_the_fixture_began_with(cases):
    """their names in order and a SHA-256 over the reference's consensus of every piece and its tags of every alignment, taken from the
    fixture as it stood before the edge_* group was appended"""
    assert [c.name for c in cases[:34]] == OLD_CASES
    h = hashlib.sha256()
    for c in cases[:34]:
        h.update(c.name.encode() + b"\0")
        for x in c.cns:
            h.update(len(x).to_bytes(8, "little") + x)
        for t in c.tags:
            h.update(len(t).to_bytes(8, "little"))
            for f in CU.TAG_FIELDS:
                h.update(np.ascontiguousarray(t[f]).tobytes())
    assert h.hexdigest() == OLD_SHA256


def test_restated_tags_equal_the_reference(cases):
    for c in cases:
        alns = [a for _, al in c.pieces for a in al]
        assert len(alns) == len(c.tags)
        for a, want in zip(alns, c.tags):
            got = CU.align_tags(*a)
            for f in CU.TAG_FIELDS:
                assert np.array_equal(got[f], want[f]), (c.name, f)


def test_restated_consensus_equals_the_reference(cases):
    for c in cases:
        for (t_len, alns), want in zip(c.pieces, c.cns):
            assert CU.consensus(t_len, alns, c.min_cov) == want, c.name


def test_consensus_is_a_function_of_the_multiset(cases):
    rng = np.random.default_rng(5)
    for c in cases[:24]:
        t_len, alns = c.pieces[0]
        assert CU.consensus(t_len, [alns[i] for i in rng.permutation(len(alns))], c.min_cov) == c.cns[0], c.name


def test_refusals():
    T = CU.random_template(np.random.default_rng(1), 80)
    ok = CU.build(T, 0, 0, [("=", 80)])
    assert CU.consensus(80, [ok, ok]) == T
    with pytest.raises(CU.Refused, match="no end node"):
        CU.consensus(80, [])
    with pytest.raises(CU.Refused, match="no end node"):
        CU.consensus(80, [CU.build(T, 0, 0, [("=", 1)])])
    with pytest.raises(CU.Refused, match="a tag at"):
        CU.consensus(79, [ok])
    with pytest.raises(CU.Refused, match="negative"):
        CU.consensus(80, [ok[:4] + (-1,)])
    with pytest.raises(CU.Refused, match="outside"):
        CU.consensus(80, [(ok[0][:10] + b"X" + ok[0][11:],) + ok[1:]])
    with pytest.raises(CU.Refused, match="alignments"):
        CU.check_piece(80, [ok] * (CU.MAX_ALNS + 1))


def test_provenance_says_what_the_docstring_says():
    prov = json.load(open(CU.PROVENANCE))
    g = np.load(CU.GOLDEN)
    assert prov["generator"] == "tests/golden/make_golden_cns.py" and "-DNDEBUG" in prov["cflags"]
    assert set(prov["sources"]) >= {"falcon.c", "DW_banded.c", "kalloc.c"} and all(len(v) == 64 for v in prov["sources"].values())
    assert prov["cases"] == len(g["names"]) and prov["pieces"] == len(g["cns_off"]) - 1 and prov["alignments"] == len(g["tag_off"]) - 1
    assert prov["tags"] == int(g["tag_off"][-1]) and prov["glibc"].startswith("glibc") and isinstance(prov["seed"], int)
    assert set(prov["reference_seconds_one_thread"]) == set(g["names"].tolist())
    b = prov["bench"]
    assert len(b["reference_seconds_per_piece"]) == b["pieces"] and b["t_len"] == 50_000 and b["reads"] == 30
    for f in (CU.GOLDEN, CU.PROVENANCE):
        assert os.path.getsize(f) <= 1085991          # the largest fixture tests/golden held before this one
