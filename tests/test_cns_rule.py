"""The consensus rule restated in integers (tests/cns_util.py) against the stored answers of the reference's own
get_align_tags and get_cns_from_align_tags (tests/golden/cns_cases.npz, written by tests/golden/make_golden_cns.py from falcon/falcon.c,
DW_banded.c and kalloc.c compiled with -DNDEBUG): tags field by field and consensus byte for byte on every case.  Runs on the CPU."""
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
