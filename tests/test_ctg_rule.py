"""The rule of DESIGN.md 4.5e as tests/ctg_util.py restates it, held to every stored case of tests/golden/ctg_cases.npz: what the REAL
second half of ovlp_to_graph.py wrote for the case under five hash seeds, in normal form (a case is stored only if all seeds agree).  The
normal form takes out what the rule states as its own -- how a unitig is named, the order of lines and of a compound's sub-list, which of
a contig's two lines is F, where a ring is cut -- and nothing else.  No GPU."""
import numpy as np
import pytest

import ctg_util as CU
import utg_util as UT

Z, CASES = CU.load_fixture()
STORED = [n for n, c in CASES.items() if c["stored"]]


def test_the_fixture_shows_every_type_and_kind_of_contig():
    assert len(STORED) >= 8
    shown = set()
    for n in STORED:
        shown.update(CASES[n]["features"])
    assert {"spur:2", "simple_dup", "compound", "contained", "repeat_bridge", "through_compound", "circular_ring", "circular_cycle"} <= shown
    # a spur over the length limit that stays, one of 60,000 that goes in the second pass, and the best_in test passed and failed
    assert CASES["spur"]["spur2"] == 2 and CASES["spur"]["simple"] == 4 and CASES["spur2"]["spur_rounds"] == 1
    assert b" spur:2 60000 " in Z["spur2_utg"].tobytes()
    y = [ln.split(b" ")[6].count(b"|") + 1 for ln in Z["yjoin_ctg"].tobytes().split(b"\n")[:-1]]
    assert sorted(y) == [1, 1, 2, 2]


@pytest.mark.parametrize("name", STORED)
def test_restatement_equals_the_script_in_normal_form(name):
    r = CU.contig_paths(CU.fixture_edges(Z, name))
    assert CU.normalise(r.utg_text, r.ctg_text) == CU.normalise(Z[name + "_utg"].tobytes(), Z[name + "_ctg"].tobytes())
    st = CU.stats_of(r)
    assert {k: v for k, v in CASES[name].items() if k in st} == st


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_outputs_agree_with_each_other(name):
    edges = CU.fixture_edges(Z, name)
    r = CU.contig_paths(edges)
    simple, table, _ = UT.unitigs(edges)
    n_u = len(table)
    ours = r.utg_text.split(b"\n")[:-1]
    # the simple lines are the unitigs' own with the type replaced; u_edge_data's order is the unitigs'
    for a, b in zip(simple.split(b"\n")[:-1], ours):
        fa, fb = a.split(b" "), b.split(b" ")
        assert fa[:3] + fa[4:] == fb[:3] + fb[4:] and fb[3] in CU.TYPE_NAMES[:5]
    assert len(ours) == len(r.table) and all(ln.split(b" ")[1] == b"NA" and ln.split(b" ")[3] in (b"compound", b"spur:2", b"repeat_bridge") for ln in ours[n_u:])
    # the ids follow the length of the whole walk (the script sorts by -path_length, :1500), not the printed length of the claimed prefix
    assert r.claimed_walk_lengths == sorted(r.claimed_walk_lengths, reverse=True) and len(r.claimed_walk_lengths) == r.ctg_text.count(b"F ctg_")
    printed = [int(ln.split(b" ")[4]) for ln in r.ctg_text.split(b"\n")[:-1] if ln.split(b" ")[0].endswith(b"F")]
    assert all(p <= w for p, w in zip(printed, r.claimed_walk_lengths))
    # duals pair up; a ring has none
    d = r.table["dual"]
    for u in range(len(d)):
        assert (d[u] == CU.NONE and u < n_u and table["circular"][u]) or d[d[u]] == u
    # every F line's R line lists the duals, reversed; no unitig is in two contigs
    seen, ids = set(), [ln.split(b" ")[0] for ln in r.ctg_text.split(b"\n")[:-1]]
    for k, cid in enumerate(ids):
        if cid.endswith(b"F"):
            f, rr = r.rows[k], r.rows[k + 1]
            assert ids[k + 1] == cid[:-1] + b"R" and [d[u] for u in reversed(f)] == list(rr)
            assert not seen & set(f) and not seen & set(rr)
            seen.update(f), seen.update(rr)


def test_where_the_script_raises_the_rule_refuses():
    edges = CU.fixture_edges(Z, "spur")
    bad = np.delete(edges, 1)                                    # an edge without its reverse
    with pytest.raises(CU.Invalid):
        CU.contig_paths(bad)
    # two short loops at one node: a -> x -> a and a -> y -> a, a made non-simple by them
    a, x, y = 1 << 1 | 1, 2 << 1 | 1, 3 << 1 | 1
    lines = []
    for v, w in ((a, x), (x, a), (a, y), (y, a)):
        lines += [(v, w, 0, 3000, 2000), (w ^ 1, v ^ 1, 3000, 0, 2000)]
    with pytest.raises(CU.Invalid, match="second short loop"):
        CU.contig_paths(CU.edges_of_g_lines(lines))
    # a bundle in which no score is positive
    g = CU.Graph()
    CU.MOTIFS["compound"](g)
    e = CU.edges_of_g_lines(g.lines)
    e["score"] = 0
    with pytest.raises(CU.Invalid, match="positive score"):
        CU.contig_paths(e)
    assert len(CU.contig_paths(e[:0]).table) == 0 and CU.contig_paths(e[:0]).ctg_text == b""
