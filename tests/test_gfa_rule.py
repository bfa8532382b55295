"""The GFA rule without a GPU: the plain-Python restatement (tests/gfa_util.py) on every case of tests/golden/utg_cases.npz, through the
unitig restatement (tests/utg_util.py, which test_utg_rule.py holds to the reference), against an independent brute force -- the dual by
reversing the node path and looking it up in a dictionary, the links by comparing t(a) and s(b) of all pairs -- and against the counts
the rule implies.  This is what lets the GPU tests compare with the restatement."""
import numpy as np
import pytest

import gfa_util as GF
import oracle_util as U
import sgraph_util as SG
import utg_util as UT

CASES = ["single", "chains", "long", "rings", "dense", "quant", "none", "forks", "typed"]


def case_edges(z, cases, name):
    c = cases[name]
    if c["kind"] == "edges":
        return UT.fixture_edges(z, name)
    return SG.string_graph_of_full_text(U.orc_dedup(UT.fixture_recs(z, c))[0], c["min_len"], c["min_idt"])[1]


@pytest.fixture(scope="module")
def fixture():
    return UT.load_fixture()


@pytest.fixture(scope="module")
def restated(fixture):
    """name -> (edges, table, paths, the restatement's answer), computed once and left alone"""
    z, cases = fixture
    out = {}
    for name in CASES:
        edges = case_edges(z, cases, name)
        _, table, paths = UT.unitigs(edges)
        out[name] = (edges, table, paths, GF.gfa(edges, table, paths))
    return out


def node_paths(edges, table, paths):
    v, w = GF.node_keys(edges)
    out = []
    for r in table:
        p = [int(e) for e in paths[int(r["first"]):int(r["first"]) + int(r["n_edges"])]]
        out.append(tuple([v[p[0]]] + [w[e] for e in p]))
    return out


def brute_duals(edges, table, paths):
    """the dual as the unitig whose node path is the reversed path with every node's end flipped; a ring's reverse is cut elsewhere, so
    rings are looked up by their set of directed edges"""
    nodes = node_paths(edges, table, paths)
    linear = {p: u for u, (p, r) in enumerate(zip(nodes, table)) if not r["circular"]}
    ring = {frozenset(zip(p, p[1:])): u for u, (p, r) in enumerate(zip(nodes, table)) if r["circular"]}
    dual = []
    for p, r in zip(nodes, table):
        rev = tuple(x ^ 1 for x in reversed(p))
        dual.append(ring[frozenset(zip(rev, rev[1:]))] if r["circular"] else linear[rev])
    return dual


@pytest.mark.parametrize("name", CASES)
def test_the_restatement_against_the_brute_force(restated, name):
    edges, table, paths, (segments, rows, directed, links, text) = restated[name]
    n_u = len(table)
    dual = brute_duals(edges, table, paths)
    assert GF.duals(edges, table, paths)[0] == dual
    assert all(dual[dual[u]] == u and dual[u] != u for u in range(n_u))
    # segments
    canon = [u for u in range(n_u) if u < dual[u]]
    assert [int(x) for x in segments["unitig"]] == canon and [int(x) for x in segments["dual"]] == [dual[u] for u in canon]
    assert len(segments) * 2 == n_u
    assert [int(x) for x in segments["n_rows"]] == [int(table["n_edges"][u]) for u in canon]
    assert [int(x) for x in segments["first_row"]] == [int(x) for x in np.concatenate([[0], np.cumsum(segments["n_rows"].astype(np.int64))[:-1]])][:len(canon)]
    # rows: the edges of the canonical paths, field by field
    assert len(rows) == int(segments["n_rows"].sum()) == int((edges["type"] == SG.G).sum()) // 2
    at = 0
    for j, u in enumerate(canon):
        for e in paths[int(table["first"][u]):int(table["first"][u]) + int(table["n_edges"][u])]:
            x, r = edges[int(e)], rows[at]
            assert (r["ctg"], r["rid0"], r["rid1"], r["s"], r["e"], r["strand0"], r["strand1"]) == (j, x["v_rid"], x["w_rid"], x["sp"], x["tp"], 1 - x["v_end"], 1 - x["w_end"])
            at += 1
        if table["circular"][u]:
            assert rows[at - 1]["rid1"] == rows[int(segments["first_row"][j])]["rid0"]      # the closing edge is there
    # links: all pairs
    s = [(int(r["s_rid"]) << 1 | int(r["s_end"])) for r in table]
    t = [(int(r["t_rid"]) << 1 | int(r["t_end"])) for r in table]
    by_s = {}
    for b in range(n_u):
        by_s.setdefault(s[b], []).append(b)
    brute = sorted((a, b) for a in range(n_u) for b in by_s.get(t[a], []))
    if n_u <= 400:
        assert brute == sorted((a, b) for a in range(n_u) for b in range(n_u) if t[a] == s[b])   # the O(U^2) comparison itself
    assert directed == brute
    dset = set(directed)
    assert all((dual[b], dual[a]) in dset and (dual[b], dual[a]) != (a, b) for a, b in directed)   # closed under the dual
    assert len(links) * 2 == len(directed)
    kept = [(a, b) for a, b in brute if (a, b) < (dual[b], dual[a])]
    seg_of = {u: j for j, u in enumerate(canon)}
    want = [(seg_of[min(a, dual[a])], seg_of[min(b, dual[b])], int(a > dual[a]), int(b > dual[b])) for a, b in kept]
    assert [(int(l["from_seg"]), int(l["to_seg"]), int(l["from_rev"]), int(l["to_rev"])) for l in links] == want
    # links_directed = the sum over the directed unitigs a of the G out-degree of t(a): i * o per non-simple node, 1 per ring
    v, w = GF.node_keys(edges)
    g = [int(e) for e in np.flatnonzero(edges["type"] == SG.G)]
    outdeg, indeg = {}, {}
    for e in g:
        outdeg[v[e]] = outdeg.get(v[e], 0) + 1
        indeg[w[e]] = indeg.get(w[e], 0) + 1
    assert len(directed) == sum(outdeg.get(t[a], 0) for a in range(n_u))
    non_simple = [x for x in set(outdeg) | set(indeg) if not (outdeg.get(x, 0) == 1 and indeg.get(x, 0) == 1)]
    assert len(directed) == sum(indeg.get(x, 0) * outdeg.get(x, 0) for x in non_simple) + int(table["circular"].sum())
    # the text
    seg, lk = GF.parse(text)
    assert list(seg) == [b"utg%06d" % u for u in canon] and set(seg.values()) <= {b"*"} and len(lk) == len(links)
    assert text.count(b"\n") == 1 + len(canon) + len(links)
    if name == "none":
        assert text == GF.HEADER


def test_the_text_with_bases(restated):
    edges, table, paths, (segments, _, _, links, _) = restated["forks"]
    bases = [b"ACGT" * (j + 1) for j in range(len(segments))]
    s2, _, _, _, text = GF.gfa(edges, table, paths, bases)
    seg, lk = GF.parse(text)
    assert list(seg.values()) == bases and len(lk) == len(links)
    assert [int(x) for x in s2["seq_len"]] == [len(b) for b in bases] and int(s2["seq_off"][1]) == 4
    assert text.startswith(GF.HEADER + b"S\tutg%06d\tACGT\tLN:i:4\n" % int(segments["unitig"][0]))


def test_what_the_cases_hold(restated):
    """the shapes the GPU test needs are in the fixture (test_gpu_gfa.py asserts them again on what the device returns)"""
    seen = set()
    for name in CASES:
        _, table, _, (segments, _, directed, _, _) = restated[name]
        if table["circular"].sum():
            seen.add("ring")
            ring = [u for u in range(len(table)) if table["circular"][u]]
            assert all((u, u) in directed for u in ring)                                        # the self link of a ring
        lin = table[table["circular"] == 0]
        if ((lin["s_rid"] == lin["t_rid"]) & (lin["s_end"] == lin["t_end"])).any():
            seen.add("linear s == t")
        if len(table) and table["n_edges"].max() > 256:
            seen.add("long")
        if any(int(s["dual"]) != int(s["unitig"]) + 1 or int(s["unitig"]) % 2 for s in segments):
            seen.add("not an adjacent pair")
    assert seen == {"ring", "linear s == t", "long", "not an adjacent pair"}
