"""The unitig rule without a GPU: the plain-Python restatement (tests/utg_util.py) reproduces every case of tests/golden/utg_cases.npz --
what the real identify_simple_paths made of the case under two hash seeds, normalised (via dropped, rings opened at their first edge,
lines in the order of their first edges).  This is what lets the GPU tests use inputs that have no fixture."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_util as U
import sgraph_util as SG
import utg_util as UT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["single", "chains", "long", "rings", "dense", "quant", "none", "forks", "typed"]


@pytest.fixture(scope="module")
def fixture():
    return UT.load_fixture()


def case_edges(z, cases, name):
    c = cases[name]
    if c["kind"] == "edges":
        return UT.fixture_edges(z, name)
    return SG.string_graph_of_full_text(U.orc_dedup(UT.fixture_recs(z, c))[0], c["min_len"], c["min_idt"])[1]


def test_fixture_is_pinned(fixture):
    z, cases = fixture
    prov = json.load(open(os.path.join(ROOT, "tests", "golden", "utg_cases.provenance.json")))
    assert prov["cases"] == cases and prov["hash_seeds"] == [1, 4242] and prov["lfc"] is False and prov["disable_chimer_bridge_removal"] is True
    assert set(cases) == set(CASES)
    for name in CASES:
        utg = z[name + "_utg"].tobytes()
        s = prov["summary"][name]
        assert hashlib.sha256(utg).hexdigest() == s["sha256"] and utg.count(b"\n") == s["unitigs"], name
    s = prov["summary"]
    assert s["single"]["unitigs"] == 2 and s["none"]["unitigs"] == 0 and z["none_utg"].tobytes() == b""
    assert s["long"]["longest_edges"] == 4099 > 2 ** 12 and s["long"]["longest_line"] > 40000
    assert s["rings"]["closed"] == 6 and s["rings"]["longest_edges"] == 1000
    assert s["chains"]["unitigs"] == 24 and s["forks"]["closed"] == 4 and s["typed"]["sha256"] == s["forks"]["sha256"] and s["typed"]["input"] > s["forks"]["input"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "utg_cases.npz")) < 1_000_000


@pytest.mark.parametrize("name", CASES)
def test_the_restatement_reproduces_the_reference(fixture, name):
    z, cases = fixture
    edges = case_edges(z, cases, name)
    text, table, paths = UT.unitigs(edges)
    assert UT.drop_via(text) == z[name + "_utg"].tobytes()
    assert UT.via_is_second_node(text)
    UT.check_against_edges(edges, text, table, paths)


def test_what_the_cases_are_there_for(fixture):
    z, cases = fixture
    _, table, _ = UT.unitigs(case_edges(z, cases, "single"))
    assert len(table) == 2 and all(table["n_edges"] == 1) and all(table["via_rid"] == table["t_rid"]) and all(table["via_end"] == table["t_end"])
    _, table, paths = UT.unitigs(case_edges(z, cases, "rings"))
    assert all(table["circular"] == 1) and sorted(table["n_edges"]) == [3, 3, 64, 64, 1000, 1000]
    assert all(paths[int(r["first"])] == min(paths[int(r["first"]):int(r["first"]) + int(r["n_edges"])]) for r in table)
    assert any(paths[int(r["first"])] != 0 for r in table)
    text, table, _ = UT.unitigs(case_edges(z, cases, "forks"))
    closed = table[(table["s_rid"] == table["t_rid"]) & (table["s_end"] == table["t_end"])]
    assert sorted(closed["circular"]) == [0, 0, 1, 1]                                     # the cycle through one non-simple node is not circular
    assert {1, 3, 5, 6} == set(int(x) for x in table["n_edges"]) and (table["n_edges"] == 1).sum() >= 6   # the chain falls into 5 + 3 + 3
    assert sorted(table["n_edges"]) == sorted(UT.unitigs(case_edges(z, cases, "typed"))[1]["n_edges"])


def test_the_checks_name_the_smallest_offending_edge(fixture):
    z, cases = fixture
    edges = UT.fixture_edges(z, "forks")
    g = [int(e) for e in np.flatnonzero(edges["type"] == SG.G)]
    bad = edges.copy()
    bad["type"][g[5]] = SG.TR                                                             # its reverse stays G
    rv = next(e for e in g if (edges["v_rid"][e], edges["v_end"][e], edges["w_rid"][e], edges["w_end"][e]) ==
              (edges["w_rid"][g[5]], 1 - edges["w_end"][g[5]], edges["v_rid"][g[5]], 1 - edges["v_end"][g[5]]))
    with pytest.raises(UT.Invalid) as ei:
        UT.unitigs(bad)
    assert (ei.value.rule, ei.value.index) == ("reverse", rv)
    bad = np.concatenate([edges, edges[g[3]:g[3] + 1]])
    with pytest.raises(UT.Invalid) as ei:
        UT.unitigs(bad)
    assert (ei.value.rule, ei.value.index) == ("duplicate", len(edges))
    bad = edges.copy()
    bad["w_rid"][g[7]] = bad["v_rid"][g[7]]
    with pytest.raises(UT.Invalid) as ei:
        UT.unitigs(bad)
    assert (ei.value.rule, ei.value.index) == ("self", g[7])


@pytest.mark.parametrize("seed,n_pairs", [(1, 1000), (2, 2500)])
def test_random_arrays_are_valid_and_partitioned(seed, n_pairs):
    edges = UT.random_symmetric_edges(seed, n_pairs)
    text, table, paths = UT.unitigs(edges)
    UT.check_against_edges(edges, text, table, paths)
    assert table["circular"].sum() >= 2 and table["n_edges"].max() > 64 and (edges["type"] != SG.G).sum() > 0
    assert 2 * n_pairs <= (edges["type"] == SG.G).sum()
