"""The chimer bridge step's rule without a GPU: the plain-Python restatement (tests/chimer_util.py) reproduces, byte for byte, every
sg_edges_list and the sorted chimers_nodes lines that the real generate_string_graph wrote with its bfs_nodes popping the smallest
(rid, end) first (tests/golden/chimer_cases*.npz, made by make_golden_chimer.py), and the flag-off file without the pass."""
import hashlib
import json
import os

import numpy as np
import pytest

import chimer_util as CU
import oracle_util as U
import sgraph_util as SG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["bridge", "bridge_tr", "no_bridge_shared", "rejoin_near", "rejoin_tr_only", "cand_needs_unreduced", "pool_choice", "leaf_start", "depth", "sim",
         "none", "single"]


@pytest.fixture(scope="module")
def fixture():
    return CU.load_fixture()


@pytest.fixture(scope="module")
def prov():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "chimer_cases.provenance.json")))


def case_text(z, name):
    return U.orc_dedup(SG.fixture_recs(z, name))[0]


def test_fixture_is_pinned(fixture, prov):
    z, cases = fixture
    assert prov["cases"] == cases and set(cases) == set(CASES)
    assert prov["disable_chimer_bridge_removal"] is False and prov["lfc"] is False
    assert prov["pinned_policy"] == "smallest" and prov["policies"] == ["smallest", "largest", "random1", "random2", "builtin"] and prov["hash_seeds"] == [1, 4242]
    for name in cases:
        s = prov["summary"][name]
        sg, nodes, off = (z[name + k].tobytes() for k in ("_sg", "_nodes", "_off"))
        assert (hashlib.sha256(sg).hexdigest(), hashlib.sha256(nodes).hexdigest(), hashlib.sha256(off).hexdigest()) == (s["sha256"], s["nodes_sha256"], s["off_sha256"]), name
        assert sg.count(b"\n") == s["edges"] == off.count(b"\n") and nodes.count(b"\n") == 2 * s["chosen"] and CU.stats_of_text(sg)[1] == s["C"], name
        recs = SG.fixture_recs(z, name)
        assert int((recs["y0"] >> np.uint64(32)).max()) < 2**31 and int((recs["y1"] >> np.uint64(32)).max()) < 2**31
    for name in ("chimer_cases.npz", "chimer_cases_sim.npz"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < 1_000_000


def test_what_the_cases_are_there_for(fixture, prov):
    z, _ = fixture
    s = prov["summary"]
    assert (s["bridge"]["G"], s["bridge"]["TR"], s["bridge"]["C"], s["bridge"]["chosen"]) == (28, 24, 4, 2)
    assert s["pool_choice"]["unanimous"] is False and all(s[k]["unanimous"] for k in ("bridge", "bridge_tr", "no_bridge_shared", "leaf_start", "depth"))
    assert all(s[k]["C"] == 0 for k in ("no_bridge_shared", "rejoin_near", "rejoin_tr_only", "cand_needs_unreduced", "none", "single"))
    assert s["no_bridge_shared"]["past_test1"] == 0 and s["rejoin_near"]["past_test1"] == 2 and s["rejoin_tr_only"]["past_test1"] == 2
    sim = s["sim"]
    assert sim["chosen"] >= 20 and sim["past_test1"] > sim["chosen"] and sim["max_out_degree"] > 64
    on, off = z["sim_sg"].tobytes().split(b"\n"), z["sim_off"].tobytes().split(b"\n")
    assert any(a != b and not a.endswith(b" C") for a, b in zip(on, off))      # a later S / R / G decision changed
    assert z["none_sg"].tobytes() == b"" and z["single_sg"].tobytes().count(b"\n") == 2


@pytest.mark.parametrize("name", CASES)
def test_the_restatement_reproduces_the_reference(fixture, prov, name):
    z, cases = fixture
    c = cases[name]
    want = z[name + "_sg"].tobytes()
    got, recs, stats, ch, nodes = CU.string_graph_of_full_text(case_text(z, name), c["min_len"], c["min_idt"])
    assert got == want
    assert b"".join(sorted(nodes.splitlines(True))) == z[name + "_nodes"].tobytes()
    counts, n_c = CU.stats_of_text(want)
    assert {k: stats[k] for k in CU.COUNTS} == counts and ch["c_edges"] == n_c and counts["edges"] - sum(counts[k] for k in CU.COUNTS[1:]) == n_c
    assert ch["chosen"] == prov["summary"][name]["chosen"] and ch["past_test1"] == prov["summary"][name]["past_test1"] and ch["candidates"] >= ch["past_test1"]
    assert np.array_equal(recs, CU.edges_of_text(want))
    # ... and without the pass it is sgraph_util's restatement, which gives the flag-off file
    off = CU.string_graph_of_full_text(case_text(z, name), c["min_len"], c["min_idt"], chimer=False)
    assert off[0] == z[name + "_off"].tobytes() == SG.string_graph_of_full_text(case_text(z, name), c["min_len"], c["min_idt"])[0]
    assert off[3] == dict.fromkeys(CU.CHIMER_STATS, 0) and off[4] == b""


def test_entry_points_are_declared_and_exported():
    import re
    from peregrine_amd import _lib, shimmer
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgx.h")).read(), flags=re.S)
    for n in ("pgx_sgraph_chimer_stats", "pgx_sgraph_chimer_nodes"):
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr) and n in _lib.EXPORTS and getattr(lib, n).argtypes, n
    assert re.search(r"#define\s+PGX_SGRAPH_CHIMER_ORDERED\s+4u", hdr) and re.search(r"PGX_SGRAPH_C\s*=\s*4\b", hdr)
    assert shimmer.SGRAPH_CHIMER_ORDERED == 4 and shimmer.SGRAPH_TYPES[4] == "C" == CU.TYPE_NAMES[4].decode() and shimmer.SGRAPH_TYPE_OTHER == CU.C
    st = lib.pgx_sgraph_chimer_stats(None, None)
    assert st == _lib.PGX_EARG and b"pgx_sgraph_chimer_stats" in lib.pgx_last_error()
