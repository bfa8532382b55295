"""The chimer bridge step on the GPU (PGX_SGRAPH_CHIMER_ORDERED: DedupStream.string_graph(chimer_ordered=True), StringGraph.chimer_stats /
chimers_nodes, both `shmr_sgraph --chimer_bridge_ordered` commands): whatever the cut of the stream into feeds, the text is byte for byte
the sg_edges_list the real generate_string_graph wrote with bfs_nodes popping the smallest (rid, end) first
(tests/golden/chimer_cases*.npz), chimers_nodes its sorted lines, and on inputs without a fixture the plain-Python restatement's
(tests/chimer_util.py, which test_chimer_rule.py holds to the same fixtures)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chimer_util as CU
import dedup_graph_util as DG
import oracle_util as U
import sgraph_util as SG
from peregrine_amd import _lib, shimmer
from peregrine_amd.shimmer import DedupStream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rec = DG.rec
LINES = np.concatenate([rec(1, 2), rec(3, 1), rec(4, 5), rec(5, 6), rec(6, 4), rec(2, 3), rec(7, 8), rec(8, 9), rec(9, 1), rec(1, 30, typ=2)])


def feed(ds, recs, way):
    if way == "one":
        assert ds.feed(recs) == b""
    elif way == "pieces":
        for a in range(0, len(recs), 1000):
            assert ds.feed(recs[a:a + 1000]) == b""
    else:
        import torch
        d = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).copy()).to("cuda:0")
        assert ds.feed_dev(d.data_ptr(), len(recs)) == b""
        torch.cuda.synchronize()


def raw_build(h, flags=0, min_len=4000, min_idt=96.0):
    lib = _lib.load()
    g = C.c_void_p(0xDEAD0000BEEF)
    rc = lib.pgx_sgraph_build(h, min_len, min_idt, flags, C.byref(g))
    return rc, g, lib.pgx_last_error()


CASES = ["bridge", "bridge_tr", "no_bridge_shared", "rejoin_near", "rejoin_tr_only", "cand_needs_unreduced", "pool_choice", "leaf_start", "depth", "sim",
         "none", "single"]


@pytest.fixture(scope="module")
def fixture():
    """name -> (records, min_len, min_idt, the pinned sg_edges_list, its edge records and counts, the sorted chimers_nodes, what the
    provenance says of the case, the flag-off file), computed once and left alone"""
    z, cases = CU.load_fixture()
    prov = json.load(open(os.path.join(ROOT, "tests", "golden", "chimer_cases.provenance.json")))["summary"]
    out = {}
    for name, c in cases.items():
        sg = z[name + "_sg"].tobytes()
        out[name] = (SG.fixture_recs(z, name), c["min_len"], c["min_idt"], sg, CU.edges_of_text(sg), CU.stats_of_text(sg), z[name + "_nodes"].tobytes(), prov[name],
                     z[name + "_off"].tobytes())
    return out


def sorted_lines(text: bytes) -> bytes:
    return b"".join(sorted(text.splitlines(True)))


def check_graph(g, sg, edges, counts, nodes, max_lines=5000):
    counts, n_c = counts
    parts = list(g.text(max_lines))
    assert all(0 < p.count(b"\n") <= max_lines and p.endswith(b"\n") for p in parts)
    assert b"".join(parts) == sg
    got = g.edges()
    assert got.dtype == SG.EDGE_DTYPE and np.array_equal(got, edges)
    assert {k: g.stats[k] for k in CU.COUNTS} == counts
    ch = g.chimer_stats
    assert ch["c_edges"] == n_c == g.stats["edges"] - sum(g.stats[k] for k in CU.COUNTS[1:])
    assert sorted_lines(g.chimers_nodes()) == nodes and ch["chosen"] * 2 == nodes.count(b"\n") and ch["candidates"] >= ch["past_test1"] >= ch["chosen"]
    return ch


@pytest.mark.parametrize("way", ["one", "pieces", "dev"])
@pytest.mark.parametrize("name", CASES)
def test_fixture_cases(fixture, name, way):
    recs, min_len, min_idt, sg, edges, counts, nodes, prov, _ = fixture[name]
    with DedupStream(graph_ready=True) as ds:
        feed(ds, recs, way)
        with ds.string_graph(min_len, min_idt, chimer_ordered=True) as g:
            ch = check_graph(g, sg, edges, counts, nodes)
            assert ch["past_test1"] == prov["past_test1"] and ch["chosen"] == prov["chosen"]
            lines = g.chimers_nodes().splitlines()
            assert all(a[:-1] == b[:-1] and {a[-1:], b[-1:]} == {b"B", b"E"} for a, b in zip(lines[::2], lines[1::2]))   # a node, then its reverse end


@pytest.mark.parametrize("name,lds,deg", [("sim", 40, None), ("sim", 0, None), ("sim", None, 16), ("sim", 7, 16), ("pool_choice", 3, None), ("pool_choice", 0, 16),
                                          ("rejoin_tr_only", 5, None)])
def test_candidates_beyond_the_lds_table(fixture, monkeypatch, name, lds, deg):
    """PGX_SGRAPH_CHIMER_LDS below the cases' set sizes: those candidates take the tests on tables in HBM (0: every one of them);
    PGX_SGRAPH_DEG_MAX 16: the transitive reduction before the step runs from HBM too"""
    recs, min_len, min_idt, sg, edges, counts, nodes, prov, _ = fixture[name]
    if lds is not None:
        monkeypatch.setenv("PGX_SGRAPH_CHIMER_LDS", str(lds))
    if deg is not None:
        monkeypatch.setenv("PGX_SGRAPH_DEG_MAX", str(deg))
    with shimmer.string_graph(recs, min_len, min_idt, chimer_ordered=True) as g:
        ch = check_graph(g, sg, edges, counts, nodes)
        assert ch["past_test1"] == prov["past_test1"]


@pytest.mark.parametrize("seed", [23, 24, 25, 26])
def test_further_seeds_against_the_restatement(seed):
    recs = CU.chimeric_sim(seed=seed, n_reads=360, genome=120_000, n_chimers=100)
    want, edges, stats, ch, nodes = CU.string_graph_of_full_text(U.orc_dedup(recs)[0], 2000, 96.0)
    assert ch["chosen"] >= 20 and ch["past_test1"] > ch["chosen"] and stats["max_out_degree"] > 64
    with shimmer.string_graph(recs, 2000, 96.0, piece=777, chimer_ordered=True) as g:
        assert g.stats == stats and g.chimer_stats == ch
        assert g.chimers_nodes() == nodes                   # creation order, not only the sorted lines
        check_graph(g, want, edges, CU.stats_of_text(want), sorted_lines(nodes), max_lines=1 << 20)


def test_without_the_flag_nothing_changes(fixture):
    recs, min_len, min_idt, sg, _, _, _, _, off = fixture["sim"]
    assert off != sg
    with shimmer.string_graph(recs, min_len, min_idt) as g:
        assert b"".join(g.text()) == off
        assert g.chimer_stats == dict.fromkeys(CU.CHIMER_STATS, 0) and g.chimers_nodes() == b""
        assert g.stats["edges"] == sum(g.stats[k] for k in CU.COUNTS[1:])


def _commands():
    exe = os.path.join(ROOT, "bin", "native", "shmr_sgraph")
    native = [exe] if os.path.exists(exe) else [os.path.join(ROOT, "bin", "native", "pgx_cli"), "shmr_sgraph"]
    return native, [sys.executable, os.path.join(ROOT, "bin", "shmr_sgraph")]


def test_both_commands_file_to_file(fixture, tmp_path):
    recs, min_len, min_idt, sg, _, _, nodes, _, _ = fixture["sim"]
    src = tmp_path / "ovlp.dat"
    recs.tofile(src)
    env = dict(os.environ, PGX_DEDUP_PIECE="4000")     # three feeds, two pieces of text
    outs, files = [], []
    for k, cmd in enumerate(_commands()):
        dst, nf = tmp_path / f"sg_edges_list.{k}", tmp_path / f"chimers_nodes.{k}"
        extra = ["--chimers-nodes", str(nf)] if k == 0 else ["--chimers-nodes=%s" % nf]
        with open(src, "rb") as fi, open(dst, "wb") as fo:
            r = subprocess.run(cmd + ["--min_len", str(min_len), "--min_idt=%s" % min_idt, "--chimer_bridge_ordered"] + extra, stdin=fi, stdout=fo, stderr=subprocess.PIPE,
                               env=env, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append(dst.read_bytes()), files.append(nf.read_bytes())
        # --chimers-nodes without the option: refused before anything is read or written
        r = subprocess.run(cmd + ["--chimers-nodes", str(tmp_path / "never")], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
        assert r.returncode != 0 and r.stdout == b"" and b"chimer_bridge_ordered" in r.stderr and not (tmp_path / "never").exists(), (cmd, r.stderr)
    assert outs[0] == outs[1] == sg
    assert files[0] == files[1] and sorted_lines(files[0]) == nodes


def test_unitigs_and_contig_paths_of_the_flagged_graph(fixture, tmp_path):
    """--utg-data / --ctg-paths written from the flagged build are what pgx_unitigs_build / pgx_ctg_paths_build make of the parsed text of
    the same graph, and graph_to_path takes the three files"""
    recs, min_len, min_idt, sg, _, _, _, _, _ = fixture["sim"]
    src = tmp_path / "ovlp.dat"
    recs.tofile(src)
    p = {k: str(tmp_path / k) for k in ("sg", "utg", "utg_data", "ctg_paths", "nodes")}
    st = shimmer.shmr_sgraph(str(src), p["sg"], min_len, min_idt, utg_path=p["utg"], utg_data_path=p["utg_data"], ctg_paths_path=p["ctg_paths"], chimer_ordered=True,
                             chimers_nodes_path=p["nodes"])
    assert open(p["sg"], "rb").read() == sg and st["edges"] == sg.count(b"\n")
    edges = shimmer.read_sg_edges_list(p["sg"])
    assert int((edges["type"] == shimmer.SGRAPH_TYPE_OTHER).sum()) == CU.stats_of_text(sg)[1] > 0
    with shimmer.unitigs(edges) as u:
        assert b"".join(u.text()) == open(p["utg"], "rb").read() != b""
    with shimmer.contig_paths(edges) as c:
        assert c.utg_text() == open(p["utg_data"], "rb").read() != b""
        assert c.ctg_text() == open(p["ctg_paths"], "rb").read() != b""
    with shimmer.graph_to_path(p["sg"], p["utg_data"], p["ctg_paths"]) as t:
        assert t.stats and sum(len(x) for x in t.text(0)) > 0
    with pytest.raises(ValueError):
        shimmer.shmr_sgraph(str(src), p["sg"], min_len, min_idt, chimers_nodes_path=p["nodes"])


def test_flag_combinations_and_error_paths():
    want = DG.select_graph_lines(U.orc_dedup(LINES)[0])
    # a plain stream: refused as without the flag, and it goes on as a plain stream
    with DedupStream() as ds:
        rc, g, msg = raw_build(ds.h, shimmer.SGRAPH_CHIMER_ORDERED)
        assert rc == _lib.PGX_ESTATE and not g.value and b"graph-mode" in msg
        assert ds.feed(LINES) == U.orc_dedup(LINES)[0]
    # with bit 1 or bit 2 those bits' refusals win; the stream takes further feeds, builds and drains
    with DedupStream(graph_ready=True) as ds:
        ds.feed(LINES[:5])
        for flags, word in ((5, b"chimer"), (6, b"lfc"), (7, b"chimer"), (12, b"flag")):
            rc, g, msg = raw_build(ds.h, flags)
            assert rc == _lib.PGX_EINVAL and not g.value and word in msg, (flags, msg)
        with pytest.raises(_lib.PgxError, match="chimer"):
            ds.string_graph(chimer_bridge_removal=True, chimer_ordered=True)
        ds.feed(LINES[5:])
        rc, g, msg = raw_build(ds.h, shimmer.SGRAPH_CHIMER_ORDERED, 0, 0.0)
        assert rc == 0 and g.value
        st = (C.c_uint64 * 10)()
        assert _lib.load().pgx_sgraph_stats(g, st) == 0 and st[0] == want.count(b"\n")
        assert _lib.load().pgx_sgraph_free(g) == 0
        assert b"".join(ds.drain()) == want
    lib = _lib.load()
    text, n = C.c_void_p(0xDEAD0000BEEF), C.c_size_t(7)
    assert lib.pgx_sgraph_chimer_nodes(None, C.byref(text), C.byref(n)) == _lib.PGX_EARG and not text.value and n.value == 0
    assert lib.pgx_sgraph_chimer_stats(None, None) == _lib.PGX_EARG
