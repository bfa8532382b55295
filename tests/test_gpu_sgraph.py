"""The string graph on the GPU (pgx_sgraph_build / _stats / _edges / _text / _free, DedupStream.string_graph, shimmer.string_graph, both
`shmr_sgraph` commands): whatever the cut of the stream into feeds, the text is the real generate_string_graph's sg_edges_list of the
fixtures (tests/golden/sgraph_cases*.npz, graph_filter_cases.npz) byte for byte, and on inputs without a fixture the plain-Python
restatement's (tests/sgraph_util.py, which test_sgraph_rule.py holds to the same fixtures)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dedup_graph_util as DG
import golden_util as G
import oracle_util as U
import sgraph_util as SG
from peregrine_amd import _lib, shimmer
from peregrine_amd.formats import OVLP_DTYPE
from peregrine_amd.shimmer import DedupStream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rec = DG.rec
CASES = ["dense", "dense_idt", "dense_len", "quant", "spur_a", "spur_b", "directed", "none", "single", "graph_filter"]
COUNTS = ("edges", "n_g", "n_tr", "n_s", "n_r")


@pytest.fixture(scope="module")
def fixture():
    """name -> (records, min_len, min_idt, the reference's sg_edges_list, its edge records and counts), computed once and left alone"""
    z, cases = SG.load_fixture()
    out = {}
    for name, c in cases.items():
        sg = z[name + "_sg"].tobytes()
        out[name] = (SG.fixture_recs(z, c["recs"]), c["min_len"], c["min_idt"], sg, SG.edges_of_text(sg), SG.stats_of_text(sg))
    gf = G.load("graph_filter_cases.npz")
    sg = gf["sg_edges_list"].tobytes()
    out["graph_filter"] = (gf["recs"], 4000, 96.0, sg, SG.edges_of_text(sg), SG.stats_of_text(sg))
    return out


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


def check_graph(g, sg, edges, counts, max_lines=5000):
    parts = list(g.text(max_lines))
    assert all(0 < p.count(b"\n") <= max_lines and p.endswith(b"\n") for p in parts)
    assert b"".join(parts) == sg
    got = g.edges()
    assert got.dtype == SG.EDGE_DTYPE == shimmer.SGRAPH_EDGE_DTYPE and np.array_equal(got, edges)
    assert {k: g.stats[k] for k in COUNTS} == counts
    assert g.stats["edges"] <= 2 * g.stats["rows_pass"] <= 2 * g.stats["rows_in"]
    if len(edges) > 10:
        assert np.array_equal(g.edges(3, 5), edges[3:8])


@pytest.mark.parametrize("way", ["one", "pieces", "dev"])
@pytest.mark.parametrize("name", CASES)
def test_fixture_cases(fixture, name, way):
    recs, min_len, min_idt, sg, edges, counts = fixture[name]
    with DedupStream(graph_ready=True) as ds:
        feed(ds, recs, way)
        with ds.string_graph(min_len, min_idt) as g:
            check_graph(g, sg, edges, counts)


@pytest.mark.parametrize("cap", [48, 3, 0])
def test_nodes_beyond_the_lds_tables(fixture, monkeypatch, cap):
    """PGX_SGRAPH_DEG_MAX below the dense case's largest out-degree (95): those nodes take the pass on tables in HBM"""
    recs, min_len, min_idt, sg, edges, counts = fixture["dense"]
    monkeypatch.setenv("PGX_SGRAPH_DEG_MAX", str(cap))
    with shimmer.string_graph(recs, min_len, min_idt) as g:
        assert g.stats["max_out_degree"] == 95 > cap
        check_graph(g, sg, edges, counts)


@pytest.mark.parametrize("seed,n_reads,genome,share,min_len", [(11, 120, 3000, 0.2, 2000), (12, 200, 9000, 0.0, 3000), (13, 90, 1500, 0.1, 0)])
def test_further_seeds_against_the_restatement(seed, n_reads, genome, share, min_len):
    recs = DG.make_records(seed=seed, n_reads=n_reads, genome=genome, contained_share=share)
    want, edges, stats = SG.string_graph_of_full_text(U.orc_dedup(recs)[0], min_len, 96.0)
    assert stats["edges"] > 500 and min(stats[k] for k in COUNTS) > 0
    with shimmer.string_graph(recs, min_len, 96.0, piece=777) as g:
        assert g.stats == stats                 # all ten: rows, nodes, the largest out-degree and the spur candidates too
        check_graph(g, want, edges, {k: stats[k] for k in COUNTS}, max_lines=1 << 20)


def _native_cmd():
    exe = os.path.join(ROOT, "bin", "native", "shmr_sgraph")
    return [exe] if os.path.exists(exe) else [os.path.join(ROOT, "bin", "native", "pgx_cli"), "shmr_sgraph"]


def test_both_commands_file_to_file(fixture, tmp_path):
    recs, min_len, min_idt, sg, _, _ = fixture["dense"]
    src = tmp_path / "ovlp.dat"
    recs.tofile(src)
    env = dict(os.environ, PGX_DEDUP_PIECE="10000")     # four feeds, two pieces of text
    outs = []
    for k, cmd in enumerate((_native_cmd(), [sys.executable, os.path.join(ROOT, "bin", "shmr_sgraph")])):
        dst = tmp_path / f"sg_edges_list.{k}"
        with open(src, "rb") as fi, open(dst, "wb") as fo:
            r = subprocess.run(cmd + ["--min_len", str(min_len), "--min_idt=%s" % min_idt], stdin=fi, stdout=fo, stderr=subprocess.PIPE, env=env, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append(dst.read_bytes())
        for flag, word in (("--lfc", b"lfc"), ("--chimer_bridge_removal", b"chimer")):
            r = subprocess.run(cmd + [flag], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
            assert r.returncode != 0 and r.stdout == b"" and word in r.stderr, (cmd, flag, r.stderr)
    assert outs[0] == outs[1] == sg
    # an empty result is an empty file
    r = subprocess.run(_native_cmd(), input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert (r.returncode, r.stdout) == (0, b""), r.stderr


def raw_build(h, flags=0, min_len=4000, min_idt=96.0):
    lib = _lib.load()
    g = C.c_void_p(0xDEAD0000BEEF)
    rc = lib.pgx_sgraph_build(h, min_len, min_idt, flags, C.byref(g))
    return rc, g, lib.pgx_last_error()


LINES = np.concatenate([rec(1, 2), rec(3, 1), rec(4, 5), rec(5, 6), rec(6, 4), rec(2, 3), rec(7, 8), rec(8, 9), rec(9, 1), rec(1, 30, typ=2)])


def test_error_paths_leave_the_stream_as_stated():
    lib = _lib.load()
    want = DG.select_graph_lines(U.orc_dedup(LINES)[0])
    # a plain stream: refused, and it goes on as a plain stream
    with DedupStream() as ds:
        rc, g, msg = raw_build(ds.h)
        assert rc == _lib.PGX_ESTATE and not g.value and b"graph-mode" in msg
        assert ds.feed(LINES) == U.orc_dedup(LINES)[0]
    # flags: each refused with its reason; the stream takes further feeds, builds and drains
    with DedupStream(graph_ready=True) as ds:
        ds.feed(LINES[:5])
        for flags, word in ((shimmer.SGRAPH_CHIMER_BRIDGE, b"chimer"), (shimmer.SGRAPH_LFC, b"lfc"), (3, b"chimer"), (8, b"flag")):
            rc, g, msg = raw_build(ds.h, flags)
            assert rc == _lib.PGX_EINVAL and not g.value and word in msg, (flags, msg)
        with pytest.raises(_lib.PgxError, match="lfc"):
            ds.string_graph(lfc=True)
        ds.feed(LINES[5:])
        with ds.string_graph(0, 0.0) as g:
            assert g.stats["rows_in"] == want.count(b"\n")
        with pytest.raises(_lib.PgxError):           # the build compacted the rows: feeds are refused as after a drain
            ds.feed(LINES[:1])
        assert b"".join(ds.drain()) == want
        # ... and the last drain released the rows
        rc, g, msg = raw_build(ds.h)
        assert rc == _lib.PGX_ESTATE and not g.value and b"drained" in msg
        assert ds.close() == (len(LINES), len(LINES))
    # m_size == 0 in a kept row: refused, the row is named, and the drain still prints every line
    recs = np.concatenate([LINES[:4], rec(61, 62, m_size=0, dist=0), LINES[4:]])
    with DedupStream(graph_ready=True) as ds:
        ds.feed(recs)
        rc, g, msg = raw_build(ds.h)
        kept = DG.select_graph_lines(U.orc_dedup(np.concatenate([LINES[:4], rec(61, 62), LINES[4:]]))[0])
        row = [ln.split()[0] for ln in kept.split(b"\n")[:-1]].index(b"000000061")
        assert rc == _lib.PGX_EINVAL and not g.value and (b"row %d " % row) in msg and b"m_size" in msg, msg
        text = b"".join(ds.drain())
        assert text.count(b"\n") == kept.count(b"\n") and b"nan" in text
    assert lib.pgx_sgraph_free(None) == 0


def test_the_graph_and_the_drain_do_not_disturb_each_other(fixture):
    recs, min_len, min_idt, sg, edges, counts = fixture["quant"]
    want = DG.select_graph_lines(U.orc_dedup(recs)[0])
    _lib.mem_ledger(reset_peak=True)
    ds = DedupStream(graph_ready=True)
    ds.feed(recs)
    g = ds.string_graph(min_len, min_idt)
    first = g.text(1000)
    head = next(first)                                   # part of the text, then the drain, then the rest
    assert b"".join(ds.drain(3000)) == want
    g2 = None
    with pytest.raises(_lib.PgxError):
        g2 = ds.string_graph(min_len, min_idt)           # the rows are gone
    assert g2 is None and ds.close() == (len(recs), U.orc_dedup(recs)[0].count(b"\n"))
    assert head + b"".join(first) == sg                  # the graph owns its arrays: the stream is closed
    assert np.array_equal(g.edges(), edges) and {k: g.stats[k] for k in COUNTS} == counts
    assert list(g.text()) == []
    g.close()
    g.close()
    with pytest.raises(_lib.PgxError):
        g.edges()
    units = C.c_uint64(0)
    assert _lib.load().pgx_timing_get(b"sgraph", None, None, C.byref(units)) == 0 and units.value > 0
    assert _lib.mem_ledger()["peak_by_tag"].get("sgraph", 0) > 0


def test_one_shot_and_write(fixture, tmp_path):
    recs, min_len, min_idt, sg, _, _ = fixture["directed"]
    with shimmer.string_graph(recs, min_len, min_idt) as g:
        assert g.write(str(tmp_path / "sg")) == len(sg)
    assert (tmp_path / "sg").read_bytes() == sg
    src = tmp_path / "ovlp.dat"
    recs.tofile(src)
    st = shimmer.shmr_sgraph(str(src), str(tmp_path / "sg2"), min_len, min_idt)
    assert (tmp_path / "sg2").read_bytes() == sg and st["edges"] == sg.count(b"\n")
    with shimmer.string_graph(np.zeros(0, OVLP_DTYPE)) as g:
        assert g.stats["edges"] == 0 and g.write(str(tmp_path / "empty")) == 0
    assert (tmp_path / "empty").read_bytes() == b""
