"""The assembly graph as GFA on the GPU (pgx_gfa_build / _build_files / _stats / _segments / _links / _rows / _text / _write / _free,
Unitigs.gfa, shimmer.assemble(gfa=True), `shmr_sgraph --gfa` in both forms): on every fixture case of test_gpu_utg.py the tables, the
rows and the text are the plain-Python restatement's (tests/gfa_util.py, which test_gfa_rule.py holds to a brute force); on simulated
reads every segment's bases are what ResidentDB.contigs makes of the restatement's rows."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gfa_util as GF
import sgraph_util as SG
import utg_util as UT
from peregrine_amd import _lib, formats, shimmer, simreads
from peregrine_amd.shimmer import DedupStream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC_CASES = ["single", "chains", "long", "rings", "dense", "quant", "none"]
EDGE_CASES = ["forks", "typed"]


@pytest.fixture(scope="module")
def fixture():
    """name -> (kind, records or edge array, min_len, min_idt), computed once and left alone"""
    z, cases = UT.load_fixture()
    out = {}
    for name, c in cases.items():
        if c["kind"] == "edges":
            out[name] = ("edges", UT.fixture_edges(z, name), 0, 0.0)
        else:
            out[name] = ("recs", UT.fixture_recs(z, c), c["min_len"], c["min_idt"])
    return out


@pytest.fixture(scope="module")
def case_edges(fixture):
    """name -> the case's edge records (of the device's string graph where the case is records), computed once and left alone"""
    out = {}
    for name, (kind, data, min_len, min_idt) in fixture.items():
        if kind == "recs":
            with shimmer.string_graph(data, min_len, min_idt) as g:
                out[name] = g.edges()
        else:
            out[name] = data
    return out


def stats_of(table, segments, rows, directed, links, bases=0):
    return dict(unitigs=len(table), segments=len(segments), rows=len(rows), links_directed=len(directed), links=len(links), bases=bases)


def check_gfa(f, u, edges, bases=None):
    """the device's tables, rows and text against the restatement's, over the device's own unitig table and paths"""
    table, paths = u.table(), u.paths()
    segments, rows, directed, links, text = GF.gfa(edges, table, paths, bases)
    got_s, got_l, got_r = f.segments(), f.links(), f.rows()
    assert got_s.dtype == GF.SEGMENT_DTYPE == shimmer.GFA_SEGMENT_DTYPE and got_l.dtype == GF.LINK_DTYPE == shimmer.GFA_LINK_DTYPE and got_r.dtype == _lib.TILE_ROW_DTYPE
    assert got_s.tobytes() == segments.tobytes() and got_l.tobytes() == links.tobytes()
    assert got_r.tobytes() == rows.astype(_lib.TILE_ROW_DTYPE).tobytes()
    assert f.stats == stats_of(table, segments, rows, directed, links, sum(len(b) for b in bases) if bases is not None else 0)
    got = f.text()
    assert got == text and f.text() == text                       # (the text is not used up)
    GF.parse(got)
    if len(segments) > 3:
        assert np.array_equal(f.segments(1, 2), segments[1:3]) and np.array_equal(f.rows(1, 2), got_r[1:3])
    return segments, rows, directed, links, text


@pytest.mark.parametrize("name", REC_CASES)
def test_fixture_cases_through_the_graph(fixture, name, tmp_path):
    _, recs, min_len, min_idt = fixture[name]
    with DedupStream(graph_ready=True) as ds:
        if len(recs):
            assert ds.feed(recs) == b""
        with ds.string_graph(min_len, min_idt) as g:
            edges = g.edges()
            with g.unitigs() as u:
                f = u.gfa(g)
                table = u.table()
                want = GF.gfa(edges, table, u.paths())
                with f:
                    check_gfa(f, u, edges)
                f = u.gfa(g)
    with f:                                                      # the graph and the unitigs are freed: the GFA owns its arrays
        assert f.text() == want[4] and f.segments().tobytes() == want[0].tobytes()
        assert f.write(str(tmp_path / "g.gfa")) == len(want[4]) and (tmp_path / "g.gfa").read_bytes() == want[4]
    if name == "none":
        assert want[4] == GF.HEADER and len(table) == 0


@pytest.mark.parametrize("name", REC_CASES + EDGE_CASES)
def test_fixture_cases_from_edge_records(case_edges, name):
    edges = case_edges[name]
    with shimmer.unitigs(edges) as u, u.gfa(edges) as f:
        check_gfa(f, u, edges)


def test_what_the_cases_hold_together(case_edges):
    """the shapes the rule's corners need, asserted on what the device returns so that a changed fixture cannot hide one"""
    seen = set()
    for name, edges in case_edges.items():
        with shimmer.unitigs(edges) as u, u.gfa(edges) as f:
            table, segments, links = u.table(), f.segments(), f.links()
        g = edges[edges["type"] == SG.G]
        if segments["circular"].sum():
            seen.add("a ring")
            ring = np.flatnonzero(segments["circular"])
            self_links = {int(l["from_seg"]) for l in links if l["from_seg"] == l["to_seg"] and l["from_rev"] == l["to_rev"] == 0}
            assert set(int(j) for j in ring) <= self_links                                     # L x + x + *
        lin = table[table["circular"] == 0]
        if ((lin["s_rid"] == lin["t_rid"]) & (lin["s_end"] == lin["t_end"])).any():
            seen.add("a linear unitig with s == t")
        if len(g) and np.unique(g["v_rid"].astype(np.int64) << 1 | g["v_end"], return_counts=True)[1].max() >= 2:
            seen.add("a node of out-degree 2")
        if len(segments) and segments["n_rows"].max() > 256:
            seen.add("a unitig of more than 256 edges")
        if ((segments["dual"] != segments["unitig"] + 1) | (segments["unitig"] % 2 == 1)).any():
            seen.add("a segment that is not the lower of an adjacent pair")
    assert seen == {"a ring", "a linear unitig with s == t", "a node of out-degree 2", "a unitig of more than 256 edges",
                    "a segment that is not the lower of an adjacent pair"}


CHILD = """
import sys, json, hashlib, numpy as np
sys.path.insert(0, %r)
from peregrine_amd import _lib, shimmer
z = np.load(%r)
out = {}
for name in z.files:
    e = z[name].view(shimmer.SGRAPH_EDGE_DTYPE).reshape(-1)
    with shimmer.unitigs(e) as u, u.gfa(e) as f:
        out[name] = [hashlib.sha256(x).hexdigest() for x in (f.text(), f.segments().tobytes(), f.links().tobytes(), f.rows().tobytes())] + [f.stats]
out["grid"] = int(_lib.load().pgx_stride_grid(2**40, 8))
print(json.dumps(out))
"""


def test_under_a_grid_of_one_workgroup(case_edges, tmp_path):
    """PGX_GRID_CAP=1 in a child process: one workgroup of the row kernel and of the link kernel takes every item, 256 at a time"""
    np.savez(tmp_path / "edges.npz", **{k: np.frombuffer(v.tobytes(), np.uint8) for k, v in case_edges.items()})
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, str(tmp_path / "edges.npz"))], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PGX_NO_TORCH="1", PGX_GRID_CAP="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().split("\n")[-1])
    assert got.pop("grid") == 1
    most_rows = most_links = 0
    for name, edges in case_edges.items():
        _, table, paths = UT.unitigs(edges)
        segments, rows, directed, links, text = GF.gfa(edges, table, paths)
        want = [hashlib.sha256(x).hexdigest() for x in (text, segments.tobytes(), links.tobytes(), rows.astype(_lib.TILE_ROW_DTYPE).tobytes())]
        assert got[name] == want + [stats_of(table, segments, rows, directed, links)], name
        most_rows, most_links = max(most_rows, len(rows)), max(most_links, len(directed))
    print("most rows", most_rows, "most directed links", most_links)
    assert most_rows > 2 * 256                                   # the workgroup takes a second and a third item of rows


# ---- sequences ----------------------------------------------------------------------------------------------------------------------
LUT = np.full(16, ord("N"), np.uint8)
LUT[[1, 2, 4, 8]] = [ord(c) for c in "ACGT"]


def read_bases(db, rid, strand) -> bytes:
    o, n = int(db.roff[rid]), int(db.rlen[rid])
    return LUT[(db.seqdb[o:o + n] >> (4 * strand)) & 15].tobytes()


def concat_sets(*dbs):
    rlen = np.concatenate([d.rlen for d in dbs])
    roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
    return formats.SeqDB(np.concatenate([d.seqdb for d in dbs]), np.arange(len(rlen), dtype=np.uint32), rlen, roff, None)


def bubble_set():
    """two haplotypes of a 60 kb genome at 12x each, the second with 4 kb inserted in the middle, in the manner of
    tests/test_gpu_assemble.py at a fifth of its size; seeds fixed.  On the GPU the graph holds the bubble: 7 segments, 8 links."""
    g = simreads.make_genome(60_000, 41)
    h = np.concatenate([g[:30_000], simreads.make_genome(4_000, 44), g[30_000:]])
    return concat_sets(simreads.simulate_reads(g, coverage=12.0, seed=17, mean_len=8000, sd_len=1500, err=0.01, wrap=0),
                       simreads.simulate_reads(h, coverage=12.0, seed=18, mean_len=8000, sd_len=1500, err=0.01, wrap=0))


def ring_set():
    """a circular genome of 40 kb at 15x: reads across the origin, so that the graph closes into rings of simple nodes; seed fixed.
    On the GPU the graph is two rings of 47 edges, one the reverse of the other."""
    g = simreads.make_genome(40_000, 51)
    return simreads.simulate_reads(g, coverage=15.0, seed=27, mean_len=8000, sd_len=1000, err=0.01, wrap=40_000)


class Job:
    """a read set on the device, its overlap records, its string graph (chimer_ordered, as assemble builds it) and unitigs"""

    def __init__(self, db):
        self.db = db
        self.rdb = shimmer.ResidentDB(db, 0)
        ix = self.rdb.index()
        self.recs, _ = self.rdb.overlap(ix.top, ix.top_mc)
        self.g = shimmer.string_graph(self.recs, chimer_ordered=True)
        self.edges = self.g.edges()
        self.u = self.g.unitigs()

    def close(self):
        self.u.close(), self.g.close(), self.rdb.close()

    def want_bases(self, rdb=None):
        """the restatement's rows through ResidentDB.contigs"""
        _, rows, _, _, _ = GF.gfa(self.edges, self.u.table(), self.u.paths())
        data, off = (rdb or self.rdb).contigs(rows.astype(_lib.TILE_ROW_DTYPE))
        return [data[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]


@pytest.fixture(scope="module")
def bubble():
    j = Job(bubble_set())
    yield j
    j.close()


def check_sequences(job, f, bases):
    segments, rows, _, links, text = check_gfa(f, job.u, job.edges, bases)
    seg, _ = GF.parse(text)                                      # (LN equals the length: parse asserts it)
    assert list(seg.values()) == bases
    for j, s in enumerate(segments):
        r0 = rows[int(s["first_row"])]
        head = read_bases(job.db, int(r0["rid0"]), int(r0["strand0"]))
        assert len(head) >= 500 and bases[j][:len(head) - 500] == head[:len(head) - 500], j
    return segments, links


def test_sequences_of_a_bubble(bubble):
    bases = bubble.want_bases()
    with bubble.u.gfa(bubble.g, bubble.rdb) as f:
        segments, links = check_sequences(bubble, f, bases)
    print("segments", len(segments), [len(b) for b in bases], "links", len(links))
    assert len(segments) >= 3 and len(links) >= 2                # the case has not degenerated
    with bubble.u.gfa(bubble.edges, bubble.rdb) as f:            # from edge records: the same file
        check_sequences(bubble, f, bases)


def test_sequences_with_the_bytes_released(bubble):
    bases = bubble.want_bases()
    rdb = shimmer.ResidentDB(bubble.db, 0)
    try:
        assert rdb.release_bytes() and not rdb.has_bytes
        with bubble.u.gfa(bubble.g, rdb) as f:
            check_sequences(bubble, f, bases)
    finally:
        rdb.close()


def test_a_circular_genome():
    job = Job(ring_set())
    try:
        table = job.u.table()
        print("unitigs", len(table), "circular", int(table["circular"].sum()), "edges", [int(x) for x in table["n_edges"]])
        bases = job.want_bases()
        with job.u.gfa(job.g, job.rdb) as f:
            segments, links = check_sequences(job, f, bases)
            rows, text = f.rows(), f.text()
        assert segments["circular"].sum() >= 1
        for j in np.flatnonzero(segments["circular"]):
            s = segments[j]
            r = rows[int(s["first_row"]):int(s["first_row"]) + int(s["n_rows"])]
            assert (r["rid1"][-1], r["strand1"][-1]) == (r["rid0"][0], r["strand0"][0])       # the path is closed
            assert all((a["rid1"], a["strand1"]) == (b["rid0"], b["strand0"]) for a, b in zip(r, r[1:]))
            assert b"L\tutg%06d\t+\tutg%06d\t+\t*\n" % (s["unitig"], s["unitig"]) in text
    finally:
        job.close()


def _native_cmd():
    exe = os.path.join(ROOT, "bin", "native", "shmr_sgraph")
    return [exe] if os.path.exists(exe) else [os.path.join(ROOT, "bin", "native", "pgx_cli"), "shmr_sgraph"]


def test_the_same_bytes_by_three_routes(bubble, tmp_path):
    with bubble.u.gfa(bubble.g, bubble.rdb) as f:
        want = f.text()
    with bubble.u.gfa(bubble.g) as f:
        topo = f.text()
    sd = str(tmp_path / "seq_dataset")
    formats.write_seqdb(sd, bubble.db)
    with bubble.u.gfa(bubble.g, sd) as f:                        # the file level: only the named reads go up
        assert f.text() == want
    got = shimmer.assemble(sd, 1, 1, gfa=True, out_dir=str(tmp_path / "out"))
    assert got["gfa"] == want and (tmp_path / "out" / "asm.gfa").read_bytes() == want
    assert set(got["stats"]["ms"]) == {"load", "index", "overlap", "graph", "contigs", "gfa"} and got["stats"]["gfa"]["segments"] >= 3
    plain = shimmer.assemble(sd, 1, 1, out_dir=str(tmp_path / "plain"))
    assert set(plain) == {"p_ctg", "a_ctg", "p_ctg_cns", "stats"} and set(plain["stats"]["ms"]) == {"load", "index", "overlap", "graph", "contigs"}
    assert "gfa" not in plain["stats"] and not (tmp_path / "plain" / "asm.gfa").exists()
    assert all(plain[k] == got[k] for k in ("p_ctg", "a_ctg", "p_ctg_cns"))
    src = tmp_path / "ovlp.dat"
    bubble.recs.tofile(src)
    with shimmer.string_graph(bubble.recs, chimer_ordered=True) as g2:
        sg = b"".join(g2.text())
    for k, cmd in enumerate((_native_cmd(), [sys.executable, os.path.join(ROOT, "bin", "shmr_sgraph")])):
        for tag, flags, expect in (("seq", ["--gfa-seqdb", sd], want), ("topo", [], topo)):
            out = tmp_path / f"g{k}.{tag}.gfa"
            with open(src, "rb") as fi:
                r = subprocess.run(cmd + ["--chimer_bridge_ordered", "--gfa", str(out)] + flags, stdin=fi, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
            assert r.returncode == 0 and r.stdout == sg, r.stderr   # stdout does not change
            assert out.read_bytes() == expect, (k, tag)
        r = subprocess.run(cmd + ["--gfa-seqdb", sd], input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 2 and b"--gfa" in r.stderr
    shimmer.shmr_sgraph(str(src), str(tmp_path / "sg"), chimer_ordered=True, gfa_path=str(tmp_path / "f.gfa"), gfa_seqdb=sd)
    assert (tmp_path / "f.gfa").read_bytes() == want and (tmp_path / "sg").read_bytes() == sg


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def raw_build(u, g, edges, n, db=None):
    lib = _lib.load()
    f = C.c_void_p(0xDEAD0000BEEF)
    rc = lib.pgx_gfa_build(u, g, edges.ctypes.data_as(C.c_void_p) if edges is not None else None, n, db, C.byref(f))
    return rc, f.value, lib.pgx_last_error()


def test_one_of_graph_and_records(fixture):
    _, recs, min_len, min_idt = fixture["chains"]
    with shimmer.string_graph(recs, min_len, min_idt) as g, g.unitigs() as u:
        edges = np.ascontiguousarray(g.edges())
        rc, f, msg = raw_build(u.h, g.h, edges, len(edges))
        assert rc == _lib.PGX_EARG and not f and b"both" in msg
        rc, f, msg = raw_build(u.h, None, None, 0)
        assert rc == _lib.PGX_EARG and not f and b"neither" in msg
        rc, f, msg = raw_build(None, g.h, None, 0)
        assert rc == _lib.PGX_EARG and not f
        with u.gfa(g) as a, u.gfa(edges) as b:                   # everything goes on
            assert a.text() == b.text() and a.stats["segments"] == 12
        lib = _lib.load()
        _lib.mem_ledger(reset_peak=True)
        with u.gfa(g) as a:
            assert _lib.mem_ledger()["peak_by_tag"].get("gfa", 0) > 0
            n = a.stats["segments"]
            assert lib.pgx_gfa_segments(a.h, n, 1, None) == _lib.PGX_EARG and lib.pgx_gfa_links(a.h, 0, a.stats["links"] + 1, None) == _lib.PGX_EARG
            assert lib.pgx_gfa_rows(a.h, a.stats["rows"] + 1, 0, None) == _lib.PGX_EARG and lib.pgx_gfa_text(a.h, None, None) == _lib.PGX_EARG
            assert lib.pgx_gfa_stats(None, None) == _lib.PGX_EARG
        a.close()
        with pytest.raises(_lib.PgxError, match="closed"):
            a.text()
        assert lib.pgx_gfa_free(None) == 0
    units = C.c_uint64(0)
    for part in (b"gfa", b"gfa_dual", b"gfa_rows", b"gfa_links", b"gfa_text"):
        assert _lib.load().pgx_timing_get(part, None, None, C.byref(units)) == 0 and units.value > 0, part


def test_the_records_of_another_graph(case_edges):
    forks, chains = case_edges["forks"], case_edges["chains"]
    g = np.flatnonzero(forks["type"] == SG.G)
    swapped = forks.copy()
    swapped[[g[2], g[9]]] = swapped[[g[9], g[2]]]                # the same records, two of them at each other's place
    short = forks.copy()
    short["type"][g[-1]] = SG.TR                                 # as many records, one G edge fewer
    assert (chains["type"] == SG.G).sum() != len(g)
    with shimmer.unitigs(forks) as u:
        for bad, n, word in ((chains, len(chains), b"G edges"), (swapped, len(swapped), b"another graph"), (short, len(short), b"G edges"), (forks, 0, b"G edges")):
            rc, f, msg = raw_build(u.h, None, np.ascontiguousarray(bad), n)
            assert rc == _lib.PGX_EARG and not f and word in msg, msg
        with u.gfa(forks) as f:                                  # the unitigs go on
            assert f.stats["segments"] * 2 == u.stats["unitigs"]
    # a path index beyond the records: the unitigs of five S records and then the G edges, held against the G edges alone
    lead = np.zeros(5, shimmer.SGRAPH_EDGE_DTYPE)
    lead["type"], lead["w_rid"] = SG.S, 1
    with shimmer.unitigs(np.concatenate([lead, forks])) as u:
        assert u.paths().max() >= len(forks)
        rc, f, msg = raw_build(u.h, None, forks, len(forks))
        assert rc == _lib.PGX_EARG and not f and b"beyond" in msg, msg


def designed_chain(short_read=3):
    """reads 0 .. 3 of 3,000 bases but one of 400, and the chain 0:E -> 1:E -> 2:E -> 3:E with its reverse, edge after edge"""
    rng = np.random.default_rng(5)
    rlen = np.full(4, 3000, np.uint32)
    rlen[short_read] = 400
    enc = []
    for n in rlen:
        codes = rng.integers(0, 4, int(n)).astype(np.uint8)
        enc.append((np.uint8(1) << codes) | ((np.uint8(8) >> codes[::-1]) << np.uint8(4)))
    roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
    db = formats.SeqDB(np.concatenate(enc).astype(np.uint8), np.arange(4, dtype=np.uint32), rlen, roff, None)
    e = np.zeros(6, shimmer.SGRAPH_EDGE_DTYPE)
    i = np.arange(3, dtype=np.uint32)
    e["v_rid"][0::2], e["w_rid"][0::2], e["v_end"][0::2], e["w_end"][0::2], e["sp"][0::2], e["tp"][0::2] = i, i + 1, SG.E, SG.E, 1000, 2000
    e["v_rid"][1::2], e["w_rid"][1::2], e["v_end"][1::2], e["w_end"][1::2], e["sp"][1::2], e["tp"][1::2] = i + 1, i, SG.B, SG.B, 2000, 1000
    e["label_rid"], e["type"], e["score"] = e["w_rid"], SG.G, 1000
    return db, e


def test_a_row_the_layout_refuses(tmp_path):
    db, edges = designed_chain()
    sd = str(tmp_path / "designed")
    formats.write_seqdb(sd, db)
    rdb = shimmer.ResidentDB(db, 0)
    try:
        with shimmer.unitigs(edges) as u:
            assert [int(x) for x in u.table()["n_edges"]] == [3, 3] and [int(x) for x in u.paths()] == [0, 2, 4, 5, 3, 1]
            with u.gfa(edges) as f:
                assert f.text() == GF.HEADER + b"S\tutg000000\t*\n"
            for src in (rdb, sd):
                with pytest.raises(_lib.PgxError) as ei:
                    u.gfa(edges, src)
                msg = str(ei.value)
                assert "code %d" % _lib.PGX_EARG in msg and "segment 0 (utg000000), position 2 of its path, edge 4" in msg and "400 bases of read 3" in msg, msg
            rc, f, _ = raw_build(u.h, None, edges, len(edges), rdb.h)
            assert rc == _lib.PGX_EARG and not f                 # no object: nothing to write
    finally:
        rdb.close()
    db, edges = designed_chain(short_read=0)
    rdb = shimmer.ResidentDB(db, 0)
    try:
        with shimmer.unitigs(edges) as u, pytest.raises(_lib.PgxError, match="segment 0 .utg000000., position 0 of its path, edge 0: .*fewer than the overhang"):
            u.gfa(edges, rdb)
    finally:
        rdb.close()


def test_after_shutdown_every_call_but_free_answers_estate(case_edges, tmp_path):
    """in a process of its own: one context per process"""
    np.save(tmp_path / "edges.npy", case_edges["forks"])
    code = ("import sys, ctypes as C, numpy as np; sys.path.insert(0, %r)\n"
            "from peregrine_amd import _lib, shimmer\n"
            "e = np.load(%r)\n"
            "u = shimmer.unitigs(e)\nf = u.gfa(e)\nlib = _lib.load()\n_lib.shutdown()\n"
            "t, tl, v = C.c_void_p(), C.c_size_t(0), C.c_void_p()\n"
            "st = (C.c_uint64 * 6)(); o = np.zeros(64, np.uint8).ctypes.data_as(C.c_void_p)\n"
            "print(lib.pgx_gfa_stats(f.h, st), lib.pgx_gfa_segments(f.h, 0, 1, o), lib.pgx_gfa_links(f.h, 0, 1, o), lib.pgx_gfa_rows(f.h, 0, 1, o),\n"
            "      lib.pgx_gfa_text(f.h, C.byref(t), C.byref(tl)), lib.pgx_gfa_write(f.h, %r.encode()), lib.pgx_gfa_build(u.h, None, e.ctypes.data_as(C.c_void_p), len(e), None, C.byref(v)),\n"
            "      lib.pgx_gfa_build_files(u.h, None, e.ctypes.data_as(C.c_void_p), len(e), None, C.byref(v)), lib.pgx_gfa_free(f.h), lib.pgx_unitigs_free(u.h))\n"
            "f.h = C.c_void_p(); u.h = C.c_void_p()\n"
            "with shimmer.unitigs(e) as u2, u2.gfa(e) as f2:\n    print(f2.stats['segments'])\n" % (ROOT, str(tmp_path / "edges.npy"), str(tmp_path / "never.gfa")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, PGX_NO_TORCH="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    e = _lib.PGX_ESTATE
    assert r.stdout.split("\n")[:2] == ["%d %d %d %d %d %d %d %d 0 0" % (e, e, e, e, e, e, e, e), "11"], r.stdout
    assert not (tmp_path / "never.gfa").exists()
