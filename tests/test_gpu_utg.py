"""Unitigs on the GPU (pgx_sgraph_unitigs / pgx_unitigs_build / _stats / _table / _paths / _text / _free, StringGraph.unitigs,
shimmer.unitigs, shimmer.read_sg_edges_list, `shmr_sgraph --utg` in both forms): on every case of tests/golden/utg_cases.npz the lines,
with via dropped, are what the real identify_simple_paths made of the case; via is the path's second node; on inputs without a fixture
the lines, the table and the paths are the plain-Python restatement's (tests/utg_util.py, which test_utg_rule.py holds to the fixture)."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import dedup_graph_util as DG
import oracle_util as U
import sgraph_util as SG
import utg_util as UT
from peregrine_amd import _lib, shimmer
from peregrine_amd.shimmer import DedupStream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC_CASES = ["single", "chains", "long", "rings", "dense", "quant", "none"]
EDGE_CASES = ["forks", "typed"]


@pytest.fixture(scope="module")
def fixture():
    """name -> (kind, records or edge array, min_len, min_idt, the reference's normalised lines), computed once and left alone"""
    z, cases = UT.load_fixture()
    out = {}
    for name, c in cases.items():
        want = z[name + "_utg"].tobytes()
        if c["kind"] == "edges":
            out[name] = ("edges", UT.fixture_edges(z, name), 0, 0.0, want)
        else:
            out[name] = ("recs", UT.fixture_recs(z, c), c["min_len"], c["min_idt"], want)
    return out


def stats_of(table, edges):
    return dict(g_edges=int((edges["type"] == SG.G).sum()), unitigs=len(table), circular=int(table["circular"].sum()),
                longest_edges=int(table["n_edges"].max()) if len(table) else 0)


def check_unitigs(u, edges, want_normalised=None, max_lines=1 << 20):
    """the text against the fixture (if any), and text, table, paths and stats against each other, the edges and the restatement"""
    parts = list(u.text(max_lines))
    assert all(0 < p.count(b"\n") <= max_lines and p.endswith(b"\n") for p in parts)
    text = b"".join(parts)
    if want_normalised is not None:
        assert UT.drop_via(text) == want_normalised
    assert UT.via_is_second_node(text)
    table, paths = u.table(), u.paths()
    assert table.dtype == UT.UNITIG_DTYPE == shimmer.UNITIG_DTYPE and paths.dtype == np.uint32
    UT.check_against_edges(edges, text, table, paths)          # includes: every G index exactly once
    assert u.stats == stats_of(table, edges)
    r_text, r_table, r_paths = UT.unitigs(edges)
    assert text == r_text and np.array_equal(table, r_table) and np.array_equal(paths, r_paths)
    if len(table) > 4:
        assert np.array_equal(u.table(2, 2), table[2:4]) and np.array_equal(u.paths(1, 3), paths[1:4])
    assert list(u.text()) == []                                  # handed out
    return text


@pytest.mark.parametrize("name", REC_CASES)
def test_fixture_cases_through_the_graph(fixture, name):
    _, recs, min_len, min_idt, want = fixture[name]
    with DedupStream(graph_ready=True) as ds:
        if len(recs):
            assert ds.feed(recs) == b""
        with ds.string_graph(min_len, min_idt) as g:
            edges = g.edges()
            u = g.unitigs()
    with u:                                                      # the graph is freed: the unitigs own their arrays
        check_unitigs(u, edges, want)


@pytest.mark.parametrize("name", REC_CASES + EDGE_CASES)
def test_fixture_cases_from_edge_records(fixture, name):
    kind, data, min_len, min_idt, want = fixture[name]
    if kind == "recs":
        with shimmer.string_graph(data, min_len, min_idt) as g:
            edges = g.edges()
    else:
        edges = data
    with shimmer.unitigs(edges) as u:
        check_unitigs(u, edges, want)


def chain_edges(n: int, score0: int = 0) -> np.ndarray:
    """one chain of n G edges from read 0's end to read n's, each followed by its reverse: two unitigs, whose lines grow by a node name
    and its separator (12 bytes) with every edge; the lengths are 0 and the one score that is not is the first edge's (score0: its digits
    shift the text's length), so nothing else on the lines changes with n"""
    e = np.zeros(2 * n, SG.EDGE_DTYPE)
    i = np.arange(n, dtype=np.uint32)
    e["v_rid"][0::2], e["w_rid"][0::2], e["v_end"][0::2], e["w_end"][0::2] = i, i + 1, SG.E, SG.E
    e["v_rid"][1::2], e["w_rid"][1::2], e["v_end"][1::2], e["w_end"][1::2] = i + 1, i, SG.B, SG.B
    e["label_rid"], e["type"], e["score"][0] = e["w_rid"], SG.G, score0
    return e


# The format kernel writes the text in tiles of 8,192 bytes, 16 bytes a store and the bytes behind the last whole 16 one by one.  What the
# fixture's cases do not show to be covered is the whole text's last tile: one of 1 .. 15 bytes (no 16-byte store at all), and one that
# ends exactly on a 16-byte store.  The chains that have such a text, found by the search below: n = 337 with score0 = 0 (8,206 bytes:
# 14 behind a tile) and n = 337 with score0 = 100 (8,208 bytes: 16 behind a tile).
TAIL_CASES = {"tail_1_15": (0, lambda length: 1 <= length % 8192 <= 15),       # (score0, the lengths wanted)
              "tail_16s": (100, lambda length: length > 8192 and length % 8192 != 0 and length % 16 == 0)}


def chain_for_tail(score0, accept):
    """the smallest n <= 4096 whose chain_edges(n, score0) has a text of a length that accept() takes (None: there is none).  The
    restatement's text grows by the same number of bytes with every edge, so two restatements give every length; the caller holds the
    chosen chain's own restated text against accept() again."""
    l1, l2 = (len(UT.unitigs(chain_edges(n, score0))[0]) for n in (1, 2))
    return next((n for n in range(1, 4097) if accept(l1 + (n - 1) * (l2 - l1))), None)


@pytest.mark.parametrize("name", ["chains", "long", "rings", "typed"] + list(TAIL_CASES))
def test_text_in_pieces(fixture, name, tmp_path):
    if name in TAIL_CASES:
        score0, accept = TAIL_CASES[name]
        n = chain_for_tail(score0, accept)
        assert n is not None
        kind, data = "edges", chain_edges(n, score0)
        want_text = UT.unitigs(data)[0]
        assert accept(len(want_text))
    else:
        kind, data, min_len, min_idt, want = fixture[name]
    if kind == "recs":
        with shimmer.string_graph(data, min_len, min_idt) as g:
            edges = g.edges()
    else:
        edges = data
    texts = []
    for max_lines in (1, 7, 1 << 20):
        with shimmer.unitigs(edges) as u:
            parts = list(u.text(max_lines))
            assert all(0 < p.count(b"\n") <= max_lines for p in parts) and len(parts) == -(-u.stats["unitigs"] // max_lines)
            texts.append(b"".join(parts))
    assert texts[0] == texts[1] == texts[2]
    if name in TAIL_CASES:
        assert texts[0] == want_text                              # byte for byte the restatement's
    else:
        assert UT.drop_via(texts[0]) == want
    if name == "long":
        with shimmer.unitigs(edges) as u:
            assert u.write(str(tmp_path / "utg")) == len(texts[0])
        assert (tmp_path / "utg").read_bytes() == texts[0] and max(len(ln) for ln in texts[0].split(b"\n")) > 40000


@pytest.mark.parametrize("seed,n_pairs", [(21, 1000), (22, 2000), (23, 4000), (24, 6000), (25, 8000)])
def test_further_seeds_against_the_restatement(seed, n_pairs):
    edges = UT.random_symmetric_edges(seed, n_pairs)
    n_g = int((edges["type"] == SG.G).sum())
    assert 2000 <= n_g <= 20000 and n_g < len(edges)
    with shimmer.unitigs(edges) as u:
        assert u.stats["circular"] >= 2 and u.stats["longest_edges"] > 64
        check_unitigs(u, edges, max_lines=1000)


def test_a_further_record_graph_through_the_whole_stack():
    recs = DG.make_records(seed=12, n_reads=200, genome=9000, contained_share=0.0)
    with shimmer.string_graph(recs, 3000, 96.0, piece=777) as g:
        edges = g.edges()
        assert g.stats["n_g"] > 100 and g.stats["n_tr"] > 0
        with g.unitigs() as u:
            text = check_unitigs(u, edges)
        assert text.count(b"\n") == u.stats["unitigs"] > 10
        assert b"".join(g.text()) == SG.string_graph(DG.select_graph_lines(U.orc_dedup(recs)[0]), 3000, 96.0)[0]   # the graph is as it was


def raw_build(edges):
    lib = _lib.load()
    e = np.ascontiguousarray(edges, shimmer.SGRAPH_EDGE_DTYPE)
    u = C.c_void_p(0xDEAD0000BEEF)
    rc = lib.pgx_unitigs_build(e.ctypes.data_as(C.c_void_p) if len(e) else None, len(e), C.byref(u))
    return rc, u, lib.pgx_last_error()


def test_error_paths_leave_everything_usable(fixture):
    _, edges, _, _, want = fixture["forks"]
    _lib.init()
    g = [int(e) for e in np.flatnonzero(edges["type"] == SG.G)]
    cases = []
    bad = edges.copy()
    bad["type"][g[5]] = SG.TR                                    # its reverse is left without a reverse
    cases.append((bad, b"reverse"))
    cases.append((np.concatenate([edges, edges[g[3]:g[3] + 1]]), b"repeats"))
    bad = edges.copy()
    bad["w_rid"][g[7]] = bad["v_rid"][g[7]]
    cases.append((bad, b"v_rid == w_rid"))
    _, recs, min_len, min_idt, _ = fixture["quant"]
    with shimmer.string_graph(recs, min_len, min_idt) as graph:
        sg = b"".join(graph.text())
        for bad, word in cases:
            with pytest.raises(UT.Invalid) as ei:
                UT.unitigs(bad)
            rc, u, msg = raw_build(bad)
            assert rc == _lib.PGX_EINVAL and not u.value and word in msg and (b"G edge %d " % ei.value.index) in msg, msg
            with pytest.raises(_lib.PgxError, match="edge %d " % ei.value.index):
                shimmer.unitigs(bad)
            with graph.unitigs() as u2:                          # the graph and the library go on
                assert u2.stats["unitigs"] > 0
        assert np.array_equal(SG.edges_of_text(sg), graph.edges())
    with shimmer.unitigs(edges) as u:
        assert UT.drop_via(b"".join(u.text())) == want
    # nothing to do: no edge at all, and no G edge
    none = edges.copy()
    none["type"] = SG.TR
    for e in (np.zeros(0, shimmer.SGRAPH_EDGE_DTYPE), none):
        with shimmer.unitigs(e) as u:
            assert u.stats == dict(g_edges=0, unitigs=0, circular=0, longest_edges=0) and list(u.text()) == [] and len(u.table()) == 0 and len(u.paths()) == 0
    # a closed handle, null arguments, ranges
    _lib.mem_ledger(reset_peak=True)
    u = shimmer.unitigs(edges)
    assert _lib.mem_ledger()["peak_by_tag"].get("unitigs", 0) > 0
    lib = _lib.load()
    assert lib.pgx_unitigs_table(u.h, u.stats["unitigs"], 1, None) == _lib.PGX_EARG and lib.pgx_unitigs_paths(u.h, 0, u.stats["g_edges"] + 1, None) == _lib.PGX_EARG
    assert lib.pgx_unitigs_text(u.h, 0, None, None, None) == _lib.PGX_EARG and lib.pgx_unitigs_stats(None, None) == _lib.PGX_EARG
    u.close()
    u.close()
    for call in (u.table, u.paths, lambda: list(u.text())):
        with pytest.raises(_lib.PgxError, match="closed"):
            call()
    assert lib.pgx_unitigs_free(None) == 0
    units = C.c_uint64(0)
    for part in (b"unitigs", b"unitigs_links", b"unitigs_rank", b"unitigs_paths", b"unitigs_text"):
        assert lib.pgx_timing_get(part, None, None, C.byref(units)) == 0 and units.value > 0, part


def test_a_doubly_damaged_input_gets_the_first_refusal(fixture):
    """the order of the refusals: v_rid == w_rid, then a repeated (v, w), then a missing reverse"""
    _, edges, _, _, _ = fixture["forks"]
    _lib.init()
    g = [int(e) for e in np.flatnonzero(edges["type"] == SG.G)]
    bad = edges.copy()
    bad["w_rid"][g[7]] = bad["v_rid"][g[7]]
    rc, u, msg = raw_build(np.concatenate([bad, bad[g[3]:g[3] + 1]]))
    assert rc == _lib.PGX_EINVAL and not u.value and b"v_rid == w_rid" in msg and (b"G edge %d " % g[7]) in msg and b"repeats" not in msg, msg
    bad = edges.copy()
    bad["type"][g[5]] = SG.TR                                    # its reverse is left without a reverse
    rc, u, msg = raw_build(np.concatenate([bad, bad[g[3]:g[3] + 1]]))
    assert rc == _lib.PGX_EINVAL and not u.value and b"repeats" in msg and (b"G edge %d " % len(edges)) in msg and b"reverse" not in msg, msg


def test_after_shutdown_every_call_but_free_answers_estate(fixture, tmp_path):
    """in a process of its own: one context per process"""
    np.save(tmp_path / "edges.npy", fixture["forks"][1])
    code = ("import sys, ctypes as C, numpy as np; sys.path.insert(0, %r)\n"
            "from peregrine_amd import _lib, shimmer\n"
            "e = np.load(%r)\n"
            "u = shimmer.unitigs(e)\nlib = _lib.load()\n_lib.shutdown()\n"
            "t, tl, d, v = C.c_void_p(), C.c_size_t(0), C.c_int(0), C.c_void_p()\n"
            "out = np.zeros(4, shimmer.UNITIG_DTYPE); p = np.zeros(4, np.uint32)\n"
            "st = (C.c_uint64 * 4)()\n"
            "print(lib.pgx_unitigs_stats(u.h, st), lib.pgx_unitigs_table(u.h, 0, 1, out.ctypes.data_as(C.c_void_p)), lib.pgx_unitigs_paths(u.h, 0, 1, p.ctypes.data_as(C.c_void_p)),\n"
            "      lib.pgx_unitigs_text(u.h, 5, C.byref(t), C.byref(tl), C.byref(d)), lib.pgx_unitigs_build(e.ctypes.data_as(C.c_void_p), len(e), C.byref(v)),\n"
            "      lib.pgx_sgraph_unitigs(None, C.byref(v)), lib.pgx_unitigs_free(u.h))\n"
            "u.h = C.c_void_p()\n"
            "with shimmer.unitigs(e) as u2:\n    print(u2.stats['unitigs'])\n" % (ROOT, str(tmp_path / "edges.npy")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, PGX_NO_TORCH="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    e = _lib.PGX_ESTATE
    assert r.stdout.split("\n")[:2] == ["%d %d %d %d %d %d 0" % (e, e, e, e, e, e), "22"], r.stdout


def _native_cmd():
    exe = os.path.join(ROOT, "bin", "native", "shmr_sgraph")
    return [exe] if os.path.exists(exe) else [os.path.join(ROOT, "bin", "native", "pgx_cli"), "shmr_sgraph"]


def test_both_commands_file_to_file(fixture, tmp_path):
    _, recs, min_len, min_idt, want = fixture["chains"]
    src = tmp_path / "ovlp.dat"
    recs.tofile(src)
    with shimmer.string_graph(recs, min_len, min_idt) as g, g.unitigs() as u:
        n = u.write(str(tmp_path / "utg.lib"))
    lib_bytes = (tmp_path / "utg.lib").read_bytes()
    assert len(lib_bytes) == n and UT.drop_via(lib_bytes) == want
    env = dict(os.environ, PGX_DEDUP_PIECE="500")                # several feeds; 500 lines of text a piece
    for k, cmd in enumerate((_native_cmd(), [sys.executable, os.path.join(ROOT, "bin", "shmr_sgraph")])):
        shas = []
        for flag in ([], ["--utg", str(tmp_path / f"utg.{k}")], [f"--utg={tmp_path}/utg.{k}b"]):
            with open(src, "rb") as fi:
                r = subprocess.run(cmd + ["--min_len", str(min_len)] + flag, stdin=fi, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
            assert r.returncode == 0 and r.stdout.count(b"\n") == 2700, r.stderr
            shas.append(hashlib.sha256(r.stdout).hexdigest())
        assert shas[0] == shas[1] == shas[2]                     # stdout does not change
        assert (tmp_path / f"utg.{k}").read_bytes() == (tmp_path / f"utg.{k}b").read_bytes() == lib_bytes
    # an empty graph writes an empty file
    r = subprocess.run(_native_cmd() + ["--utg", str(tmp_path / "empty")], input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert (r.returncode, r.stdout) == (0, b"") and (tmp_path / "empty").read_bytes() == b"", r.stderr
    r = subprocess.run(_native_cmd() + ["--utg"], input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode != 0 and b"--utg" in r.stderr


def test_read_sg_edges_list_round_trips(fixture, tmp_path):
    for name in ("dense", "rings"):
        _, recs, min_len, min_idt, want = fixture[name]
        with shimmer.string_graph(recs, min_len, min_idt) as g:
            edges = g.edges()
            g2 = shimmer.string_graph(recs, min_len, min_idt)
            assert g2.write(str(tmp_path / "sg")) > 0
            g2.close()
        got = shimmer.read_sg_edges_list(str(tmp_path / "sg"))
        assert got.dtype == shimmer.SGRAPH_EDGE_DTYPE and np.array_equal(got, edges)
        with shimmer.unitigs(got) as u:
            assert UT.drop_via(b"".join(u.text())) == want
    # the script's fifth type, and what is not a line of the file
    (tmp_path / "c").write_bytes(b"000000001:E 000000002:E 000000002  1000     0  5000 99.60 C\n000000002:B 000000001:B 000000001  1200  9000  5000 99.60 TR\n")
    got = shimmer.read_sg_edges_list(str(tmp_path / "c"))
    assert list(got["type"]) == [shimmer.SGRAPH_TYPE_OTHER, 1] and shimmer.SGRAPH_TYPE_OTHER != 0 and got["sp"][1] == 1200 and got["v_end"][0] == 1
    with shimmer.unitigs(got) as u:
        assert u.stats["g_edges"] == 0
    (tmp_path / "bad").write_bytes(b"000000001:E 000000002:E 5\n")
    with pytest.raises(ValueError):
        shimmer.read_sg_edges_list(str(tmp_path / "bad"))
