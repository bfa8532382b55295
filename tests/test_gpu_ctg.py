"""Contig paths on the GPU (pgx_unitigs_contig_paths / pgx_ctg_paths_build / _stats / _table / _rows / _utg_text / _ctg_text / _free,
Unitigs.contig_paths, shimmer.contig_paths, ContigPaths, `shmr_sgraph --utg-data --ctg-paths` in both forms).  Every comparison is byte
for byte with the plain-Python restatement of the rule (tests/ctg_util.py, which test_ctg_rule.py holds to the fixture), and on the stored
cases of tests/golden/ctg_cases.npz also, in normal form, with what the REAL second half of ovlp_to_graph.py wrote.  On the tangled real
graphs (`dense`, `quant`) and on random graphs the script has no single answer (its files change with the hash seed): those are held to
the restatement alone.  The two commands read overlap records, not edges, so they run on the record cases; the hand-made cases go through
the library's two builders and the Python API."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import ctg_util as CU
import sgraph_util as SG
import utg_util as UT
from peregrine_amd import _lib, shimmer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z, CASES = CU.load_fixture()
STORED = [n for n, c in CASES.items() if c["stored"]]
_want = {}


def restated(name, edges):
    """the restatement's result for a named input, computed once and left alone"""
    if name not in _want:
        _want[name] = CU.contig_paths(edges)
    return _want[name]


def check(c, want, max_lines=1 << 20):
    """texts, table, rows and statistics of live contig paths against the restatement's"""
    st = dict(c.stats)
    # every walk from a start node is made on the device (a walk left over by the 64 rounds would go to the host: these graphs have none)
    assert st.pop("host_us") >= 0 and st.pop("device_walks") == want.start_edges and st == CU.stats_of(want)
    parts = list(c.utg_pieces(max_lines))
    assert all(0 < p.count(b"\n") <= max_lines and p.endswith(b"\n") for p in parts)
    utg, ctg = b"".join(parts), c.ctg_text(max_lines)
    assert utg == want.utg_text
    assert ctg == want.ctg_text
    t = c.table()
    assert t.dtype == CU.CTG_UNITIG_DTYPE == shimmer.CTG_UNITIG_DTYPE and np.array_equal(t, want.table)
    if len(t) > 3:
        assert np.array_equal(c.table(1, 2), t[1:3])
    rows = c.rows()
    assert len(rows) == len(want.rows) and all(list(a) == list(b) for a, b in zip(rows, want.rows))
    assert c.utg_text() == b"" and c.ctg_text() == b""           # handed out
    return utg, ctg


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases_both_builders(name):
    edges = CU.fixture_edges(Z, name)
    want = restated(name, edges)
    with shimmer.contig_paths(edges) as c:
        utg, ctg = check(c, want)
    if name in STORED:
        assert CU.normalise(utg, ctg) == CU.normalise(Z[name + "_utg"].tobytes(), Z[name + "_ctg"].tobytes())
    with shimmer.unitigs(edges) as u:
        simple = b"".join(u.text())
        with u.contig_paths() as c:
            check(c, want, max_lines=3)
            with u.contig_paths() as c2:                         # a second one of the same unitigs, which are as they were
                assert c2.utg_text() == utg and c2.ctg_text() == ctg
        assert simple == UT.unitigs(edges)[0] and list(u.text()) == []
        for a, b in zip(simple.split(b"\n")[:-1], utg.split(b"\n")):  # the simple lines are the unitigs' with the type replaced
            fa, fb = a.split(b" "), b.split(b" ")
            assert fa[:3] + fa[4:] == fb[:3] + fb[4:]


BIG = {"ctg63": lambda: CU.chain_with_tips(63), "ctg64": lambda: CU.chain_with_tips(64), "ctg65": lambda: CU.chain_with_tips(65),
       "ctg300": lambda: CU.chain_with_tips(300), "ladder": lambda: CU.ladder(45), "spur5001": lambda: CU.long_spur(5001)}


@pytest.mark.parametrize("name", sorted(BIG))
def test_sizes_at_which_the_kernels_can_go_wrong(name):
    edges = BIG[name]()
    want = restated(name, edges)
    longest = lambda t: max(len(ln) for ln in t.split(b"\n"))   # noqa: E731
    if name.startswith("ctg"):
        assert CU.stats_of(want)["longest_ctg"] == int(name[3:]) and (name != "ctg300" or longest(want.ctg_text) > 8192)
    if name == "ladder":
        assert CU.stats_of(want)["compound"] == 2 and longest(want.utg_text) > 8192 + 4096 and b"~NA~" in want.ctg_text
    if name == "spur5001":
        ln = [x for x in want.utg_text.split(b"\n") if b" spur:2 " in x]
        assert len(ln) == 2 and all(x.split(b" ")[6].count(b"~") == 5000 for x in ln)
    texts = []
    for max_lines in (1, 5, 1 << 20):
        with shimmer.contig_paths(edges) as c:
            texts.append(check(c, want, max_lines))
    assert texts[0] == texts[1] == texts[2]                      # ... and across runs


# ctg_paths is written in tiles of 8,192 bytes, 16 bytes a store and the bytes behind the last whole 16 one by one (the piece scheme that
# utg_data of the unitigs has its tail cases for in test_gpu_utg.py).  The whole text's last tile as the cases above do not show it: one of
# 1 .. 15 bytes (no 16-byte store at all), and one that ends exactly on a 16-byte store (no byte-wise tail).
TAIL_CASES = {"tail_1_15": lambda length: 1 <= length % 8192 <= 15,
              "tail_16s": lambda length: length > 8192 and length % 8192 != 0 and length % 16 == 0}


def contigs_for_tail(n_unitigs: int, n_short: int) -> np.ndarray:
    """chain_with_tips(n_unitigs) and n_short further chains of one unitig, each a contig of its own: ctg_paths grows by a triple on both
    of the long contig's lines with every unitig, and by two short lines with every further chain"""
    parts = [CU.chain_with_tips(n_unitigs)]
    for k in range(n_short):
        g = CU.Graph(base=300000 + 10 * k)
        g.chain([1, 2, 3, 4])
        parts.append(CU.edges_of_g_lines(g.lines))
    return np.concatenate(parts)


def shape_for_tail(accept):
    """(edges, the restatement's result) of the first contigs_for_tail(n, k), 100 <= n < 260 and k < 8, whose ctg_paths has a length that
    accept() takes (None: there is none).  The restatement is run where a straight line through its lengths at n = 100 and 101 comes
    within 4 bytes of such a length (the digits of the summed lengths and scores move the real one by a few bytes); the caller holds the
    chosen text against accept() again."""
    base = [len(CU.contig_paths(contigs_for_tail(100, k)).ctg_text) for k in range(8)]
    step = len(CU.contig_paths(contigs_for_tail(101, 0)).ctg_text) - base[0]
    for n in range(100, 260):
        for k in range(8):
            if any(accept(base[k] + (n - 100) * step + d) for d in range(-4, 5)):
                edges = contigs_for_tail(n, k)
                want = CU.contig_paths(edges)
                if accept(len(want.ctg_text)):
                    return edges, want
    return None


@pytest.mark.parametrize("name", sorted(TAIL_CASES))
def test_ctg_paths_whose_last_tile_is_a_tail_case(name):
    found = shape_for_tail(TAIL_CASES[name])
    assert found is not None
    edges, want = found
    assert TAIL_CASES[name](len(want.ctg_text))                  # before anything runs on the GPU: the case is a tail case
    lines = want.ctg_text.count(b"\n")
    for max_lines in (1, 7, 1 << 20):
        with shimmer.contig_paths(edges) as c:
            parts = list(c.ctg_pieces(max_lines))
            assert all(0 < p.count(b"\n") <= max_lines and p.endswith(b"\n") for p in parts) and len(parts) == -(-lines // max_lines)
            assert b"".join(parts) == want.ctg_text              # byte for byte the restatement's
            assert c.utg_text(max_lines) == want.utg_text


def test_the_empty_graph_and_a_graph_without_g_edges():
    none = CU.fixture_edges(Z, "spur")
    none["type"] = SG.TR
    for e in (np.zeros(0, shimmer.SGRAPH_EDGE_DTYPE), none):
        with shimmer.contig_paths(e) as c:
            assert {k: v for k, v in c.stats.items() if k not in ("host_us", "device_walks")} == CU.stats_of(CU.contig_paths(e))
            assert c.stats["unitigs"] == 0 and c.utg_text() == b"" and c.ctg_text() == b"" and len(c.table()) == 0 and c.rows() == []
        with shimmer.unitigs(e) as u, u.contig_paths() as c:
            assert c.stats["ctg_lines"] == 0 and c.utg_text() == b""


@pytest.fixture(scope="module")
def record_cases():
    """name -> (records, min_len, min_idt) of the tangled real graphs of utg_cases.npz"""
    z, cases = UT.load_fixture()
    return {n: (UT.fixture_recs(z, cases[n]), cases[n]["min_len"], cases[n]["min_idt"]) for n in ("chains", "dense", "quant")}


@pytest.mark.parametrize("name", ["dense", "quant"])
def test_real_graphs_against_the_restatement(record_cases, name):
    recs, min_len, min_idt = record_cases[name]
    with shimmer.string_graph(recs, min_len, min_idt) as g:
        edges = g.edges()
        u = g.unitigs()
    want = restated(name, edges)
    assert CU.stats_of(want)["ctg_lines"] > 10
    with u, u.contig_paths() as c:                               # the graph is freed: the unitigs own their arrays
        check(c, want, max_lines=11)


@pytest.mark.parametrize("seed,n_pairs", [(31, 1000), (32, 3000), (33, 6000)])
def test_random_graphs_against_the_restatement(seed, n_pairs):
    edges = UT.random_symmetric_edges(seed, n_pairs)
    try:
        want = CU.contig_paths(edges)
    except CU.Invalid:
        with pytest.raises(_lib.PgxError):
            shimmer.contig_paths(edges)
        return
    with shimmer.contig_paths(edges) as c:
        check(c, want, max_lines=1000)


def test_tiling_end_to_end_equals_the_real_graph_to_path(tmp_path):
    """our two texts and the case's sg_edges_list through the tiling paths: what the REAL graph_to_path.py wrote for the same three texts
    (stored in the fixture; tie-free cases only, chosen as make_golden_tiling.py chooses them)"""
    done = 0
    for name in STORED:
        if not CASES[name].get("tiling"):
            continue
        sg = tmp_path / (name + ".sg")
        sg.write_bytes(Z[name + "_sg"].tobytes())
        edges = shimmer.read_sg_edges_list(str(sg))
        assert np.array_equal(edges, CU.fixture_edges(Z, name))
        with shimmer.contig_paths(edges) as c, c.tiling(str(sg)) as t:     # no utg_data or ctg_paths file is written
            assert b"".join(t.text(0)) == Z[name + "_p"].tobytes() and b"".join(t.text(1)) == Z[name + "_a"].tobytes()
        with shimmer.contig_paths(edges) as c:
            assert c.write(str(tmp_path / "utg"), str(tmp_path / "ctg")) > 0
        with shimmer.graph_to_path(str(sg), str(tmp_path / "utg"), str(tmp_path / "ctg")) as t:
            assert b"".join(t.text(0)) == Z[name + "_p"].tobytes() and b"".join(t.text(1)) == Z[name + "_a"].tobytes()
        done += 1
    assert done >= 8


def test_contigs_end_to_end_equal_the_layout_of_the_real_tiling_paths(tmp_path):
    """... and on to the contig FASTA: ContigPaths.tiling(sg).contigs() on every such case against the layout (shimmer.path_to_contig) of
    the tiling paths the REAL graph_to_path.py wrote.  The layout takes arbitrary bytes, so the reads are random: one per read id of the
    case, 1,500 bytes longer than the largest sp / tp (the ids a case does not use get 16 bytes)."""
    from peregrine_amd import formats
    done = 0
    for name in STORED:
        if not CASES[name].get("tiling"):
            continue
        edges = CU.fixture_edges(Z, name)
        n = int(max(edges["v_rid"].max(), edges["w_rid"].max())) + 1
        rlen = np.full(n, 16, np.uint32)
        rlen[np.unique(np.concatenate([edges["v_rid"], edges["w_rid"]]))] = int(max(edges["sp"].max(), edges["tp"].max())) + 1500
        roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
        seq = np.random.default_rng(len(name)).integers(0, 256, int(rlen.sum()), dtype=np.uint8)
        prefix = str(tmp_path / (name + "_reads"))
        formats.write_seqdb(prefix, formats.SeqDB(seq, np.arange(n, dtype=np.uint32), rlen, roff))
        sg = tmp_path / (name + ".sg")
        sg.write_bytes(Z[name + "_sg"].tobytes())
        with shimmer.contig_paths(edges) as c, c.tiling(str(sg)) as t:
            for which in ("p", "a"):
                ref_path = tmp_path / ("%s.%s_ctg_tiling_path" % (name, which))
                ref_path.write_bytes(Z["%s_%s" % (name, which)].tobytes())
                got = t.contigs(which, prefix, str(tmp_path / "ours.fa"))
                want = shimmer.path_to_contig(prefix, str(ref_path), str(tmp_path / "ref.fa"))
                assert got == want and (tmp_path / "ours.fa").read_bytes() == (tmp_path / "ref.fa").read_bytes(), (name, which)
                done += which == "p" and got["contigs"] > 0
    assert done >= 8


def test_tiling_of_a_live_graph_without_files(record_cases, tmp_path):
    recs, min_len, min_idt = record_cases["chains"]
    with shimmer.string_graph(recs, min_len, min_idt) as g:
        g2 = shimmer.string_graph(recs, min_len, min_idt)
        g2.write(str(tmp_path / "sg"))
        g2.close()
        with g.unitigs() as u, u.contig_paths() as c:
            with c.tiling(g) as t:
                live = (b"".join(t.text(0)), b"".join(t.text(1)))
        with g.unitigs() as u, u.contig_paths() as c:
            c.write(str(tmp_path / "utg"), str(tmp_path / "ctg"))
    with shimmer.graph_to_path(str(tmp_path / "sg"), str(tmp_path / "utg"), str(tmp_path / "ctg")) as t:
        assert (b"".join(t.text(0)), b"".join(t.text(1))) == live and len(live[0]) > 0


def _native_cmd():
    exe = os.path.join(ROOT, "bin", "native", "shmr_sgraph")
    return [exe] if os.path.exists(exe) else [os.path.join(ROOT, "bin", "native", "pgx_cli"), "shmr_sgraph"]


@pytest.mark.parametrize("name", ["chains", "quant"])
def test_both_commands(record_cases, name, tmp_path):
    recs, min_len, min_idt = record_cases[name]
    src = tmp_path / "ovlp.dat"
    recs.tofile(src)
    with shimmer.string_graph(recs, min_len, min_idt) as g:
        want = restated("cmd_" + name, g.edges())
        sg_text = b"".join(g.text())
        with g.unitigs() as u:
            utg_simple = b"".join(u.text())
    env = dict(os.environ, PGX_DEDUP_PIECE="500")                # several feeds; 500 lines of text a piece
    for k, cmd in enumerate((_native_cmd(), [sys.executable, os.path.join(ROOT, "bin", "shmr_sgraph")])):
        p = lambda s: str(tmp_path / ("%s.%d" % (s, k)))   # noqa: E731
        runs = ([], ["--utg", p("utg")], ["--utg-data", p("ud")], ["--ctg-paths=" + p("cp")], ["--utg", p("utg2"), "--utg-data=" + p("ud2"), "--ctg-paths", p("cp2")])
        for flags in runs:
            with open(src, "rb") as fi:
                r = subprocess.run(cmd + ["--min_len", str(min_len), "--min_idt", str(min_idt)] + flags, stdin=fi, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
            assert r.returncode == 0, r.stderr
            assert r.stdout == sg_text                           # stdout does not change
        assert open(p("utg"), "rb").read() == open(p("utg2"), "rb").read() == utg_simple    # nor does --utg
        assert open(p("ud"), "rb").read() == open(p("ud2"), "rb").read() == want.utg_text
        assert open(p("cp"), "rb").read() == open(p("cp2"), "rb").read() == want.ctg_text
    r = subprocess.run(_native_cmd() + ["--utg-data", str(tmp_path / "e1"), "--ctg-paths", str(tmp_path / "e2")], input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert (r.returncode, r.stdout) == (0, b"") and (tmp_path / "e1").read_bytes() == b"" and (tmp_path / "e2").read_bytes() == b"", r.stderr


def raw_build(edges):
    lib = _lib.load()
    e = np.ascontiguousarray(edges, shimmer.SGRAPH_EDGE_DTYPE)
    c = C.c_void_p(0xDEAD0000BEEF)
    rc = lib.pgx_ctg_paths_build(e.ctypes.data_as(C.c_void_p) if len(e) else None, len(e), C.byref(c))
    return rc, c, lib.pgx_last_error()


def test_error_paths_leave_everything_usable():
    _lib.init()
    edges = CU.fixture_edges(Z, "all")
    want = restated("all", edges)
    lib = _lib.load()
    # what pgx_unitigs_build checks
    rc, c, msg = raw_build(np.delete(edges, 1))
    assert rc == _lib.PGX_EINVAL and not c.value and b"no reverse" in msg, msg
    # where the script raises: two short loops at one node; a bundle without a positive score
    a, x, y = 1 << 1 | 1, 2 << 1 | 1, 3 << 1 | 1
    lines = []
    for v, w in ((a, x), (x, a), (a, y), (y, a)):
        lines += [(v, w, 0, 3000, 2000), (w ^ 1, v ^ 1, 3000, 0, 2000)]
    zero = CU.fixture_edges(Z, "compound")
    zero["score"] = 0
    for bad, word in ((CU.edges_of_g_lines(lines), b"second short loop"), (zero, b"positive score")):
        with pytest.raises(CU.Invalid):
            CU.contig_paths(bad)
        rc, c, msg = raw_build(bad)
        assert rc == _lib.PGX_EINVAL and not c.value and word in msg, msg
        with shimmer.unitigs(bad) as u:                          # the unitigs stay as they were
            before = u.table()
            with pytest.raises(_lib.PgxError):
                u.contig_paths()
            assert np.array_equal(u.table(), before) and b"".join(u.text()) == UT.unitigs(bad)[0]
    # the unitigs freed first: utg_data, which reads their paths, is refused; the rest goes on
    u = shimmer.unitigs(edges)
    c = u.contig_paths()
    c._keep = None
    u.close()
    with pytest.raises(_lib.PgxError, match="unitigs"):
        c.utg_text()
    assert c.ctg_text() == want.ctg_text and np.array_equal(c.table(), want.table)
    c.close()
    # ... and so it is when later unitigs get the freed ones' address: a serial number tells them apart, not the pointer
    u = shimmer.unitigs(edges)
    c = u.contig_paths()
    c._keep = None
    u.close()
    later = [shimmer.unitigs(CU.fixture_edges(Z, "spur")) for _ in range(4)]
    with pytest.raises(_lib.PgxError, match="unitigs"):
        c.utg_text()
    assert c.ctg_text() == want.ctg_text
    c.close()
    for x in later:
        x.close()
    # null arguments, ranges, a closed handle, the ledger and the timers
    u = shimmer.unitigs(edges)
    _lib.mem_ledger(reset_peak=True)
    c = u.contig_paths()
    assert _lib.mem_ledger()["peak_by_tag"].get("ctg_paths", 0) > 0
    assert lib.pgx_ctg_paths_table(c.h, c.stats["unitigs"], 1, None) == _lib.PGX_EARG and lib.pgx_ctg_paths_stats(None, None) == _lib.PGX_EARG
    assert lib.pgx_ctg_paths_utg_text(c.h, 0, None, None, None) == _lib.PGX_EARG and lib.pgx_unitigs_contig_paths(None, C.byref(C.c_void_p())) == _lib.PGX_EARG
    assert c.utg_text() == want.utg_text
    c.close()
    c.close()
    for call in (c.table, c.rows, c.utg_text, c.ctg_text):
        with pytest.raises(_lib.PgxError, match="closed"):
            call()
    assert lib.pgx_ctg_paths_free(None) == 0
    units = C.c_uint64(0)
    for part in (b"ctg_paths", b"ctg_paths_graph", b"ctg_paths_clean", b"ctg_paths_walk", b"ctg_paths_text"):
        assert lib.pgx_timing_get(part, None, None, C.byref(units)) == 0 and units.value > 0, part


def test_after_shutdown_every_call_but_free_answers_estate(tmp_path):
    """in a process of its own: one context per process"""
    np.save(tmp_path / "edges.npy", CU.fixture_edges(Z, "spur"))
    code = ("import sys, ctypes as C, numpy as np; sys.path.insert(0, %r)\n"
            "from peregrine_amd import _lib, shimmer\n"
            "e = np.load(%r)\n"
            "c = shimmer.contig_paths(e)\nu = shimmer.unitigs(e)\nlib = _lib.load()\n_lib.shutdown()\n"
            "t, tl, d, v = C.c_void_p(), C.c_size_t(0), C.c_int(0), C.c_void_p()\n"
            "out = np.zeros(4, shimmer.CTG_UNITIG_DTYPE)\n"
            "st = (C.c_uint64 * 15)()\n"
            "print(lib.pgx_ctg_paths_stats(c.h, st), lib.pgx_ctg_paths_table(c.h, 0, 1, out.ctypes.data_as(C.c_void_p)), lib.pgx_ctg_paths_rows(c.h, None, None),\n"
            "      lib.pgx_ctg_paths_utg_text(c.h, 5, C.byref(t), C.byref(tl), C.byref(d)), lib.pgx_ctg_paths_ctg_text(c.h, 5, C.byref(t), C.byref(tl), C.byref(d)),\n"
            "      lib.pgx_ctg_paths_build(e.ctypes.data_as(C.c_void_p), len(e), C.byref(v)), lib.pgx_unitigs_contig_paths(u.h, C.byref(v)), lib.pgx_ctg_paths_free(c.h))\n"
            "c.h = C.c_void_p()\n"
            "with shimmer.contig_paths(e) as c2:\n    print(c2.stats['unitigs'], hash(c2.ctg_text()) != 0)\n" % (ROOT, str(tmp_path / "edges.npy")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, PGX_NO_TORCH="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    e = _lib.PGX_ESTATE
    assert r.stdout.split("\n")[:2] == ["%d %d %d %d %d %d %d 0" % (e, e, e, e, e, e, e), "6 True"], r.stdout


def test_shmr_sgraph_function_writes_the_files(record_cases, tmp_path):
    recs, min_len, min_idt = record_cases["chains"]
    recs.tofile(tmp_path / "ovlp.dat")
    a, b = [str(tmp_path / n) for n in ("plain", "with")]
    shimmer.shmr_sgraph(str(tmp_path / "ovlp.dat"), a, min_len, min_idt)
    shimmer.shmr_sgraph(str(tmp_path / "ovlp.dat"), b, min_len, min_idt, utg_data_path=b + ".utg", ctg_paths_path=b + ".ctg")
    assert hashlib.sha256(open(a, "rb").read()).digest() == hashlib.sha256(open(b, "rb").read()).digest()
    want = restated("cmd_chains", shimmer.read_sg_edges_list(a))
    assert open(b + ".utg", "rb").read() == want.utg_text and open(b + ".ctg", "rb").read() == want.ctg_text
