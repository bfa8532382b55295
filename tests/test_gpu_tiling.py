"""Tiling paths on the GPU (pgx_sgraph_parse, pgx_tiling_build / _stats / _rows / _names / _text / _free / _chunk, shimmer.TilingPaths,
shimmer.graph_to_path, StringGraph.tiling, `graph_to_path.py` in both forms): on every case of tests/golden/tiling_cases.npz the two files
are byte for byte what the real graph_to_path.py wrote; on inputs without a fixture they are the restatement's (tests/tiling_util.py,
which test_tiling_rule.py holds to the fixture)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sgraph_util as SG
import tiling_util as TU
from peregrine_amd import _lib, shimmer
from peregrine_amd.shimmer import DedupStream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z, CASES = TU.load_fixture()
NAMES = sorted(CASES)
COUNTS = ("sg_lines", "g_edges", "utg_simple", "utg_contained", "utg_compound", "ctg_kept", "ctg_skipped", "ctg_empty", "p_rows", "a_rows", "alternates",
          "compound_tie_rounds")


def put(d, sg, utg, ctg):
    os.makedirs(d, exist_ok=True)
    for fn, data in (("sg_edges_list", sg), ("utg_data", utg), ("ctg_paths", ctg)):
        with open(os.path.join(d, fn), "wb") as f:
            f.write(data)
    return [os.path.join(d, fn) for fn in ("sg_edges_list", "utg_data", "ctg_paths")]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """case -> (the three input paths, the script's p file, its a file), written once and left alone"""
    top = tmp_path_factory.mktemp("tiling")
    out = {}
    for case in NAMES:
        sg, utg, ctg, p, a = TU.case_files(Z, case)
        out[case] = (put(str(top / case), sg, utg, ctg), p, a)
    return out


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("case", NAMES)
def test_fixture_through_the_file_level(files, case, tmp_path):
    inputs, p, a = files[case]
    st = shimmer.graph_to_path(*inputs, str(tmp_path / "p"), str(tmp_path / "a"))
    assert (read(tmp_path / "p"), read(tmp_path / "a")) == (p, a)
    assert {k: st[k] for k in COUNTS} == {k: CASES[case][k] for k in COUNTS}


@pytest.mark.parametrize("case", NAMES)
def test_fixture_in_small_pieces(files, case, tmp_path, monkeypatch):
    """PGX_TILING_PIECE = 600 bytes: ten lines to a piece, every cut inside a line"""
    inputs, p, a = files[case]
    monkeypatch.setenv("PGX_TILING_PIECE", "600")
    shimmer.graph_to_path(*inputs, str(tmp_path / "p"), str(tmp_path / "a"))
    assert (read(tmp_path / "p"), read(tmp_path / "a")) == (p, a)
    if case in ("long", "real_dense"):
        assert os.path.getsize(inputs[0]) > 20 * 600
        assert np.array_equal(shimmer.parse_sg_edges_list(inputs[0]), shimmer.read_sg_edges_list(inputs[0]))


@pytest.mark.parametrize("case", NAMES)
def test_fixture_through_the_class(files, case, tmp_path):
    """text in pieces, rows and names equal to the parse of the text, write()"""
    inputs, p, a = files[case]
    with shimmer.graph_to_path(*inputs) as t:
        assert {k: t.stats[k] for k in COUNTS} == {k: CASES[case][k] for k in COUNTS}
        for which, want in (("p", p), ("a", a)):
            rows, names = t.rows(which), t.names(which)
            want_rows, want_names = TU.rows_of_text(want)
            assert names == want_names and rows.dtype == _lib.TILE_ROW_DTYPE
            assert [tuple(int(r[f]) for f in ("ctg", "rid0", "rid1", "s", "e", "strand0", "strand1")) for r in rows] == want_rows
            if len(rows) > 4:
                assert np.array_equal(t.rows(which, 2, 2), rows[2:4])
        parts = list(t.text(0, 7))
        assert all(0 < x.count(b"\n") <= 7 and x.endswith(b"\n") for x in parts) and b"".join(parts) == p
        assert list(t.text("p")) == []                      # handed out
        assert t.write(str(tmp_path / "p"), str(tmp_path / "a")) == len(a)
        assert read(tmp_path / "p") == b"" and read(tmp_path / "a") == a
    t.close()
    with pytest.raises(_lib.PgxError, match="closed"):
        t.rows("p")


TOOLS = {"python": [sys.executable, os.path.join(ROOT, "bin", "graph_to_path.py")], "native": [os.path.join(ROOT, "bin", "native", "graph_to_path.py")]}


@pytest.mark.parametrize("case", NAMES)
@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_fixture_through_the_commands(files, tool, case, tmp_path):
    """the script's command line: defaults in the working directory, the six options, nothing on stdout"""
    inputs, p, a = files[case]
    if case == "bubble2":                                       # the defaults: ./sg_edges_list ./utg_data ./ctg_paths
        put(str(tmp_path), *TU.case_files(Z, case)[:3])
        args = ["--improper-p-ctg"]
    else:
        args = ["--proper-a-ctg", "--seqdb-prefix", "nowhere", "--sg-edges-list-fn", inputs[0], "--utg-data-fn=" + inputs[1], "--ctg-paths-fn", inputs[2]]
    out = subprocess.run(TOOLS[tool] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0 and out.stdout == b"", out.stderr
    assert (read(tmp_path / "p_ctg_tiling_path"), read(tmp_path / "a_ctg_tiling_path")) == (p, a)


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_the_commands_refuse_and_write_nothing(files, tool, tmp_path):
    inputs = files["one_edge"][0]
    out = subprocess.run(TOOLS[tool] + ["--sg-edges-list-fn", inputs[0], "--utg-data-fn", inputs[1], "--ctg-paths-fn", inputs[1]], cwd=str(tmp_path), stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 1 and b"line 0" in out.stderr and not (tmp_path / "p_ctg_tiling_path").exists()


# ---- contigs from the rows of a built tiling -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bio(tmp_path_factory):
    """the read set of tests/contig_util.py's simulator and the `bio` tiling path of contig_cases.npz turned into the three inputs: a G line per
    row, a simple unitig and a contig row per contig.  -> (seqdb prefix, the three paths, the golden FASTA)"""
    import contig_util as CU
    from peregrine_amd import formats
    g = np.load(os.path.join(ROOT, "tests", "golden", "contig_cases.npz"))
    tmp = tmp_path_factory.mktemp("tiling_contigs")
    prefix = str(tmp / "reads")
    formats.write_seqdb(prefix, CU.make_db())
    b, by = TU.Builder(1), {}
    for f in (ln.split() for ln in str(g["path_bio"]).splitlines()):
        v, w = (TU.key(int(x[:-2]), x[-1] == "E") for x in f[1:3])
        b.sg.append("%s %s %09d %5d %5d %5d %5.2f G\n" % (TU.name(v), TU.name(w), w >> 1, int(f[4]), int(f[5]), 5000, 99.9))
        by.setdefault(f[0], [v]).append(w)
    for ctg, nodes in by.items():
        u = "%s~%s~%s" % (TU.name(nodes[0]), TU.name(nodes[1]), TU.name(nodes[-1]))
        b.utg.append("%s %s %s simple 0 0 %s\n" % (TU.name(nodes[0]), TU.name(nodes[1]), TU.name(nodes[-1]), "~".join(TU.name(x) for x in nodes)))
        b.contig(ctg, [u], nodes[-1])
    return prefix, put(str(tmp / "in"), *b.files()), g["fasta_bio"].tobytes()


def test_contigs_from_the_rows_equal_the_layout_of_the_written_file(bio, tmp_path):
    prefix, inputs, fasta = bio
    with shimmer.graph_to_path(*inputs) as t:
        assert t.stats["p_rows"] == 52 and t.stats["ctg_kept"] == 6
        st = t.contigs("p", prefix, str(tmp_path / "rows.fa"))
        assert t.contigs("a", prefix, str(tmp_path / "rows_a.fa")) == dict(contigs=0, bases=0) and read(tmp_path / "rows_a.fa") == b""
        t.write(str(tmp_path / "p"), str(tmp_path / "a"))
    assert st == shimmer.path_to_contig(prefix, str(tmp_path / "p"), str(tmp_path / "text.fa")) and st["contigs"] == 6
    assert read(tmp_path / "rows.fa") == read(tmp_path / "text.fa") == fasta
    with shimmer.graph_to_path(*inputs) as t, pytest.raises(_lib.PgxError, match="reads_missing.idx"):
        t.contigs("p", prefix + "_missing", str(tmp_path / "none.fa"))
    assert not (tmp_path / "none.fa").exists()


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_the_commands_lay_the_contigs_out(bio, tool, tmp_path):
    prefix, inputs, fasta = bio
    out = subprocess.run(TOOLS[tool] + ["--seqdb-prefix", prefix, "--sg-edges-list-fn", inputs[0], "--utg-data-fn", inputs[1], "--ctg-paths-fn", inputs[2], "--p-ctg-fa", "p.fa",
                                        "--a-ctg-fa=a.fa"], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0 and out.stdout == b"", out.stderr
    assert read(tmp_path / "p.fa") == fasta and read(tmp_path / "a.fa") == b"" and read(tmp_path / "p_ctg_tiling_path").count(b"\n") == 52


@pytest.mark.parametrize("case", NAMES)
def test_parse_equals_read_sg_edges_list(files, case):
    path = files[case][0][0]
    want = shimmer.read_sg_edges_list(path)
    got, hund = shimmer.parse_sg_edges_list(path, hundredths=True)
    assert got.dtype == shimmer.SGRAPH_EDGE_DTYPE and np.array_equal(got, want)
    fields = [ln.split() for ln in read(path).decode().split("\n") if ln.strip()]
    assert hund.tolist() == [TU.hundredths(f[6]) for f in fields]
    if case.startswith("real_"):
        with shimmer.unitigs(got) as u:                         # the records feed pgx_unitigs_build
            assert u.stats["g_edges"] == CASES[case]["g_edges"]


def test_a_device_graph_equals_the_file_route(tmp_path):
    """a StringGraph whose edges stay on the device, its own unitig lines, a contig per unitig: the files of the file route"""
    zs, sc = SG.load_fixture()
    c = sc["dense"]
    with DedupStream(graph_ready=True) as ds:
        ds.feed(SG.fixture_recs(zs, c["recs"]))
        with ds.string_graph(c["min_len"], c["min_idt"]) as g:
            with g.unitigs() as u:
                utg = b"".join(u.text())
            lines = [ln.split(b" ") for ln in utg.split(b"\n")[:-1]]
            ctg = b"".join(b"%06dF ctg_linear %s %s %s %s %s\n" % (k, b"~".join(f[:3]), f[2], f[4], f[5], b"~".join(f[:3])) for k, f in enumerate(lines))
            t = g.tiling(utg, ctg)
            sg = b"".join(g.text())
    with t:                                                     # the graph is freed: the tiling paths own their arrays
        got = b"".join(t.text("p")), b"".join(t.text("a"))
        st = t.stats
    inputs = put(str(tmp_path), sg, utg, ctg)
    want_st = shimmer.graph_to_path(*inputs, str(tmp_path / "p"), str(tmp_path / "a"))
    assert got == (read(tmp_path / "p"), read(tmp_path / "a")) == TU.tiling_rule(sg, utg, ctg)[:2]
    assert {k: st[k] for k in COUNTS} == {k: want_st[k] for k in COUNTS}
    assert st["ctg_kept"] > 10 and st["ctg_skipped"] > 10 and st["ctg_kept"] + st["ctg_skipped"] + st["ctg_empty"] == len(lines) and st["p_rows"] > 50


def test_a_constructed_tie(tmp_path):
    """two minimum-weight paths share their first edge: whichever the first round takes, the other is gone.  Ours is forward Dijkstra's: the
    neighbour inserted first (read 5)"""
    b = TU.Builder(99)
    s, t, x, a, bb, c = (TU.key(r, TU.E) for r in (1, 2, 3, 5, 6, 7))
    for v, w, score in ((s, x, 1), (x, a, 4), (x, bb, 4), (a, t, 10), (bb, t, 10), (s, c, 20), (c, t, 30)):
        b.edge(v, w, 100, score)
    b.contig("000000F", [b.compound(s, t, [b.simple([s, x]), b.simple([x, a, t]), b.simple([x, bb, t]), b.simple([s, c, t])])], t)
    inputs = put(str(tmp_path), *b.files())
    with shimmer.graph_to_path(*inputs) as tl:
        p, a_text = b"".join(tl.text("p")), b"".join(tl.text("a"))
        assert tl.stats["compound_tie_rounds"] == 1 and tl.stats["alternates"] == 1
    assert (p, a_text) == TU.tiling_rule(*b.files())[:2]
    assert b"000000005:E" in a_text and b"000000006:E" not in a_text and b"000000007:E" in p


def test_equal_weights_across_branches_sort_by_the_names(tmp_path):
    """two disjoint branches of one weight: a tie in round 0 (counted), and a descending sort that the node names decide.  The script's order
    of the two rounds depends on networkx here, so this is held to the restatement only"""
    b = TU.Builder(98)
    s, t, a, bb = (TU.key(r, TU.E) for r in (1, 2, 999999999, 1000000006))
    for v, w, score in ((s, a, 5), (a, t, 10), (s, bb, 7), (bb, t, 8)):
        b.edge(v, w, 100, score)
    b.contig("000000F", [b.compound(s, t, [b.simple([s, a, t]), b.simple([s, bb, t])])], t)
    inputs = put(str(tmp_path), *b.files())
    with shimmer.graph_to_path(*inputs) as tl:
        got = b"".join(tl.text("p")), b"".join(tl.text("a"))
        assert tl.stats["compound_tie_rounds"] == 1 and tl.stats["alternates"] == 1
    assert got == TU.tiling_rule(*b.files())[:2]
    assert b"999999999:E" in got[0] and b"1000000006:E" in got[1]   # as strings '999999999:E' > '1000000006:E', though the read id is smaller


def test_a_long_line_in_a_later_piece_is_named_after_what_comes_before_it(tmp_path, monkeypatch):
    monkeypatch.setenv("PGX_TILING_PIECE", "600")
    b = TU.Builder(97)
    b.contig("000000F", [b.simple([TU.key(r, TU.E) for r in range(1, 32)])], TU.key(31, TU.E))
    assert len(b.sg) == 30 and all(55 < len(ln) < 70 for ln in b.sg)
    b.sg[25] = b.sg[25].replace(" ", " " * 60)                  # 420 bytes more: longer than 256, over the end of its piece
    inputs = put(str(tmp_path), *b.files())
    with pytest.raises(_lib.PgxError, match="sg_edges_list: line 25 is longer"):
        shimmer.graph_to_path(*inputs, str(tmp_path / "p"), str(tmp_path / "a"))
    b.sg[12] = b.sg[12].replace(".", "x")                       # an earlier refused line, in an earlier piece, is the one reported
    inputs = put(str(tmp_path), *b.files())
    with pytest.raises(_lib.PgxError, match="sg_edges_list: line 12 has an identity"):
        shimmer.parse_sg_edges_list(inputs[0])
    assert not (tmp_path / "p").exists()


# The primary file is written in tiles of 8,192 bytes, 16 bytes a store and the bytes behind the last whole 16 one by one (the piece scheme
# that utg_data of the unitigs has its tail cases for in test_gpu_utg.py).  The whole text's last tile as the cases above do not show it: one
# of 1 .. 15 bytes (no 16-byte store at all), and one that ends exactly on a 16-byte store (no byte-wise tail).
TAIL_CASES = {"tail_1_15": lambda length: 1 <= length % 8192 <= 15,
              "tail_16s": lambda length: length > 8192 and length % 8192 != 0 and length % 16 == 0}


def chain_files(n_rows, score):
    """one contig of one simple unitig of n_rows edges, all of one length, score and identity: a primary file of n_rows lines, in which only
    the running length's digits -- and with `score` the score's -- change the length of a line"""
    b = TU.Builder(96)
    nodes = [TU.key(r, TU.E) for r in range(1, n_rows + 2)]
    b.contig("000000F", [b.simple(nodes, length=1000, score=score, s=100, idt="99.50")], nodes[-1])
    return b.files()


def chain_for_tail(accept):
    """(n_rows, score) of the first chain_files, score a power of ten times 7 and n_rows <= 400, whose primary file has a length that accept()
    takes (None: there is none).  The first n lines of a longer chain's file are the file of the chain of n rows, so one run of the rule per
    score gives every length; the caller holds the chosen chain's own file against accept() again."""
    for score in (7, 70, 700, 7000, 70000):
        total = 0
        for n, line in enumerate(TU.tiling_rule(*chain_files(400, score))[0].split(b"\n")[:-1], 1):
            total += len(line) + 1
            if accept(total):
                return n, score
    return None


@pytest.mark.parametrize("name", sorted(TAIL_CASES))
def test_a_primary_file_whose_last_tile_is_a_tail_case(name, tmp_path):
    found = chain_for_tail(TAIL_CASES[name])
    assert found is not None
    n_rows, score = found
    want = TU.tiling_rule(*chain_files(n_rows, score))[0]
    assert TAIL_CASES[name](len(want)) and want.count(b"\n") == n_rows   # before anything runs on the GPU: the case is a tail case
    inputs = put(str(tmp_path), *chain_files(n_rows, score))
    for max_lines in (1, 7, 1 << 20):
        with shimmer.graph_to_path(*inputs) as t:
            parts = list(t.text("p", max_lines))
            assert all(0 < x.count(b"\n") <= max_lines and x.endswith(b"\n") for x in parts) and len(parts) == -(-n_rows // max_lines)
            assert b"".join(parts) == want                      # byte for byte the rule's
            assert list(t.text("a")) == []


def test_a_pipe_is_refused(tmp_path):
    inputs = put(str(tmp_path), *_base().files())
    fifo = str(tmp_path / "fifo")
    os.mkfifo(fifo)
    fd = os.open(fifo, os.O_RDWR)                               # (keeps the open for reading from blocking)
    try:
        with pytest.raises(_lib.PgxError, match="size"):
            shimmer.parse_sg_edges_list(fifo)
    finally:
        os.close(fd)


def test_random_graphs_against_the_rule(tmp_path):
    for seed in range(100):
        sg, utg, ctg = TU.random_case(seed)
        assert sg.count(b"\n") <= 2000
        want_p, want_a, want_st = TU.tiling_rule(sg, utg, ctg)
        inputs = put(str(tmp_path), sg, utg, ctg)
        with shimmer.graph_to_path(*inputs) as t:
            assert (b"".join(t.text("p", 1000)), b"".join(t.text("a"))) == (want_p, want_a), seed
            assert {k: t.stats[k] for k in COUNTS} == want_st, seed


# ---- the refused inputs: the file and the 0-based line the message names, and no output file afterwards ------------------------------------
def _base():
    b = TU.Builder(31)
    s, t = TU.key(1, TU.E), TU.key(2, TU.E)
    c, nxt = TU.bubble(b, s, t, 10, 2, [1, 2])
    b.contig("000000F", [b.simple([TU.key(5, TU.E), TU.key(6, TU.B), s]), c], t)
    return b


def _edit(lines, k, fn):
    lines[k] = fn(lines[k])


def _field(i, new):
    def fn(ln):
        f = ln.split()
        f[i] = new(f[i]) if callable(new) else new
        return " ".join(f) + "\n"
    return fn


def _errors():
    """name -> (builder after the damage, file, line)"""
    out = {}

    def case(name, file, line, damage):
        b = _base()
        damage(b)
        out[name] = (b, file, line)

    g_lines = lambda b: [k for k, ln in enumerate(b.sg) if ln.split()[7] == "G"]   # noqa: E731
    case("sg_7_fields", "sg_edges_list", 3, lambda b: _edit(b.sg, 3, lambda ln: " ".join(ln.split()[:7]) + "\n"))
    case("sg_9_fields", "sg_edges_list", 2, lambda b: _edit(b.sg, 2, lambda ln: ln[:-1] + " x\n"))
    case("utg_6_fields", "utg_data", 1, lambda b: _edit(b.utg, 1, lambda ln: " ".join(ln.split()[:6]) + "\n"))
    case("ctg_8_fields", "ctg_paths", 0, lambda b: _edit(b.ctg, 0, lambda ln: ln[:-1] + " x\n"))
    case("assertion", "sg_edges_list", 1, lambda b: _edit(b.sg, 1, lambda ln: _field(4, ln.split()[3])(_field(3, ln.split()[4])(ln))))
    case("unitig_missing", "ctg_paths", 0, lambda b: _edit(b.ctg, 0, _field(6, lambda x: x.replace("000000005:E~000000006:B", "000000005:E~000000007:B"))))
    case("unitig_dropped_type", "ctg_paths", 0, lambda b: _edit(b.utg, len(b.utg) - 1, _field(3, "spur:2")))
    case("sub_missing", "utg_data", 1, lambda b: b.utg.pop(0))
    case("edge_missing", "ctg_paths", 0, lambda b: _edit(b.sg, len(b.sg) - 1, _field(7, "TR")))
    case("bundle_edge_missing", "utg_data", 2, lambda b: _edit(b.sg, 0, _field(7, "R")))

    def nested(b):
        b.utg[0] = b.utg[0].replace(" simple ", " compound ").rsplit(" ", 1)[0] + " 000000005:E~000000006:B~000000001:E\n"
    case("sub_compound", "utg_data", 2, nested)
    case("s_absent", "utg_data", 2, lambda b: _edit(b.utg, 2, lambda ln: ln.replace("000000001:E NA", "000000005:E NA")) or _edit(
        b.ctg, 0, _field(6, lambda x: x.replace("000000001:E~NA", "000000005:E~NA"))))
    case("weight_zero", "utg_data", 2, lambda b: _edit(b.sg, 0, _field(5, "0")))
    case("weight_huge", "utg_data", 2, lambda b: _edit(b.sg, 0, _field(5, str(1 << 40))))
    case("vw_twice", "sg_edges_list", len(_base().sg), lambda b: b.sg.append(b.sg[1]))
    case("key_twice", "utg_data", len(_base().utg), lambda b: b.utg.append(b.utg[0]))
    case("name_short", "sg_edges_list", 0, lambda b: _edit(b.sg, 0, _field(0, lambda x: x[1:])))
    case("name_letters", "sg_edges_list", 0, lambda b: _edit(b.sg, 0, _field(1, lambda x: "00000000x" + x[9:])))
    case("rid_unpadded", "sg_edges_list", 4, lambda b: _edit(b.sg, 4, _field(2, lambda x: x.lstrip("0"))))
    case("idt_3_digits", "sg_edges_list", 2, lambda b: _edit(b.sg, 2, _field(6, "99.625")))
    case("idt_exponent", "sg_edges_list", 2, lambda b: _edit(b.sg, 2, _field(6, "9.9e1")))
    case("idt_nan", "sg_edges_list", 2, lambda b: _edit(b.sg, 2, _field(6, "nan")))
    case("number_float", "sg_edges_list", 2, lambda b: _edit(b.sg, 2, _field(3, "12.0")))
    case("line_too_long", "sg_edges_list", 1, lambda b: _edit(b.sg, 1, lambda ln: ln.replace(" ", " " * 40)))
    assert all(k < len(_base().sg) for k in g_lines(_base()))
    return out


ERRORS = _errors()


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_refused_inputs_name_the_line_and_write_nothing(name, tmp_path):
    b, file, line = ERRORS[name]
    inputs = put(str(tmp_path), *b.files())
    with pytest.raises(_lib.PgxError) as ei:
        shimmer.graph_to_path(*inputs, str(tmp_path / "p"), str(tmp_path / "a"))
    msg = str(ei.value)
    assert "code %d" % _lib.PGX_EINVAL in msg and os.path.join(str(tmp_path), file) + ": line %d" % line in msg, msg
    assert not (tmp_path / "p").exists() and not (tmp_path / "a").exists()
    with pytest.raises(TU.RuleError):                           # the restatement refuses it too
        TU.tiling_rule(*b.files())
    st = shimmer.graph_to_path(*put(str(tmp_path / "ok"), *_base().files()), str(tmp_path / "p"), str(tmp_path / "a"))   # the library is usable afterwards
    assert st["p_rows"] > 0 and st["alternates"] == 1


def test_the_assertion_is_refused_before_a_repeated_edge(tmp_path):
    """the order of the refusals: an input with both damages gets the assertion's, on its own line"""
    b = _base()
    b.sg.append(b.sg[1])                                                                          # vw_twice
    _edit(b.sg, 1, lambda ln: _field(4, ln.split()[3])(_field(3, ln.split()[4])(ln)))             # assertion
    inputs = put(str(tmp_path), *b.files())
    with pytest.raises(_lib.PgxError) as ei:
        shimmer.graph_to_path(*inputs, str(tmp_path / "p"), str(tmp_path / "a"))
    msg = str(ei.value)
    assert "code %d" % _lib.PGX_EINVAL in msg and os.path.join(str(tmp_path), "sg_edges_list") + ": line 1:" in msg, msg
    assert "the script asserts it" in msg and "repeats" not in msg, msg
    assert not (tmp_path / "p").exists() and not (tmp_path / "a").exists()


def test_lines_the_script_only_counts_are_not_parsed(tmp_path):
    """a TR line with fields that are no numbers, a dropped unitig type with a path of anything: the script reads neither"""
    b = _base()
    want = TU.tiling_rule(*b.files())[:2]
    b.sg.insert(1, "x y z a b c d TR\n"), b.utg.append("a b c spur:2 x y z\n")
    inputs = put(str(tmp_path), *b.files())
    shimmer.graph_to_path(*inputs, str(tmp_path / "p"), str(tmp_path / "a"))
    assert (read(tmp_path / "p"), read(tmp_path / "a")) == want
    with pytest.raises(_lib.PgxError, match="line 1 "):        # pgx_sgraph_parse hands every line out as numbers
        shimmer.parse_sg_edges_list(inputs[0])
