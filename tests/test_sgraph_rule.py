"""The string graph's rule without a GPU: the plain-Python restatement (tests/sgraph_util.py) reproduces, byte for byte, every
sg_edges_list the real generate_string_graph wrote (tests/golden/sgraph_cases.npz, and the one of graph_filter_cases.npz from that file's
records).  This is what lets the GPU tests use inputs that have no fixture."""
import hashlib
import json
import os

import numpy as np
import pytest

import dedup_graph_util as DG
import golden_util as G
import oracle_util as U
import sgraph_util as SG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    return SG.load_fixture()


def case_text(z, cases, name):
    return U.orc_dedup(SG.fixture_recs(z, cases[name]["recs"]))[0]


def test_fixture_is_pinned(fixture):
    z, cases = fixture
    prov = json.load(open(os.path.join(ROOT, "tests", "golden", "sgraph_cases.provenance.json")))
    assert prov["cases"] == cases and prov["disable_chimer_bridge_removal"] is True and prov["lfc"] is False and len(prov["hash_seeds"]) == 2
    assert set(cases) == {"dense", "dense_idt", "dense_len", "quant", "spur_a", "spur_b", "directed", "none", "single"}
    for name in cases:
        sg = z[name + "_sg"].tobytes()
        s = prov["summary"][name]
        assert hashlib.sha256(sg).hexdigest() == s["sha256"] and sg.count(b"\n") == s["edges"], name
    d = prov["summary"]["dense"]
    assert d["max_out_degree"] > 64 and min(d["G"], d["TR"], d["S"], d["R"]) > 0
    assert z["none_sg"].tobytes() == b"" and prov["summary"]["single"]["edges"] == 2
    assert z["spur_a_sg"].tobytes() != z["spur_b_sg"].tobytes()
    for name in ("sgraph_cases.npz", "sgraph_cases_quant.npz"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < 1_000_000


@pytest.mark.parametrize("name", ["dense", "dense_idt", "dense_len", "quant", "spur_a", "spur_b", "directed", "none", "single"])
def test_the_restatement_reproduces_the_reference(fixture, name):
    z, cases = fixture
    c = cases[name]
    want = z[name + "_sg"].tobytes()
    got, recs, stats = SG.string_graph_of_full_text(case_text(z, cases, name), c["min_len"], c["min_idt"])
    assert got == want
    assert {k: stats[k] for k in ("edges", "n_g", "n_tr", "n_s", "n_r")} == SG.stats_of_text(want)
    assert np.array_equal(recs, SG.edges_of_text(want))


def test_the_graph_filter_fixtures_graph_from_its_records():
    z = G.load("graph_filter_cases.npz")
    text = U.orc_dedup(z["recs"])[0]
    assert text == z["text"].tobytes()
    got, _, stats = SG.string_graph_of_full_text(text, 4000, 96.0)
    assert got == z["sg_edges_list"].tobytes()
    assert stats["rows_in"] == DG.graph_stats(text)["lines_kept"] and stats["edges"] > 1000


def test_what_the_cases_are_there_for(fixture):
    z, cases = fixture
    _, _, d = SG.string_graph_of_full_text(case_text(z, cases, "dense"), 2000, 96.0)
    assert d["max_out_degree"] > 64 and d["spur_candidates"] > 0
    # the spur pass depends on the order of the nodes: the same three lines, two orders, two answers
    a = SG.string_graph_of_full_text(case_text(z, cases, "spur_a"))[0]
    b = SG.string_graph_of_full_text(case_text(z, cases, "spur_b"))[0]
    assert sorted(a.split(b"\n")) != sorted(b.split(b"\n"))
    # the quantised case has ties of length within an out-list and of score: either tie rule reversed changes the output
    text = case_text(z, cases, "quant")
    want = z["quant_sg"].tobytes()
    rows = SG.rows_of_text(DG.select_graph_lines(text))
    assert len({r[2] for r in rows}) < len(rows) // 4


def test_entry_points_are_declared_exported_and_need_a_device_context(tmp_path):
    import ctypes as C
    import re
    import subprocess
    import sys
    from peregrine_amd import _lib, shimmer
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    names = ("pgx_sgraph_build", "pgx_sgraph_stats", "pgx_sgraph_edges", "pgx_sgraph_text", "pgx_sgraph_free")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgx.h")).read(), flags=re.S)
    for n in names:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr) and n in _lib.EXPORTS and getattr(lib, n).argtypes, n
    # the numpy mirrors against what a C compiler makes of the header
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pgx.h"\nint main(void) { printf("%zu %zu %zu %zu %d\\n", sizeof(pgx_sgraph_edge), '
                   'offsetof(pgx_sgraph_edge, score), offsetof(pgx_sgraph_edge, type), sizeof(pgx_sgraph_stats_t), PGX_EINVAL); return 0; }\n')
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    d = SG.EDGE_DTYPE
    assert subprocess.check_output([str(tmp_path / "sz")], text=True).split() == [str(v) for v in (d.itemsize, d.fields["score"][1], d.fields["type"][1], 80, _lib.PGX_EINVAL)]
    assert d == shimmer.SGRAPH_EDGE_DTYPE and d.itemsize == 40
    # without pgx_init (a child process) the build answers PGX_ESTATE and clears its output
    code = ("import ctypes as C\nfrom peregrine_amd import _lib\nlib = _lib.load()\ng = C.c_void_p(0xDEAD0000BEEF)\n"
            "print(lib.pgx_sgraph_build(None, 4000, 96.0, 0, C.byref(g)), g.value, lib.pgx_sgraph_free(None), lib.pgx_last_error().decode())\n")
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ, PGX_NO_TORCH="1", PYTHONPATH=ROOT), timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("%d None 0 pgx_sgraph_build: no device context" % _lib.PGX_ESTATE), out.stdout
