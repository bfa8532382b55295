"""shmr_dedup's graph mode without a GPU: the selection rule (tests/dedup_graph_util.py) leaves the string graph's loader the input it
takes from the full text; the golden case (tests/golden/graph_filter_cases.npz: the real reference's text and the real
generate_string_graph's sg_edges_list) is pinned; the three entry points are declared, exported and refuse to run without a device."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import dedup_graph_util as DG
import golden_util as G
import oracle_util as U
from peregrine_amd import _lib
from peregrine_amd.formats import OVLP_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DEDUP = os.path.join(U.REF_DIR, "shmr_dedup")
NAMES = ("pgx_dedup_open_graph", "pgx_dedup_drain", "pgx_dedup_graph_stats")
FILTERS = [(0, 0.0), (4000, 96.0), (10000, 99.5)]


@pytest.fixture(scope="module")
def cases():
    """name -> text of a generated record set: the real reference's where its binary is present, else the fixture's"""
    z = G.load("graph_filter_cases.npz")
    recs, text = DG.make_records(), z["text"].tobytes()
    assert recs.dtype == OVLP_DTYPE and recs.tobytes() == z["recs"].tobytes()   # the fixture's records ARE the generated set
    out = {"fixture": text}
    if os.path.exists(REF_DEDUP):
        for name, r in (("fixture", recs), ("seed 7", DG.make_records(7, n_reads=150, genome=20_000)), ("seed 8, few marked", DG.make_records(8, n_reads=150, genome=20_000, contained_share=0.05))):
            out[name] = subprocess.run([REF_DEDUP], input=r.tobytes(), stdout=subprocess.PIPE, check=True).stdout
        assert out["fixture"] == text
    return out


def test_the_loader_takes_the_same_input_from_the_filtered_text(cases):
    for name, text in cases.items():
        kept = DG.select_graph_lines(text)
        for min_len, min_idt in FILTERS:
            full, part = DG.loader_input(text, min_len, min_idt), DG.loader_input(kept, min_len, min_idt)
            assert full == part, (name, min_len, min_idt)
            assert len(full) > 0, (name, min_len, min_idt)
        # the two loader filters really cut: what they are checked against
        n = [len(DG.loader_input(text, *f)) for f in FILTERS]
        assert n[0] == kept.count(b"\n") and n[0] > n[1] > n[2] > 0, (name, n)


def test_the_filtered_text_is_a_subsequence_that_drops_lines(cases):
    for name, text in cases.items():
        kept = DG.select_graph_lines(text)
        assert DG.is_subsequence(kept, text), name
        assert not DG.is_subsequence(kept + b"x\n", text)
        assert DG.select_graph_lines(kept) == kept, name          # nothing left to mark: the rule is idempotent
        assert all(ln.endswith(b" overlap") for ln in kept.split(b"\n")[:-1])


def test_the_random_case_keeps_a_real_share(cases):
    text = cases["fixture"]
    st = DG.graph_stats(text)
    reads = {f for ln in text.split(b"\n")[:-1] for f in ln.split()[:2]}
    share, marked = st["lines_kept"] / st["lines_total"], st["contained_reads"] / len(reads)
    print(f"graph filter fixture: {len(reads)} reads, {marked:.1%} marked; {st['lines_kept']} of {st['lines_total']} lines kept ({share:.1%})")
    assert 0.05 <= share <= 0.95, share
    assert 0.2 <= marked <= 0.4 and len(reads) == 300, (marked, len(reads))
    # what the set is there for: all three printed types, type values beyond 2, self pairs, recurrences that would mark other reads
    recs = G.load("graph_filter_cases.npz")["recs"]
    assert {ln.split()[-1] for ln in text.split(b"\n")[:-1]} == {b"overlap", b"contains", b"contained"}
    assert set(np.unique(recs["ovlp_type"]).tolist()) >= {0, 1, 2, 3, 7}
    assert sum(ln.split()[0] == ln.split()[1] for ln in text.split(b"\n")[:-1]) == 12
    assert len(recs) - st["lines_total"] > 2000
    lost = U.orc_dedup(np.concatenate([recs, recs]))[0]           # (every record again: all of them lose)
    assert lost == text


def test_fixture_is_pinned():
    z = G.load("graph_filter_cases.npz")
    text, sg = z["text"].tobytes(), z["sg_edges_list"].tobytes()
    prov = json.loads(str(z["provenance"]))
    assert prov == json.load(open(os.path.join(ROOT, "tests", "golden", "graph_filter_cases.provenance.json")))
    assert U.orc_dedup(z["recs"])[0] == text                        # the oracle's restatement agrees with the reference binary
    assert prov["filtered_text_gives_the_same_sg_edges_list"] is True and prov["disable_chimer_bridge_removal"] is True
    assert hashlib.sha256(sg).hexdigest() == prov["sg_edges_sha256"] and sg.count(b"\n") == prov["sg_edges"] > 1000
    assert DG.graph_stats(text) == {k: prov[k] for k in ("contained_reads", "lines_kept", "lines_total")}
    # every edge of the real graph joins two reads that the filtered text still names
    named = {f for ln in DG.select_graph_lines(text).split(b"\n")[:-1] for f in ln.split()[:2]}
    assert {e.split(b":")[0] for ln in sg.split(b"\n")[:-1] for e in ln.split()[:2]} <= named
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "graph_filter_cases.npz")) < (1 << 20)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_graph_entry_points_are_exported_and_need_a_device_context(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgx.h")).read(), flags=re.S)
    exported = {ln.split()[-1].split("@")[0] for ln in subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True).splitlines() if ln.strip()}
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), n
        assert n in exported and n in _lib.EXPORTS and getattr(lib, n).argtypes, n
    # without pgx_init (a child process: another test of this one may have made a context) all three answer PGX_ESTATE
    code = ("import ctypes as C\nfrom peregrine_amd import _lib\nlib = _lib.load()\nh, t, n, d, a = C.c_void_p(), C.c_void_p(0xDEAD0000BEEF), C.c_size_t(9), C.c_int(9), C.c_uint64(9)\n"
            "r = [lib.pgx_dedup_open_graph(0, C.byref(h)), lib.pgx_dedup_drain(None, 5, C.byref(t), C.byref(n), C.byref(d)), lib.pgx_dedup_graph_stats(None, C.byref(a), None, None)]\n"
            "print(r, h.value, t.value, n.value, d.value, a.value, lib.pgx_last_error().decode())\n")
    env = dict(os.environ, PGX_NO_TORCH="1", PYTHONPATH=ROOT)
    out = subprocess.run([os.sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("[%d, %d, %d] None None 0 0 9 " % ((_lib.PGX_ESTATE,) * 3)), out.stdout
    assert "pgx_dedup_graph_stats: no device context" in out.stdout
