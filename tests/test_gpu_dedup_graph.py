"""The dedup stream's graph mode on the GPU (pgx_dedup_open_graph / _drain / _graph_stats, DedupStream(graph_ready=True),
shimmer.dedup_graph_ready, `shmr_dedup -g` of both drop-ins): whatever the cut of the stream into feeds and of the text into drains, the
output is the selection rule (tests/dedup_graph_util.py) applied to the reference's text of the whole stream, byte for byte."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dedup_graph_util as DG
import golden_util as G
import oracle_util as U
from peregrine_amd import _lib, shimmer
from peregrine_amd.formats import OVLP_DTYPE
from peregrine_amd.shimmer import DedupStream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DEDUP = os.path.join(U.REF_DIR, "shmr_dedup")
rec = DG.rec
TOP = 2**32 - 1


def full_text(recs):
    """the real reference's stdout where its binary travels with the tree, else the oracle's restatement"""
    if len(recs) == 0:
        return b""      # (the reference prints a line of uninitialised memory on an empty stream; the library writes nothing)
    if os.path.exists(REF_DEDUP):
        return subprocess.run([REF_DEDUP], input=np.ascontiguousarray(recs).tobytes(), stdout=subprocess.PIPE, check=True).stdout
    return U.orc_dedup(recs)[0]


def cat(*parts):
    return np.concatenate(parts)


def drained(recs, piece=0, max_lines=1 << 20, before_drain=None):
    """the text of a graph-mode stream fed recs in pieces of `piece` records (0: one feed), its stats after the drain, close()'s counts"""
    n = len(recs)
    cuts = list(range(0, n, piece)) + [n] if piece else [0, n]
    with DedupStream(graph_ready=True) as ds:
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert ds.feed(recs[a:b]) == b""
        if before_drain:
            before_drain(ds)
        parts = list(ds.drain(max_lines))
        assert all(0 < p.count(b"\n") <= max_lines and p.endswith(b"\n") for p in parts)
        stats = ds.stats
        counts = ds.close()
    return b"".join(parts), stats, counts


def check(recs, piece=0, **kw):
    full = full_text(recs)
    want = DG.select_graph_lines(full)
    got, stats, counts = drained(recs, piece, **kw)
    assert got == want, (piece, kw)
    assert stats == DG.graph_stats(full) and counts == (len(recs), full.count(b"\n"))
    return want, full


# reads 1 .. 9 overlap each other; the marks of 1 (a `contained` line) and of 4 (a `contains` line) come at the END of the stream
LATE = cat(rec(1, 2), rec(3, 1), rec(4, 5), rec(5, 6), rec(6, 4), rec(2, 3), rec(7, 8), rec(8, 9), rec(9, 1), rec(2, 5, dist=333),
           rec(3, 7), rec(7, 4), rec(1, 30, typ=2), rec(31, 4, typ=1))


@pytest.mark.parametrize("piece", [1, 7, 0])
def test_a_mark_that_arrives_after_the_lines_it_voids(piece):
    held = []
    want, full = check(LATE, piece, before_drain=lambda ds: held.append(ds.stats["lines_kept"]))
    assert want.count(b"\n") == 6 and full.count(b"\n") == 14
    # fed record by record, the rows of 1's and 4's lines were in the store when their marks came: only the final pass drops them
    # (in feeds of 7 the marks share the second feed with five lines, of which they void two before the append)
    assert held[0] == {1: 12, 7: 10, 0: 6}[piece]


def test_a_mark_that_arrives_first_keeps_its_reads_rows_out_of_the_store():
    recs = cat(LATE[12:], LATE[:12])
    held = []
    want, _ = check(recs, 2, before_drain=lambda ds: held.append(ds.stats))
    assert want == DG.select_graph_lines(full_text(LATE))           # the same lines as with late marks
    assert held[0] == dict(contained_reads=2, lines_kept=6, lines_total=14)


def test_a_record_that_lost_first_wins_marks_nothing():
    recs = cat(rec(10, 11), rec(11, 12), rec(10, 11, typ=2), rec(11, 10, typ=2), rec(10, 11, typ=1), rec(12, 13), rec(12, 11, typ=1), rec(13, 12, typ=3))
    for piece in (0, 1, 3):
        want, full = check(recs, piece)
        assert want == full and want.count(b"\n") == 3                # 10, 11, 12 stay unmarked: every later record repeats a pair


def test_self_pairs_mark_nothing_and_are_dropped():
    recs = cat(rec(20, 20, typ=2), rec(21, 21, typ=1), rec(22, 22), rec(20, 21), rec(21, 22), rec(22, 23), rec(23, 23, typ=7))
    want, full = check(recs, 2)
    assert full.count(b"\n") == 7 and [ln.split()[:2] for ln in want.split(b"\n")[:-1]] == [[b"000000020", b"000000021"], [b"000000021", b"000000022"], [b"000000022", b"000000023"]]


def test_every_type_value_but_0_and_1_marks_rid0():
    recs = cat(rec(40, 41), rec(41, 42), rec(42, 43), rec(43, 44), rec(44, 45), rec(40, 50, typ=3), rec(51, 42, typ=255), rec(52, 44, typ=1))
    want, full = check(recs, 3)
    assert {ln.split()[-1] for ln in full.split(b"\n")[:-1]} == {b"overlap", b"contained", b"contains"}
    assert [int(ln.split()[0]) for ln in want.split(b"\n")[:-1]] == [41, 42]     # 40 (type 3), 51 -- not 42 -- (type 255) and 44 (contains) are marked


def edge_set(marked, others):
    """overlap lines between all the reads named, then a `contained` line per marked read"""
    reads = sorted(set(marked) | set(others))
    lines = [rec(a, b) for i, a in enumerate(reads) for b in reads[i + 1:]]
    return cat(*lines, *[rec(m, 1000 + k, typ=2) for k, m in enumerate(marked)])


@pytest.mark.parametrize("marked,others", [((0, 31, 64, TOP), (1, 30, 32, 63, 65, TOP - 1)), ((32, 63), (0, 31, 33, 62, 64, TOP))])
def test_read_ids_at_the_edges_of_the_bitmaps_words(marked, others):
    recs = edge_set(marked, others)
    want, _ = check(recs)
    ids = {int(x) & TOP for ln in want.split(b"\n")[:-1] for x in ln.split()[:2]}
    assert ids == set(others)
    # the bitmap grows with the largest marked id: the marks one feed each, smallest first, after all the overlap lines
    _lib.mem_ledger(reset_peak=True)
    n = len(recs) - len(marked)
    got = []
    with DedupStream(graph_ready=True) as ds:
        ds.feed(recs[:n])
        for k in range(len(marked)):
            ds.feed(recs[n + k:n + k + 1])
            got.append(ds.stats["contained_reads"])
        assert b"".join(ds.drain()) == want
    assert got == list(range(1, len(marked) + 1))
    peak = _lib.mem_ledger()["peak_by_tag"].get("dedup", 0)
    assert (peak >= (512 << 20)) == (TOP in marked), peak               # 2^32 bits only when the top id is MARKED, not when it is merely seen


def raw_drain(h, max_lines):
    lib = _lib.load()
    text, tl, done = C.c_void_p(), C.c_size_t(7), C.c_int(7)
    rc = lib.pgx_dedup_drain(h, max_lines, C.byref(text), C.byref(tl), C.byref(done))
    data = C.string_at(text.value, tl.value) if text.value else None
    lib.pgx_free(text)
    return rc, data, done.value


def test_degenerate_streams():
    # nothing marked: the plain stream's text minus the self-pair lines
    recs = cat(LATE[:12], rec(5, 5), rec(6, 6, typ=0))
    with DedupStream() as ds:
        plain = ds.feed(recs)
    want, full = check(recs, 5)
    assert full == plain and want == b"".join(ln + b"\n" for ln in plain.split(b"\n")[:-1] if ln.split()[0] != ln.split()[1]) and want.count(b"\n") == 12
    # everything marked, and the empty stream: no text, done with the first drain call
    for recs in (cat(rec(1, 2), rec(2, 3), rec(3, 1), rec(1, 9, typ=2), rec(9, 2, typ=1), rec(3, 9, typ=5)), np.zeros(0, OVLP_DTYPE)):
        check(recs)
        with DedupStream(graph_ready=True) as ds:
            ds.feed(recs)
            assert raw_drain(ds.h, 1) == (0, b"", 1) and raw_drain(ds.h, 1) == (0, b"", 1)
            assert ds.stats["lines_kept"] == 0
    assert shimmer.dedup_graph_ready(np.zeros(0, OVLP_DTYPE)) == b""


@pytest.mark.parametrize("max_lines", [1, 3, 1 << 20])
def test_drains_of_any_size_give_the_same_bytes(max_lines):
    recs = cat(LATE[:6], rec(60, 61, m_size=0, dist=0), rec(61, 62, m_size=0, dist=-3), LATE[6:], rec(62, 63, m_size=0, dist=4))   # inf / nan: the host's lines
    want, _ = check(recs, 4, max_lines=max_lines)
    assert want.count(b"\n") == 9 and sum(b"nan" in ln or b"inf" in ln for ln in want.split(b"\n")) == 3
    assert shimmer.dedup_graph_ready(recs) == want


def test_feed_dev_from_a_tensor():
    import torch
    recs = G.load("graph_filter_cases.npz")["recs"]
    want = DG.select_graph_lines(G.load("graph_filter_cases.npz")["text"].tobytes())
    d = torch.from_numpy(recs.view(np.uint8).copy()).to("cuda:0")
    half = len(recs) // 2
    with DedupStream(graph_ready=True) as ds:
        assert ds.feed_dev(d.data_ptr(), half) == b""
        assert ds.feed(recs[half:half + 100]) == b""
        assert ds.feed_dev(d.data_ptr() + (half + 100) * 64, len(recs) - half - 100) == b""
        assert b"".join(ds.drain(5000)) == want


def test_a_feed_after_the_first_drain_is_refused_and_the_drain_goes_on():
    lib = _lib.load()
    want = DG.select_graph_lines(full_text(LATE))
    r1 = np.ascontiguousarray(LATE[:1])
    with DedupStream(graph_ready=True) as ds:
        ds.feed(LATE)
        rc, first, done = raw_drain(ds.h, 2)
        assert (rc, done) == (0, 0) and first.count(b"\n") == 2
        text, tl = C.c_void_p(0xDEAD0000BEEF), C.c_size_t(5)
        for fn, ptr in ((lib.pgx_dedup_feed, r1.ctypes.data_as(C.c_void_p)), (lib.pgx_dedup_feed_dev, C.c_void_p(64))):
            assert fn(ds.h, ptr, 1, C.byref(text), C.byref(tl)) == _lib.PGX_ESTATE and not text.value and tl.value == 0
            assert b"drain" in lib.pgx_last_error()
        with pytest.raises(_lib.PgxError):
            ds.feed(LATE[:1])
        assert first + b"".join(ds.drain(3)) == want
        assert ds.close() == (len(LATE), 14)
    # the graph calls refuse a plain stream (which stays usable), max_lines == 0 and null outputs
    with DedupStream() as ds:
        assert raw_drain(ds.h, 5)[0] == _lib.PGX_ESTATE and lib.pgx_dedup_graph_stats(ds.h, None, None, None) == _lib.PGX_ESTATE
        assert ds.feed(LATE) == full_text(LATE)
    with DedupStream(graph_ready=True) as ds:
        assert raw_drain(ds.h, 0)[0] == _lib.PGX_EARG


@pytest.mark.parametrize("piece", [1000, 0])
def test_the_fixtures_case(piece):
    z = G.load("graph_filter_cases.npz")
    recs, text = z["recs"], z["text"].tobytes()
    got, stats, counts = drained(recs, piece, max_lines=3000)
    assert got == DG.select_graph_lines(text)
    assert stats == DG.graph_stats(text) and counts == (len(recs), text.count(b"\n"))
    units = C.c_uint64(0)
    assert _lib.load().pgx_timing_get(b"dedup", None, None, C.byref(units)) == 0 and units.value > 0


def _native_cmd():
    exe = os.path.join(ROOT, "bin", "native", "shmr_dedup")
    return [exe] if os.path.exists(exe) else [os.path.join(ROOT, "bin", "native", "pgx_cli"), "shmr_dedup"]


def test_both_commands_with_and_without_g():
    z = G.load("graph_filter_cases.npz")
    raw, text = z["recs"].tobytes(), z["text"].tobytes()
    want = DG.select_graph_lines(text)
    env = dict(os.environ, PGX_DEDUP_PIECE="5000")     # four feeds, two drains
    for cmd in (_native_cmd(), [sys.executable, os.path.join(ROOT, "bin", "shmr_dedup")]):
        for flags, expect in (["-g"], want), ([], text):
            r = subprocess.run(cmd + flags, input=raw, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
            assert r.returncode == 0, r.stderr
            assert r.stdout == expect, (cmd, flags)
    assert subprocess.run(_native_cmd() + ["-g"], input=b"", stdout=subprocess.PIPE, check=True, timeout=120).stdout == b""
