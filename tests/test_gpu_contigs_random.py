"""Contig layout on the GPU against the numpy statement of the reference script (contig_util.layout over the oracle's ovlp_match), in full
and byte for byte, on inputs made to reach what the golden paths of test_gpu_contigs.py cannot: 21,000 rows in 2,000 contigs (rows beyond
one workgroup, scans beyond one tile), tiles with tens of covering segments and several whole contigs, every byte phase of the stitch
copy, and the three device-side error kinds, alone and mixed.  tests/test_contig_paths.py holds the inputs to those properties on the CPU."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import contig_util as CU
import oracle_util as U
from peregrine_amd import _lib, formats, shimmer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = ("bytes", "released", "compacted")
TILE = 4096


@contextlib.contextmanager
def _batch(value):
    saved = os.environ.pop("PGX_CONTIGS_BATCH", None)
    if value is not None:
        os.environ["PGX_CONTIGS_BATCH"] = str(value)
    try:
        yield
    finally:
        os.environ.pop("PGX_CONTIGS_BATCH", None)
        if saved is not None:
            os.environ["PGX_CONTIGS_BATCH"] = saved


def _first_difference(case, data, off):
    """the first differing contig, its offset, the tile, and the segments the statement has on that byte"""
    want = np.frombuffer(b"".join(case.fasta.split(b"\n")[1::2]), np.uint8)
    got = np.frombuffer(data, np.uint8)
    if len(got) != len(want):
        return "the output has %d bytes, the statement %d" % (len(got), len(want))
    p = int(np.flatnonzero(got != want)[0])
    c = int(np.searchsorted(case.ctg_off, p, side="right")) - 1
    local = p - int(case.ctg_off[c])
    cover = [s for s in case.segs[c][0] if s[4] and s[1] <= local < s[1] + s[4]]
    return ("byte %d: contig %d (%s) offset %d, tile %d byte %d: got %r, want %r; segments on it (row, start, read, source, length, strand): %s; "
            "%d bytes differ in all" % (p, c, case.names[c], local, p // TILE, p % TILE, chr(got[p]), chr(want[p]), cover, int((got != want).sum())))


@pytest.mark.parametrize("state", STATES)
def test_random_paths_equal_the_statement(state):
    case = CU.case(state != "released")          # (a database with an ambiguous base cannot be released)
    rdb = shimmer.ResidentDB(case.db, 0)
    if state == "released":
        assert rdb.release_bytes() and not rdb.has_bytes and rdb.side_bytes == 0
    elif state == "compacted":
        assert rdb.compact_bytes() and not rdb.has_bytes and rdb.side_bytes > 0
    rows, names = CU.tile_rows(case.text)
    data, off = rdb.contigs(rows)
    assert np.array_equal(off.astype(np.int64), case.ctg_off), "contig %d starts elsewhere" % int(np.flatnonzero(off.astype(np.int64) != case.ctg_off)[0])
    assert CU.fasta_of(data, off, names) == case.fasta, _first_difference(case, data, off)
    # the alignments of the same rows, one by one
    rl, _ = case.db.by_rid()
    keys = np.zeros(len(rows), _lib.ALIGN_KEY2_DTYPE)
    keys["rid0"], keys["rid1"], keys["dir0"], keys["dir1"] = rows["rid0"], rows["rid1"], rows["strand0"], rows["strand1"]
    keys["q_off"] = rl[rows["rid0"]].astype(np.int64) - CU.H
    keys["t_off"] = rl[rows["rid1"]].astype(np.int64) - np.abs(rows["e"].astype(np.int64) - rows["s"]) - CU.H
    got = rdb.align2(keys).view(np.int32).reshape(-1, 8)
    want = np.array(case.matches, np.int32)
    differ = np.flatnonzero((got != want).any(axis=1))
    assert len(differ) == 0, (len(differ), int(differ[0]), keys[differ[0]], got[differ[0]], want[differ[0]])
    rdb.close()


@pytest.fixture(scope="module")
def engineered():
    """the short-read set with the engineered reads appended, resident with its bytes"""
    case = CU.case(True)
    db, ids = CU.engineered_reads(case.db)
    rdb = shimmer.ResidentDB(db, 0)
    yield case, db, ids, rdb
    rdb.close()


def _paths_of_total(case, db):
    """[(delta, text, the statement's segments, total)] with total = 4096 m + delta, m >= 2, for delta = 0, 1, -1: the first contigs of the
    random path, then one-row contigs of a read against itself (seg == 0: the contig is the read) whose lengths add up to what is missing"""
    fillers = CU.filler_contigs(case, 40)
    base = sum(n for _, n in case.segs[:len(fillers)])
    rl = case.db.rlen.astype(np.int64)
    present = sorted(set(rl[rl > CU.H].tolist()))
    mid = present[len(present) // 2]
    out = []
    for delta in (0, 1, -1):
        need = (delta - base) % TILE
        need += TILE if need < 2 * CU.H + 2 else 0
        lens = [mid] * ((need - 2 * CU.H - 2) // mid)            # then two reads for the rest, which is beyond 1,002
        rest = need - sum(lens)
        lens += next([a, rest - a] for a in present if rest - a in present)
        ends = [["%d:E %d:E 0 %d %d 0 0 x self" % (r, r, n - 1, n)] for n in lens for r in [int(np.flatnonzero(rl == n)[0])]]
        text = CU.assemble(fillers + ends)
        segs = CU.segments(db, text, U.orc_ovlp_match)
        total = sum(n for _, n in segs)
        assert (total - delta) % TILE == 0 and (total - delta) // TILE >= 2 and segs[-1][0][1][4] == 0 and segs[-1][1] == lens[-1], (delta, total)
        out.append((delta, text, segs, total))
    return out


def test_totals_at_the_tile_size(engineered):
    """Outputs of exactly 4096 m, 4096 m + 1 and 4096 m - 1 bytes (the last tile full, one byte into the next, one byte short), and the
    smallest call there is.  A row's span cannot set the total: seg counts w's bases from the end of the longest exact run to w's end, so
    the step of ctg_len is the same for every span that keeps the run.  The total is set by the LENGTH of the last contig's first read
    instead -- a read against itself adds nothing -- and held to the statement before the GPU sees it."""
    case, db, ids, rdb = engineered
    for delta, text, segs, total in _paths_of_total(case, db):
        rows, names = CU.tile_rows(text)
        data, off = rdb.contigs(rows)
        assert len(data) == total and int(off[-1]) == total
        assert CU.fasta_of(data, off, names) == CU.paint(db, names, segs), (delta, total)
    # one contig of one 500-base read and one row
    c = next(c for c, (sg, _) in enumerate(case.segs) if len(sg) == 2 and sg[0][4] == CU.H)
    text = next(ln for ln in case.text.splitlines() if ln.startswith(case.names[c] + " ")) + "\n"
    rows, names = CU.tile_rows(text)
    data, off = rdb.contigs(rows)
    assert len(rows) == 1 and CU.fasta_of(data, off, names) == CU.layout(db, text, U.orc_ovlp_match)


def test_chunk_in_batches_equals_one_call(tmp_path):
    """the file level on the random path, whole and in batches of 1, 7 and 500 contigs: the same FASTA, the statement's, contigs in the order
    of their first line in the file (the file interleaves them)"""
    case = CU.case(True)
    prefix, tp = str(tmp_path / "reads"), str(tmp_path / "random.path")
    formats.write_seqdb(prefix, case.db)
    open(tp, "w").write(case.text)
    for batch in (None, 1, 7, 500):
        out = str(tmp_path / ("out.%s.fa" % batch))
        with _batch(batch):
            st = shimmer.path_to_contig(prefix, tp, out)
        assert open(out, "rb").read() == case.fasta, batch
        assert st == dict(contigs=len(case.names), bases=int(case.ctg_off[-1])), (batch, st)
    with _batch(None):
        r = subprocess.run([os.path.join(ROOT, "bin", "native", "path_to_contig.py"), prefix, tp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == case.fasta, (r.returncode, r.stderr[-500:])


SAYS = dict(source="e - seg < 0", start="would start before its contig's first base", end="ends beyond the end of its contig")


def test_device_side_errors_name_the_smallest_row(engineered, tmp_path):
    """BAD_SOURCE, BAD_START and BAD_END (for a contig's first read and for a later segment), each alone, twice more than 256 rows apart in
    both file orders, and mixed: the resident call names the smallest offending ROW in contig order whatever its kind, the file level that
    row's LINE (contigs interleaved: the two differ), and no output file appears.  Argument errors of the library on valid memory only."""
    case, db, ids, rdb = engineered
    prefix = str(tmp_path / "reads")
    formats.write_seqdb(prefix, db)
    lib = _lib.load()
    cases = CU.error_paths(db, ids, CU.filler_contigs(case), U.orc_ovlp_match)
    assert len(cases) == 15
    failed = []
    for name, text, (row, kind), line in cases:
        rows, _ = CU.tile_rows(text)
        try:
            rdb.contigs(rows)
            msg = "no error"
        except _lib.PgxError as e:
            msg = str(e)
        if not ("code %d" % _lib.PGX_EARG in msg and "row %d:" % row in msg and SAYS[kind] in msg):
            failed.append((name, "resident", "want row %d (%s)" % (row, kind), msg))
        tp, out = str(tmp_path / "bad.path"), str(tmp_path / "bad.fa")
        open(tp, "w").write(text)
        rc = lib.pgx_contigs_chunk(prefix.encode(), tp.encode(), out.encode(), None, None)
        msg = lib.pgx_last_error().decode()
        if not (rc == _lib.PGX_EARG and "row %d:" % line in msg and SAYS[kind] in msg and not os.path.exists(out)):
            failed.append((name, "chunk", "want line %d (%s)" % (line, kind), rc, msg, os.path.exists(out)))
    assert not failed, "\n".join(str(f) for f in failed)
    # the database is as usable as before
    text = CU.assemble(CU.filler_contigs(case, 60))
    rows, names = CU.tile_rows(text)
    data, off = rdb.contigs(rows)
    assert CU.fasta_of(data, off, names) == CU.layout(db, text, U.orc_ovlp_match)
