"""pgx_seqdb_from_fasta / pgx_seqdb_save on the GPU (ResidentDB.from_fasta, .save): the golden cases against the reference binary's files,
random texts against the plain restatement of the grammar (tests/fasta_util.py), the shapes at which the four passes' tiles and
wavefronts end, the device-pointer form, equivalence with a database loaded from files, the refusals and the memory ledger."""
import os

import numpy as np
import pytest

import fasta_util as F
from peregrine_amd import _lib, formats, shimmer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096   # a block's tile of text / pool bytes in every pass (pgx_fasta.hip)


def golden_cases():
    z = np.load(os.path.join(ROOT, "tests", "golden", "fasta_cases.npz"))
    return [(str(k), z["text_" + str(k)].tobytes(), z["seqdb_" + str(k)].tobytes(), z["idx_" + str(k)].tobytes()) for k in z["order"]]


CASES = golden_cases()


def files_of_db(rdb, tmp_path, tag="db"):
    pre = str(tmp_path / tag)
    rdb.save(pre)
    with open(pre + ".seqdb", "rb") as f, open(pre + ".idx", "rb") as g:
        return f.read(), g.read()


def check_against_restatement(text, tmp_path, tag="db"):
    """from_fasta(text) against the restatement: names, counts and the two files; answers the restatement's (names, seqs)"""
    names, seqs = F.parse_fasta(text)
    rdb = shimmer.ResidentDB.from_fasta(text, 0)
    try:
        assert rdb.names == [n.decode("latin-1") for n in names]
        assert (rdb.n_reads, rdb.n_bases) == (len(names), sum(map(len, seqs)))
        got = files_of_db(rdb, tmp_path, tag)
        want = F.files_of(names, seqs)
        assert got[1] == want[1]
        assert got[0] == want[0], "first differing byte %d" % next(i for i, (a, b) in enumerate(zip(got[0], want[0])) if a != b)
    finally:
        rdb.close()
    return names, seqs


@pytest.mark.parametrize("name,text,seqdb,idx", CASES, ids=[c[0] for c in CASES])
def test_golden_cases_equal_the_reference_files(name, text, seqdb, idx, tmp_path):
    rdb = shimmer.ResidentDB.from_fasta(text, 0)
    try:
        got_db, got_idx = files_of_db(rdb, tmp_path)
        assert got_idx == idx and got_db == seqdb
        lines = idx.decode("latin-1").split("\n")[:-1]
        assert rdb.names == [ln.split(" ")[1] for ln in lines]
        assert rdb.n_reads == len(lines) and rdb.n_bases == len(seqdb)
    finally:
        rdb.close()


def test_random_texts_equal_the_restatement(tmp_path):
    done = 0
    for k, t in enumerate(F.random_texts()):
        try:
            F.parse_fasta(t)
        except F.Refused as r:
            assert r.kind == "no record"
            with pytest.raises(_lib.PgxError, match=r"code -6.*no record"):
                shimmer.ResidentDB.from_fasta(t, 0)
            continue
        check_against_restatement(t, tmp_path)
        done += 1
    assert done > 250


def _acgt(n, seed):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


@pytest.mark.parametrize("n", [2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1])
def test_text_lengths_around_wavefronts_and_tiles(n, tmp_path):
    check_against_restatement((b">r\n" + _acgt(n, n))[:n] if n > 3 else b">r"[:n], tmp_path)
    check_against_restatement((b">a b\n" + _acgt(n, n + 1))[:n - 1] + b"\n" if n > 6 else b">\n", tmp_path)


def test_a_text_of_one_byte():
    for t in (b">", b"A", b"\n"):
        with pytest.raises(_lib.PgxError, match=r"code -6.*no record"):
            shimmer.ResidentDB.from_fasta(t, 0)


BORDERS = sorted({b + d for b in (64, 128, 192, 256, 320, TILE, 2 * TILE) for d in (-1, 0, 1)})


@pytest.mark.parametrize("what", ["newline", "header", "crlf"])
def test_marks_on_every_border(what, tmp_path):
    """a '\\n', a header marker and a "\\r\\n" pair on, before and after the wavefront borders of a tile's first rounds and the tile borders:
    in the text (marks, gather) and, as the text is all sequence behind a 3-byte header, nearly the same borders of the pool (encode)"""
    base = bytearray(b">r\n" + _acgt(2 * TILE + 200, 5))
    for at in BORDERS:
        t = bytearray(base)
        if what == "newline":
            t[at:at + 1] = b"\n"
        elif what == "header":
            t[at - 1:at + 3] = b"\n>x\n"
        else:
            t[at - 1:at + 1] = b"\r\n"
        check_against_restatement(bytes(t), tmp_path)
    # ... and the pool's borders exactly: records whose first base is pool byte `at`
    for at in (64, 256, TILE, 2 * TILE):
        for d in (-1, 0, 1):
            check_against_restatement(b">a\n" + _acgt(at + d, at) + b"\n>b\n" + _acgt(TILE + 77, d + 7) + b"\n", tmp_path)


def test_an_empty_record_between_two_long_ones(tmp_path):
    names, seqs = check_against_restatement(b">a\n" + _acgt(3 * TILE + 5, 1) + b"\n>empty\n>b\n" + _acgt(2 * TILE + 9, 2) + b"\n>last\n", tmp_path)
    assert [len(s) for s in seqs] == [3 * TILE + 5, 0, 2 * TILE + 9, 0]


def test_five_thousand_records_of_one_base(tmp_path):
    bases = _acgt(5000, 3)
    names, seqs = check_against_restatement(b"".join(b">%d\n%c\n" % (i, bases[i]) for i in range(5000)), tmp_path)
    assert len(names) == 5000 and all(len(s) == 1 for s in seqs)


def test_one_long_line_and_the_same_bases_in_short_lines(tmp_path):
    """3 MiB in one record: the gather and the mirrored encode cross some 770 tiles; the same bases in 60-byte lines are the same database"""
    n = 3 << 20
    seq = _acgt(n, 11)
    want = F.biseq(seq).tobytes()
    dbs = []
    for tag, text in (("one", b">ctg\n" + seq + b"\n"), ("wrapped", b">ctg\n" + b"\n".join(seq[i:i + 60] for i in range(0, n, 60)))):
        rdb = shimmer.ResidentDB.from_fasta(text, 0)
        try:
            assert (rdb.names, rdb.n_reads, rdb.n_bases) == (["ctg"], 1, n)
            dbs.append(files_of_db(rdb, tmp_path, tag))
        finally:
            rdb.close()
    assert dbs[0] == dbs[1] and dbs[0][0] == want and dbs[0][1] == b"000000000 ctg %d 0\n" % n


def test_a_partial_last_tile(tmp_path):
    check_against_restatement(b">a\n" + b"\n".join(_acgt(70, i) for i in range(100)) + b"\n>b x\n" + _acgt(TILE + 1234, 4), tmp_path)


def test_the_device_pointer_form(tmp_path):
    import torch
    text = b"junk\n>a c\n" + b"\r\n".join(_acgt(61, i) for i in range(150)) + b"\n>b\n\n>c\n" + _acgt(TILE + 3, 9)
    host = shimmer.ResidentDB.from_fasta(text, 0)
    t = torch.zeros(len(text) + 5, dtype=torch.uint8, device="cuda:0")
    t[5:].copy_(torch.frombuffer(bytearray(text), dtype=torch.uint8), non_blocking=True)   # (filled on torch's stream right before the call, unaligned)
    dev = shimmer.ResidentDB.from_fasta(t[5:], 0)
    try:
        assert dev.names == host.names == ["a", "b", "c"] and (dev.n_reads, dev.n_bases) == (host.n_reads, host.n_bases)
        assert files_of_db(dev, tmp_path, "dev") == files_of_db(host, tmp_path, "host") == F.files_of(*F.parse_fasta(text))
    finally:
        host.close(), dev.close()


def test_equivalence_with_the_loaded_database(tmp_path):
    """a from_fasta database and a ResidentDB of the files shmr_mkseqdb wrote from the same text: equal index arrays, equal bytes per read,
    and both give their bytes up"""
    from peregrine_amd import simreads
    g = simreads.make_genome(60_000, 31)
    db = simreads.simulate_reads(g, coverage=6.0, seed=8, mean_len=5000, sd_len=800)
    lut = np.full(16, ord("N"), np.uint8)
    lut[[1, 2, 4, 8]] = [ord(c) for c in "ACGT"]
    text = b"".join(b">read%05d x\n" % r + lut[db.seqdb[int(o):int(o) + int(n)] & 0x0F].tobytes() + b"\n" for r, n, o in zip(db.rid, db.rlen, db.roff))
    fa = tmp_path / "reads.fa"
    fa.write_bytes(text)
    (tmp_path / "reads.lst").write_text(str(fa) + "\n")
    shimmer.shmr_mkseqdb(str(tmp_path / "reads.lst"), str(tmp_path / "mk"))
    a = shimmer.ResidentDB.from_fasta(text, 0)
    loaded = formats.read_seqdb(str(tmp_path / "mk"))
    b = shimmer.ResidentDB(loaded, 0)
    try:
        assert files_of_db(a, tmp_path, "fa") == (open(str(tmp_path / "mk.seqdb"), "rb").read(), open(str(tmp_path / "mk.idx"), "rb").read())
        assert a.names == list(loaded.names) and a.n_reads == b.n_reads and a.n_bases == b.n_bases
        for tc, c in ((1, 1), (2, 2)):
            x, y = a.index(tc, c), b.index(tc, c)
            assert len(x.top) > 100 and np.array_equal(x.top, y.top)
            assert np.array_equal(formats.mc_as_sorted_pairs(x.top_mc), formats.mc_as_sorted_pairs(y.top_mc))
            assert (x.bases, x.reads) == (y.bases, y.reads)
        for r, n in zip(loaded.rid, loaded.rlen):
            assert np.array_equal(a.read_bytes(int(r), int(n)), b.read_bytes(int(r), int(n))), int(r)
        ix = a.index()
        ov_a, ov_b = a.overlap(ix.top, ix.top_mc)[0], b.overlap(ix.top, ix.top_mc)[0]
        assert len(ov_a) > 20 and formats.ovlp_fields_equal(ov_a, ov_b)
        assert a.release_bytes() and b.release_bytes() and not a.has_bytes and not b.has_bytes
        with pytest.raises(_lib.PgxError, match=r"code -5.*released"):
            a.save(str(tmp_path / "gone"))
        assert not os.path.exists(str(tmp_path / "gone.seqdb"))
        assert np.array_equal(a.index().top, ix.top)   # (from the packs)
    finally:
        a.close(), b.close()


def test_contig_layout_and_compaction_on_a_from_fasta_database():
    """the read set of tests/test_gpu_contigs.py (one read with ambiguous bases) as FASTA text: pgx_contigs_resident on the database gives the
    golden contigs with the bytes in place and compacted, and read_bytes answers the same bytes in both states"""
    import contig_util as CU
    g = np.load(os.path.join(ROOT, "tests", "golden", "contig_cases.npz"))
    d = CU.make_db()
    lut = np.full(16, ord("N"), np.uint8)
    lut[[1, 2, 4, 8]] = [ord(c) for c in "ACGT"]
    text = b"".join(b">r%d\n" % r + lut[d.seqdb[int(o):int(o) + int(n)] & 0x0F].tobytes() + b"\n" for r, n, o in zip(d.rid, d.rlen, d.roff))
    rdb = shimmer.ResidentDB.from_fasta(text, 0)
    try:
        rows, names = CU.tile_rows(str(g["path_bio"]))
        want = g["fasta_bio"].tobytes()
        before = [rdb.read_bytes(int(r), int(n)) for r, n in zip(d.rid, d.rlen)]
        assert all(np.array_equal(b, d.seqdb[int(o):int(o) + int(n)]) for b, n, o in zip(before, d.rlen, d.roff))
        assert CU.fasta_of(*rdb.contigs(rows), names) == want
        assert not rdb.release_bytes() and rdb.compact_bytes() and not rdb.has_bytes and rdb.side_bytes > 0
        assert CU.fasta_of(*rdb.contigs(rows), names) == want
        assert all(np.array_equal(rdb.read_bytes(int(r), int(n)), b) for r, n, b in zip(d.rid, d.rlen, before))
    finally:
        rdb.close()


def test_refusals_name_what_they_refuse_and_the_library_goes_on(tmp_path):
    text = b">r1\nACGT\n+\nIIII\n@r2\nAC\n+\nII\n"
    with pytest.raises(_lib.PgxError, match=r"code -6.*'\+' at byte offset 9:"):
        shimmer.ResidentDB.from_fasta(text, 0)
    far = b">r1\n" + _acgt(3 * TILE, 1) + b"\n+\n" + _acgt(2 * TILE, 2) + b"\n+x\n"
    with pytest.raises(_lib.PgxError, match=r"code -6.*'\+' at byte offset %d:" % (4 + 3 * TILE + 1)):
        shimmer.ResidentDB.from_fasta(far, 0)
    for t in (b"", b"no header\nat all\n", b"junk\n>"):
        with pytest.raises(_lib.PgxError, match=r"code -6.*no record"):
            shimmer.ResidentDB.from_fasta(t, 0)
    check_against_restatement(b"+\n+junk\n>r1 +\nAC+\n", tmp_path)   # a '+' before the first header's line, or in mid-line, is none
    check_against_restatement(b">r1\nACGT\n", tmp_path)


def test_the_ledger_shows_the_work_and_returns_to_its_level():
    import gc
    gc.collect()
    shimmer.ResidentDB.from_fasta(b">w\nACGT\n", 0).close()   # (the library is up)
    before = _lib.mem_ledger(reset_peak=True)["live_bytes"]
    text = b">a\n" + b"\n".join(_acgt(80, i) for i in range(4000)) + b"\n"
    rdb = shimmer.ResidentDB.from_fasta(text, 0)
    led = _lib.mem_ledger()
    assert led["peak_by_tag"].get("fasta", 0) >= len(text) + rdb.n_bases   # the text copy and the pool, at the least
    assert led["peak_by_tag"].get("seqdb.bytes", 0) >= rdb.n_bases + 1024
    assert led["live_bytes"] - before < led["peak_live_bytes"] - before   # the text copy, the tables and the pool are gone again
    rdb.close()
    assert _lib.mem_ledger()["live_bytes"] == before
