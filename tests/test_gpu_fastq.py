"""The read-database builder on the GPU (pgx_reads.hip: ResidentDB.from_reads, pgx_seqdb_builder_*, pgx_seqdb_from_files, pg_asm
--reads-on-gpu): the golden cases against the reference binary's files, random texts against the plain restatement of the grammar
(tests/fastq_util.py) with refusals compared as refusals, the shapes at which the passes' tiles and wavefronts end, texts fed in pieces
at every cut, a chain of 5,000 records, the device-pointer form, several files, a list of a plain and a .gz file against pgx_mkseqdb,
the refusals, the memory ledger, and a whole job (the read set of tests/test_gpu_assemble.py) against assemble(prefix)."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import fastq_util as Q
from peregrine_amd import _lib, formats, shimmer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096   # a block's tile of text / pool bytes in every pass (pgx_fasta_k.h)
REFUSED = b"@r1\nACGTA\n+\nII\r\r\r\n\nI\n@r2\nA\n+\nI\n"   # (tests/test_fastq_rule.py: the one class that is not evaluated)


def golden_cases():
    z = np.load(os.path.join(ROOT, "tests", "golden", "fastq_cases.npz"))
    return [(str(k), [z["text_%s_%d" % (k, i)].tobytes() for i in range(int(z["files_" + str(k)]))], z["seqdb_" + str(k)].tobytes(),
             z["idx_" + str(k)].tobytes()) for k in z["order"]]


CASES = golden_cases()


def files_of_db(rdb, tmp_path, tag="db"):
    pre = str(tmp_path / tag)
    rdb.save(pre)
    with open(pre + ".seqdb", "rb") as f, open(pre + ".idx", "rb") as g:
        return f.read(), g.read()


class Builder:
    """the C entry points, a piece at a time"""

    def __init__(self, reserve=0):
        _lib.init(0)
        self.lib, self.b = _lib.load(), C.c_void_p()
        _lib.check(self.lib.pgx_seqdb_builder_open(reserve, C.byref(self.b)), "pgx_seqdb_builder_open")

    def feed(self, piece: bytes, ends_file: bool):
        _lib.check(self.lib.pgx_seqdb_builder_feed(self.b, piece, len(piece), 0, int(ends_file)), "pgx_seqdb_builder_feed")

    def feed_in(self, text: bytes, size: int):
        cuts = list(range(0, len(text), size)) or [0]
        for i, at in enumerate(cuts):
            self.feed(text[at:at + size], i == len(cuts) - 1)

    def finish(self):
        """(names, .seqdb bytes, read lengths) of the database, which is freed"""
        h, names, nl, nr, nb = C.c_void_p(), C.c_void_p(), C.c_size_t(0), C.c_uint64(0), C.c_uint64(0)
        _lib.check(self.lib.pgx_seqdb_builder_finish(self.b, C.byref(h), C.byref(names), C.byref(nl), C.byref(nr), C.byref(nb)), "pgx_seqdb_builder_finish")
        try:
            nm = C.string_at(names.value, nl.value).split(b"\n")[:-1]
            self.lib.pgx_free(names)
            rlen = np.zeros(int(nr.value), np.uint32)
            _lib.check(self.lib.pgx_seqdb_read_lengths(h, rlen.ctypes.data_as(C.c_void_p), len(rlen)), "pgx_seqdb_read_lengths")
            assert int(rlen.sum()) == int(nb.value) and len(nm) == len(rlen)
            seqs = []
            for r, n in enumerate(rlen):
                out = np.zeros(int(n), np.uint8)
                if n:
                    _lib.check(self.lib.pgx_seqdb_read_bytes(h, r, out.ctypes.data_as(C.c_void_p), int(n)), "pgx_seqdb_read_bytes")
                seqs.append(out.tobytes())
            return nm, seqs
        finally:
            self.lib.pgx_seqdb_free(h)

    def close(self):
        self.lib.pgx_seqdb_builder_close(self.b)
        self.b = C.c_void_p()


def encoded(names, seqs):
    return list(names), [Q.biseq(s).tobytes() for s in seqs]


def check_against_restatement(texts, tmp_path, tag="db"):
    """from_reads(texts) against the restatement: names, counts, lengths and the two files; answers the restatement's (names, seqs)"""
    names, seqs = Q.reads_of_files(texts, Q.parse_reads)
    if not names:
        with pytest.raises(_lib.PgxError, match=r"code -6.*no record"):
            shimmer.ResidentDB.from_reads(texts, 0)
        return names, seqs
    rdb = shimmer.ResidentDB.from_reads(texts, 0)
    try:
        assert rdb.names == [n.decode("latin-1") for n in names]
        assert (rdb.n_reads, rdb.n_bases) == (len(names), sum(map(len, seqs)))
        assert rdb.rlen_by_rid.tolist() == [len(s) for s in seqs]
        got = files_of_db(rdb, tmp_path, tag)
        want = Q.files_of(names, seqs)
        assert got[1] == want[1]
        assert got[0] == want[0], "first differing byte %d" % next(i for i, (a, b) in enumerate(zip(got[0], want[0])) if a != b)
    finally:
        rdb.close()
    return names, seqs


@pytest.mark.parametrize("name,texts,seqdb,idx", CASES, ids=[c[0] for c in CASES])
def test_golden_cases_equal_the_reference_files(name, texts, seqdb, idx, tmp_path):
    if not idx:
        with pytest.raises(_lib.PgxError, match=r"code -6.*no record"):
            shimmer.ResidentDB.from_reads(texts, 0)
        return
    rdb = shimmer.ResidentDB.from_reads(texts, 0)
    try:
        got_db, got_idx = files_of_db(rdb, tmp_path)
        assert got_idx == idx and got_db == seqdb
        lines = idx.decode("latin-1").split("\n")[:-1]
        assert rdb.names == [ln.split(" ")[1] for ln in lines]
        assert rdb.n_reads == len(lines) and rdb.n_bases == len(seqdb)
    finally:
        rdb.close()


@pytest.mark.parametrize("name,texts,seqdb,idx", [c for c in CASES if c[3] and max(map(len, c[1])) < 1000], ids=[c[0] for c in CASES if c[3] and max(map(len, c[1])) < 1000])
def test_golden_cases_in_pieces_of_five_bytes(name, texts, seqdb, idx):
    b = Builder()
    try:
        for t in texts:
            b.feed_in(t, 5)
        names, seqs = b.finish()
        assert b"".join(seqs) == seqdb
        assert names == [ln.split(b" ")[1] for ln in idx.split(b"\n")[:-1]]
    finally:
        b.close()


def test_random_texts_equal_the_restatement(tmp_path):
    done = refused = 0
    for t in Q.random_texts() + [REFUSED]:
        a = Q.answer(Q.parse_reads, t)
        if isinstance(a[0], str):
            with pytest.raises(_lib.PgxError, match=r"code -6.*empty quality line at byte offset %d " % a[1]):
                shimmer.ResidentDB.from_reads([t], 0)
            refused += 1
            continue
        done += len(check_against_restatement([t], tmp_path)[0]) > 0
    assert done > 200 and refused >= 1


def _acgt(n, seed):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def _fq(name, seq, qual=None):
    return b"@" + name + b"\n" + seq + b"\n+\n" + (b"I" * len(seq) if qual is None else qual) + b"\n"


def _exact(n, seed):
    """one four-line record of exactly n >= 8 bytes"""
    name = b"r" * (1 + (n - 7) % 2)
    return _fq(name, _acgt((n - 6 - len(name)) // 2, seed))


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1])
def test_text_lengths_around_wavefronts_and_tiles(n, tmp_path):
    if n < 8:
        for t in (b"@r\n"[:n], b"\n@"[:n], b"+\n"[:n]):
            check_against_restatement([t], tmp_path)
        return
    t = _exact(n, n)
    assert len(t) == n and len(check_against_restatement([t], tmp_path)[0]) == 1
    assert len(check_against_restatement([_exact(n + 1, n)[:-1]], tmp_path)[0]) == 1          # the quality's last line without its '\n'
    assert len(check_against_restatement([_exact(n - 4, n) + b"@s\nA"], tmp_path)[0]) == 2    # the last record ends with the text
    assert len(check_against_restatement([_exact(n - 1, n) + b"@"], tmp_path)[0]) == 1         # a marker as the last byte starts none
    check_against_restatement([_exact(n + 2, n)[:-3]], tmp_path)                               # a truncated quality: no record


BORDERS = sorted({b + d for b in (64, 128, 192, 256, 320, TILE, 2 * TILE) for d in (-1, 0, 1)})


@pytest.mark.parametrize("what", ["plus", "at", "newline"])
def test_marks_on_every_border(what, tmp_path):
    """the '+' line, an '@' header behind a quality block and a '\\n' inside the sequence and the quality on, before and after the wavefront
    borders of a tile's first rounds and the tile borders"""
    for at in BORDERS:
        if what == "plus":      # "@r\n" + (at - 4) bases + "\n": the '+' is byte `at`
            t = _fq(b"r", _acgt(at - 4, at)) + _fq(b"s", b"ACG")
            assert t[at] == 0x2B and t[at - 1] == 0x0A
        elif what == "at":      # the second record's '@' is byte `at`
            k = (at - 7) // 2
            t = _fq(b"r", _acgt(k, at)) + b"x" * (at - 7 - 2 * k) + _fq(b"s", _acgt(5, 1))
            assert t[at] == 0x40
        else:                   # multi-line sequence and quality, line breaks at `at` and at `at` behind the '+'
            s = _acgt(2 * TILE + 300, at)
            t = b"@r\n" + s[:at - 3] + b"\n" + s[at - 3:] + b"\n+\n" + b"5" * (at - 1) + b"\n" + b"@" * (len(s) - at + 1) + b"\n" + _fq(b"s", b"AC")
            assert t[at] == 0x0A
        names, seqs = check_against_restatement([t], tmp_path)
        assert len(names) == 2
    for at in (64, 256, TILE, 2 * TILE):   # ... and the pool's borders: records whose first base is pool byte `at`
        for d in (-1, 0, 1):
            check_against_restatement([_fq(b"a", _acgt(at + d, at)) + _fq(b"b", _acgt(TILE + 77, d + 7))], tmp_path)


SMALL = (b"junk\n@r1 c\nACGTAC\nGT\n+r1\nIIII\n@III\n>f1\nACG\nT\n@r2\r\nAC\r\n+\r\n@I\r\nxx@r3\n\r\n+\n\n\r\n@r4\nACGTACGTAC\n+\n+IIIIIIII\n@\n"
         b">f2 x\nAC\n\nGT\n@r5\n\n+\n\n@r6\nTTTT\n+\nIIII\n@r7 two lines\nACGTAC\nGTACGT\n+\n>IIIII\n+IIIII\n\n>f3\n\r\nA\r\n@r8\nA\n+\nI")


def test_two_pieces_at_every_cut_position():
    want = encoded(*Q.parse_reads(SMALL))
    assert want == encoded(*Q.kseq_loop_q(SMALL)) and len(want[0]) == 11 and 180 <= len(SMALL) <= 220
    b = Builder()
    try:
        for cut in range(len(SMALL) + 1):
            b.feed(SMALL[:cut], False)
            b.feed(SMALL[cut:], True)
            assert b.finish() == want, cut
    finally:
        b.close()


@pytest.mark.parametrize("size", [1, 7, 64])
def test_small_pieces(size):
    texts = [SMALL, b"@t\nAC\n+\nI\n@dropped\nA\n+\nI\n", SMALL[5:]]   # (the second file stops early)
    want = encoded(*Q.reads_of_files(texts, Q.parse_reads))
    assert len(want[0]) == 22
    b = Builder()
    try:
        for t in texts:
            b.feed_in(t, size)
        assert b.finish() == want
    finally:
        b.close()


def test_a_record_longer_than_three_pieces():
    seq = _acgt(3 * TILE + 500, 3)
    text = _fq(b"a", b"ACGT") + b"@long x\n" + seq[:TILE] + b"\n" + seq[TILE:] + b"\n+\n" + b"@" * len(seq) + b"\n" + _fq(b"b", b"GG")
    b = Builder(reserve=16)   # (the store grows)
    try:
        b.feed_in(text, 1000)
        assert b.finish() == encoded([b"a", b"long", b"b"], [b"ACGT", seq, b"GG"])
    finally:
        b.close()


def test_five_thousand_records_of_one_base(tmp_path):
    """a chain of 5,000 under the successor function (20,000 lines: 16 doubling rounds), every quality line a marker line"""
    bases = _acgt(5000, 3)
    names, seqs = check_against_restatement([b"".join(b"@%d\n%c\n+\n@\n" % (i, bases[i]) for i in range(5000))], tmp_path)
    assert len(names) == 5000 and all(len(s) == 1 for s in seqs)


def test_the_device_pointer_form(tmp_path):
    import torch
    texts = [b"junk\n" + b"".join(_fq(b"r%d c" % i, _acgt(61 + i, i)) for i in range(150)), b">f\n" + _acgt(TILE + 3, 9)]
    host = shimmer.ResidentDB.from_reads(texts, 0)
    tens = []
    for text in texts:
        t = torch.zeros(len(text) + 5, dtype=torch.uint8, device="cuda:0")
        t[5:].copy_(torch.frombuffer(bytearray(text), dtype=torch.uint8), non_blocking=True)   # (filled on torch's stream right before the call, unaligned)
        tens.append(t[5:])
    dev = shimmer.ResidentDB.from_reads(tens, 0)
    try:
        assert dev.names == host.names and len(dev.names) == 151 and (dev.n_reads, dev.n_bases) == (host.n_reads, host.n_bases)
        assert files_of_db(dev, tmp_path, "dev") == files_of_db(host, tmp_path, "host") == Q.files_of(*Q.reads_of_files(texts, Q.parse_reads))
    finally:
        host.close(), dev.close()


def test_several_files_rid_runs_on_and_a_stopped_file_does_not_stop_the_next(tmp_path):
    texts = [_fq(b"a1", b"ACGT") + b"@a2\nACGT\n+\nII\n" + _fq(b"a3", b"AC"), b"nothing here\n", _fq(b"c1", b"GGG") + b">c2\nTT\n", b"", b"@d1\nA\n+\nI"]
    names, seqs = check_against_restatement(texts, tmp_path)
    assert names == [b"a1", b"c1", b"c2", b"d1"]
    rdb = shimmer.ResidentDB.from_reads(texts, 0)
    try:
        assert files_of_db(rdb, tmp_path)[1] == b"000000000 a1 4 0\n000000001 c1 3 4\n000000002 c2 2 7\n000000003 d1 1 9\n"
    finally:
        rdb.close()


def test_from_files_plain_and_gz_equals_mkseqdb(tmp_path, monkeypatch):
    """a list of a plain FASTQ and a .gz FASTA file in pieces of 4,096 bytes against pgx_mkseqdb + a load of its files: the two files of
    .save(), one index chunk and one overlap chunk"""
    from peregrine_amd import simreads
    g = simreads.make_genome(60_000, 31)
    db = simreads.simulate_reads(g, coverage=6.0, seed=8, mean_len=5000, sd_len=800)
    lut = np.full(16, ord("N"), np.uint8)
    lut[[1, 2, 4, 8]] = [ord(c) for c in "ACGT"]
    recs = [(b"read%05d" % r, lut[db.seqdb[int(o):int(o) + int(n)] & 0x0F].tobytes()) for r, n, o in zip(db.rid, db.rlen, db.roff)]
    half = len(recs) // 2
    fq, fa = tmp_path / "a.fastq", tmp_path / "b.fa.gz"
    fq.write_bytes(b"".join(b"@" + nm + b" x\n" + s + b"\n+\n" + b"@" * len(s) + b"\n" for nm, s in recs[:half]))
    with gzip.open(str(fa), "wb") as f:
        f.write(b"".join(b">" + nm + b"\n" + b"\n".join(s[i:i + 70] for i in range(0, len(s), 70)) + b"\n" for nm, s in recs[half:]))
    lst = tmp_path / "reads.lst"
    lst.write_text("%s\n%s\n" % (fq, fa))
    shimmer.shmr_mkseqdb(str(lst), str(tmp_path / "mk"))
    monkeypatch.setenv("PGX_FROM_READS_PIECE", "4096")
    a = shimmer.ResidentDB.from_reads(str(lst), 0)
    loaded = formats.read_seqdb(str(tmp_path / "mk"))
    b = shimmer.ResidentDB(loaded, 0)
    try:
        assert files_of_db(a, tmp_path, "gpu") == (open(str(tmp_path / "mk.seqdb"), "rb").read(), open(str(tmp_path / "mk.idx"), "rb").read())
        assert a.names == list(loaded.names) == [nm.decode() for nm, _ in recs] and (a.n_reads, a.n_bases) == (b.n_reads, b.n_bases)
        assert np.array_equal(a.rlen_by_rid, b.rlen_by_rid)
        x, y = a.index(2, 1), b.index(2, 1)
        assert len(x.top) > 100 and np.array_equal(x.top, y.top)
        assert np.array_equal(formats.mc_as_sorted_pairs(x.top_mc), formats.mc_as_sorted_pairs(y.top_mc))
        ix = a.index()
        ov_a, ov_b = a.overlap(ix.top, ix.top_mc, 2, 1)[0], b.overlap(ix.top, ix.top_mc, 2, 1)[0]
        assert len(ov_a) > 20 and formats.ovlp_fields_equal(ov_a, ov_b)
    finally:
        a.close(), b.close()


def test_refusals_name_what_they_refuse_and_the_library_goes_on(tmp_path):
    with pytest.raises(_lib.PgxError, match=r"code -6.*empty quality line at byte offset %d of the file" % (REFUSED.index(b"\n\n") + 1)):
        shimmer.ResidentDB.from_reads([REFUSED], 0)
    b = Builder()
    try:
        b.feed(_fq(b"ok", b"ACGT") * 40, False)   # (committed, and the offset counts from the start of the file)
        with pytest.raises(_lib.PgxError, match=r"code -6.*byte offset %d of the file" % (40 * 16 + REFUSED.index(b"\n\n") + 1)):
            b.feed(REFUSED, True)
    finally:
        b.close()
    for texts in ([], [b""], [b"no header\nat all\n", b"junk\n@"], [b"@r\n+\nI\n"]):
        with pytest.raises(_lib.PgxError, match=r"code -6.*no record"):
            shimmer.ResidentDB.from_reads(texts, 0)
    (tmp_path / "bad.lst").write_text(str(tmp_path / "no_such_file.fq") + "\n")
    with pytest.raises(_lib.PgxError, match=r"no_such_file.fq"):
        shimmer.ResidentDB.from_reads(str(tmp_path / "bad.lst"), 0)
    with pytest.raises(_lib.PgxError, match=r"no_such.lst"):
        shimmer.ResidentDB.from_reads(str(tmp_path / "no_such.lst"), 0)
    check_against_restatement([_fq(b"r1", b"ACGT")], tmp_path)


def test_the_ledger_shows_the_work_and_returns_to_its_level():
    import gc
    gc.collect()
    shimmer.ResidentDB.from_reads([b"@w\nACGT\n+\nIIII\n"], 0).close()   # (the library is up)
    before = _lib.mem_ledger(reset_peak=True)["live_bytes"]
    text = b"".join(_fq(b"r%d" % i, _acgt(80, i)) for i in range(4000))
    b = Builder()
    try:
        b.feed(text[:len(text) // 2 + 7], False)
        assert _lib.mem_ledger()["live_bytes"] > before   # the store and the carry
        b.feed(text[len(text) // 2 + 7:], True)
        led = _lib.mem_ledger()
        assert led["peak_by_tag"].get("reads", 0) >= len(text) // 2 + 4000 * 40   # a text copy and its pool, at the least
        assert led["peak_by_tag"].get("seqdb.bytes", 0) >= 4000 * 80 + 1024
        names, seqs = b.finish()   # (the database is freed in there)
        assert len(names) == 4000 and all(len(s) == 80 for s in seqs)
    finally:
        b.close()
    assert _lib.mem_ledger()["live_bytes"] == before
    # pgx_shutdown with a builder open: its device state goes, its calls are refused, close still works
    b = Builder()
    b.feed(text[:1000], False)
    lib = _lib.load()
    lib.pgx_shutdown()
    try:
        _lib._inited = None
        _lib.init(0)
        with pytest.raises(_lib.PgxError, match=r"code -5.*pgx_shutdown ran"):
            b.feed(text[1000:2000], False)
    finally:
        b.close()
    shimmer.ResidentDB.from_reads([b"@w\nACGT\n+\nIIII\n"], 0).close()
    assert _lib.mem_ledger()["live_bytes"] <= before


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """the read set of tests/test_gpu_assemble.py and what assemble(prefix) gives for its files"""
    import test_gpu_assemble as A
    d, db = tmp_path_factory.mktemp("asm_reads"), A.read_set()
    formats.write_seqdb(str(d / "seq_dataset"), db)
    want = shimmer.assemble(str(d / "seq_dataset"), A.N_INDEX, A.N_OVLP, A.N_MAP, A.N_CNS, with_alt=True, mc_lower=A.MC_LOWER, mc_upper=A.MC_UPPER)
    assert len(want["p_ctg"]) > 50_000 and want["a_ctg"] and len(want["p_ctg_cns"]) > 50_000
    return dict(db=db, want=want)


def _reads_as_fastq(job, path, gz=False):
    lut = np.full(16, ord("N"), np.uint8)
    lut[[1, 2, 4, 8]] = [ord(c) for c in "ACGT"]
    db = job["db"]
    data = b"".join(b"@read%06d\n" % r + lut[db.seqdb[int(o):int(o) + int(n)] & 0x0F].tobytes() + b"\n+\n" + b"@" * int(n) + b"\n"
                    for r, n, o in zip(db.rid, db.rlen, db.roff))
    half = data.index(b"\n@read%06d\n" % (len(db.rid) // 2)) + 1
    open(path + ".1.fastq", "wb").write(data[:half])
    open(path + ".2.fastq", "wb").write(data[half:])
    open(path + ".lst", "w").write("%s.1.fastq\n%s.2.fastq\n" % (path, path))
    return path + ".lst"


def test_assemble_of_a_from_reads_database_equals_assemble_of_the_files(job, tmp_path):
    import test_gpu_assemble as A
    rdb = shimmer.ResidentDB.from_reads(_reads_as_fastq(job, str(tmp_path / "reads")), 0)
    try:
        got = shimmer.assemble(rdb, A.N_INDEX, A.N_OVLP, A.N_MAP, A.N_CNS, with_alt=True, mc_lower=A.MC_LOWER, mc_upper=A.MC_UPPER)
        for k in ("p_ctg", "a_ctg", "p_ctg_cns"):
            assert got[k] == job["want"][k], k
        assert rdb.h and rdb.n_reads == len(job["db"].rid)   # (left open)
    finally:
        rdb.close()


def test_pg_asm_reads_on_gpu_writes_the_same_three_files(job, tmp_path):
    import test_gpu_assemble as A
    lst = _reads_as_fastq(job, str(tmp_path / "reads"))
    exe = [sys.executable, os.path.join(ROOT, "bin", "pg_asm")]
    r = subprocess.run([*exe, lst, str(A.N_INDEX), str(A.N_OVLP), str(A.N_MAP), str(A.N_CNS), "--with-alt", "--reads-on-gpu", "--output", str(tmp_path / "wd")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr
    for k in ("p_ctg", "a_ctg", "p_ctg_cns"):
        assert (tmp_path / "wd" / (k + ".fa")).read_bytes() == job["want"][k], k
    assert not (tmp_path / "wd" / "0-seqdb").exists()
