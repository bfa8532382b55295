"""Contig layout on the GPU (pgx_align_batch2, pgx_contigs_resident, pgx_contigs_chunk, the two path_to_contig.py drop-ins) against the
golden output of the reference script (tests/golden/contig_cases.npz) and the oracle's ovlp_match, in the three states of a read
database: bytes present, released (2-bit packs only), compacted (packs + the side store of the reads with ambiguous bases)."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import contig_util as CU
import oracle_util as U
from peregrine_amd import _lib, formats, shimmer
from peregrine_amd.formats import SeqDB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = ("bytes", "released", "compacted")


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "contig_cases.npz"))
    return {k: (g[k].tobytes() if k.startswith("fasta_") else str(g[k])) for k in g.files}


@pytest.fixture(scope="module")
def db(golden):
    d = CU.make_db()
    assert CU.seqdb_sha256(d) == golden["seqdb_sha256"]
    return d


def resident(db, state):
    """a ResidentDB in `state`.  A database with an ambiguous base cannot be released: that state runs on the read set without the
    planted N (the bio paths do not touch that read, so its golden output stands)."""
    rdb = shimmer.ResidentDB(CU.make_db(plant_n=False) if state == "released" else db, 0)
    if state == "released":
        assert rdb.release_bytes() and not rdb.has_bytes and rdb.side_bytes == 0
    elif state == "compacted":
        assert rdb.compact_bytes() and not rdb.has_bytes and rdb.side_bytes > 0
    return rdb


@pytest.mark.parametrize("state", STATES)
def test_align_batch2_vs_oracle(db, state):
    src = CU.make_db(plant_n=False) if state == "released" else db
    rdb = resident(db, state)
    rng = np.random.default_rng(31)
    n = 240
    keys = np.zeros(n, _lib.ALIGN_KEY2_DTYPE)
    keys["rid0"], keys["rid1"] = rng.integers(0, src.n_reads, n), rng.integers(0, src.n_reads, n)
    keys["rid1"][:40] = keys["rid0"][:40]                       # a read against itself: long matches at an offset
    if state != "released":
        keys["rid0"][40:60] = CU.N_READ                         # the read with ambiguous bases, as query and as target
        keys["rid1"][60:80] = CU.N_READ
    keys["dir0"], keys["dir1"] = rng.integers(0, 2, n), rng.integers(0, 2, n)
    keys["dir1"][:40] = keys["dir0"][:40]
    l0, l1 = src.rlen[keys["rid0"]].astype(np.int64), src.rlen[keys["rid1"]].astype(np.int64)
    keys["q_off"] = l0 - rng.integers(1, 900, n)
    keys["t_off"] = l1 - rng.integers(1, 2500, n)
    keys["t_off"][:40] = np.maximum(keys["q_off"][:40].astype(np.int64) - rng.integers(0, 90, 40), 0)
    keys["t_off"][200:] = 0
    keys["q_off"][230:] = l0[230:]                              # an empty query
    got = rdb.align2(keys)
    rl, ro = src.by_rid()
    for i, k in enumerate(keys):
        q = src.seqdb[int(ro[k["rid0"]]) + int(k["q_off"]):int(ro[k["rid0"]]) + int(rl[k["rid0"]])]
        t = src.seqdb[int(ro[k["rid1"]]) + int(k["t_off"]):int(ro[k["rid1"]]) + int(rl[k["rid1"]])]
        assert tuple(int(x) for x in got[i]) == U.orc_ovlp_match(q, int(k["dir0"]), t, int(k["dir1"]), 100), (i, k)
    # t_off == 0 is pgx_align_batch
    k1 = np.zeros(40, _lib.ALIGN_KEY_DTYPE)
    for f in ("rid0", "rid1", "q_off", "dir0", "dir1"):
        k1[f] = keys[f][200:]
    assert np.array_equal(rdb.align(k1), got[200:])
    rdb.close()


@pytest.mark.parametrize("state", STATES)
def test_resident_equals_golden(db, golden, state):
    rdb = resident(db, state)
    _lib.mem_ledger(reset_peak=True)
    for tag in ("bio",) if state == "released" else ("bio", "adv"):
        rows, names = CU.tile_rows(golden["path_" + tag])
        data, off = rdb.contigs(rows)
        assert CU.fasta_of(data, off, names) == golden["fasta_" + tag], (state, tag)
    if state != "bytes":     # what the call held without the seqdb's bytes is booked under its own tag
        assert _lib.mem_ledger()["peak_by_tag"].get("contigs", 0) > 0
    rdb.close()


def test_every_nibble_value(db):
    """a database of arbitrary bytes: every nibble that is not one-hot comes out as N, on both strands"""
    rng = np.random.default_rng(5)
    n, ln = 12, 3000
    seq = rng.integers(0, 256, n * ln, dtype=np.uint8)
    d = SeqDB(seq, np.arange(n, dtype=np.uint32), np.full(n, ln, np.uint32), (np.arange(n) * ln).astype(np.uint64))
    text = "".join("c%d %d:%s %d:%s 0 %d %d 0 0 x y\n" % (i // 3, i, "EB"[i & 1], (i + 5) % n, "BE"[(i >> 1) & 1], *((900, 2400) if (i >> 1) & 1 else (2100, 600)))
                   for i in range(n))
    rows, names = CU.tile_rows(text)
    rdb = shimmer.ResidentDB(d, 0)
    data, off = rdb.contigs(rows)
    assert CU.fasta_of(data, off, names) == CU.layout(d, text, U.orc_ovlp_match)
    rdb.close()


@pytest.fixture(scope="module")
def files(db, golden, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("contigs")
    prefix = str(tmp / "reads")
    formats.write_seqdb(prefix, db)
    paths = {}
    for tag in ("bio", "adv"):
        paths[tag] = str(tmp / (tag + ".path"))
        open(paths[tag], "w").write(golden["path_" + tag])
    return prefix, paths, tmp


@pytest.mark.parametrize("tag", ("bio", "adv"))
def test_chunk_and_drop_ins_equal_golden(files, golden, tag):
    prefix, paths, tmp = files
    out = str(tmp / (tag + ".fa"))
    st = shimmer.path_to_contig(prefix, paths[tag], out)
    assert open(out, "rb").read() == golden["fasta_" + tag]
    assert st["contigs"] == golden["fasta_" + tag].count(b">") and st["bases"] == len(golden["fasta_" + tag]) - sum(
        len(l) + 2 for l in golden["fasta_" + tag].split(b"\n") if l.startswith(b">"))
    for exe in ([sys.executable, os.path.join(ROOT, "bin", "path_to_contig.py")], [os.path.join(ROOT, "bin", "native", "path_to_contig.py")]):
        r = subprocess.run(exe + [prefix, paths[tag]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == golden["fasta_" + tag], (exe, r.returncode, r.stderr[-500:])


def test_two_batches_equal_one(files, golden):
    prefix, paths, tmp = files
    for tag in ("bio", "adv"):
        out = str(tmp / (tag + ".2.fa"))
        os.environ["PGX_CONTIGS_BATCH"] = "2"
        try:
            shimmer.path_to_contig(prefix, paths[tag], out)
        finally:
            os.environ.pop("PGX_CONTIGS_BATCH")
        assert open(out, "rb").read() == golden["fasta_" + tag], tag


def _size_class(b):   # the device block cache's classes (pgx_api.cpp): powers of two up to 1 MiB, then eighths of a power of two
    c = 256
    while c < b and c < (1 << 20):
        c <<= 1
    if c >= b:
        return c
    p2 = 1 << 20
    while p2 * 2 <= b:
        p2 <<= 1
    return -(-b // (p2 >> 3)) * (p2 >> 3)


def test_sub_database_holds_the_named_reads_only(db, files, golden):
    prefix, paths, tmp = files
    gc.collect()
    rows, _ = CU.parse_path(golden["path_bio"])
    named = sorted({r[1] for r in rows} | {r[3] for r in rows})
    nbytes = int(db.rlen[named].sum()) + 1024            # the reads' bytes and the database's zero tail
    _lib.init(0)
    _lib.mem_ledger(reset_peak=True)      # (answers the peak so far, then starts it again from what is live now)
    base = _lib.mem_ledger()
    assert base["peak_by_tag"].get("seqdb.bytes", 0) == 0, "another read database is alive"
    shimmer.path_to_contig(prefix, paths["bio"], str(tmp / "ledger.fa"))
    peak = _lib.mem_ledger()["peak_by_tag"]
    cls = _size_class(nbytes)
    # a block is booked with its size class, and may be served by a cached block up to an eighth larger
    assert 0 < peak["seqdb.bytes"] <= cls + cls // 8 < db.seqdb.size, (peak, nbytes, db.seqdb.size)
    assert peak.get("contigs", 0) > 0


def _bad_cases(db):
    """(name, tiling path text, the row the message must name)"""
    short = db.n_reads - 1                      # a read of 300 bases, appended by the fixture below
    ok = "c0 1:E 2:E 0 1000 3000 0 0 x y\n"
    return [
        ("nine fields", ok + "c0 1:E 2:E 0 1000 3000 0 0 x\n", 1),
        ("blank line", ok + "\n" + ok, 1),
        ("unparsable s", ok + ok + "c0 1:E 2:E 0 1e3 3000 0 0 x y\n", 2),
        ("unparsable e", "c0 1:E 2:E 0 1000 3000.0 0 0 x y\n", 0),
        ("node without strand", ok + "c0 1 2:E 0 1000 3000 0 0 x y\n", 1),
        ("rid absent", ok + "c1 1:E 999999:E 0 1000 3000 0 0 x y\n", 1),
        ("l0 < H", ok + "c0 %d:E 2:E 0 1000 3000 0 0 x y\n" % short, 1),
        ("|e-s|+H > l1", ok + "c0 1:E %d:E 0 0 1 0 0 x y\n" % short, 1),
        ("e <= s", ok + ok + "c0 1:E 2:E 0 3000 1000 0 0 x y\n", 2),
        ("e <= s after the transform", ok + "c0 1:E 2:B 0 1000 3000 0 0 x y\n", 1),
        ("e - seg < 0", ok + "c0 1:E 2:E 0 10 700 0 0 x y\n" + ok + "c1 3:E 4:E 0 10 700 0 0 x y\n", 1),
    ]


def test_errors_name_the_row_and_write_nothing(db, tmp_path):
    d = SeqDB(np.concatenate([db.seqdb, db.seqdb[:300]]), np.arange(db.n_reads + 1, dtype=np.uint32), np.append(db.rlen, np.uint32(300)),
              np.append(db.roff, np.uint64(db.seqdb.size)))
    prefix = str(tmp_path / "reads")
    formats.write_seqdb(prefix, d)
    _lib.init(0)
    lib = _lib.load()
    for name, text, row in _bad_cases(d):
        tp, out = str(tmp_path / "bad.path"), str(tmp_path / "bad.fa")
        open(tp, "w").write(text)
        rc = lib.pgx_contigs_chunk(prefix.encode(), tp.encode(), out.encode(), None, None)
        msg = lib.pgx_last_error().decode()
        assert rc == _lib.PGX_EARG and ("row %d:" % row) in msg and not os.path.exists(out), (name, rc, msg)
        for exe in ([sys.executable, os.path.join(ROOT, "bin", "path_to_contig.py")], [os.path.join(ROOT, "bin", "native", "path_to_contig.py")]):
            if name in ("e - seg < 0", "nine fields"):
                r = subprocess.run(exe + [prefix, tp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
                assert r.returncode == 1 and r.stdout == b"" and ("row %d:" % row).encode() in r.stderr, (name, exe, r)
    # the resident call reports the same (its rows are numbered as given)
    rdb = shimmer.ResidentDB(d, 0)
    rows, _ = CU.tile_rows("c0 1:E 2:E 0 1000 3000 0 0 x y\nc0 1:E 2:E 0 10 700 0 0 x y\n")
    with pytest.raises(_lib.PgxError, match=r"code -1.*row 1:"):
        rdb.contigs(rows)
    rdb.close()
