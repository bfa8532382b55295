"""pg_asm_cns.py on the GPU against the fixture the real script wrote (tests/golden/cnsjob_cases.npz) and against the restatement of
tests/cnsjob_util.py.  First the layout alone (pgx_cns_layout / shimmer.cns_layout): the fixture's cases, seeded random rows, its refusals by
code and message, the ledger.  Then the whole job: the FASTA of shimmer.pg_asm_cns, of pgx_cns_job_resident and of both executables on every
case and chunk, with the pieces cut across batches and the map cut across pieces of the file, seeded random small jobs end to end, the
job's refusals -- those of the parser, of the databases and the one passed through from the consensus call, with the contig and the
segment named -- and the ledger."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cnsjob_util as J
from peregrine_amd import _lib, formats, shimmer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _lengths(db, lacking=()):
    rl, _ = db.by_rid()
    out = np.full(len(rl), -1, np.int64)
    out[db.rid] = db.rlen
    out[list(lacking)] = -1
    return out


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and len(g) == len(w), (len(g), len(w))
        for f in w.dtype.names:
            assert np.array_equal(g[f], w[f]), (f, np.flatnonzero(g[f] != w[f])[:5])


def _chunks():
    return [(c.name, i) for c in J.load_cases() for i in range(len(c.chunks))]


@pytest.mark.parametrize("name,i", _chunks())
def test_layout_equals_the_scripts_and_the_restatements(name, i):
    case = next(c for c in J.load_cases() if c.name == name)
    total, my, _, want, _ = case.chunks[i]
    rows = J.chunk_rows(J.parse_map(case.map_text), total, my)
    lens = _lengths(case.ref_db)
    pieces, reads = shimmer.cns_layout(J.rows_array(rows), lens)
    _same((pieces, reads), J.tables(J.layout(rows, {c: int(n) for c, n in enumerate(lens) if n >= 0})))
    # ... and the script's own words: `left right n_mapped` per group, and the offsets it printed, which are the entries' shifts
    groups = [(c["ctg"], seg, g) for c in want for seg, g in enumerate(c["groups"])]
    assert [(int(p["ctg"]), int(p["seg"]), int(p["left"]) + J.FLANK, int(p["left"]) + int(p["t_len"]), int(p["n_mapped"])) for p in pieces] == \
           [(ctg, seg, g["left"], g["right"], g["n_mapped"]) for ctg, seg, g in groups]
    for p, (_, _, g) in zip(pieces, groups):
        mine = reads[int(p["read_first"]):int(p["read_first"]) + int(p["n_read"])]
        assert sorted((int(e["read"]), int(e["strand"]), int(e["read_shift"]) + int(p["left"])) for e in mine) == sorted(g["offsets"])
        assert np.all(np.diff(mine["read_shift"]) >= 0)


def random_job(rng, n_ctg=9, n_reads=40):
    """small contigs up to 3 kb, one of 110 kb without reads, rows at random places: (rows, ctg_len)"""
    lens = np.concatenate([rng.integers(1, 3001, n_ctg - 1), [110_000]]).astype(np.int64)
    rows = []
    for _ in range(int(rng.integers(1, 400))):
        ctg = int(rng.integers(0, n_ctg - 1))
        rd, strand = int(rng.integers(0, n_reads)), int(rng.integers(0, 2))
        p1 = int(rng.integers(-50, lens[ctg] + 200))
        rb = p1 - int(rng.integers(-300, 3300)) // int(rng.choice([1, 25, 50, 51]))
        rows.append((ctg, p1, p1 + 9, rd, rb, rb + 9, strand, 1, 1))
    rows.append((n_ctg - 1, int(rng.integers(0, 110_000)), 0, 0, 0, 0, 0, 0, 0))       # the long contig: rows, and groups without them
    for p1 in rng.integers(0, 110_000, int(rng.integers(0, 4))):
        rows.append((n_ctg - 1, int(p1), 0, int(rng.integers(0, n_reads)), int(rng.integers(0, 900)), 0, int(rng.integers(0, 2)), 0, 0))
    return [rows[i] for i in rng.permutation(len(rows))], lens


def test_random_small_jobs_equal_the_restatement():
    rng = np.random.default_rng(20261023)
    done = 0
    for _ in range(40):
        rows, lens = random_job(rng)
        try:
            want = J.tables(J.layout(rows, {c: int(n) for c, n in enumerate(lens)}))
        except J.Refused:
            with pytest.raises(_lib.PgxError, match="code -6"):
                shimmer.cns_layout(J.rows_array(rows), lens)
            continue
        _same(shimmer.cns_layout(J.rows_array(rows), lens), want)
        done += 1
    assert done >= 20
    _same(shimmer.cns_layout(np.zeros((0, 9), np.int64), lens), J.tables([]))


def test_refusals_name_the_row_or_the_contig_and_the_library_goes_on():
    case = next(c for c in J.load_cases() if c.name == "edges")
    rows = J.chunk_rows(J.parse_map(case.map_text), 3, 0)
    lens = _lengths(case.ref_db)
    good = shimmer.cns_layout(J.rows_array(rows), lens)
    first3 = next(i for i, r in enumerate(rows) if r[0] == 3)
    above = next(i for i, r in enumerate(rows) if r[0] >= 3)
    zero = lens.copy()
    zero[3] = 0
    far = list(rows)
    far[7] = (far[7][0], 1 << 29, *far[7][2:])
    strand = list(rows)
    strand[5] = (*strand[5][:6], 2, *strand[5][7:])
    # two rows that close groups beyond the 105,000 bases of contig 12: the first one's template leaves the contig (the second one's is cut
    # to the contig's end by the tail rule)
    beyond = [(12, 107_000, 0, 1, 0, 0, 0, 0, 0), (12, 160_000, 0, 1, 0, 0, 0, 0, 0)]
    for bad_rows, bad_lens, words in ((rows, _lengths(case.ref_db, lacking=[3]), (f"row {first3}", "contig 3", "not in the idx")),
                                      (rows, lens[:3], (f"row {above}:", f"contig {rows[above][0]} is", "not in the idx")),
                                      (rows, zero, (f"row {first3}", "contig 3", "length 0")),
                                      (far, lens, ("row 7", "2^29")),
                                      (strand, lens, ("row 5", "strand")),
                                      (beyond, lens, ("contig 12 segment 0", "outside the contig"))):
        with pytest.raises(_lib.PgxError) as e:
            shimmer.cns_layout(J.rows_array(bad_rows), bad_lens)
        assert "code -6" in str(e.value) and "pgx_cns_layout" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
        _same(shimmer.cns_layout(J.rows_array(rows), lens), good)


def test_ledger_shows_the_job_and_returns_to_its_level():
    case = next(c for c in J.load_cases() if c.name == "bio")
    rows = J.rows_array(J.parse_map(case.map_text))
    lens = _lengths(case.ref_db)

    def tag_bytes():
        _lib.mem_ledger(reset_peak=True)   # the peak starts again from now: peak_by_tag is the live bytes by owner
        return _lib.mem_ledger()["peak_by_tag"].get("cns.job", 0)

    _lib.init()
    level = tag_bytes()
    shimmer.cns_layout(rows, lens)
    assert _lib.mem_ledger()["peak_by_tag"].get("cns.job", 0) >= level + rows.nbytes
    assert tag_bytes() == level


# ---- the whole job ------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{case: (read prefix, ref prefix, map path)}: the fixture's databases and maps as files"""
    d = tmp_path_factory.mktemp("cnsjob")
    out = {}
    for c in J.load_cases():
        rp, cp, mp = str(d / (c.name + "_reads")), str(d / (c.name + "_ref")), str(d / (c.name + ".map"))
        formats.write_seqdb(rp, c.read_db)
        formats.write_seqdb(cp, c.ref_db)
        open(mp, "w").write(c.map_text)
        out[c.name] = (rp, cp, mp)
    return out


def _job(files, name, total, my, tmp_path, env=None):
    """pg_asm_cns to a file, with `env` set around the call: (the file's bytes, the stats)"""
    out = str(tmp_path / f"{name}_{total}_{my}.fa")
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        st = shimmer.pg_asm_cns(*files[name], total, my, out=out)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return open(out, "rb").read(), st


@pytest.mark.parametrize("name,i", _chunks())
def test_fasta_of_the_library_equals_the_scripts_stdout(files, tmp_path, name, i):
    case = next(c for c in J.load_cases() if c.name == name)
    total, my, want, lay, runs = case.chunks[i]
    got, st = _job(files, name, total, my, tmp_path)
    assert got == want
    assert (st["n_contigs"], st["n_pieces"], st["n_batches"]) == (len(lay), len(runs), 1)
    assert st["n_called"] + st["n_by_rule"] == len(runs) and st["n_reads"] == sum(len(g["offsets"]) for c in lay for g in c["groups"])
    groups = [g for c in lay for g in c["groups"]]
    assert st["n_called"] == sum(1 for g, run in zip(groups, runs) if run["aln_base"] >= 3 * (g["right"] - g["left"] + J.FLANK))
    # cut across batches, and the map in many pieces of the file
    for env in ({"PGX_CNS_JOB_BATCH": "1"}, {"PGX_CNS_JOB_BATCH": "3"}, {"PGX_CNS_JOB_MAP_PIECE": "4096"}):
        got, st = _job(files, name, total, my, tmp_path, env)
        assert got == want, env
        if "PGX_CNS_JOB_BATCH" in env:
            assert st["n_batches"] == -(-len(runs) // int(env["PGX_CNS_JOB_BATCH"]))
    # the resident form, from rows
    rdb, cdb = shimmer.ResidentDB(case.read_db), shimmer.ResidentDB(case.ref_db)
    try:
        text, off = shimmer.cns_job_resident(rdb, cdb, J.rows_array(J.parse_map(case.map_text)), total, my, case.ref_db.names)
    finally:
        rdb.close(), cdb.close()
    assert text == want and len(off) == len(lay) + 1 and int(off[-1]) == len(want)
    assert all(text[int(o):int(o) + 1] == b">" for o in off[:-1])


@pytest.mark.parametrize("name,i", _chunks())
def test_fasta_of_both_executables_equals_the_scripts_stdout(files, name, i):
    case = next(c for c in J.load_cases() if c.name == name)
    total, my, want, _, _ = case.chunks[i]
    for exe in ([os.path.join(ROOT, "bin", "native", "pg_asm_cns.py")], [sys.executable, os.path.join(ROOT, "bin", "pg_asm_cns.py")]):
        r = subprocess.run(exe + [*files[name], str(total), str(my)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and r.stdout == want, (exe, r.returncode, r.stderr[-500:])


def random_db_job(rng):
    """contigs up to 3 kb and one of 110 kb without reads, short reads drawn from the contigs, rows near their true places"""
    b = J.Builder(int(rng.integers(1 << 30)))
    for length in rng.integers(1, 3001, 5):
        c = b.contig(int(length))
        for _ in range(int(rng.integers(0, 7))):
            pos = int(rng.integers(0, length))
            n = int(rng.integers(1, length - pos + 1))
            if n < 40:
                continue
            strand = int(rng.integers(0, 2))
            rd = b.read(c, pos, n, strand)
            for _ in range(int(rng.integers(1, 5))):
                x = int(rng.integers(0, n))
                b.row(c, pos + x + int(rng.integers(-60, 61)), rd, x, strand)
    big = b.contig(110_000)
    for p1 in rng.integers(0, 110_000, int(rng.integers(1, 4))):
        b.row(big, int(p1), 0, 5, 0)
    if not b.reads:
        b.reads.append(b"ACGTACGTAC")
    return b, b.map_text(rng.permutation(len(b.rows)))


def test_random_small_jobs_equal_the_restatement_end_to_end():
    rng = np.random.default_rng(20261024)
    done = 0
    for _ in range(6):
        b, text = random_db_job(rng)
        rdb, cdb = b.dbs()
        total, my = int(rng.integers(1, 4)), int(rng.integers(0, 4))
        try:
            want = J.job(rdb, cdb, text, total, my)
        except (J.Refused, J.CU.Refused):
            want = None
        r, c = shimmer.ResidentDB(rdb), shimmer.ResidentDB(cdb)
        try:
            if want is None:
                with pytest.raises(_lib.PgxError, match="code -6"):
                    shimmer.cns_job_resident(r, c, J.rows_array(J.parse_map(text)), total, my, cdb.names)
            else:
                assert shimmer.cns_job_resident(r, c, J.rows_array(J.parse_map(text)), total, my, cdb.names)[0] == want
                done += 1
        finally:
            r.close(), c.close()
    assert done >= 4


def test_job_refusals_name_the_line_or_the_contig_and_the_library_goes_on(files, tmp_path):
    case = next(c for c in J.load_cases() if c.name == "edges")
    rp, cp, mp = files["edges"]
    want = case.chunks[1][2]
    lines = case.map_text.splitlines(keepends=True)

    def variant(db, path, drop=(), zero=()):
        keep = [i for i, r in enumerate(db.rid) if int(r) not in drop]
        rlen = db.rlen.copy()
        rlen[list(zero)] = 0
        formats.write_seqdb(path, formats.SeqDB(db.seqdb, db.rid[keep], rlen[keep], db.roff[keep], [db.names[i] for i in keep]))
        return path

    def mapped(text, name):
        p = str(tmp_path / name)
        open(p, "w").write(text)
        return p

    first4 = next(i for i, ln in enumerate(lines) if ln.split()[0] == "4") + 1
    read_of_7 = next(int(ln.split()[3]) for ln in lines if ln.split()[0] == "7")
    eight = lines[:5] + [" ".join(lines[5].split()[:8]) + "\n"] + lines[6:]
    word = lines[:9] + [lines[9].replace(" ", " x", 1)] + lines[10:]
    big = lines[:2] + [" ".join(["1", str(1 << 29)] + lines[2].split()[2:]) + "\n"] + lines[3:]
    blank = lines[:3] + ["\n"] + lines[3:]
    cases = ((rp, cp, mapped("".join(eight), "eight.map"), 3, 1, -6, ("line 6 ", "nine fields")),
             (rp, cp, mapped("".join(word), "word.map"), 3, 1, -6, ("line 10 ", "decimal integer")),
             (rp, cp, mapped("".join(big), "big.map"), 3, 1, -6, ("line 3 ", "does not fit")),
             (rp, cp, mapped("".join(blank), "blank.map"), 3, 1, -6, ("line 4 ", "nine fields")),
             (rp, variant(case.ref_db, str(tmp_path / "lacks4"), drop=[4]), mp, 3, 1, -6, (f"line {first4}:", "contig 4 is not in the idx")),
             (rp, variant(case.ref_db, str(tmp_path / "zero4"), zero=[4]), mp, 3, 1, -6, (f"line {first4}:", "contig 4 has length 0")),
             (variant(case.read_db, str(tmp_path / "lacksread"), drop=[read_of_7]), cp, mp, 3, 1, -6, ("contig 7 segment 0", f"read {read_of_7} is not in the idx")),
             (rp, cp, mp, 0, 1, -6, ("total_chunks == 0",)))
    for a, b, m, total, my, code, words in cases:
        with pytest.raises(_lib.PgxError) as e:
            shimmer.pg_asm_cns(a, b, m, total, my, out=str(tmp_path / "never.fa"))
        assert f"code {code}" in str(e.value) and "pgx_cns_job" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
        assert _job(files, "edges", 3, 1, tmp_path)[0] == want
    assert not os.path.exists(str(tmp_path / "never.fa"))


def test_a_refusal_of_the_consensus_call_passes_through_with_contig_and_segment_named(files, tmp_path):
    """a piece with more than 65,535 alignments (the call's refusal, section 4.7): contig 3 is 57 copies of a unit of 51 bases, 1,200 reads of
    its first 40 bases each mapped at 55 offsets 51 apart -- every entry matches where it is put, 66,000 entries in the contig's one
    group.  It is the job's second piece (contig 5, answered first, is a good one): whether it is piece 1 of one batch or piece 0 of the
    second, the message names piece 1, contig 3, segment 0."""
    rng = np.random.default_rng(20261025)
    b = J.Builder(20261026)
    for _ in range(3):
        b.contig(40)                                  # ids 0 .. 2: not in the map
    unit = J.CU.random_template(rng, 51)
    b.truth.append(unit * 57)
    b.contigs.append(unit * 57)                       # contig 3: 2,907 bases
    b.contig(40)
    good = b.contig(2400)                             # contig 5
    for k in range(4):
        b.mapped(good, 0, 2400, k & 1, every=300)
    first = len(b.reads)
    b.reads += [unit[:40]] * 1200
    rows = [(3, 51 * k, 51 * k + 9, first + r, 0, 9, 0, 1, 1) for r in range(1200) for k in range(55)]
    text = b.map_text() + "".join(" ".join(str(v) for v in r) + "\n" for r in rows)
    rdb, cdb = b.dbs()
    rp, cp, mp = str(tmp_path / "many_reads"), str(tmp_path / "many_ref"), str(tmp_path / "many.map")
    formats.write_seqdb(rp, rdb)
    formats.write_seqdb(cp, cdb)
    open(mp, "w").write(text)
    lay = J.layout(J.parse_map(text), {int(r): int(n) for r, n in zip(cdb.rid, cdb.rlen)})
    assert [(c["ctg"], [len(g["entries"]) for g in c["groups"]]) for c in lay][1] == (3, [66_000])
    want = J.job(rdb, cdb, b.map_text(), 1, 0)         # the good contig alone
    for env in ({}, {"PGX_CNS_JOB_BATCH": "1"}):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            with pytest.raises(_lib.PgxError) as e:
                shimmer.pg_asm_cns(rp, cp, mp, 1, 0, out=str(tmp_path / "never.fa"))
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        msg = str(e.value)
        assert "code -6" in msg and "pgx_cns_job" in msg and "piece 1:" in msg and "more than 65535 alignments" in msg, msg
        assert "(piece 1 is contig 3 segment 0)" in msg, msg
        assert not os.path.exists(str(tmp_path / "never.fa"))
        # ... and the library goes on: the same databases, the good contig's rows alone
        good_map = str(tmp_path / "good.map")
        open(good_map, "w").write(b.map_text())
        out = str(tmp_path / "good.fa")
        shimmer.pg_asm_cns(rp, cp, good_map, 1, 0, out=out)
        assert open(out, "rb").read() == want


def test_ledger_shows_the_whole_job_and_returns_to_its_level(files, tmp_path):
    def tag_bytes():
        _lib.mem_ledger(reset_peak=True)
        return _lib.mem_ledger()["peak_by_tag"].get("cns.job", 0)

    _lib.init()
    level = tag_bytes()
    _, st = _job(files, "bio", 1, 0, tmp_path)
    assert _lib.mem_ledger()["peak_by_tag"].get("cns.job", 0) >= level + st["pool_bytes"]
    assert tag_bytes() == level
