"""The reference's consensus script py/scripts/pg_asm_cns.py restated in plain Python over aln_util and cns_util: chunk filter, groups,
read entries, pieces and stitch; the seeded databases of its fixture and the reader of tests/golden/cnsjob_cases.npz.  Nothing here is the
reference's code: it is the rule of DESIGN.md section 4.7b, which tests/golden/make_golden_cnsjob.py checked against the real script, run
as a child process, when it wrote the fixture.

A row is nine integers `ctg p1 p2 read rb re strand mc0 mc1`.  A layout is a list of contigs in the order the script answers them:
    {"ctg": id, "groups": [{"left": left_anchor, "right": right, "n_mapped": rows, "offsets": [(read, strand, offset), ...] in the order
                            the script prints them, "entries": [(read, strand, read_shift), ...] in the order it aligns them}, ...]}
"""
import hashlib
import os
import re

import numpy as np

import aln_util as AU
import cns_util as CU
from peregrine_amd.formats import SeqDB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cnsjob_cases.npz")
PROVENANCE = os.path.join(ROOT, "tests", "golden", "cnsjob_cases.provenance.json")
FIRST_ANCHOR, FLANK, JOIN, KEEP, CHAIN = 1000, 1000, 50_000, 100_000, 50
STITCH_Q, STITCH_T, STITCH_BAND = 1000, 1050, 400
# what pgx_cns_layout answers (include/pgx.h: pgx_cns_job_piece, pgx_cns_job_read)
JOB_PIECE_DTYPE = np.dtype([("ctg", "<u4"), ("seg", "<u4"), ("left", "<i4"), ("t_len", "<u4"), ("n_mapped", "<u4"), ("read_first", "<u4"), ("n_read", "<u4"),
                            ("pad", "<u4")])
JOB_READ_DTYPE = np.dtype([("piece", "<u4"), ("read", "<u4"), ("read_shift", "<i4"), ("strand", "<u4")])


class Refused(ValueError):
    """the script has no answer: it dies on a Python exception or reads outside its buffers"""


# ---- rows -----------------------------------------------------------------------------------------------------------------------------------
def parse_map(text):
    """the rows of a map file's text; the first line without nine integer fields is named.  A line ends at '\\n' and nowhere else, as in the
    library (the script's text-mode read also ends one at a lone '\\r': there the library sees one line of too many fields and refuses it)"""
    rows = []
    lines = text.split("\n")
    if lines and lines[-1] == "":          # the file's last line ends with '\n': nothing follows it
        lines.pop()
    for no, line in enumerate(lines, 1):
        f = line.strip().split()
        try:
            row = tuple(int(c) for c in f)
        except ValueError:
            raise Refused(f"line {no}: not an integer")
        if len(row) != 9:
            raise Refused(f"line {no}: {len(row)} fields")
        rows.append(row)
    return rows


def chunk_rows(rows, total, my):
    if total == 0:
        raise Refused("total_chunks == 0")
    return [r for r in rows if my % total == r[0] % total]


# ---- groups (pg_asm_cns.py:68-98) -------------------------------------------------------------------------------------------------------------
def groups_of(rows, length):
    """[[left_anchor, right, rows], ...] of one contig's rows (file order) and its length"""
    rows = sorted(rows, key=lambda r: r[1])
    out, left, cur = [], FIRST_ANCHOR, []
    for r in rows:
        if r[1] - left < JOIN:
            cur.append(r)
        else:
            out.append([left, r[1], cur if r[1] - left < KEEP else []])
            cur, left = [], r[1]
    if length - left >= KEEP:
        out.append([left, length, []])
    elif length - left > FLANK:
        out.append([left, length, cur])
    elif out:
        out[-1][1] = length
        out[-1][2] = out[-1][2] + cur
    else:
        out.append([left, length, []])
    return out


# ---- the reads of a group (pg_asm_cns.py:115-139) --------------------------------------------------------------------------------------------
def entries_of(left_anchor, rows):
    """(offsets in the script's print order, entries sorted by read_shift) of a group's rows"""
    left = left_anchor - FLANK
    by_key = {}
    for r in rows:
        by_key.setdefault((r[3], r[6]), []).append(r[1] - r[4])
    offsets = []
    for (read, strand), v in by_key.items():
        v = sorted(v)
        cur = v[0]
        offsets.append((read, strand, cur))
        for x in v:
            if x > cur + CHAIN:
                cur = x
                offsets.append((read, strand, cur))
    entries = sorted(((rd, st, o - left) for rd, st, o in offsets), key=lambda e: e[2])
    return offsets, entries


def layout(rows, ctg_len):
    """the layout of rows that passed the chunk filter; ctg_len: {contig: length}"""
    by_ctg = {}
    for r in rows:
        by_ctg.setdefault(r[0], []).append(r)
    out = []
    for ctg, rs in by_ctg.items():
        if ctg not in ctg_len:
            raise Refused(f"contig {ctg} is not in the idx")
        if ctg_len[ctg] == 0:
            raise Refused(f"contig {ctg} has length 0")
        gs = []
        for seg, (left, right, mapped) in enumerate(groups_of(rs, ctg_len[ctg])):
            if right - (left - FLANK) <= 0 or right > ctg_len[ctg]:
                raise Refused(f"contig {ctg} segment {seg}: a template outside the contig")
            offsets, entries = entries_of(left, mapped)
            gs.append(dict(left=left, right=right, n_mapped=len(mapped), offsets=offsets, entries=entries))
        out.append(dict(ctg=ctg, groups=gs))
    return out


def tables(lay):
    """(pieces, reads) of a layout as pgx_cns_layout answers them"""
    pieces, reads = [], []
    for c in lay:
        for seg, g in enumerate(c["groups"]):
            pieces.append((c["ctg"], seg, g["left"] - FLANK, g["right"] - g["left"] + FLANK, g["n_mapped"], len(reads), len(g["entries"]), 0))
            reads += [(len(pieces) - 1, rd, sh, st) for rd, st, sh in g["entries"]]
    return np.array(pieces, JOB_PIECE_DTYPE), np.array(reads, JOB_READ_DTYPE)


def rows_array(rows):
    return np.array(rows, np.int64).reshape(-1, 9)


# ---- the databases ----------------------------------------------------------------------------------------------------------------------------
_CODE = np.zeros(256, np.uint8)
for _b, _c in zip(b"ACGTacgt", (1, 2, 4, 8, 1, 2, 4, 8)):
    _CODE[_b] = _c
_COMP = bytes.maketrans(b"ACGTNacgtn", b"TGCANtgcan")
_BASE = np.frombuffer(b"NACNGNNNTNNNNNNN", np.uint8)


def revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


def encode(seq):
    """the seqdb bytes of a sequence: the base's code in the low nibble, the reverse complement's base at the same place in the high one"""
    s = np.frombuffer(bytes(seq), np.uint8)
    return _CODE[s] | (_CODE[np.frombuffer(revcomp(seq), np.uint8)] << 4)


def decode(bseq, strand):
    b = np.asarray(bseq, np.uint8)
    return _BASE[(b & 15) if strand == 0 else (b >> 4)].tobytes()


def db_of(seqs, names, ids=None):
    ids = list(range(len(seqs))) if ids is None else list(ids)
    lens = np.array([len(s) for s in seqs], np.uint32)
    off = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64) if len(seqs) else np.zeros(0, np.uint64)
    data = np.concatenate([encode(s) for s in seqs]) if len(seqs) else np.zeros(0, np.uint8)
    return SeqDB(data, np.array(ids, np.uint32), lens, off, list(names))


def db_sha256(db):
    h = hashlib.sha256(np.ascontiguousarray(db.seqdb).tobytes())
    for r, n, ln, o in zip(db.rid, db.names, db.rlen, db.roff):
        h.update(b"%d %s %d %d\n" % (int(r), n.encode(), int(ln), int(o)))
    return h.hexdigest()


def seq_of(db, i, strand=0):
    rl, ro = db.by_rid()
    return decode(db.seqdb[int(ro[i]):int(ro[i]) + int(rl[i])], strand)


class Builder:
    """contigs, reads drawn from them and map rows, from one seeded generator"""

    def __init__(self, seed, rate=0.01):
        self.rng, self.rate = np.random.default_rng(seed), rate
        self.truth, self.contigs, self.reads, self.rows = [], [], [], []

    def contig(self, length, polish=0.003):
        """a contig of exactly `length` bases: the truth with substitutions at `polish`"""
        t = CU.random_template(self.rng, length)
        a = np.frombuffer(t, np.uint8).copy()
        hit = self.rng.random(length) < polish
        a[hit] = self.rng.choice(np.frombuffer(b"ACGT", np.uint8), int(hit.sum()))
        self.truth.append(t)
        self.contigs.append(a.tobytes())
        return len(self.contigs) - 1

    def read(self, ctg, pos, length, strand):
        """a read of the truth of ctg from pos on; strand 1: the database holds its reverse complement"""
        s = CU.mutate(self.rng, self.truth[ctg][max(pos, 0):pos + length], self.rate)
        self.reads.append(revcomp(s) if strand else s)
        return len(self.reads) - 1

    def row(self, ctg, p1, read, rb, strand):
        self.rows.append((ctg, p1, p1 + 60, read, rb, rb + 60, strand, 3, 5))

    def mapped(self, ctg, pos, length, strand, every=600, jitter=4, lo=None, hi=None):
        """a read with map rows at its true positions, a few bases off: rows with lo <= p1 < hi only"""
        rd = self.read(ctg, pos, length, strand)
        for x in range(100, length - 100, every):
            p1 = pos + x + int(self.rng.integers(-jitter, jitter + 1))
            if (lo is None or p1 >= lo) and (hi is None or p1 < hi) and p1 >= 0:
                self.row(ctg, p1, rd, x, strand)
        return rd

    def dbs(self):
        return (db_of(self.reads, ["read%05d" % i for i in range(len(self.reads))]),
                db_of(self.contigs, ["ctg%03d" % i for i in range(len(self.contigs))]))

    def map_text(self, order=None):
        rows = self.rows if order is None else [self.rows[i] for i in order]
        return "".join(" ".join(str(v) for v in r) + "\n" for r in rows)


def build_bio(seed=20261021):
    """two contigs of 120 kb and 60 kb, reads of 8 kb at 1 % on both strands, about 6x"""
    b = Builder(seed)
    for length in (120_000, 60_000):
        c = b.contig(length)
        for _ in range(6 * length // 8000):
            pos = int(b.rng.integers(-4000, length - 4000))
            pos = max(pos, 0)
            b.mapped(c, pos, min(8000, length - pos), int(b.rng.integers(0, 2)))
    order = b.rng.permutation(len(b.rows))
    return b, b.map_text(order)


def build_edges(seed=20261022):
    """hand-placed rows: see tests/golden/make_golden_cnsjob.py"""
    b = Builder(seed)
    blocks = []                       # rows per contig, interleaved below

    def block(fn):
        n0 = len(b.rows)
        fn()
        blocks.append(list(range(n0, len(b.rows))))

    # contig lengths 1 .. 2002: one read each where it fits
    for length in (1, 999, 1000, 1999, 2000, 2001, 2002):
        c = b.contig(length)
        def small(c=c, length=length):
            if length < 300:
                b.reads.append(b"ACGT" * 10)
                b.row(c, 0, len(b.reads) - 1, 0, 0)
                return
            for k in range(4):
                b.mapped(c, 0, length, k & 1, every=300)
            if length == 2002:
                r = b.read(c, 0, 400, 0)
                b.row(c, 2102, r, 100, 0)          # a shift AT the template's end (p1 beyond the contig, p1 - 1000 < 50000 all the same)
                b.row(c, 2500, r, 30, 1)           # ... and beyond it, the same read on the other strand
                b.row(c, 1980, b.read(c, 1500, 500, 0), 0, 0)   # 22 bases before the end: the second acceptance condition on almost nothing
        block(small)
    # A: p1 - left_anchor of 49,999 joins, 50,000 closes and keeps; tail of exactly 1,000 merged into the group that had rows
    A = b.contig(52_000)
    def rows_a():
        r0 = b.mapped(A, 49_000, 2800, 0, every=250, lo=0, hi=50_999)
        b.row(A, 50_999, r0, 1999, 0)               # 49,999: joins
        r1 = b.read(A, 50_500, 1500, 1)
        b.row(A, 51_000, r1, 400, 1)                # 50,000: closes the group, joins none (its offset would make an entry)
        b.row(A, 51_400, r1, 900, 1)                # open rows: behind the group's own after the merge
        b.row(A, 500, b.read(A, 0, 1500, 0), 500, 0)   # p1 < 1000
        b.row(A, 700, len(b.reads) - 1, 700, 0)
    block(rows_a)
    # B: 99,999 closes and keeps its rows; a tail of 1,001 is a group of its own
    B = b.contig(102_000)
    def rows_b():
        r = b.mapped(B, 1000, 3000, 0, every=500)
        r2 = b.read(B, 100_500, 1500, 0)
        b.row(B, 100_999, r2, 499, 0)               # 99,999: closes, rows kept
        b.row(B, 101_500, r2, 1000, 0)
        b.row(B, 101_500, r, 7, 1)                  # equal p1 in file order; one read in two groups, and on both strands
    block(rows_b)
    # C: 100,000 closes WITHOUT rows; a tail of 1,000 merged into that group, which takes the open rows
    C = b.contig(102_000)
    def rows_c():
        b.mapped(C, 2000, 2000, 1, every=400)       # dropped with the group
        r = b.read(C, 100_200, 1800, 0)
        b.row(C, 101_000, r, 800, 0)                # 100,000: closes, no rows
        b.row(C, 101_300, r, 1100, 0)
        b.row(C, 101_350, r, 1100, 0)               # offsets 50 apart: one entry
        b.row(C, 101_351, r, 1100, 0)               # 51 above the entry: a second one
        r2 = b.read(C, 100_000, 1900, 1)
        for d in (0, 40, 80):                       # a chain of 40 + 40: the second entry at + 80
            b.row(C, 101_200 + d, r2, 1200, 1)
        r3 = b.read(C, 100_200, 1700, 0)
        b.row(C, 101_300, r3, 1100, 0)              # equal p1 and equal shifts with r's first row: file order decides
    block(rows_c)
    # D / E: tails of 99,999 (a group with the open rows) and 100,000 (a group without)
    D, E = b.contig(100_999), b.contig(101_000)
    block(lambda: b.mapped(D, 500, 2000, 0, every=500))
    block(lambda: b.mapped(E, 500, 2000, 1, every=500))
    # F: a called segment, a lower-case one, a called tail
    F = b.contig(105_000)
    def rows_f():
        for k in range(26):
            b.mapped(F, k * 1700, 8000, k & 1, every=700, hi=51_000)
        far = b.read(F, 50_000, 3000, 0)
        b.row(F, 51_005, far, 1005, 0)              # closes the first group
        b.row(F, 101_010, far, 2990, 0)             # closes the second: its only rows are one read's -- lower case
        b.row(F, 60_000, far, 2000, 0)              # the second group's only row: a read that lies 8 kb from where the row puts it
        for k in range(6):
            b.mapped(F, 99_800 + 100 * k, 5000 - 100 * k, k & 1, every=300, lo=101_011)   # negative shifts in the tail's template
    block(rows_f)
    order, at = [], [0] * len(blocks)
    while any(a < len(bl) for a, bl in zip(at, blocks)):      # contig ids interleaved in the file, three rows at a time
        for i, bl in enumerate(blocks):
            order += bl[at[i]:at[i] + 3]
            at[i] += 3
    return b, b.map_text(order)


BUILDERS = dict(bio=build_bio, edges=build_edges)
CHUNKS = dict(bio=[(1, 0)], edges=[(3, 0), (3, 1), (3, 2), (3, 3)])


# ---- the job ------------------------------------------------------------------------------------------------------------------------------
def script_accepts(t_len, read_len, shift, answer):
    """pg_asm_cns.py:189-216 on the aligner's answer (zeros where the read or the template was clipped to nothing)"""
    span = abs(answer[3] - answer[2])
    if shift < 0:
        return abs(span - (read_len + shift)) < 48
    return abs(span - read_len) < 48 or abs(t_len - shift - span) < 48


def piece(template, reads, aligner=None):
    """(segment, accepted flags as the script prints them, aln_count, aln_base) of one group: template and [(read bytes, shift)]"""
    al = aligner or (lambda q, t, band: AU.align(q, t, band)[0])
    alns, aln_base, used = AU.piece_alignments(template, reads, al)
    said = []
    for (read, shift), u in zip(reads, used):
        clipped = (len(read) + shift <= 0) if shift < 0 else (len(template) - shift <= 0)
        said.append(script_accepts(len(template), len(read), shift, AU.ZERO) if clipped else bool(u))
    if aln_base / len(template) < 3:
        seg = bytes(template).lower()
    else:
        seg = CU.consensus(len(template), alns, 1)
    return seg, said, 1 + sum(said), aln_base


def stitch(segments, aligner=None):
    """pg_asm_cns.py:251-271"""
    al = aligner or (lambda q, t, band: AU.align(q, t, band, want_str=False)[0])
    s0 = segments[0]
    kept = [s0]
    for seg, s1 in enumerate(segments[1:], 1):
        if len(s0) < STITCH_Q or len(s1) < STITCH_T:
            raise Refused(f"segment {seg}: a stitch of {len(s0)} against {len(s1)} bytes")
        a = al(s0[-STITCH_Q:], s1[:STITCH_T], STITCH_BAND)
        if a[3] < STITCH_Q:
            kept[-1] = kept[-1][:-(STITCH_Q - a[3])]
        kept.append(s1[a[5]:])
        s0 = s1
    return b"".join(kept)


def job(read_db, ref_db, map_text, total, my, aligner=None, details=None):
    """the script's stdout; details, a list, receives per group (ctg, seg, accepted flags, aln_count, aln_base)"""
    rows = chunk_rows(parse_map(map_text), total, my)
    rl, ro = ref_db.by_rid()
    have = set(int(r) for r in ref_db.rid)
    lay = layout(rows, {c: int(rl[c]) for c in have})
    names = {int(r): n for r, n in zip(ref_db.rid, ref_db.names)}
    rdl, rdo = read_db.by_rid()
    reads_have = set(int(r) for r in read_db.rid)
    out = bytearray()
    for c in lay:
        ctg, segs = c["ctg"], []
        for seg, g in enumerate(c["groups"]):
            s = int(ro[ctg]) + g["left"] - FLANK
            template = decode(ref_db.seqdb[s:s + g["right"] - g["left"] + FLANK], 0)
            reads = []
            for rd, st, sh in g["entries"]:
                if rd not in reads_have:
                    raise Refused(f"read {rd} is not in the idx")
                reads.append((decode(read_db.seqdb[int(rdo[rd]):int(rdo[rd]) + int(rdl[rd])], st), sh))
            text, said, n, base = piece(template, reads, aligner)
            if details is not None:
                details.append((ctg, seg, said, n, base))
            segs.append(text)
        out += b">" + names[ctg].encode() + b"\n" + stitch(segs, aligner) + b"\n"
    return bytes(out)


# ---- the script's stderr ----------------------------------------------------------------------------------------------------------------------
def parse_stderr(text, name_to_ctg):
    """the layout the script printed, and per group (accepted reads in order, aln_count, aln_base)"""
    lay, runs = [], []
    for line in text.splitlines():
        line = line.strip()
        m = re.fullmatch(r"ctg (\S+)", line)
        if m:
            lay.append(dict(ctg=name_to_ctg[m.group(1)], groups=[]))
            continue
        m = re.fullmatch(r"sg\d+ (-?\d+) (-?\d+) (-?\d+) (\d+)", line)
        if m:
            lay[-1]["groups"].append(dict(left=int(m.group(1)), right=int(m.group(2)), n_mapped=int(m.group(4)), offsets=[]))
            runs.append(dict(accepted=[]))
            continue
        m = re.fullmatch(r"\((\d+), (\d+)\) (-?\d+)", line)
        if m:
            lay[-1]["groups"][-1]["offsets"].append((int(m.group(1)), int(m.group(2)), int(m.group(3))))
            continue
        m = re.fullmatch(r"(\d+) is algined .*", line)
        if m:
            runs[-1]["accepted"].append(int(m.group(1)))
            continue
        m = re.fullmatch(r"aln_count:(\d+), aln_base: (\d+), .*", line)
        if m:
            runs[-1]["aln_count"], runs[-1]["aln_base"] = int(m.group(1)), int(m.group(2))
    return lay, runs


# ---- the fixture --------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, read_db, ref_db, map_text, chunks):
        self.name, self.read_db, self.ref_db, self.map_text, self.chunks = name, read_db, ref_db, map_text, chunks
        # chunks: [(total, my, stdout, layout, runs)]


_cases = None


def load_cases():
    """the fixture's cases with their databases regenerated from the seeds (and checked against the stored SHA-256)"""
    global _cases
    if _cases is not None:
        return _cases
    import json
    g = np.load(GOLDEN)
    out = []
    for name in g["names"].tolist():
        b, text = BUILDERS[name]()
        rdb, cdb = b.dbs()
        assert text == str(g[f"{name}_map"]) and db_sha256(rdb) == str(g[f"{name}_read_sha256"]) and db_sha256(cdb) == str(g[f"{name}_ref_sha256"]), name
        chunks = []
        for total, my in CHUNKS[name]:
            k = f"{name}_{total}_{my}"
            lay, runs = json.loads(str(g[k + "_layout"]))
            for c in lay:
                for grp in c["groups"]:
                    grp["offsets"] = [tuple(o) for o in grp["offsets"]]
            chunks.append((total, my, g[k + "_stdout"].tobytes(), lay, runs))
        out.append(Case(name, rdb, cdb, text, chunks))
    _cases = out
    return out
