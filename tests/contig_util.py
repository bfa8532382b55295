"""Shared by tests/golden/make_golden_contigs.py and the contig-layout tests: the fixture's read set (simreads by seed plus planted
ambiguous bases), the tiling-path parser, and a numpy statement of what py/scripts/path_to_contig.py computes over any ovlp_match."""
from __future__ import annotations

import functools
import hashlib

import numpy as np

from peregrine_amd import simreads
from peregrine_amd.formats import SeqDB

H = 500
BAND = 100
GENOME = dict(length=40_000, seed=11)
READS = dict(n_reads=300, seed=5, mean_len=5000, sd_len=500, err=5e-5, wrap=0)   # HiFi-like: the longest exact run of a stitch reaches its end
N_READ = 7   # its last 500 forward bases are planted as N (nibble 0): a query that matches nothing -> q_m_end = t_m_end = 0
BASES = np.full(16, ord("N"), np.uint8)
BASES[[1, 2, 4, 8]] = [ord(c) for c in "ACGT"]


def make_db(plant_n: bool = True) -> SeqDB:
    db = simreads.simulate_reads(simreads.make_genome(**GENOME), **READS)
    if not plant_n:
        return db
    seq = db.seqdb.copy()
    o, n = int(db.roff[N_READ]), int(db.rlen[N_READ])
    seq[o + n - H:o + n] &= 0xF0       # forward bases l - 500 .. l - 1
    seq[o:o + H] &= 0x0F               # the same bases on the reverse strand
    return SeqDB(seq, db.rid, db.rlen, db.roff, db.names)


def seqdb_sha256(db: SeqDB) -> str:
    return hashlib.sha256(np.ascontiguousarray(db.seqdb).tobytes()).hexdigest()


def parse_path(text: str):
    """rows in contig order (contigs by first appearance, file order inside): (ctg index, rid0, strand0, rid1, strand1, s, e, line); names"""
    names, rows = [], {}
    for line, raw in enumerate(text.splitlines()):
        f = raw.strip().split()
        ctg_id, v, w, _r, s, e = f[0], f[1].split(":"), f[2].split(":"), f[3], int(f[4]), int(f[5])
        assert len(f) == 10
        if ctg_id not in rows:
            rows[ctg_id] = []
            names.append(ctg_id)
        rows[ctg_id].append((rows[ctg_id][0][0] if rows[ctg_id] else len(names) - 1, int(v[0]), 0 if v[1] == "E" else 1, int(w[0]), 0 if w[1] == "E" else 1, s, e, line))
    return [r for n in names for r in rows[n]], names


def tile_rows(text: str):
    from peregrine_amd import _lib
    rows, names = parse_path(text)
    a = np.zeros(len(rows), _lib.TILE_ROW_DTYPE)
    for i, (c, r0, s0, r1, s1, s, e, _line) in enumerate(rows):
        a[i] = (c, r0, r1, s, e, s0, s1, [0, 0])
    return a, names


class Recording:
    """match, with the answers kept in call order (segments() calls it once per row, in contig order)"""

    def __init__(self, match):
        self.match, self.calls = match, []

    def __call__(self, *a):
        self.calls.append(tuple(int(x) for x in self.match(*a)))
        return self.calls[-1]


def segments(db: SeqDB, text: str, match, strict: bool = True):
    """What layout() knows before it paints: per contig ([(row, start, rid, src, length, strand)], ctg_len) -- `length` bytes of read rid's
    strand from byte `src` of the read go to `start` in the contig; row is the row's index in contig order, -1 for the contig's first read
    (whole, at 0); ctg_len is the contig's final length.  match(q_bytes, q_strand, t_bytes, t_strand, band) -> the 8 ovlp_match fields.
    strict: ValueError at a row the reference script raises at or reads out of bounds at (its checks, and e - seg < 0)."""
    rl, ro = db.by_rid()
    rows, names = parse_path(text)
    by_ctg = [[] for _ in names]
    for i, r in enumerate(rows):
        by_ctg[r[0]].append((i, r))
    read = lambda r: db.seqdb[int(ro[r]):int(ro[r]) + int(rl[r])]
    out = []
    for mine in by_ctg:
        _, r0, s0, *_ = mine[0][1]
        segs = [(-1, 0, r0, 0, int(rl[r0]), s0)]
        ctg_len = int(rl[r0])
        for i, (_, r0, s0, r1, s1, s, e, line) in mine:
            l0, l1 = int(rl[r0]), int(rl[r1])
            if l0 < H or abs(e - s) + H > l1:
                raise ValueError(f"row {line}")
            m = match(read(r0)[l0 - H:], s0, read(r1)[l1 - abs(e - s) - H:], s1, BAND)
            t_m_end, q_m_end = m[6], m[7]
            if s1:
                s, e = l1 - s, l1 - e
            seg = e - s + H - t_m_end
            if e <= s or (strict and e - seg < 0):
                raise ValueError(f"row {line}")
            start = ctg_len - H + q_m_end
            segs.append((i, start, r1, e - seg, seg, s1))
            ctg_len = start + seg
        out.append((segs, ctg_len))
    return out


KINDS = ("source", "start", "end")   # e - seg < 0; a segment that starts before its contig; one that ends beyond its contig's end


def offences(db: SeqDB, text: str, match):
    """[(row in contig order, kind)], ascending: every row layout() cannot lay out, and why.  The contig's first read counts for the
    contig's first row; of two kinds on one row the earlier in KINDS stands."""
    bad = {}
    for segs, ctg_len in segments(db, text, match, strict=False):
        first = segs[1][0]
        for row, start, _rid, src, n, _st in segs:
            i = first if row < 0 else row
            kinds = [src < 0 and row >= 0, n > 0 and start < 0, n > 0 and start >= 0 and start + n > ctg_len]
            for k in (k for k in range(3) if kinds[k]):
                bad[i] = min(bad.get(i, k), k)
    return [(i, KINDS[k]) for i, k in sorted(bad.items())]


def paint(db: SeqDB, names, segs) -> bytes:
    """the FASTA of segments()'s answer: every segment copied in row order, later ones over earlier ones, over a background of N"""
    rl, ro = db.by_rid()
    out = []
    for name, (sg, ctg_len) in zip(names, segs):
        ctg = np.full(max(ctg_len, 0), ord("N"), np.uint8)
        for row, start, rid, src, n, st in sg:
            if n and (start < 0 or start + n > ctg_len):
                raise ValueError("a segment outside its contig (row %d in contig order)" % row)
            b = db.seqdb[int(ro[rid]) + src:int(ro[rid]) + src + n]
            ctg[start:start + n] = BASES[(b >> 4) if st else (b & 15)]
        out.append(b">" + name.encode() + b"\n" + ctg.tobytes() + b"\n")
    return b"".join(out)


def layout(db: SeqDB, text: str, match) -> bytes:
    """The FASTA of a tiling path, stated with numpy: match(q_bytes, q_strand, t_bytes, t_strand, band) -> the 8 ovlp_match fields.
    Raises ValueError where the reference script raises or reads out of bounds."""
    return paint(db, parse_path(text)[1], segments(db, text, match))


def fasta_of(data: bytes, off, names) -> bytes:
    """the FASTA text of pgx_contigs_resident's (bytes, offsets)"""
    return b"".join(b">" + n.encode() + b"\n" + data[int(off[c]):int(off[c + 1])] + b"\n" for c, n in enumerate(names))


# ---- a short-read set and tiling paths of any size, valid by the statement above (tests/test_contig_paths.py holds the conditions) -------
_COMP = np.array([3, 2, 1, 0], np.uint8)


def encode(codes) -> np.ndarray:
    """2-bit codes of a read's forward strand -> its seqdb bytes (low nibble: the base, high nibble: the reverse complement's)"""
    codes = np.asarray(codes, np.uint8)
    return ((np.uint8(1) << codes) | ((np.uint8(8) >> codes[::-1]) << np.uint8(4))).astype(np.uint8)


def db_of(reads) -> SeqDB:
    """reads: a list of seqdb byte arrays, rid = position"""
    rlen = np.array([len(r) for r in reads], np.uint32)
    roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
    return SeqDB(np.concatenate(reads), np.arange(len(reads), dtype=np.uint32), rlen, roff, None)


class ReadSet:
    """db, and what the simulation knows: gpos[i][j] = the genome position of base j of read i's strand 0 (an inserted base: that of the
    base in front of it; descending for a read drawn from the genome's reverse strand), n_rids = the reads with planted ambiguous bases"""

    def __init__(self, db, gpos, n_rids):
        self.db, self.gpos, self.n_rids = db, gpos, n_rids

    def oriented(self, node):
        g = self.gpos[node[0]]
        return g[::-1] if node[1] else g


def short_read_db(seed: int, n_reads: int = 3000, genome_len: int = 200_000, err: float = 0.01, n_exact: int = 120, n_near: int = 60,
                  plant_n: bool = False) -> ReadSet:
    """~15x of a random genome in reads of 500 .. 1,500 bases, n_exact of them of exactly 500 (the shortest the layout takes) and n_near of
    500 .. 520; simreads' error model (per base, with probability err: one of 4 substitutions, a deletion, 4 insertions).  plant_n: ~2 % of
    the reads get ambiguous bases -- at the read's start, mid-read plus its last base on strand 0 only, a run of 40, one base of strand 0."""
    rng = np.random.Generator(np.random.PCG64(seed))
    genome = rng.integers(0, 4, genome_len, dtype=np.uint8)
    lens = np.concatenate([np.full(n_exact, H), rng.integers(H, H + 21, n_near), rng.integers(H, 1501, n_reads - n_exact - n_near)])
    lens = lens[rng.permutation(n_reads)]
    reads, gpos = [], []
    for ln in lens:
        n = int(ln) + 60                                   # (1 % deletions of 560 .. 1,560 bases never take 60)
        g0 = int(rng.integers(0, genome_len - n))
        kind = np.where(rng.random(n) < err, rng.integers(0, 9, n), -1)
        base = np.where((kind >= 0) & (kind < 4), kind, genome[g0:g0 + n]).astype(np.uint8)
        emit = np.ones(n, np.int64)
        emit[kind == 4], emit[kind >= 5] = 0, 2
        pos = np.cumsum(emit) - emit
        codes, gp = np.empty(int(emit.sum()), np.uint8), np.empty(int(emit.sum()), np.int64)
        keep, ins = emit > 0, kind >= 5
        codes[pos[keep]], gp[pos[keep]] = base[keep], g0 + np.flatnonzero(keep)
        codes[pos[ins] + 1], gp[pos[ins] + 1] = kind[ins] - 5, g0 + np.flatnonzero(ins)
        codes, gp = codes[:ln], gp[:ln]
        if rng.integers(0, 2):
            codes, gp = _COMP[codes[::-1]], gp[::-1]
        reads.append(encode(codes))
        gpos.append(gp)
    n_rids = []
    if plant_n:
        n_rids = sorted(int(r) for r in rng.choice(n_reads, n_reads // 50, replace=False))
        for j, r in enumerate(n_rids):
            e, n = reads[r], len(reads[r])
            both = {0: [0, 1, 2], 1: [n // 2 + 7], 2: list(range(n // 3, n // 3 + 40)), 3: []}[j % 4]
            fwd = {0: [], 1: [n - 1], 2: [], 3: [int(rng.integers(0, n))]}[j % 4]
            for p in both:
                e[p] &= 0xF0
                e[n - 1 - p] &= 0x0F
            for p in fwd:
                e[p] &= 0xF0
    return ReadSet(db_of(reads), gpos, n_rids)


def dovetails(rs: ReadSet, rng, lo: int, hi: int, per_node: int):
    """[(v, w, x)]: true dovetails by the genome positions -- nodes (rid, strand) that run in the same direction, w reaching lo .. hi genome
    bases beyond v's end; w's bases from x on lie beyond v's last base (500 <= x < |w|: the row of the edge is valid)"""
    n = rs.db.n_reads
    out = []
    for d in (1, -1):
        st = np.array([0 if (g[-1] - g[0]) * d > 0 else 1 for g in rs.gpos])      # the strand of each read that runs in direction d
        endc = np.array([d * int(rs.oriented((j, st[j]))[-1]) for j in range(n)])
        order = np.argsort(endc, kind="stable")
        sorted_end = endc[order]
        for i in range(n):
            a, b = np.searchsorted(sorted_end, [endc[i] + lo, endc[i] + hi + 1])
            cand = order[a:b]
            for j in (cand if len(cand) <= per_node else rng.choice(cand, per_node, replace=False)):
                j = int(j)
                x = int(np.searchsorted(d * rs.oriented((j, st[j])), endc[i], side="right"))
                if j != i and H <= x < int(rs.db.rlen[j]):
                    out.append(((i, int(st[i])), (j, int(st[j])), x))
    return out


def edge_row(v, w, x, lw):
    """(v, w, s, e) of the tiling-path row that appends w's bases from x on (make_golden_contigs.row)"""
    return (v, w, x, lw) if w[1] == 0 else (v, w, lw - x, 0)


def row_text(ctg, v, w, s, e, kind="x") -> str:
    return "%s %d:%s %d:%s %d %d %d %d 99.9 0 %s" % (ctg, v[0], "EB"[v[1]], w[0], "EB"[w[1]], w[0], s, e, abs(e - s), kind)


class _Geometry:
    """a row's (q_m_end, seg, valid) by the statement, every alignment computed once"""

    def __init__(self, db, match):
        self.db, self.match, self.known = db, match, {}
        self.rl, self.ro = db.by_rid()

    def __call__(self, v, w, s, e):
        key = (v, w, s, e)
        if key not in self.known:
            rl, ro, seq = self.rl, self.ro, self.db.seqdb
            l0, l1, span = int(rl[v[0]]), int(rl[w[0]]), abs(e - s)
            if l0 < H or span + H > l1:
                self.known[key] = (0, 0, False)
            else:
                m = self.match(seq[int(ro[v[0]]) + l0 - H:int(ro[v[0]]) + l0], v[1], seq[int(ro[w[0]]) + l1 - span - H:int(ro[w[0]]) + l1], w[1], BAND)
                if w[1]:
                    s, e = l1 - s, l1 - e
                seg = e - s + H - m[6]
                self.known[key] = (int(m[7]), int(seg), e > s and e - seg >= 0)
        return self.known[key]


class _Contig:
    """rows accepted one by one: never a row the statement rejects, never a non-empty segment in front of the contig"""

    def __init__(self, geom, first_len):
        self.geom, self.rows, self.ctg_len, self.max_end = geom, [], first_len, first_len

    def add(self, row) -> bool:
        q, seg, ok = self.geom(*row)
        start = self.ctg_len - H + q
        if not ok or (seg > 0 and start < 0) or start + seg < H:
            return False
        self.rows.append(row)
        self.ctg_len = start + seg
        if seg > 0:
            self.max_end = max(self.max_end, self.ctg_len)
        return True

    def pop(self, state):
        self.rows.pop()
        self.ctg_len, self.max_end = state

    @property
    def whole(self) -> bool:   # no segment ends beyond the contig's end
        return self.ctg_len >= self.max_end


TILE = 4096


def random_path(rs: ReadSet, seed: int, match, min_rows: int = 20_500, min_mixed: int = 1_700, n_single: int = 320, n_dense: int = 6,
                window: int = 6) -> str:
    """A tiling path over rs, valid by the statement (no row of it is one layout() raises at): contigs of 8 .. 16 rows that mix
      short   true dovetails with 1 .. 40 bases of overhang        long    true dovetails with 41 .. 900
      arb     unrelated but valid rows (make_golden_contigs.arbitrary: s' >= 500, span >= 600)
      self    a read against itself (seg == 0)                      amb     a row whose v or w has planted ambiguous bases (if rs has any)
    then n_single one-row contigs whose first read has exactly 500 bases, consecutive in contig order (several whole contigs per 4 KiB of
    output), n_dense contigs of 60 short dovetails (tens of segments per 4 KiB), and for each length 1 .. 7 a contig that steers a segment of
    that length onto a 4 KiB boundary of the concatenated output with unrelated rows of known step in front of it.  Contigs whose row count
    can end on a multiple of 256 rows do.  In the file the rows of `window` contigs are interleaved line by line; contigs appear in the order
    they were generated in, so the offsets the steering counted on hold."""
    rng = np.random.Generator(np.random.PCG64(seed))
    db, geom = rs.db, _Geometry(rs.db, match)
    rl = db.rlen.astype(np.int64)
    n = db.n_reads
    short = dovetails(rs, rng, 1, 40, 8)
    long_ = dovetails(rs, rng, 41, 900, 2)
    amb_set = set(rs.n_rids)
    amb_edges = [t for t in short + long_ if t[0][0] in amb_set or t[1][0] in amb_set]
    by_v = {}
    for t in short + long_:
        by_v.setdefault(t[0], []).append(t)
    roomy = np.flatnonzero(rl >= 1400)            # targets of the unrelated rows: any span of 600 .. 900 fits behind s' >= 500
    exact = np.flatnonzero(rl == H)
    node = lambda r: (int(r), int(rng.integers(0, 2)))
    as_row = lambda t: edge_row(t[0], t[1], t[2], int(rl[t[1][0]]))

    def arb(v=None, w=None, span=None):
        v, w = v or node(rng.integers(0, n)), w or node(rng.choice(roomy))
        lw = int(rl[w[0]])
        span = span or int(rng.integers(600, lw - H + 1))
        s2 = int(rng.integers(H, lw - span + 1))
        return (v, w, s2, s2 + span) if w[1] == 0 else (v, w, lw - s2, lw - s2 - span)

    def self_row(v=None):
        v = v or node(rng.integers(0, n))
        k = int(rng.integers(1, min(90, int(rl[v[0]]) - H) + 1)) if rl[v[0]] > H else 0
        return edge_row(v, v, int(rl[v[0]]) - k, int(rl[v[0]])) if k else arb(v=v)

    def draw(kind, last_w):
        if kind in ("short", "long"):
            pool = [t for t in by_v.get(last_w, []) if (t[2] + 40 >= rl[t[1][0]]) == (kind == "short")] if last_w and rng.random() < 0.5 else []
            pool = pool or (short if kind == "short" else long_)
            return as_row(pool[int(rng.integers(0, len(pool)))])
        if kind == "self":
            return self_row()
        if kind == "amb" and amb_set:
            if rng.random() < 0.5 and amb_edges:
                return as_row(amb_edges[int(rng.integers(0, len(amb_edges)))])
            r = node(rs.n_rids[int(rng.integers(0, len(rs.n_rids)))])
            return arb(v=r) if rng.random() < 0.5 or rl[r[0]] < 1100 else arb(w=r, span=600)
        return arb()

    def grow(c, rows_wanted, kinds, weights):
        """rows of the given kinds until c has rows_wanted, the last one chosen so that the contig is whole"""
        while len(c.rows) < rows_wanted - 1:
            c.add(draw(kinds[int(rng.choice(len(kinds), p=weights))], c.rows[-1][1] if c.rows else None))
        for attempt in range(200):
            state = (c.ctg_len, c.max_end)
            cand = draw(kinds[int(rng.choice(len(kinds), p=weights))], None) if c.whole and attempt == 0 else arb()
            if c.add(cand):
                if c.whole:
                    return
                c.pop(state)
        raise AssertionError("no row closes the contig")

    kinds = ("short", "long", "arb", "self", "amb")
    weights = np.array([0.33, 0.29, 0.24, 0.05, 0.09 if amb_set else 0.0])
    weights = weights / weights.sum()
    contigs, off, n_rows = [], 0, 0

    def first_of(kind, v=None):
        """a contig from a first row of `kind` (its v is the contig's first read)"""
        for attempt in range(200):
            if v is None:
                row = draw(kind, None)
            elif kind == "self":
                row = self_row(v)
            else:
                row = as_row(by_v[v][int(rng.integers(0, len(by_v[v])))]) if kind != "arb" and by_v.get(v) and attempt < 8 else arb(v=v)
            c = _Contig(geom, int(rl[row[0][0]]))
            if c.add(row):
                return c
        raise AssertionError("no first row")

    def close(c):
        nonlocal off, n_rows
        assert c.whole
        contigs.append(c.rows)
        off += c.ctg_len
        n_rows += len(c.rows)

    def mixed():
        to_edge = 256 - n_rows % 256
        c = first_of(kinds[int(rng.choice(len(kinds), p=weights))])
        grow(c, to_edge if 8 <= to_edge <= 16 else int(rng.integers(8, 17)), kinds, weights)
        close(c)

    def single():
        v = node(exact[int(rng.integers(0, len(exact)))])
        close(first_of("self" if rng.random() < 0.15 else "short", v))   # (whole: _Contig.add takes no row that ends before base 500)

    def dense():
        c = first_of("short")
        grow(c, 60, ("short",), np.array([1.0]))
        close(c)

    pads = {}     # step of ctg_len -> an unrelated row that takes it (a row's seg and step do not depend on the contig it stands in)
    for _ in range(3000):
        r = arb()
        q, seg, ok = geom(*r)
        if ok and seg > 0 and q - H + seg > 0:
            pads.setdefault(q - H + seg, r)
    pad_steps = sorted(pads)

    def steered(length, cut):
        """a contig in which byte `cut` of a `length`-byte segment is the first byte of a tile of the concatenated output: unrelated rows in
        front of it whose steps add up to what is missing (cut == 0 / == length: the segment begins / ends at the boundary)"""
        fit = [as_row(t) for t in short]
        fit = [r for r in fit if geom(*r)[2] and geom(*r)[1] == length and geom(*r)[0] >= H - length]
        assert fit, length
        r = fit[int(rng.integers(0, len(fit)))]
        for _ in range(400):
            c = first_of("arb")
            need = (-cut - (off + c.ctg_len - H + geom(*r)[0])) % TILE
            while need > pad_steps[-1] or need not in pads:
                step = pad_steps[int(rng.integers(0, len(pad_steps)))]
                if not c.add(pads[step]):
                    break
                need = (need - step) % TILE
                if len(c.rows) > 12:
                    break
            if need in pads and c.add(pads[need]) and c.add(r):
                assert (off + c.ctg_len - length + cut) % TILE == 0
                grow(c, len(c.rows) + 2, kinds, weights)
                return close(c)
        raise AssertionError("no rows of the steps wanted")

    plan = ["mixed"] * min_mixed
    for what, count in (("dense", n_dense), ("steered", 1)):
        for _ in range(count):
            plan.insert(int(rng.integers(1, len(plan))), what)
    plan.insert(len(plan) // 3, "single")
    for what in plan:
        if what == "mixed":
            mixed()
        elif what == "dense":
            dense()
        elif what == "single":
            for _ in range(n_single):
                single()
        else:
            for length, cut in [(1, 0), (1, 1)] + [(ln, int(rng.integers(1, ln))) for ln in range(2, 8)]:
                steered(length, cut)
    while n_rows < min_rows:
        mixed()
    # the file: contigs enter in order, the rows of `window` of them interleaved
    short_rows, long_rows = {as_row(t) for t in short}, {as_row(t) for t in long_}

    def kind_of(row):   # the file's last column (no program reads it): what the row is
        k = "self" if row[0] == row[1] else "short" if row in short_rows else "long" if row in long_rows else "arb"
        return k + ("+amb" if row[0][0] in amb_set or row[1][0] in amb_set else "")

    lines, active, nxt = [], [], 0
    while active or nxt < len(contigs):
        if nxt < len(contigs) and len(active) < window:
            active.append([nxt, 0])
            nxt += 1
            a = active[-1]
        else:
            a = active[int(rng.integers(0, len(active)))]
        lines.append(row_text("ctg%05d" % a[0], *contigs[a[0]][a[1]], kind_of(contigs[a[0]][a[1]])))
        a[1] += 1
        if a[1] == len(contigs[a[0]]):
            active.remove(a)
    return "\n".join(lines) + "\n"


# ---- hand-made reads: the error paths of the layout ---------------------------------------------------------------------------------------
def engineered_reads(db: SeqDB | None = None, seed: int = 23):
    """(db + five reads, their rids by name).  X: 500 random bases.
      v     700 random bases + X                      v500  X alone: the shortest first read there is
      w     300 random bases + the first 501 of X[:200] + 49 random bases + X[200:]: the window of a row with |e - s| = 1.  The longest exact
            run of v's (v500's) last 500 bases against it is X[200:452], behind the insertion: q_m_end = 452, t_m_end = 501, so seg = 0 and
            ctg_len steps by 452 - 500 = -48
      u, u2 9,000 random bases each, unrelated to everything"""
    rng = np.random.Generator(np.random.PCG64(seed))
    rand = lambda n: rng.integers(0, 4, n, dtype=np.uint8)
    x = rand(H)
    made = dict(v=np.concatenate([rand(700), x]), v500=x, w=np.concatenate([rand(300), x[:200], rand(49), x[200:]])[:300 + H + 1], u=rand(9000), u2=rand(9000))
    n0 = db.n_reads if db is not None else 0
    reads = ([db.seqdb[int(o):int(o) + int(n)] for o, n in zip(db.roff, db.rlen)] if db is not None else []) + [encode(c) for c in made.values()]
    return db_of(reads), {name: n0 + i for i, name in enumerate(made)}


def pull_back(ids, v="v") -> str:
    """the row (without its contig id) that takes 48 bases off ctg_len and adds nothing"""
    return "%d:E %d:E 0 800 801 0 0 x pull" % (ids[v], ids["w"])


def unrelated(ids, match, db, v="u", w="u2", q_below=H, nth=0) -> str:
    """a row of unrelated engineered reads, valid whatever the match (s >= 500, span >= 600), with q_m_end < q_below and a step of ctg_len
    of at least 100: the nth such span from 600 up, found with the statement"""
    rl, ro = db.by_rid()
    rv, rw = ids[v], ids[w]
    for span in range(600, 2000):
        m = match(db.seqdb[int(ro[rv]) + int(rl[rv]) - H:int(ro[rv]) + int(rl[rv])], 0, db.seqdb[int(ro[rw]) + int(rl[rw]) - span - H:int(ro[rw]) + int(rl[rw])], 0, BAND)
        if m[7] < q_below and m[7] - m[6] + span >= 100:
            if nth == 0:
                return "%d:E %d:E 0 %d %d 0 0 x arb" % (rv, rw, 4000, 4000 + span)
            nth -= 1
    raise AssertionError("no such span")


def assemble(contigs, late=()) -> str:
    """a tiling path of contigs given as lists of rows without contig id: contigs appear in order, the rows of three of them interleaved
    round-robin; a contig in `late` shows its first row in its turn and the rest of its rows at the very end of the file"""
    lines, tail, active, nxt = [], [], [], 0
    while active or nxt < len(contigs):
        while nxt < len(contigs) and len(active) < 3:
            active.append([nxt, 0])
            nxt += 1
        for a in list(active):
            c, i = a
            (tail if c in late and i > 0 else lines).append("e%04d %s" % (c, contigs[c][i]))
            a[1] += 1
            if a[1] == len(contigs[c]):
                active.remove(a)
    return "\n".join(lines + tail) + "\n"


def error_paths(db: SeqDB, ids, fillers, match):
    """[(name, text, (row in contig order, kind), line)]: tiling paths over the engineered reads with exactly the offences named (stated
    here by design; tests/test_contig_paths.py holds them to offences()), between valid filler contigs (lists of rows without contig id, in
    all more than 256 rows).  `line` is the file line of the row a message must name: the smallest offending row in contig order."""
    grow1, grow2 = unrelated(ids, match, db), unrelated(ids, match, db, v="u2", w="u")
    blocks = dict(
        source=([grow1, "%d:E %d:E 0 10 700 0 0 x bad" % (ids["v"], ids["u"])], 1),                 # seg > 1,000 > e = 700
        start=([pull_back(ids, "v500"), unrelated(ids, match, db, q_below=40)], 1),                  # ctg_len = 452: 452 - 500 + q_m_end < 0
        end_first=([pull_back(ids)], 0),                                                             # ctg_len = 1,200 - 48 < the first read
        end=([grow1, grow2, pull_back(ids)], 1),                                                     # row 1 ends 48 bases beyond the end
    )
    assert sum(len(f) for f in fillers) > 256 and len(fillers) >= 8
    few, cases = fillers[:3], []

    def case(name, contigs, late=()):
        """contigs: filler row lists and block names; the expected row is that of the first block in contig order"""
        lists, want, n = [], None, 0
        for c in contigs:
            rows, bad = (c, None) if isinstance(c, list) else blocks[c]
            if bad is not None and want is None:
                want = (n + bad, c.split("_")[0])
            lists.append(rows)
            n += len(rows)
        text = assemble(lists, late)
        line = [r[7] for r in parse_path(text)[0]][want[0]]
        cases.append((name, text, want, line))

    for kind in blocks:
        case(kind + " alone", few + [kind] + fillers[3:6])
    for kind in ("source", "start", "end"):
        case("two of " + kind + " far apart", few + [kind] + fillers + [kind])
        case("two of " + kind + " far apart, the first one's line last", [kind] + fillers + [kind], late=(0,))
    case("two contigs, an offence each", few + ["start", "end_first"] + fillers[3:6])
    case("two contigs, an offence each, the other way round", few + ["end_first", "start"] + fillers[3:6], late=(3,))
    case("start at a small row, source at a large one", few + ["start"] + fillers + ["source"])
    case("end at a small row, source at a large one", few + ["end"] + fillers + ["source"])
    case("first read's end at a small row, source at a large one", ["end_first"] + fillers + ["source"], late=())
    return cases


class Case:
    """a read set, its random path, and the statement's answer to it over `match`, computed once per process"""

    def __init__(self, plant_n, match):
        self.rs = short_read_db(101, plant_n=plant_n)
        self.db = self.rs.db
        self.text = random_path(self.rs, 7, match)
        self.rows, self.names = parse_path(self.text)
        rec = Recording(match)
        self.segs = segments(self.db, self.text, rec)
        self.matches = rec.calls                                       # per row in contig order
        self.fasta = paint(self.db, self.names, self.segs)
        self.first_row = [sg[1][0] for sg, _ in self.segs] + [len(self.rows)]
        self.ctg_off = np.concatenate([[0], np.cumsum([n for _, n in self.segs])]).astype(np.int64)
        # the segments in the device's numbering k = row + contig + 1: (dst in the concatenated output, absolute source byte, length, contig)
        _, ro = self.db.by_rid()
        self.flat = np.array([(self.ctg_off[c] + start, int(ro[rid]) + src, n, c) for c, (sg, _) in enumerate(self.segs) for _, start, rid, src, n, _ in sg],
                             np.int64)


@functools.lru_cache(maxsize=None)
def case(plant_n: bool) -> Case:
    import oracle_util as U
    return Case(plant_n, U.orc_ovlp_match)


def filler_contigs(c: Case, n_rows: int = 300):
    """the first contigs of the random path as lists of rows without contig id, until they hold more than n_rows rows"""
    by, out, n = {}, [], 0
    for ln in c.text.splitlines():
        cid, body = ln.split(" ", 1)
        by.setdefault(cid, []).append(body)
    for name in c.names:
        out.append(by[name])
        n += len(by[name])
        if n > n_rows:
            return out
