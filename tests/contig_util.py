"""Shared by tests/golden/make_golden_contigs.py and the contig-layout tests: the fixture's read set (simreads by seed plus planted
ambiguous bases), the tiling-path parser, and a numpy statement of what py/scripts/path_to_contig.py computes over any ovlp_match."""
from __future__ import annotations

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
        rows[ctg_id].append((names.index(ctg_id), int(v[0]), 0 if v[1] == "E" else 1, int(w[0]), 0 if w[1] == "E" else 1, s, e, line))
    return [r for n in names for r in rows[n]], names


def tile_rows(text: str):
    from peregrine_amd import _lib
    rows, names = parse_path(text)
    a = np.zeros(len(rows), _lib.TILE_ROW_DTYPE)
    for i, (c, r0, s0, r1, s1, s, e, _line) in enumerate(rows):
        a[i] = (c, r0, r1, s, e, s0, s1, [0, 0])
    return a, names


def layout(db: SeqDB, text: str, match) -> bytes:
    """The FASTA of a tiling path, stated with numpy: match(q_bytes, q_strand, t_bytes, t_strand, band) -> the 8 ovlp_match fields.
    Raises ValueError where the reference script raises or reads out of bounds."""
    rl, ro = db.by_rid()
    rows, names = parse_path(text)
    out = []
    for c, name in enumerate(names):
        mine = [r for r in rows if r[0] == c]
        _, r0, s0, *_ = mine[0]
        read = lambda r: db.seqdb[int(ro[r]):int(ro[r]) + int(rl[r])]
        nib = lambda b, st: (b >> 4) if st else (b & 15)
        segs = [(0, BASES[nib(read(r0), s0)])]
        ctg_len = int(rl[r0])
        for _, r0, s0, r1, s1, s, e, line in mine:
            l0, l1 = int(rl[r0]), int(rl[r1])
            if l0 < H or abs(e - s) + H > l1:
                raise ValueError(f"row {line}")
            m = match(read(r0)[l0 - H:], s0, read(r1)[l1 - abs(e - s) - H:], s1, BAND)
            t_m_end, q_m_end = m[6], m[7]
            if s1:
                s, e = l1 - s, l1 - e
            seg = e - s + H - t_m_end
            if e <= s or e - seg < 0:
                raise ValueError(f"row {line}")
            start = ctg_len - H + q_m_end
            segs.append((start, BASES[nib(read(r1)[e - seg:e], s1)]))
            ctg_len = start + seg
        ctg = np.full(ctg_len, ord("N"), np.uint8)
        for start, b in segs:
            if len(b) and (start < 0 or start + len(b) > ctg_len):
                raise ValueError("a segment outside its contig")
            ctg[start:start + len(b)] = b
        out.append(b">" + name.encode() + b"\n" + ctg.tobytes() + b"\n")
    return b"".join(out)


def fasta_of(data: bytes, off, names) -> bytes:
    """the FASTA text of pgx_contigs_resident's (bytes, offsets)"""
    return b"".join(b">" + n.encode() + b"\n" + data[int(off[c]):int(off[c + 1])] + b"\n" for c, n in enumerate(names))
