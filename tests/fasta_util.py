"""The FASTA record grammar that pgx_seqdb_from_fasta evaluates, twice, in plain Python.  TEST INFRASTRUCTURE.

parse_fasta: the grammar as the kernels state it -- per-byte and per-line predicates and sums, no reader state.
kseq_loop:   a byte-at-a-time reader, written from the loop of the reference's kseq reader (its buffer of KS_BUF bytes included: the
             reader learns of the end of its input only from a refill that comes back short).
Both answer (names, seqs): lists of bytes in record order, or raise Refused(kind, offset).
biseq / files_of: the two-strand encoding and the two files shmr_mkseqdb writes of such records."""
from __future__ import annotations

import numpy as np

KS_BUF = 16384
MARKERS = b">@"
SPACE = b" \t\n\v\f\r"


class Refused(ValueError):
    def __init__(self, kind: str, offset: int = -1):
        super().__init__(f"{kind} at {offset}" if offset >= 0 else kind)
        self.kind, self.offset = kind, offset


def parse_fasta(b: bytes):
    n = len(b)
    eof_seen = n % KS_BUF != 0
    m0 = min((i for i in range(n) if b[i] in MARKERS), default=None)
    if m0 is None or (m0 == n - 1 and eof_seen):
        raise Refused("no record")
    starts = [m0] + [i for i in range(m0 + 1, n) if b[i - 1] == 0x0A]
    plus = [i for i in starts[1:] if b[i] == 0x2B]
    if plus:
        raise Refused("fastq", min(plus))
    text_end = n - 1 if b[n - 1] == 0x0A else n
    ends = [s - 1 for s in starts[1:]] + [text_end]
    names, seqs = [], []
    first_of_record = False
    for j, (s, e) in enumerate(zip(starts, ends)):
        header = j == 0 or (e > s and b[s] in MARKERS)
        if header:
            if s == n - 1 and eof_seen:
                continue   # ends the previous record, starts none
            i = s + 1
            while i < n and b[i] not in SPACE:
                i += 1
            names.append(b[s + 1:i])
            seqs.append(b"")
            first_of_record = True
        elif e > s:
            line = b[s:e]
            lone = len(line) == 1
            if line[-1] == 0x0D and not (lone and (first_of_record or (e == n and eof_seen))):
                line = line[:-1]
            seqs[-1] += line
            first_of_record = False
    return names, seqs


class _Stream:
    """the reader's buffered stream: getc, and getuntil with its early return at a known end of input"""

    def __init__(self, b: bytes):
        self.b, self.pos = b, 0          # pos: where the next refill reads from
        self.buf, self.begin, self.is_eof = b"", 0, False

    def _refill(self) -> bool:
        self.buf, self.begin = self.b[self.pos:self.pos + KS_BUF], 0
        self.pos += len(self.buf)
        if len(self.buf) < KS_BUF:
            self.is_eof = True
        return len(self.buf) > 0

    def offset(self) -> int:   # of the next byte
        return self.pos - len(self.buf) + self.begin

    def getc(self) -> int:
        if self.begin >= len(self.buf):
            if self.is_eof or not self._refill():
                return -1
        c = self.buf[self.begin]
        self.begin += 1
        return c

    def getuntil(self, delims, out: bytearray, is_line: bool):
        """appends up to a byte of delims; returns (-1 | len(out), the delimiter met or 0)"""
        if self.begin >= len(self.buf) and self.is_eof:
            return -1, 0
        met = 0
        while True:
            if self.begin >= len(self.buf):
                if self.is_eof or not self._refill():
                    break
            i = self.begin
            while i < len(self.buf) and self.buf[i] not in delims:
                i += 1
            out += self.buf[self.begin:i]
            self.begin = i + 1
            if i < len(self.buf):
                met = self.buf[i]
                break
        if is_line and len(out) > 1 and out[-1] == 0x0D:
            del out[-1]
        return len(out), met


def kseq_loop(b: bytes):
    ks, last = _Stream(b), 0
    names, seqs = [], []
    while True:
        if last == 0:
            c = ks.getc()
            while c != -1 and c not in MARKERS:
                c = ks.getc()
            if c == -1:
                break
            last = c
        name = bytearray()
        got, c = ks.getuntil(SPACE, name, False)
        if got < 0:
            break
        if c != 0x0A:
            ks.getuntil(b"\n", bytearray(), True)
        seq = bytearray()
        while True:
            at = ks.offset()
            c = ks.getc()
            if c == -1 or c in b">+@":
                break
            if c == 0x0A:
                continue
            seq.append(c)
            ks.getuntil(b"\n", seq, True)
        if c == 0x2B:
            raise Refused("fastq", at)
        last = c if c != -1 and c in MARKERS else 0
        names.append(bytes(name))
        seqs.append(bytes(seq))
        if c == -1:
            break
    if not names:
        raise Refused("no record")
    return names, seqs


_FWD = np.zeros(256, np.uint8)
_REV = np.zeros(256, np.uint8)
for _c, _f, _r in ((b"Aa", 1, 8), (b"Cc", 2, 4), (b"Gg", 4, 2), (b"Tt", 8, 1)):
    for _x in _c:
        _FWD[_x], _REV[_x] = _f, _r


def biseq(seq: bytes) -> np.ndarray:
    s = np.frombuffer(seq, np.uint8)
    return (_REV[s[::-1]] << 4 | _FWD[s]).astype(np.uint8)


def files_of(names, seqs):
    """(.seqdb bytes, .idx bytes) as shmr_mkseqdb writes them"""
    idx, off = [], 0
    for r, (nm, s) in enumerate(zip(names, seqs)):
        idx.append(b"%09d %s %d %d\n" % (r, nm, len(s), off))
        off += len(s)
    db = np.concatenate([biseq(s) for s in seqs]) if seqs else np.zeros(0, np.uint8)
    return db.tobytes(), b"".join(idx)


def random_texts(count: int = 300, seed: int = 20261020):
    """texts of 0 to 400 bytes over an alphabet weighted towards '\\n', '\\r', '>', '@', blank and ACGTN, none with a line-start '+'"""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"\n\n\n\n\n\n\r\r\r>>>@@  \tACGTNACGTNACGTNacgtRY+x1", np.uint8)
    out = []
    for k in range(count):
        n = int(rng.integers(0, 401))
        t = bytearray(alphabet[rng.integers(0, len(alphabet), n)].tobytes())
        if k % 4 and n:
            t[0] = ord(">")   # (most texts start with a header, so that most hold several records)
        for i in range(n):
            if t[i] == 0x2B and (i == 0 or t[i - 1] == 0x0A):
                t[i] = ord("A")
        out.append(bytes(t))
    return out
