"""The FASTA/FASTQ record grammar that the read-database builder (pgx_reads.hip) evaluates, twice, in plain Python.
TEST INFRASTRUCTURE.

kseq_loop_q: the byte-at-a-time reader of fasta_util.kseq_loop extended by the '+' branch of the reference's kseq reader (its buffer of
             KS_BUF bytes included).  It reads every text; a record the reader calls truncated ends the file's records.
parse_reads: the grammar as the kernels state it -- predicates of a byte or a line, prefix sums, one successor function, and the chain
             from line 0 under it.  Raises Refused("cr", offset) for the one class it does not evaluate: an empty line inside a quality
             block at which the reader's strip of one trailing '\\r' from the ACCUMULATED string removes a byte (offset: that line's).
Both answer (names, seqs) of one file, possibly empty.  reads_of_files: the records of several files, in order."""
from __future__ import annotations

from bisect import bisect_left

import numpy as np

from fasta_util import KS_BUF, MARKERS, SPACE, Refused, _Stream, biseq, files_of  # noqa: F401

STOPS = b">+@"


def kseq_loop_q(b: bytes):
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
            c = ks.getc()
            if c == -1 or c in STOPS:
                break
            if c == 0x0A:
                continue
            seq.append(c)
            ks.getuntil(b"\n", seq, True)
        if c != -1 and c in MARKERS:
            last = c
        if c == 0x2B:
            c = ks.getc()
            while c != -1 and c != 0x0A:
                c = ks.getc()
            if c == -1:
                break   # no quality string
            qual = bytearray()
            while True:
                got, _ = ks.getuntil(b"\n", qual, True)
                if got < 0 or len(qual) >= len(seq):
                    break
            last = 0
            if len(qual) != len(seq):
                break   # truncated, or longer than the sequence
        names.append(bytes(name))
        seqs.append(bytes(seq))
        if c == -1:
            break
    return names, seqs


def parse_reads(b: bytes):
    n = len(b)
    eof_seen = n % KS_BUF != 0
    m0 = min((i for i in range(n) if b[i] in MARKERS), default=None)
    if m0 is None:
        return [], []
    start = [m0] + [i for i in range(m0 + 1, n) if b[i - 1] == 0x0A]
    L = len(start)
    text_end = n - 1 if b[n - 1] == 0x0A else n
    end = [s - 1 for s in start[1:]] + [text_end]
    term = [True] * (L - 1) + [b[n - 1] == 0x0A]
    length = [e - s for s, e in zip(start, end)]
    fm = [min((i for i in range(s, e) if b[i] in MARKERS), default=None) for s, e in zip(start, end)]
    stop = [ln > 0 and b[s] in STOPS for s, ln in zip(start, length)]
    K = [ln - 1 if ln and b[e - 1] == 0x0D else ln for ln, e in zip(length, end)]
    lone = [ln == 1 and b[s] == 0x0D for s, ln in zip(start, length)]
    PS = [0]
    for k in K:
        PS.append(PS[-1] + k)
    stops = [j for j in range(L) if stop[j]]
    full = [j for j in range(L) if length[j]]
    marked = [j for j in range(L) if fm[j] is not None]
    # an empty line at which the reader's strip can take a byte of an earlier line: the line in front of it is all '\r', or ends "\r\r"
    susp = [j for j in range(1, L) if length[j] == 0 and (all(x == 0x0D for x in b[start[j - 1]:end[j - 1]]) or b[start[j - 1]:end[j - 1]].endswith(b"\r\r"))]

    def nxt(lst, j):   # the first entry >= j, or L
        i = bisect_left(lst, j)
        return lst[i] if i < len(lst) else L

    def first_adj(lo, hi):   # 1: the first non-empty line in [lo, hi) is exactly "\r" (K counted it as 0, the reader keeps it)
        f = nxt(full, lo)
        return (1, f) if f < hi and lone[f] else (0, L)

    END, BADREC, NOREC = L, L + 1, L + 2

    def successor(j):
        """(the record's sequence lines end in front of line k | None: no record, the successor)"""
        if eof_seen and fm[j] == n - 1:
            return None, NOREC
        k = nxt(stops, j + 1)
        if k == L:
            return k, END
        if b[start[k]] in MARKERS:
            return k, k
        if not term[k]:
            return None, BADREC
        slen = PS[k] - PS[j + 1] + first_adj(j + 1, k)[0]
        q0 = k + 1
        if q0 >= L:
            return (k, END) if slen == 0 else (None, BADREC)
        adj, f = first_adj(q0, L)

        def kept(m):   # of the lines q0 .. m
            return PS[m + 1] - PS[q0] + (adj if f <= m else 0)
        lo, hi = q0, L   # the smallest m with kept(m) >= slen
        while lo < hi:
            mid = (lo + hi) // 2
            if kept(mid) >= slen:
                hi = mid
            else:
                lo = mid + 1
        m = lo
        if m == L:
            return None, BADREC
        i = bisect_left(susp, q0 + 1)
        if i < len(susp) and susp[i] <= m:   # the reader's own sum over these lines, a line at a time
            ln = tail = 0   # of the accumulated string: its length, its trailing '\r's
            for t in range(q0, m + 1):
                line = b[start[t]:end[t]]
                cr = len(line) - len(line.rstrip(b"\r"))
                tail = tail + cr if cr == len(line) else cr
                ln += len(line)
                if ln > 1 and tail:
                    if not line:
                        raise Refused("cr", start[t])
                    ln, tail = ln - 1, tail - 1
        if kept(m) != slen:
            return None, BADREC
        return k, nxt(marked, m + 1)

    names, seqs = [], []
    j = 0
    while j < L:
        k, j_next = successor(j)
        if k is not None:
            h = fm[j]
            i = h + 1
            while i < n and b[i] not in SPACE:
                i += 1
            names.append(b[h + 1:i])
            seq, first = b"", True
            for t in range(j + 1, k):
                if length[t]:
                    line = b[start[t]:end[t]]
                    if line[-1] == 0x0D and not (len(line) == 1 and (first or (end[t] == n and eof_seen))):
                        line = line[:-1]
                    seq, first = seq + line, False
            seqs.append(seq)
        j = j_next
    return names, seqs


def reads_of_files(texts, parse=kseq_loop_q):
    names, seqs = [], []
    for t in texts:
        nm, sq = parse(t)
        names += nm
        seqs += sq
    return names, seqs


def answer(fn, text):
    try:
        return fn(text)
    except Refused as r:
        return (r.kind, r.offset)


def random_texts(count: int = 300, seed: int = 20261021):
    """texts of 0 to 400 bytes over an alphabet weighted towards '\\n', '\\r', '>', '@' and '+'; every third one is a run of FASTQ records
    with such bytes thrown in, so that whole quality blocks are read"""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"\n\n\n\n\n\n\n\r\r>>@@++++  \tACGTNACGTNACGTNacgtRYI5x1", np.uint8)
    acgt = np.frombuffer(b"ACGTacgtN", np.uint8)
    qual = np.frombuffer(b"I5@>+!~FF:,", np.uint8)
    out = []
    for k in range(count):
        n = int(rng.integers(0, 401))
        if k % 3 == 2:
            t = bytearray()
            r = 0
            while len(t) < n:
                ln = int(rng.integers(0, 12))
                nl = b"\r\n" if rng.integers(0, 5) == 0 else b"\n"
                s, q = acgt[rng.integers(0, len(acgt), ln)].tobytes(), qual[rng.integers(0, len(qual), ln)].tobytes()
                if ln > 3 and rng.integers(0, 3) == 0:   # two lines each
                    s, q = s[:2] + nl + s[2:], q[:3] + nl + q[3:]
                t += b"@r%d c" % r + nl + s + nl + b"+" + nl + q + nl
                r += 1
            for _ in range(int(rng.integers(0, 3)) if t else 0):   # damage
                i = int(rng.integers(0, len(t)))
                t[i] = alphabet[rng.integers(0, len(alphabet))]
            t = t[:max(n, 1)] if rng.integers(0, 2) else t
        else:
            t = bytearray(alphabet[rng.integers(0, len(alphabet), n)].tobytes())
            if k % 4 and n:
                t[0] = ord("@")
        out.append(bytes(t))
    return out


def padded_texts():
    """damaged FASTQ/FASTA texts grown to 16,384, 16,385 and 32,768 bytes (the reader's buffer): what the end of the input does"""
    tails = [b"@e\nAC\n+\nII\n", b"@e\nAC\n+\nII", b"@e\nAC\n+\nI\n\r", b"@e\nAC\n+\nI\r\n", b"@e\nAC\n+\n", b"@e\nAC\n+", b"@e\nAC\n\r", b"@e\nAC\n@",
             b"@e\nAC\n+\nII\n>", b"@e\n\n+\n", b"@e\nAC\n+\nII\nxx@", b">e\nAC\n>f", b"@e\nAC\n+\nI\n", b"@e\nA\r\n+\nI\r", b"@e\n\r\n+\n\r"]
    rec = b"@r\nACGTACGTAC\n+\nIIIIIIIIII\n"
    out = []
    for size in (KS_BUF, KS_BUF + 1, 2 * KS_BUF):
        for tl in tails:
            body = rec * (size // len(rec) + 1)
            pad = size - len(tl)
            cut = (pad // len(rec)) * len(rec)
            filler = b">f\n" + b"A" * (pad - cut - 4) + b"\n" if pad - cut >= 4 else b"\n" * (pad - cut)
            t = body[:cut] + filler + tl
            assert len(t) == size, (len(t), size)
            out.append(t)
    return out
