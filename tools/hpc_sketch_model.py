#!/usr/bin/env python3
"""The rule behind pgx_sketch_hpc.hip, as a Python model checked against the compiled reference (CPU only, about a minute):

    mm_sketch(is_hpc = 1) makes one iteration per maximal run of equal unambiguous bases (decided on codes: `a` and `A` are one run) and one
    per ambiguous base.  A run pushes its length (the queue is cleared by an ambiguous base), shifts its code into both k-mers (never
    flushed), and -- unless the k-mer is its own reverse complement, which makes no entry and does not advance `l` -- is an ENTRY:
    finite iff l >= k and span < 256, key x = hash << 8 | span with span the sum of the last k run lengths, y = rid << 32 | i << 1 | strand
    with i the raw index of the run's last base.  An ambiguous base sets l = 0 and is one infinite entry.  Every comparison is on the
    whole x.

    1. a read without ambiguous bases = the closed form of pgx_sketch_fast.hip over its entries with l >= k, those with span >= 256 as
       keys of 2^64 - 1 that take part in every window and are never emitted;
    2. a read with ambiguous bases = for every segment (a maximal stretch of entries with l >= k) in order: that closed form WITHOUT its
       last element iff the rightmost smallest of the segment's last w entries is finite; then the rightmost smallest of the last w
       stream entries of the whole read (infinite ones included), if finite.
    (2 contains 1: a read without ambiguous bases is one segment.)

`machine` is a transcription of the loop, `sketch` the restatement the kernels implement.  Both against oracle/_ref/libshimmer_ref.so on
4,000 adversarial strings (runs of 120 to 300 bases, ambiguous bases, mixed case, tandem repeats of period 2 to 8), w in {3, 5, 24, 80},
k in {4, 6, 12, 16}.  Result of the committed run: 4000 trials, 0 mismatches of either.   usage: python tools/hpc_sketch_model.py [trials]"""
import ctypes as C
import os
import sys

import numpy as np

INF = (1 << 64) - 1
CODE = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3, 85: 3, 117: 3, 0: 0, 1: 1, 2: 2, 3: 3}   # src/mm_sketch.c:10-21


def hash64(key, mask):
    key = (~key + (key << 21)) & mask
    key = key ^ key >> 24
    key = ((key + (key << 3)) + (key << 8)) & mask
    key = key ^ key >> 14
    key = ((key + (key << 2)) + (key << 4)) & mask
    key = key ^ key >> 28
    key = (key + (key << 31)) & mask
    return key


def stream(seq, k):
    """the machine's entries in order: (x or INF, position << 1 | strand, segment or -1).  Segment s >= 0: an entry with l >= k, after s
    ambiguous bases."""
    n, i, mask, top = len(seq), 0, (1 << 2 * k) - 1, 2 * (k - 1)
    fwd = rev = l = seg = 0
    runs, out = [], []
    while i < n:
        c = CODE.get(seq[i], 4)
        if c < 4:
            j = i
            while j + 1 < n and CODE.get(seq[j + 1], 4) == c:
                j += 1
            runs.append(j - i + 1)
            i = j
            if len(runs) > k:
                runs.pop(0)
            span = sum(runs)
            fwd = (fwd << 2 | c) & mask
            rev = (rev >> 2) | ((3 ^ c) << top)
            if fwd != rev:
                z = 0 if fwd < rev else 1
                l += 1
                if l >= k:
                    out.append(((hash64((fwd, rev)[z], mask) << 8 | span) if span < 256 else INF, i << 1 | z, seg))
                else:
                    out.append((INF, 0, -1))
        else:
            l, runs = 0, []
            seg += 1
            out.append((INF, 0, -1))
        i += 1
    return out


def closed_form(E, w):
    """the closed form over the entries E = [(x, y)]: (emitted entries, whether the rightmost smallest of the last w is finite)"""
    n, X = len(E), [e[0] for e in E]
    if n == 0:
        return [], False

    def rightmost_smallest(lo, hi):
        b = lo
        for v in range(lo, hi):
            if X[v] <= X[b]:
                b = v
        return b
    pending = X[rightmost_smallest(max(0, n - w), n)] != INF
    if n < w:
        m = rightmost_smallest(0, n)
        return ([E[m]] if X[m] != INF else []), pending
    nwin = n - w + 1
    WM = [min(X[s:s + w]) for s in range(nwin)]
    m = rightmost_smallest(0, w - 1) if w > 1 else -1
    out = []
    for p in range(n):
        if X[p] == INF:
            continue
        emit = max(WM[max(0, p - w + 1):min(p, nwin - 1) + 1]) == X[p]
        if w > 1 and p <= w - 2 and X[p] == X[m]:
            emit = True if p != m else X[w - 1] > X[m]
        if emit:
            out.append(E[p])
    return out, pending


def sketch(seq, w, k, rid=0):
    """restatement 2 (which contains 1): [(x, y)]"""
    S = stream(seq, k)
    segs = {}
    for x, y, s in S:
        if s >= 0:
            segs.setdefault(s, []).append((x, y))
    out = []
    for s in sorted(segs):
        o, pending = closed_form(segs[s], w)
        out += o[:-1] if pending else o
    best = None
    for e in S[-w:]:
        if best is None or e[0] <= best[0]:
            best = e
    if best is not None and best[0] != INF:
        out.append(best[:2])
    return [(x, rid << 32 | y) for x, y in out]


def machine(seq, w, k, rid=0):
    """the loop itself (src/mm_sketch.c:84-150 with is_hpc = 1), restated over entries: [(x, y)]"""
    BIG = (INF, INF)
    buf, bp, mn, mp, out = [BIG] * w, 0, BIG, 0, []
    l = 0
    n, i, mask, top = len(seq), 0, (1 << 2 * k) - 1, 2 * (k - 1)
    fwd = rev = 0
    runs = []
    while i < n:
        c, info, skip = CODE.get(seq[i], 4), BIG, False
        if c < 4:
            j = i
            while j + 1 < n and CODE.get(seq[j + 1], 4) == c:
                j += 1
            runs.append(j - i + 1)
            i = j
            if len(runs) > k:
                runs.pop(0)
            span = sum(runs)
            fwd = (fwd << 2 | c) & mask
            rev = (rev >> 2) | ((3 ^ c) << top)
            if fwd == rev:
                skip = True
            else:
                z = 0 if fwd < rev else 1
                l += 1
                if l >= k and span < 256:
                    info = (hash64((fwd, rev)[z], mask) << 8 | span, rid << 32 | i << 1 | z)
        else:
            l, runs = 0, []
        if not skip:
            buf[bp] = info
            if l == w + k - 1 and mn[0] != INF:
                for j in list(range(bp + 1, w)) + list(range(0, bp)):
                    if mn[0] == buf[j][0] and buf[j][1] != mn[1]:
                        out.append(buf[j])
            if info[0] <= mn[0]:
                if l >= w + k and mn[0] != INF:
                    out.append(mn)
                mn, mp = info, bp
            elif bp == mp:
                if l >= w + k - 1 and mn[0] != INF:
                    out.append(mn)
                mn = (INF, mn[1])
                for j in list(range(bp + 1, w)) + list(range(0, bp + 1)):
                    if mn[0] >= buf[j][0]:
                        mn, mp = buf[j], j
                if l >= w + k - 1 and mn[0] != INF:
                    for j in list(range(bp + 1, w)) + list(range(0, bp + 1)):
                        if mn[0] == buf[j][0] and mn[1] != buf[j][1]:
                            out.append(buf[j])
            bp = (bp + 1) % w
        i += 1
    if mn[0] != INF:
        out.append(mn)
    return out


def adversarial(rng):
    """one string of the committed run: geometric runs in mixed case, runs of 120 to 300, ambiguous bases, tandem units of 2 to 8"""
    n = int(rng.integers(1, 1500))
    s = bytearray()
    while len(s) < n:
        u = rng.random()
        if u < 0.02:
            s += bytes([b"ACGT"[rng.integers(0, 4)]]) * int(rng.integers(120, 300))
        elif u < 0.04:
            s += b"N" * int(rng.integers(1, 4))
        elif u < 0.1:
            unit = bytes(b"ACGT"[x] for x in rng.integers(0, 4, int(rng.integers(2, 9))))
            s += unit * int(rng.integers(3, 30))
        else:
            s += bytes([b"ACGTacgt"[rng.integers(0, 8)]]) * int(rng.geometric(0.6))
    return bytes(s[:n])


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import oracle_util as U
    trials = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
    rng = np.random.default_rng(4)
    bad_machine = bad_sketch = 0
    for t in range(trials):
        k, w = int(rng.choice([4, 6, 12, 16])), int(rng.choice([3, 5, 24, 80]))
        seq = adversarial(rng)
        v = U.RefV()
        U.ref().mm_sketch(None, C.c_char_p(seq), C.c_int(len(seq)), C.c_int(w), C.c_int(k), C.c_uint32(7), C.c_int(1), C.byref(v))
        want = [(int(x), int(y)) for x, y in U._take_ref(v, U.MM_DTYPE).tolist()]
        a, b = machine(seq, w, k, 7), sketch(seq, w, k, 7)
        bad_machine += a != want
        bad_sketch += b != want
        if (a != want or b != want) and bad_machine + bad_sketch < 5:
            print("MISMATCH", t, "w", w, "k", k, "len", len(seq), len(want), len(a), len(b))
    print("trials", trials, "mismatches of the machine", bad_machine, "of the restatement", bad_sketch)
    return 1 if bad_machine or bad_sketch else 0


if __name__ == "__main__":
    sys.exit(main())
