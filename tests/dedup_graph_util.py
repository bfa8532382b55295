"""shmr_dedup's graph mode in plain Python: which lines of a preads.ovl text the string graph's loader can use, and what the loader
makes of a text.  TEST INFRASTRUCTURE, written from the rule's description ("shmr_dedup -g"), not from the loader:

  a line has 13 blank-separated fields  rid0 rid1 score identity strand0 bgn0 end0 len0 strand1 bgn1 end1 len1 type
  1. rid0 == rid1: the line is ignored, it marks nothing
  2. type `contained` marks rid0, type `contains` marks rid1 (as contained reads); neither goes on
  3. only `overlap` lines go on, and of them only those with neither read marked by ANY line of the text
The loader additionally drops an `overlap` line whose identity is below min_idt or with a read shorter than min_len; marks do not depend
on either.  Read ids are compared as the strings `%09d` prints, which map one to one onto the 32-bit ids.
"""
import numpy as np

from peregrine_amd.formats import OVLP_DTYPE


def _fields(text: bytes):
    return [ln.split() for ln in text.split(b"\n")[:-1]]


def marked_reads(text: bytes) -> set:
    marked = set()
    for f in _fields(text):
        if f[0] == f[1]:
            continue
        if f[12] == b"contained":
            marked.add(f[0])
        elif f[12] == b"contains":
            marked.add(f[1])
    return marked


def select_graph_lines(text: bytes) -> bytes:
    """the selection rule, text to text: the lines a graph-mode stream hands out, in their order"""
    marked = marked_reads(text)
    lines = text.split(b"\n")[:-1]
    return b"".join(ln + b"\n" for ln, f in zip(lines, _fields(text))
                    if f[12] == b"overlap" and f[0] != f[1] and f[0] not in marked and f[1] not in marked)


def loader_input(text: bytes, min_len: int = 4000, min_idt: float = 96.0) -> list:
    """the loader's effective input: the 12-tuples (ids as text, score, identity, 2 x (strand, bgn, end, len)) that survive its two loops"""
    marked, data = set(), []
    for f in _fields(text):
        if f[0] == f[1]:
            continue
        if f[12] == b"contained":
            marked.add(f[0])
        elif f[12] == b"contains":
            marked.add(f[1])
        elif f[12] == b"overlap":
            t = (f[0], f[1], int(f[2]), float(f[3]), *(int(x) for x in f[4:12]))
            if t[3] < min_idt or t[7] < min_len or t[11] < min_len:
                continue
            data.append(t)
    return [t for t in data if t[0] not in marked and t[1] not in marked]


def graph_stats(text: bytes) -> dict:
    """what DedupStream(graph_ready=True).stats reports after the drain, from the full text"""
    return dict(contained_reads=len(marked_reads(text)), lines_kept=select_graph_lines(text).count(b"\n"), lines_total=text.count(b"\n"))


def is_subsequence(part: bytes, whole: bytes) -> bool:
    it = iter(whole.split(b"\n"))
    return all(any(ln == w for w in it) for ln in part.split(b"\n")[:-1])


def rec(rid0, rid1, typ=0, m_size=5000, dist=20, pos0=100, pos1=100, rl0=9000, rl1=8000, s0=0, s1=0, q_bgn=1000, q_end=9000, t_bgn=0, t_end=8000):
    """one ovlp_t record"""
    r = np.zeros(1, OVLP_DTYPE)
    r["y0"] = (int(rid0) << 32) | (int(pos0) << 1) | (s0 & 1)
    r["y1"] = (int(rid1) << 32) | (int(pos1) << 1) | (s1 & 1)
    r["rl0"], r["rl1"], r["strand0"], r["strand1"], r["ovlp_type"] = rl0, rl1, s0, s1, typ
    r["m_size"], r["dist"], r["q_bgn"], r["q_end"], r["t_bgn"], r["t_end"] = m_size, dist, q_bgn, q_end, t_bgn, t_end
    r["t_m_end"], r["q_m_end"] = t_end, q_end
    return r


def make_records(seed: int = 2026, n_reads: int = 300, genome: int = 40_000, contained_share: float = 0.3) -> np.ndarray:
    """About 20 k records over n_reads reads laid on a line: a record per pair of reads that share >= 500 bases, as a dovetail of the left
    read into the right one (either may be rid0).  A chosen third of the reads is contained: a line between one of them and a read outside
    the set says so three times in ten (`contained` when it is rid0 -- also as type values 3 .. 7 --, `contains` when it is rid1).  On
    top: recurrences of earlier pairs that WOULD mark a read outside the set (they lose first-wins, so they must not), and self pairs
    of every type."""
    rng = np.random.default_rng(seed)
    rlen = rng.integers(2000, 16000, n_reads)
    start = rng.integers(0, genome, n_reads)
    inset = rng.random(n_reads) < contained_share
    parts = []
    for i in range(n_reads):
        for j in range(n_reads):
            if i == j or not (start[i] < start[j] or (start[i] == start[j] and i < j)):
                continue
            ovl = int(min(start[i] + rlen[i], start[j] + rlen[j]) - start[j])   # i is the left read
            if ovl < 500:
                continue
            dist = int(rng.integers(0, max(1, ovl // 18)))                       # identity between about 94.5 and 100
            if rng.random() < 0.5:
                a, b = i, j
                kw = dict(q_bgn=int(start[j] - start[i]), q_end=int(start[j] - start[i]) + ovl, t_end=ovl, s1=0)
            else:
                a, b = j, i
                kw = dict(q_bgn=0, q_end=ovl, t_end=ovl, s1=1)
            typ = 0
            if inset[a] != inset[b] and rng.random() < 0.3:
                typ = (2 if rng.random() < 0.8 else int(rng.integers(3, 8))) if inset[a] else 1
            parts.append(rec(a, b, typ, m_size=ovl, dist=dist, rl0=int(rlen[a]), rl1=int(rlen[b]), **kw))
    first = np.concatenate(parts)
    rng.shuffle(first)
    # recurrences: the pair again, in either order, typed so that it would mark a read OUTSIDE the set
    again = []
    cut = len(first) * 3 // 4
    for k in rng.choice(cut, len(first) // 6, replace=False):   # (of pairs in the stream's first part: they always lose)
        a, b = int(first["y0"][k] >> np.uint64(32)), int(first["y1"][k] >> np.uint64(32))
        if rng.random() < 0.5:
            a, b = b, a
        typ = 2 if not inset[a] else (1 if not inset[b] else 0)
        again.append(rec(a, b, typ, rl0=int(rlen[a]), rl1=int(rlen[b])))
    again = np.concatenate(again)
    selfs = np.concatenate([rec(int(r), int(r), t, rl0=int(rlen[r]), rl1=int(rlen[r])) for t, r in enumerate(np.flatnonzero(~inset)[:12])])
    tail = np.concatenate([again, selfs])
    rng.shuffle(tail)
    mixed = np.concatenate([first[cut:], tail[: len(tail) // 2]])   # some recurrences arrive among first occurrences
    rng.shuffle(mixed)
    return np.concatenate([first[:cut], mixed, tail[len(tail) // 2:]])
