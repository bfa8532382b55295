"""falcon.align of the reference (falcon/DW_banded.c:104-315) restated in plain integers, the inner loop of py/scripts/pg_asm_cns.py
(:143-244) over it and cns_util.consensus, and the reader of tests/golden/aln_cases.npz.  Nothing here is the reference's code: it is the
rule of DESIGN.md section 4.7a, which tests/golden/make_golden_aln.py checked against the real functions case by case when it wrote the
fixture.

An answer is (aln_str_size, dist, aln_q_s, aln_q_e, aln_t_s, aln_t_e, q_aln_str, t_aln_str), the fields of the reference's `alignment`.
"""
import os

import numpy as np

import cns_util as CU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "aln_cases.npz")
PROVENANCE = os.path.join(ROOT, "tests", "golden", "aln_cases.provenance.json")
EXIT_END, EXIT_BAND, EXIT_STEPS = "a", "b", "c"      # an end was reached; the band grew wider than 2 * band; max_d steps were used
ZERO = (0, 0, 0, 0, 0, 0, b"", b"")


def _snake(q, x, t, y, n):
    """how many of the next n bytes of q from x and of t from y are equal"""
    i = 0
    while i < n:
        s = min(n - i, 64)
        if q[x + i:x + i + s] == t[y + i:y + i + s]:
            i += s
            continue
        while q[x + i] == t[y + i]:
            i += 1
        break
    return i


def align(q, t, band, want_str=True, info=None):
    """(answer, exit).  info, a dict, receives max_nk (the widest row of diagonals), cells (the visited (d, k)) and snakes (the lengths
    of the path's snakes, d = 0 first) -- what the generator aims at the kernels' windows with."""
    q, t = bytes(q), bytes(t)
    q_len, t_len = len(q), len(t)
    max_d = int(0.3 * float(q_len + t_len)) if q_len > 0 and t_len > 0 else 0
    V = {1: 0}
    best_m, min_k, max_k = -1, 0, 0
    trace = []                                # per d: (min_k, [(x2, from_above), ...])
    max_nk = cells = 0
    for d in range(max_d):
        if max_k - min_k > 2 * band:
            if info is not None:
                info.update(max_nk=max_nk, cells=cells, snakes=[])
            return ZERO, EXIT_BAND
        row, new_v, end = [], {}, None
        max_nk = max(max_nk, (max_k - min_k) // 2 + 1)
        for k in range(min_k, max_k + 1, 2):
            lo, hi = V.get(k - 1, 0), V.get(k + 1, 0)
            above = k == min_k or (k != max_k and lo < hi)
            x = hi if above else lo + 1
            y = x - k
            m = _snake(q, x, t, y, min(q_len - x, t_len - y)) if x < q_len and y < t_len else 0
            x, y = x + m, y + m
            row.append((x, above))
            new_v[k] = x
            best_m = max(best_m, x + y)
            if x >= q_len or y >= t_len:
                end = k
                break
        trace.append((min_k, row))
        cells += len(row)
        if end is not None:
            k, x = end, new_v[end]
            y = x - k
            if info is not None:
                info.update(max_nk=max_nk, cells=cells)
            if not want_str:
                if info is not None:
                    info["snakes"] = []
                return ((x + y + d) // 2, d, 0, x, 0, y, b"", b""), EXIT_END
            steps = []                        # (x1, k, x2, above) from d down to 0
            for cd in range(d, -1, -1):
                mk, r = trace[cd]
                x2, above = r[(k - mk) // 2]
                pk = k + 1 if above else k - 1
                if cd > 0:
                    pmk, pr = trace[cd - 1]
                    x1 = pr[(pk - pmk) // 2][0] + (0 if above else 1)
                else:
                    x1 = 0
                steps.append((x1, k, x2, above))
                k = pk
            qs, ts = bytearray(), bytearray()
            for cd, (x1, k, x2, above) in enumerate(reversed(steps)):
                y1 = x1 - k
                if cd > 0:
                    if above:
                        qs += b"-"; ts.append(t[y1 - 1])
                    else:
                        qs.append(q[x1 - 1]); ts += b"-"
                qs += q[x1:x2]; ts += t[y1:y1 + x2 - x1]
            if info is not None:
                info["snakes"] = [s[2] - s[0] for s in reversed(steps)]
            return (len(qs), d, 0, x, 0, y, bytes(qs), bytes(ts)), EXIT_END
        new_min, new_max = max_k, min_k
        for k in range(min_k, max_k + 1, 2):
            if 2 * new_v[k] - k >= best_m - band:
                new_min, new_max = min(new_min, k), max(new_max, k)
        V = new_v
        max_k, min_k = new_max + 1, new_min - 1
    if info is not None:
        info.update(max_nk=max_nk, cells=cells, snakes=[])
    return ZERO, EXIT_STEPS


def piece_alignments(template, reads, aligner=None):
    """what pg_asm_cns.py:152-230 hands to get_align_tags for one piece: ([(q, t, s1, s2, t_offset), ...] with the back-bone first,
    aln_base, one flag per read: accepted).  aligner(q, t, band) -> answer; None: the restatement above."""
    al = aligner or (lambda q, t, band: align(q, t, band)[0])
    T = bytes(template)
    a = al(T, T, 50)
    alns, used, aln_base = [(a[6], a[7], a[2], a[4], 0)], [], 0
    for read, shift in reads:
        read = bytes(read)
        q, t, t_offset = (read[-shift:], T, 0) if shift < 0 else (read, T[shift:], shift)
        if len(q) <= 0 or len(t) <= 0:                    # clipped to nothing
            used.append(False)
            continue
        a = al(q, t, 150)
        span = abs(a[3] - a[2])
        ok = abs(span - len(q)) < 48 or (shift >= 0 and abs(len(T) - shift - span) < 48)
        used.append(ok)
        if ok:
            alns.append((a[6], a[7], a[2], a[4], t_offset))
            aln_base += abs(a[5] - a[4])
    return alns, aln_base, used


def consensus_reads(template, reads, min_cov=1, aligner=None):
    """pg_asm_cns.py:143-244 for one piece: (consensus, accepted flags, answered by the low-coverage rule)"""
    alns, aln_base, used = piece_alignments(template, reads, aligner)
    if aln_base / len(template) < 3:
        return bytes(template).lower(), used, True
    return CU.consensus(len(template), alns, min_cov), used, False


# ---- hand-made sequences for the windows --------------------------------------------------------------------------------------------------
def with_insertions(rng, template, n, spacing, first=None):
    """a read of template with exactly n single-base insertions, `spacing` template bases apart (the first after `first` bases), each
    different from the template base after it: n steps of the front, snakes of `spacing` between them"""
    T = bytes(template)
    first = spacing if first is None else first
    assert first + (n - 1) * spacing < len(T)
    out, at = bytearray(), 0
    for i in range(n):
        nxt = first + i * spacing
        out += T[at:nxt]
        out.append(next(b for b in b"ACGT" if b != T[nxt] and b != T[nxt - 1]))
        at = nxt
    return bytes(out + T[at:])


def bench_piece(rng, t_len, cov, read_len, rate):
    """(template, [(read, read_shift), ...]): a piece as pg_asm_cns.py meets it, cov * t_len / read_len reads of read_len bases drawn
    from the template and its random flanks and mutated with cns_util.mutate at `rate`, read_shift a few bases off the true start.
    What tools/cns_align_bench.py times; make_golden_aln.py times its first pieces on the reference."""
    flank = read_len // 2
    G = CU.random_template(rng, t_len + 2 * flank)
    T = G[flank:flank + t_len]
    reads = []
    for _ in range(cov * t_len // read_len):
        pos = int(rng.integers(0, t_len + 2 * flank - read_len + 1))
        reads.append((CU.mutate(rng, G[pos:pos + read_len], rate), pos - flank + int(rng.integers(-5, 6))))
    return T, reads


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------
class Pool:
    """sequences stored once, by content"""

    def __init__(self):
        self.seqs, self.index = [], {}

    def add(self, s):
        s = bytes(s)
        if s not in self.index:
            self.index[s] = len(self.seqs)
            self.seqs.append(s)
        return self.index[s]

    def arrays(self):
        return dict(seq=np.frombuffer(b"".join(self.seqs), np.uint8), seq_off=np.concatenate([[0], np.cumsum([len(s) for s in self.seqs])]).astype(np.int64))


def expand_strings(q, t, ops):
    """(q_aln_str, t_aln_str) of a path from (0, 0) given as run-length operations (cns_util.ops_of)"""
    ops = np.asarray(ops, np.uint32)
    op = np.repeat(ops >> np.uint32(28), ops & np.uint32(0x0FFFFFFF))
    qb, tb = np.frombuffer(bytes(q), np.uint8), np.frombuffer(bytes(t), np.uint8)
    qs, ts = np.full(len(op), 45, np.uint8), np.full(len(op), 45, np.uint8)
    qs[op != CU.OP_D] = qb[:int((op != CU.OP_D).sum())]
    ts[op != CU.OP_I] = tb[:int((op != CU.OP_I).sum())]
    return qs.tobytes(), ts.tobytes()


class AlnCase:
    def __init__(self, name, q, t, band, want_str, answer, exit_kind):
        self.name, self.q, self.t, self.band, self.want_str, self.answer, self.exit = name, q, t, band, want_str, answer, exit_kind


class PieceCase:
    def __init__(self, name, min_cov, pieces, cns, used, by_rule):
        self.name, self.min_cov, self.pieces, self.cns, self.used, self.by_rule = name, min_cov, pieces, cns, used, by_rule


BIG = 10_000          # cases with a sequence longer than this run once, not in the shuffles
_cases = None


def load_cases():
    """(alignment cases, piece cases) of the fixture, expanded once.  A piece case holds pieces = [(template, [(read, shift), ...])]."""
    global _cases
    if _cases is not None:
        return _cases
    g = np.load(GOLDEN)
    pool, off = g["seq"].tobytes(), g["seq_off"]
    whole = [pool[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    part = lambda sid, s, n: whole[int(sid)] if (int(s), int(n)) == (0, len(whole[int(sid)])) else whole[int(sid)][int(s):int(s) + int(n)]
    alns = []
    for i, name in enumerate(g["aln_names"].tolist()):
        q = part(g["aln_q"][i, 0], g["aln_q"][i, 1], g["aln_q"][i, 2])
        t = part(g["aln_t"][i, 0], g["aln_t"][i, 1], g["aln_t"][i, 2])
        f = [int(v) for v in g["aln_fields"][i]]
        qs, ts = expand_strings(q, t, g["aln_ops"][int(g["aln_ops_off"][i]):int(g["aln_ops_off"][i + 1])]) if g["aln_want"][i] else (b"", b"")
        alns.append(AlnCase(name, q, t, int(g["aln_band"][i]), bool(g["aln_want"][i]), (*f, qs, ts), str(g["aln_exit"][i])))
    pieces = []
    cns, cns_off = g["cns"].tobytes(), g["cns_off"]
    for c, name in enumerate(g["pc_names"].tolist()):
        ps, want, used, rule = [], [], [], []
        for p in range(int(g["pc_piece_off"][c]), int(g["pc_piece_off"][c + 1])):
            r0, r1 = int(g["piece_read_off"][p]), int(g["piece_read_off"][p + 1])
            ps.append((whole[int(g["piece_tmpl"][p])], [(whole[int(g["read_seq"][r])], int(g["read_shift"][r])) for r in range(r0, r1)]))
            want.append(cns[int(cns_off[p]):int(cns_off[p + 1])])
            used.append(g["read_used"][r0:r1].astype(bool))
            rule.append(bool(g["piece_by_rule"][p]))
        pieces.append(PieceCase(name, int(g["pc_min_cov"][c]), ps, want, used, rule))
    _cases = (alns, pieces)
    return _cases
