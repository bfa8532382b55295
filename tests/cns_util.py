"""The consensus call of the reference's falcon/falcon.c (get_align_tags, get_cns_from_align_tags) restated in integers, the builders of
alignment strings, and the reader of tests/golden/cns_cases.npz.  Nothing here is the reference's code: it is the rule of DESIGN.md
section 4.7, which tests/golden/make_golden_cns.py checked against the real functions case by case when it wrote the fixture.

An alignment is (q, t, s1, s2, t_offset): two byte strings of equal length over ACGTNacgtn and '-', the start pair of falcon.align and the
offset of the aligned template part in the piece.  A piece is (t_len, [alignment, ...]).
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cns_cases.npz")
PROVENANCE = os.path.join(ROOT, "tests", "golden", "cns_cases.provenance.json")
ALPHABET = b"ACGTNacgtn-"
MAX_ALNS = 65535
TAG_FIELDS = ("t_pos", "delta", "q_base", "p_t_pos", "p_delta", "p_q_base")
# what pgx_cns_tags answers (include/pgx.h: pgx_cns_tag)
TAG_DTYPE = np.dtype([("t_pos", "<i4"), ("p_t_pos", "<i4"), ("delta", "u1"), ("q_base", "u1"), ("p_delta", "u1"), ("p_q_base", "u1")])
OP_M, OP_I, OP_D = 0, 1, 2     # a column with both bases; a read base against a gap; a template base against a gap


class Refused(ValueError):
    """the reference has no answer for this piece (it reads through an end iterator, or past an array)"""


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------
def align_tags(q, t, s1, s2, t_offset):
    """the tags of one alignment as a TAG_DTYPE array: column k's own (t_pos, delta, q_base) and the previous column's; column 0 follows
    (t_offset - 1, 0, '.').  The walk ends before the first column whose delta would be 255 or whose template position is negative."""
    q, t = np.frombuffer(bytes(q), np.uint8), np.frombuffer(bytes(t), np.uint8)
    assert len(q) == len(t)
    n = len(q)
    qn, tn = q != 45, t != 45
    j = int(s2) - 1 + np.cumsum(tn, dtype=np.int64)
    cq = np.cumsum(qn, dtype=np.int64)
    last = np.maximum.accumulate(np.where(tn, np.arange(n), -1)) if n else np.zeros(0, np.int64)
    jj = cq - np.where(last >= 0, cq[np.maximum(last, 0)], 0)
    stop = np.flatnonzero((jj >= 255) | (j + int(t_offset) < 0))
    n = int(stop[0]) if len(stop) else n
    out = np.zeros(n, TAG_DTYPE)
    out["t_pos"], out["delta"], out["q_base"] = j[:n] + int(t_offset), jj[:n], q[:n]
    if n:
        out["p_t_pos"][0], out["p_delta"][0], out["p_q_base"][0] = int(t_offset) - 1, 0, ord(".")
        out["p_t_pos"][1:], out["p_delta"][1:], out["p_q_base"][1:] = out["t_pos"][:-1], out["delta"][:-1], out["q_base"][:-1]
    return out


def tag_key(t_pos, delta, base):
    """(uint64)(int)t_pos << 32 | delta << 8 | base: a position of -1 becomes the largest"""
    return ((int(t_pos) & 0xFFFFFFFF) << 32) | (int(delta) << 8) | int(base)


def check_piece(t_len, alns, name="piece"):
    if len(alns) > MAX_ALNS:
        raise Refused(f"{name}: {len(alns)} alignments")
    for q, t, s1, s2, t_offset in alns:
        if t_offset < 0:
            raise Refused(f"{name}: negative t_offset")
        if len(q) != len(t) or bytes(q).translate(None, ALPHABET) or bytes(t).translate(None, ALPHABET):
            raise Refused(f"{name}: a byte outside {ALPHABET.decode()}")


def consensus(t_len, alns, min_cov=1, name="piece"):
    """the consensus of one piece (bytes), or Refused"""
    check_piece(t_len, alns, name)
    tags = [align_tags(*a) for a in alns]
    tags = np.concatenate(tags) if tags else np.zeros(0, TAG_DTYPE)
    if len(tags) and int(tags["t_pos"].max()) >= t_len:
        raise Refused(f"{name}: a tag at {int(tags['t_pos'].max())} of {t_len}")
    coverage = np.bincount(tags["t_pos"][tags["delta"] == 0], minlength=t_len).tolist()
    count = {}
    for tg in tags.tolist():
        e = (tag_key(tg[0], tg[2], tg[3]), tag_key(tg[1], tg[4], tg[5]))
        count[e] = count.get(e, 0) + 1
    best, via = {}, {}            # node -> doubled score, node -> the predecessor key of its best edge
    top, end = 0, None
    for c, p in sorted(count):
        s = 2 * count[(c, p)] - (coverage[c >> 32] - 1)
        if c not in best:
            best[c], via[c] = s, p
        if p & 0xFF == 46 or p not in best:
            continue
        new = s + best[p]
        if new > best[c]:
            best[c], via[c] = new, p
            if new > top:
                top, end = new, c
    if end is None:
        raise Refused(f"{name}: no end node")
    out, node = bytearray(), end
    while True:
        b = node & 0xFF
        if b != 45:
            out.append(b if coverage[node >> 32] > min_cov else ord(chr(b).lower()))
        node = via[node]
        if node & 0xFF == 46:
            break
    return bytes(out[::-1])


# ---- alignment strings ----------------------------------------------------------------------------------------------------------------------
def ops_of(q, t):
    """run-length operations of an alignment: (op << 28 | length) per run"""
    q, t = np.frombuffer(bytes(q), np.uint8), np.frombuffer(bytes(t), np.uint8)
    op = np.where(t == 45, OP_I, np.where(q == 45, OP_D, OP_M)).astype(np.uint32)
    if not len(op):
        return np.zeros(0, np.uint32)
    cut = np.flatnonzero(np.diff(op)) + 1
    start = np.concatenate([[0], cut])
    return (op[start] << np.uint32(28)) | np.diff(np.concatenate([start, [len(op)]])).astype(np.uint32)


def expand(template, read, s2, t_offset, ops):
    """(q, t) from the piece's template, the read's aligned bases (q without its gaps) and the operations"""
    ops = np.asarray(ops, np.uint32)
    op = np.repeat(ops >> np.uint32(28), ops & np.uint32(0x0FFFFFFF))
    tb = np.frombuffer(bytes(template), np.uint8)[int(t_offset) + int(s2):]
    rb = np.frombuffer(bytes(read), np.uint8)
    q, t = np.full(len(op), 45, np.uint8), np.full(len(op), 45, np.uint8)
    q[op != OP_D] = rb[:int((op != OP_D).sum())]
    t[op != OP_I] = tb[:int((op != OP_I).sum())]
    assert int((op != OP_D).sum()) == len(rb)
    return q.tobytes(), t.tobytes()


def build(template, t_offset, s2, script):
    """a hand-made alignment against template[t_offset + s2:]: script is a list of ('=', n) n matching columns, ('X', bases) mismatch
    columns with these read bases, ('I', bases) inserted read bases, ('D', n) n deleted template bases"""
    q, t, pos = bytearray(), bytearray(), t_offset + s2
    for kind, v in script:
        if kind == "=":
            q += template[pos:pos + v]; t += template[pos:pos + v]; pos += v
        elif kind == "X":
            q += v; t += template[pos:pos + len(v)]; pos += len(v)
        elif kind == "I":
            q += v; t += b"-" * len(v)
        elif kind == "D":
            q += b"-" * v; t += template[pos:pos + v]; pos += v
    assert pos <= len(template) and len(q) == len(t)
    return bytes(q), bytes(t), 0, s2, t_offset


def random_template(rng, n, letters=b"ACGT", homopolymers=False):
    a = rng.choice(np.frombuffer(letters, np.uint8), n)
    if homopolymers:     # stretch every base into a run of 1 .. 8
        a = np.repeat(a, rng.integers(1, 9, n))[:n]
    return a.tobytes()


def mutate(rng, seq, rate):
    """a read of seq with substitutions, insertions and deletions at `rate` in all"""
    a = np.frombuffer(seq, np.uint8)
    u = rng.random(len(a))
    sub, dele, ins = u < rate / 3, (u >= rate / 3) & (u < 2 * rate / 3), (u >= 2 * rate / 3) & (u < rate)
    b = np.where(sub, rng.choice(np.frombuffer(b"ACGT", np.uint8), len(a)), a)
    out = np.zeros(2 * len(a), np.uint8)
    out[0::2] = np.where(dele, 0, b)
    out[1::2] = np.where(ins, rng.choice(np.frombuffer(b"ACGT", np.uint8), len(a)), 0)
    return out[out != 0].tobytes()


def synthetic_piece(rng, t_len, n_reads, rate=0.12, min_frac=0.3):
    """a piece whose alignments are drawn column by column (no aligner): the back-bone and n_reads reads over random spans, each template
    base matched, substituted or deleted and followed by a few inserted bases at `rate` in all.  What tools/cns_bench.py times."""
    tb = rng.choice(np.frombuffer(b"ACGT", np.uint8), t_len)
    template = tb.tobytes()
    alns = [(template, template, 0, 0, 0)]
    acgt = np.frombuffer(b"ACGT", np.uint8)
    for _ in range(n_reads):
        span = int(rng.integers(int(t_len * min_frac), t_len + 1))
        a = int(rng.integers(0, t_len - span + 1))
        seg = tb[a:a + span]
        u = rng.random(span)
        qcol = np.where(u < rate / 3, rng.choice(acgt, span), seg)
        qcol = np.where((u >= rate / 3) & (u < 2 * rate / 3), 45, qcol).astype(np.uint8)
        n_ins = np.where(u >= 1 - rate / 3, rng.integers(1, 4, span), 0)
        n_ins[-1] = 0
        at = np.cumsum(1 + n_ins) - n_ins - 1            # column of every template base
        total = int(span + n_ins.sum())
        q, t = rng.choice(acgt, total).astype(np.uint8), np.full(total, 45, np.uint8)
        q[at], t[at] = qcol, seg
        t_offset = int(rng.integers(0, a + 1)) if rng.random() < 0.5 else 0
        alns.append((q.tobytes(), t.tobytes(), 0, a - t_offset, t_offset))
    return t_len, alns


LETTERS = b"ACGTNacgtn"


def wide_position(T, at, K, n_full):
    """a piece (template, alignments) with exactly K distinct insertion nodes after template base at - 1: n_full back-bone copies and ten
    reads, read r inserting K // 10 + (r < K % 10) bases of which the one at delta d + 1 is LETTERS[(d + r) % 10] (ten different letters
    per delta).  The nodes (at - 1, 0) and (at, 0) are then K + 1 apart in key order.  With n_full = 12 the direct edge between the two
    scores 12 - 9 = 3 and every insertion edge 2 - 21: the consensus is the template."""
    alns = [build(T, 0, 0, [("=", len(T))]) for _ in range(n_full)]
    for r in range(10):
        ins = bytes(LETTERS[(d + r) % 10] for d in range(K // 10 + (r < K % 10)))
        alns.append(build(T, 0, 0, [("=", at), ("I", ins), ("=", len(T) - at)]))
    return T, alns


def distinct_keys(alns):
    """the sorted distinct tag keys of a piece's alignments (the nodes of the rule, in its order) as uint64"""
    tags = [align_tags(*a) for a in alns]
    tags = np.concatenate(tags) if tags else np.zeros(0, TAG_DTYPE)
    pos = tags["t_pos"].astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    return np.unique(pos << np.uint64(32) | tags["delta"].astype(np.uint64) << np.uint64(8) | tags["q_base"].astype(np.uint64))


def node_distance(alns, key_a, key_b):
    """how many places the node key_b = (t_pos, delta, base) lies after key_a among the piece's nodes in key order: the difference of
    node indices that the scoring ring and the back-track window see"""
    keys = distinct_keys(alns).tolist()
    return keys.index(tag_key(*key_b)) - keys.index(tag_key(*key_a))


# ---- rows as the library takes them -------------------------------------------------------------------------------------------------------
FILLER = b"\x00.X*\xff"
LAYOUTS = ("packed", "interleaved", "scattered", "shared")


def rows_of(pieces, layout="packed", rng=None):
    """pieces: [(t_len, [alignment, ...]), ...] -> (rows, q_str, t_str, piece_tlen) in the dtypes of pgx_cns_call.
      packed       rows piece by piece, the strings back to back in row order (what shimmer._cns_rows makes)
      interleaved  the rows in a random permutation across all pieces, the strings back to back in that order
      scattered    rows piece by piece; the strings in a random order of their own with runs of 1 .. 70 bytes of FILLER before, between
                   and after them, the same bytes at the same places of both buffers
      shared       interleaved, and alignments of a piece with the same two strings point at one copy of them"""
    from peregrine_amd import _lib
    assert layout in LAYOUTS
    items = [(p, a) for p, (_, alns) in enumerate(pieces) for a in alns]
    order = np.arange(len(items)) if layout in ("packed", "scattered") else rng.permutation(len(items))
    rows = np.zeros(len(items), _lib.CNS_ALN_DTYPE)
    slots, slot_of, seen = [], [], {}
    for i in order.tolist():
        p, (q, t, s1, s2, t_offset) = items[i]
        q, t = bytes(q), bytes(t)
        assert len(q) == len(t)
        key = (p, q, t) if layout == "shared" else len(slot_of)
        if key not in seen:
            seen[key] = len(slots)
            slots.append((q, t))
        slot_of.append(seen[key])
    fill = lambda: rng.choice(np.frombuffer(FILLER, np.uint8), int(rng.integers(1, 71))).tobytes() if layout == "scattered" else b""
    qs, ts, at = bytearray(), bytearray(), [0] * len(slots)
    for s in (rng.permutation(len(slots)) if layout == "scattered" else np.arange(len(slots))).tolist():
        f = fill()
        qs += f; ts += f
        at[s] = len(qs)
        qs += slots[s][0]; ts += slots[s][1]
    f = fill()
    qs += f; ts += f
    for r, i in enumerate(order.tolist()):
        p, (q, t, s1, s2, t_offset) = items[i]
        rows[r] = (p, t_offset, s1, s2, at[slot_of[r]], len(q), 0)
    return rows, np.frombuffer(bytes(qs), np.uint8), np.frombuffer(bytes(ts), np.uint8), np.array([t_len for t_len, _ in pieces], np.uint32)


def call_rows(rows, q_str, t_str, piece_tlen, min_cov=1, entry="pgx_cns_call", stats=None, null_text=False):
    """pgx_cns_call or pgx_cns_call_dev (`entry` names it) on raw rows, as shimmer.consensus calls them: the consensus of every piece as
    bytes, or _lib.PgxError.  The number of pieces is len(piece_tlen), the string bytes len(q_str): rows may name anything.  For the device
    entry the rows and both strings are uploaded with torch.  null_text: pass no place for the text (an argument error)."""
    import ctypes as C
    from peregrine_amd import _lib
    assert entry in ("pgx_cns_call", "pgx_cns_call_dev")
    _lib.init()
    rows = np.ascontiguousarray(rows, _lib.CNS_ALN_DTYPE)
    q_str, t_str = np.ascontiguousarray(q_str, np.uint8), np.ascontiguousarray(t_str, np.uint8)
    tlen = np.ascontiguousarray(piece_tlen, np.uint32)
    assert len(q_str) == len(t_str)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    if entry == "pgx_cns_call_dev":
        import torch
        dev = torch.device("cuda", _lib._inited)
        held = [torch.from_numpy(a.view(np.uint8).copy()).to(dev) for a in (rows, q_str, t_str)]
        torch.cuda.synchronize(dev)
        args = [C.c_void_p(x.data_ptr() if x.numel() else 0) for x in held]
    else:
        args = [ptr(rows), ptr(q_str), ptr(t_str)]
    off = np.zeros(len(tlen) + 1, np.uint64)
    st = _lib.CnsStats()
    text = C.c_void_p()
    rc = getattr(_lib.load(), entry)(args[0], len(rows), args[1], args[2], len(q_str), ptr(tlen), len(tlen), int(min_cov),
                                     None if null_text else C.byref(text), ptr(off), C.byref(st))
    _lib.check(rc, entry)
    data = C.string_at(text.value, int(off[-1]))
    _lib.load().pgx_free(text)
    if stats is not None:
        stats.update(st.asdict())
    return [data[int(off[p]):int(off[p + 1])] for p in range(len(tlen))]


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------------
def pack_cases(cases):
    """cases: [(name, min_cov, [(template, [alignment, ...]), ...])] -> the input arrays of the fixture.  A piece given as (template,
    [alignment, ...], repeat) stands for its alignments `repeat` times over and is stored once (piece_repeat)."""
    names, min_cov, case_piece_off, tmpl, tmpl_off, piece_aln_off, piece_repeat = [], [], [0], [], [0], [0], []
    t_offset, s1, s2, reads, read_off, ops, ops_off = [], [], [], [], [0], [], [0]
    for name, mc, pieces in cases:
        names.append(name); min_cov.append(mc)
        for template, alns, *rep in pieces:
            piece_repeat.append(rep[0] if rep else 1)
            tmpl.append(np.frombuffer(template, np.uint8)); tmpl_off.append(tmpl_off[-1] + len(template))
            for q, t, a1, a2, off in alns:
                r = bytes(q).replace(b"-", b"")
                o = ops_of(q, t)
                assert expand(template, r, a2, off, o) == (bytes(q), bytes(t)), name
                t_offset.append(off); s1.append(a1); s2.append(a2)
                reads.append(np.frombuffer(r, np.uint8)); read_off.append(read_off[-1] + len(r))
                ops.append(o); ops_off.append(ops_off[-1] + len(o))
            piece_aln_off.append(piece_aln_off[-1] + len(alns))
        case_piece_off.append(len(tmpl))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return dict(names=np.array(names), min_cov=np.array(min_cov, np.int32), case_piece_off=np.array(case_piece_off, np.int64),
                tmpl=cat(tmpl, np.uint8), tmpl_off=np.array(tmpl_off, np.int64), piece_aln_off=np.array(piece_aln_off, np.int64),
                piece_repeat=np.array(piece_repeat, np.int32),
                aln_t_offset=np.array(t_offset, np.int32), aln_s1=np.array(s1, np.int32), aln_s2=np.array(s2, np.int32),
                reads=cat(reads, np.uint8), read_off=np.array(read_off, np.int64), ops=cat(ops, np.uint32), ops_off=np.array(ops_off, np.int64))


def pack_tags(tag_lists):
    """the tags of every alignment, positions stored as differences along the concatenation (they compress 50-fold that way)"""
    allt = np.concatenate(tag_lists) if tag_lists else np.zeros(0, TAG_DTYPE)
    out = dict(tag_off=np.concatenate([[0], np.cumsum([len(t) for t in tag_lists])]).astype(np.int64))
    for f in TAG_FIELDS:
        out["tag_" + f] = np.diff(allt[f].astype(np.int64), prepend=0).astype(np.int32) if f.endswith("t_pos") else allt[f].copy()
    return out


class Case:
    def __init__(self, name, min_cov, pieces, cns, tags):
        self.name, self.min_cov, self.pieces, self.cns, self.tags = name, min_cov, pieces, cns, tags   # pieces: [(t_len, [alignment])]


def batches_by_min_cov(cases, skip=("edge_full_count",)):
    """all pieces of the cases in one batch per min_cov: {min_cov: (pieces, the reference's consensus of each)}.  skip: cases left out
    (the 65,535 alignments of edge_full_count run alone: in every batch they would only slow it)"""
    out = {}
    for c in cases:
        if c.name not in skip:
            pieces, want = out.setdefault(c.min_cov, ([], []))
            pieces += c.pieces
            want += c.cns
    return out


_cases = None


def load_cases():
    """the fixture's cases, expanded once: pieces as (t_len, alignments), the reference's consensus per piece and tags per alignment"""
    global _cases
    if _cases is not None:
        return _cases
    g = np.load(GOLDEN)
    tags = np.zeros(int(g["tag_off"][-1]), TAG_DTYPE)
    for f in TAG_FIELDS:
        tags[f] = np.cumsum(g["tag_" + f].astype(np.int64)) if f.endswith("t_pos") else g["tag_" + f]
    tmpl, reads, ops, cns = g["tmpl"].tobytes(), g["reads"].tobytes(), g["ops"], g["cns"].tobytes()
    out = []
    for ci, name in enumerate(g["names"].tolist()):
        pieces, want, wtags = [], [], []
        for p in range(int(g["case_piece_off"][ci]), int(g["case_piece_off"][ci + 1])):
            template = tmpl[int(g["tmpl_off"][p]):int(g["tmpl_off"][p + 1])]
            alns, ptags = [], []
            for a in range(int(g["piece_aln_off"][p]), int(g["piece_aln_off"][p + 1])):
                q, t = expand(template, reads[int(g["read_off"][a]):int(g["read_off"][a + 1])], g["aln_s2"][a], g["aln_t_offset"][a],
                              ops[int(g["ops_off"][a]):int(g["ops_off"][a + 1])])
                alns.append((q, t, int(g["aln_s1"][a]), int(g["aln_s2"][a]), int(g["aln_t_offset"][a])))
                ptags.append(tags[int(g["tag_off"][a]):int(g["tag_off"][a + 1])])
            rep = int(g["piece_repeat"][p])            # the stored alignments stand for `rep` times as many (the same objects over again)
            pieces.append((len(template), alns * rep))
            wtags += ptags * rep
            want.append(cns[int(g["cns_off"][p]):int(g["cns_off"][p + 1])])
        out.append(Case(name, int(g["min_cov"][ci]), pieces, want, wtags))
    _cases = out
    return out
