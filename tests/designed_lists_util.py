"""Read databases whose shimmer lists are written by hand, a literal Python restatement of build_map's loop, and the designs the
designed-list tests run (tests/test_designed_lists_rule.py on the CPU, tests/test_gpu_designed_lists.py on the GPU).

A design is a list of loci.  A locus has its own random segment, a list of (offset, hash, span) shimmers and a list of read starts;
its reads are error-free forward copies of the segment (optionally with a few planted substitutions), so a shimmer sits at
consistent offsets in every read of its locus and ovlp_match accepts the pairs a bucket proposes.  What a simulated read set holds
by chance -- a first-key group of exactly 49 buckets, a list head whose multiplicity equals mc_upper, a position gap of exactly 99 --
is placed here on purpose, and the model below (never a kernel) says what every design contains.
TEST INFRASTRUCTURE: imported only from tests/."""
from __future__ import annotations

import functools
from collections import Counter
from dataclasses import dataclass, field

import numpy as np

import oracle_util as U
from peregrine_amd.formats import MM_DTYPE, MC_DTYPE, SeqDB

READ_LEN = 700
STARTS3 = (0, 40, 110)     # three reads: 0/40 end as a containment (660 common bases), 0/110 and 40/110 as overlaps
BIG_UPPER = 1 << 20        # mc_upper for designs whose first keys occur thousands of times
VISIT_LANE_MAX, VISIT_WAVE_MAX = 48, 3153     # pgx_internal.h


@dataclass
class Locus:
    shimmers: list           # (offset in the segment, hash, span), ascending offsets; an offset is the k-mer's LAST base, as in mm_sketch
    starts: tuple = STARTS3  # one read per entry: segment[start : start + read_len]
    read_len: int = READ_LEN
    subs: int = 0            # substitutions planted in every read of the locus, at random places (the shimmers are written, not sketched)


def key(h: int, span: int = 16) -> int:
    return (h << 8) | span


def build_db(loci, seed=1, split=None, absent=None):
    """(SeqDB, MM_DTYPE list ordered by rid then position, MC_DTYPE table).  split: {hash: k} spreads that hash's count over k rows
    (no row reaches the sum); absent: {hash: count} adds rows for hashes that occur nowhere in the list."""
    rng = np.random.default_rng(seed)
    chunks, rlen, xs, ys = [], [], [], []
    rid = 0
    for lc in loci:
        seg = rng.integers(0, 4, lc.read_len + max(lc.starts), dtype=np.uint8)
        for s in lc.starts:
            codes = seg[s:s + lc.read_len].copy()
            if lc.subs:
                at = rng.choice(lc.read_len, lc.subs, replace=False)
                codes[at] = (codes[at] + rng.integers(1, 4, lc.subs, dtype=np.uint8)) & 3
            # seqdb byte: low nibble the forward base one-hot, high nibble the reverse strand's base at the same index
            chunks.append((np.uint8(1) << codes) | ((np.uint8(8) >> codes[::-1]) << np.uint8(4)))
            rlen.append(lc.read_len)
            last = -1
            for off, h, span in lc.shimmers:
                pos = off - s
                if pos < span - 1 or pos >= lc.read_len:   # (a real shimmer lies inside its read: pos >= span - 1)
                    continue
                assert pos > last and 0 < span < 256 and 0 <= h < 1 << 56
                last = pos
                xs.append(key(h, span)), ys.append((rid << 32) | (pos << 1))
            rid += 1
    rlen = np.array(rlen, np.uint32)
    roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
    db = SeqDB(np.concatenate(chunks).astype(np.uint8), np.arange(rid, dtype=np.uint32), rlen, roff, None)
    mm = np.zeros(len(xs), MM_DTYPE)
    mm["x"], mm["y"] = np.array(xs, np.uint64), np.array(ys, np.uint64)
    rows = []
    for h, c in sorted(Counter(x >> 8 for x in xs).items()):
        k = (split or {}).get(h, 1)
        assert k == 1 or c >= k
        rows += [(h, c // k + (1 if i < c % k else 0)) for i in range(k)]
    rows += list((absent or {}).items())
    order = rng.permutation(len(rows))
    mc = np.zeros(len(rows), MC_DTYPE)
    mc["mer"] = np.array([rows[i][0] for i in order], np.uint64)
    mc["count"] = np.array([rows[i][1] for i in order], np.uint32)
    return db, mm, mc


# ------------------------------------------------------------------------------------------------------------
# the model: build_map's loop (src/shmr_utils.c:295-404), statement for statement
# ------------------------------------------------------------------------------------------------------------
@dataclass
class Group:
    key1s: list = field(default_factory=list)    # in first-insertion order
    recs: dict = field(default_factory=dict)     # key1 -> [(pos of y0, dir)] in insertion order
    trail: bool = False                          # the group's last put was of a present key


@dataclass
class Model:
    groups: dict          # key0 -> Group, in first-insertion order
    n_records: int
    drops: Counter        # why a shimmer or a pair gave no record: "low", "high", "head", "gap", "read", "chunk"
    count: dict           # the aggregated multiplicities

    def n_buckets(self, ovlp_upper=120):          # the buckets shmr_overlap visits (shmr_overlap.c:216)
        return sum(2 < len(r) <= ovlp_upper for g in self.groups.values() for r in g.recs.values())

    def n_big(self):
        return sum(len(g.key1s) > VISIT_LANE_MAX for g in self.groups.values())

    def max_group(self):
        return max((len(g.key1s) for g in self.groups.values()), default=0)


def build_map_model(mm, mc, rlen, mychunk=1, total=1, lower=2, upper=240) -> Model:
    cnt = Counter()
    for mer, c in zip(mc["mer"].tolist(), mc["count"].tolist()):   # aggregate_mm_count: rows of one hash add up
        cnt[mer] += c
    xs, ys = mm["x"].tolist(), mm["y"].tolist()
    groups, drops, nrec, n = {}, Counter(), 0, len(xs)

    def put(k0, k1, y0, d):
        g = groups.setdefault(k0, Group())
        g.trail = k1 in g.recs
        if not g.trail:
            g.key1s.append(k1)
        g.recs.setdefault(k1, []).append(((y0 & 0xFFFFFFFF) >> 1, d))

    def flip(y, x):                                # the reverse strand's coordinate (:376-396)
        return (int(rlen[y >> 32]) - (((y & 0xFFFFFFFF) >> 1) + 1) + (x & 0xFF) - 1) << 1

    s = 0
    while s < n and not lower <= cnt[xs[s] >> 8] < upper:          # the scan starts STRICTLY below upper (:309-320)
        drops["head"] += lower <= cnt[xs[s] >> 8] <= upper
        s += 1
    if s < n:
        ax, ay = xs[s], ys[s]
        for i in range(s + 1, n):
            bx, by = xs[i], ys[i]
            c = cnt[bx >> 8]
            if c < lower or c > upper:                             # later shimmers: upper INCLUSIVE; the anchor stays (:327)
                drops["low" if c < lower else "high"] += 1
                continue
            if ay >> 32 == by >> 32:
                if ((((by >> 1) & 0xFFFFFFF) - ((ay >> 1) & 0xFFFFFFF)) & 0xFFFFFFFF) < 100:   # (:332) the anchor advances
                    drops["gap"] += 1
                    ax, ay = bx, by
                    continue
                if (ax >> 8) % total == mychunk % total:           # forward record, owned by key0's chunk (:337)
                    put(ax, bx, ay, 0)
                    nrec += 1
                else:
                    drops["chunk"] += 1
                if (bx >> 8) % total == mychunk % total:           # reverse record (:362)
                    put(bx, ax, flip(by, bx), 1)
                    nrec += 1
                else:
                    drops["chunk"] += 1
            else:
                drops["read"] += 1
            ax, ay = bx, by                                        # (:402)
    return Model(groups, nrec, drops, dict(cnt))


# ------------------------------------------------------------------------------------------------------------
# the designs
# ------------------------------------------------------------------------------------------------------------
@dataclass
class Built:
    db: SeqDB
    mm: np.ndarray
    mc: np.ndarray
    runs: list                        # overlap keyword sets (ResidentDB.overlap's names), every one run under every dispatch
    env: dict = field(default_factory=dict)    # extra environment for one more device-visit run per keyword set
    wave_overflow: bool = False       # a group beyond what a wavefront replays: the host builds the visit order

    def model(self, kw) -> Model:
        rl, _ = self.db.by_rid()
        return build_map_model(self.mm, self.mc, rl, kw.get("mychunk", 1), kw.get("total_chunk", 1), kw.get("mc_lower", 2),
                               kw.get("mc_upper", 240))

    def oracle(self, kw):
        return U.orc_overlap(self.db, self.mm, self.mc, mychunk=kw.get("mychunk", 1), total=kw.get("total_chunk", 1),
                             mc_lower=kw.get("mc_lower", 2), mc_upper=kw.get("mc_upper", 240), bestn=kw.get("bestn", 4),
                             ovlp_upper=kw.get("ovlp_upper", 120))


TABLE_SIZES = (1, 2, 3, 4, 6, 7, 12, 13, 25, 26, 47, 48, 49, 50, 98, 99, 100, 196, 197, 198, 393, 394, 395, 787, 788, 789, 790, 1576,
               1577, 1578, 3152, 3153)
# a put into a table of nb slots that holds upper_of(nb) = (uint32)(nb * 0.77 + 0.5) keys doubles it first (khash.h:180, :298-306).
# (1,024 slots: 788.48 + 0.5 -> 788.  The rounding shows at 32, 128, 2,048 and 4,096 slots: 24.64, 98.56, 1576.96, 3153.92.)
RESIZE_AT = tuple(int(nb * 0.77 + 0.5) for nb in (4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048))
assert RESIZE_AT == (3, 6, 12, 25, 49, 99, 197, 394, 788, 1577) and set(RESIZE_AT) < set(TABLE_SIZES)
assert all(n + 1 in TABLE_SIZES for n in RESIZE_AT)
assert int(4096 * 0.77 + 0.5) == VISIT_WAVE_MAX + 1 and [int(nb * 0.77) for nb in (32, 128, 2048)] == [24, 98, 1576]


def _keys(shape, n, rng):
    """n distinct (hash, span) keys.  real: hash below 2^24, span 16 -- khash's integer hash leaves the span in the low bits, so all
    of them share ONE home slot in tables of up to 256 slots; wide: uniform 56-bit hashes with 0 and 2^56 - 1 in front (a key with
    bit 63 set; a count-table key of hash + 1 = 1); mixed: hashes used twice, under different spans."""
    if shape == "real":
        return [(int(h), 16) for h in rng.choice(1 << 24, n, replace=False)]
    if shape == "wide":
        hs = {0, (1 << 56) - 1}
        while len(hs) < n:
            hs.update(int(h) for h in rng.integers(0, 1 << 56, n - len(hs), dtype=np.uint64))
        rest = sorted(hs - {0, (1 << 56) - 1})
        return [(0, 16), ((1 << 56) - 1, 16)] + [(rest[i], 16) for i in rng.permutation(len(rest))]
    assert shape == "mixed"
    hs = [int(h) for h in rng.choice(1 << 30, (n + 1) // 2, replace=False)]
    spans = (16, 17, 20, 24, 31, 56)
    out = []
    for i, h in enumerate(hs):
        a = spans[i % len(spans)]
        out += [(h, a), (h, spans[(i + 1 + i // len(spans) % (len(spans) - 1)) % len(spans)])]
    assert len(set(out)) == len(out)
    out = [out[i] for i in rng.permutation(len(out))]
    return out[:n]


def _star(k1, k2s, trail, fan_in=False):
    """one group: k1 before (fan_in: after) every key of k2s, a locus each.  The last locus has three reads (its second and third
    put are of a present key: trail) or one (the bucket sits in the table and is not visited)."""
    loci = []
    for i, k2 in enumerate(k2s):
        a, b = (k2, k1) if fan_in else (k1, k2)
        loci.append(Locus([(200, *a), (500, *b)], STARTS3 if trail or i + 1 < len(k2s) else (0,)))
    return loci


def _check_stars(b, kw, want):
    """want: {key0: (buckets, trail)} -- asserted from the model"""
    m = b.model(kw)
    for k0, (n, trail) in want.items():
        g = m.groups[k0]
        assert len(g.key1s) == n and g.trail == trail, (hex(k0), len(g.key1s), g.trail, n, trail)
        sizes = sorted(len(r) for r in g.recs.values())
        assert sizes == ([3] * n if trail else [1] + [3] * (n - 1)), (hex(k0), sizes[:4])
    return m


def table_sizes(shape, trail):
    rng = np.random.default_rng({"real": 11, "wide": 12, "mixed": 13}[shape] + 100 * trail)
    ks = _keys(shape, len(TABLE_SIZES) + sum(TABLE_SIZES), rng)
    firsts, rest = ks[:len(TABLE_SIZES)], ks[len(TABLE_SIZES):]
    if shape == "wide":   # hash 0 and 2^56 - 1 as first keys of wavefront groups on resize boundaries (they are second keys of reversed buckets too)
        assert firsts[0][0] == 0 and firsts[1][0] == (1 << 56) - 1
        firsts[0], firsts[TABLE_SIZES.index(49)] = firsts[TABLE_SIZES.index(49)], firsts[0]
        firsts[1], firsts[TABLE_SIZES.index(789)] = firsts[TABLE_SIZES.index(789)], firsts[1]
    loci, want, at = [], {}, 0
    for k1, n in zip(firsts, TABLE_SIZES):
        loci += _star(k1, rest[at:at + n], trail)
        want[key(*k1)] = (n, trail)
        at += n
    b = Built(*build_db(loci, seed=5), runs=[dict(mc_lower=1, mc_upper=BIG_UPPER)])
    m = _check_stars(b, b.runs[0], want)
    assert m.n_big() == sum(n > VISIT_LANE_MAX for n in TABLE_SIZES) and m.max_group() == VISIT_WAVE_MAX
    x = b.mm["x"]
    if shape == "real":     # one home slot: a group of 65 or more keys walks into the second batch of 64 probe positions
        h32 = (x >> np.uint64(33) ^ x ^ x << np.uint64(11)) & np.uint64(255)
        assert len(np.unique(h32)) == 1 and int(x.max()) < 1 << 32
    if shape == "wide":
        assert (x >> np.uint64(63)).any() and (x >> np.uint64(8) == 0).any() and int(b.mc["mer"].max()) == (1 << 56) - 1
    if shape == "mixed":
        hs, sp = np.unique(x >> np.uint64(8)), np.unique(x & np.uint64(255))
        assert len(hs) < len(np.unique(x)) and len(sp) > 4
    return b


def fan_in(trail):
    """groups that arise only from REVERSED records: many distinct first keys before one common second key"""
    rng = np.random.default_rng(31 + trail)
    sizes = (48, 49, 197, 788, 789)
    ks = _keys("real", len(sizes) + sum(sizes), rng)
    loci, want, at = [], {}, len(sizes)
    for k1, n in zip(ks, sizes):
        loci += _star(k1, ks[at:at + n], trail, fan_in=True)
        want[key(*k1)] = (n, trail)
        at += n
    b = Built(*build_db(loci, seed=6), runs=[dict(mc_lower=1, mc_upper=BIG_UPPER)])
    m = _check_stars(b, b.runs[0], want)
    assert all(d == 1 for k0 in want for r in m.groups[k0].recs.values() for _, d in r) and m.n_big() == 4
    return b


def beyond_a_wavefront():
    rng = np.random.default_rng(41)
    ks = _keys("real", 1 + VISIT_WAVE_MAX + 1, rng)
    b = Built(*build_db(_star(ks[0], ks[1:], True), seed=7), runs=[dict(mc_lower=1, mc_upper=BIG_UPPER)], wave_overflow=True)
    m = _check_stars(b, b.runs[0], {key(*ks[0]): (VISIT_WAVE_MAX + 1, True)})
    assert m.max_group() == VISIT_WAVE_MAX + 1
    return b


# ---- join rules: one small design per rule ---------------------------------------------------------------------------------
def _pairs_loci(n, h0, gap=300, starts=STARTS3, first=200):
    return [Locus([(first, h0 + 2 * i, 16), (first + gap, h0 + 2 * i + 1, 16)], starts) for i in range(n)]


def _differs(a, kwa, b, kwb):
    """the oracle's answer on the two sides of an edge"""
    (_, sa), (_, sb) = a.oracle(kwa), b.oracle(kwb)
    assert (sa["n_records"], sa["n_buckets"], sa["n_align"]) != (sb["n_records"], sb["n_buckets"], sb["n_align"]), (sa, sb)


def rule_gap(gap):
    b = Built(*build_db(_pairs_loci(5, 1000, gap=gap), seed=8), runs=[{}])
    other = Built(*build_db(_pairs_loci(5, 1000, gap=199 - gap), seed=8), runs=[{}])
    m = b.model({})
    assert (m.n_records, m.drops["gap"]) == ((0, 15) if gap == 99 else (30, 0))
    _differs(b, {}, other, {})
    return b


def rule_anchor_advances():
    """three shimmers 60 apart: no pair, although the outer two are 120 apart"""
    loci = [Locus([(200, 1000 + 3 * i, 16), (260, 1001 + 3 * i, 16), (320, 1002 + 3 * i, 16)]) for i in range(4)]
    b = Built(*build_db(loci, seed=9), runs=[{}])
    m = b.model({})
    assert m.n_records == 0 and m.drops["gap"] == 2 * 12
    two = [Locus([lc.shimmers[0], lc.shimmers[2]]) for lc in loci]
    _differs(b, {}, Built(*build_db(two, seed=9), runs=[{}]), {})
    return b


def rule_list_head():
    """the list's first shimmer occurs 15 times: mc_upper 15 (count == upper: the scan starts one shimmer later), 16, 14"""
    loci = [Locus([(200, 7, 16), (500, 1000 + i, 16)]) for i in range(5)]
    b = Built(*build_db(loci, seed=10), runs=[dict(mc_upper=u) for u in (15, 16, 14)])
    ms = [b.model(kw) for kw in b.runs]
    assert ms[0].count[7] == 15 and b.mm["x"][0] == key(7)
    assert [m.n_records for m in ms] == [28, 30, 0] and [m.drops["head"] for m in ms] == [1, 0, 0]
    _differs(b, b.runs[0], b, b.runs[1]), _differs(b, b.runs[0], b, b.runs[2])
    return b


def rule_later_elements():
    """a middle shimmer at lower - 1 / lower and at upper / upper + 1: skipped, its neighbours pair across it (the anchor stays)"""
    loci = []
    for i in range(4):      # a, c occur 6 times, the middle one 3 times
        loci.append(Locus([(150, 100 + i // 2, 16), (300, 200 + i, 16), (450, 300 + i // 2, 16)]))
    for i in range(4):      # a, c occur 6 times, the middle one 12 times
        loci.append(Locus([(150, 400 + i // 2, 16), (300, 500, 16), (450, 600 + i // 2, 16)]))
    b = Built(*build_db(loci, seed=11), runs=[dict(mc_lower=lo, mc_upper=up) for lo in (3, 4) for up in (12, 11)])
    for kw in b.runs:
        m = b.model(kw)
        assert {m.count[h] for h in (100, 300, 400, 600)} == {6} and m.count[200] == 3 and m.count[500] == 12
        low, high = kw["mc_lower"] == 4, kw["mc_upper"] == 11
        assert (m.drops["low"], m.drops["high"]) == (12 * low, 12 * high)
        assert (key(300) in m.groups[key(100)].recs) == low and (key(200) in m.groups[key(100)].recs) == (not low)
        assert (key(600) in m.groups[key(400)].recs) == high and (key(500) in m.groups[key(400)].recs) == (not high)
    _differs(b, b.runs[0], b, b.runs[1]), _differs(b, b.runs[0], b, b.runs[2])
    return b


def rule_split_rows():
    """multiplicities that reach a threshold only as the sum of their rows; rows for hashes that occur nowhere"""
    loci = [Locus([(150, 100 + i, 16), (300, 50, 16), (450, 200 + i, 16)]) for i in range(3)]     # hash 50: 9 times, rows 3 + 3 + 3
    loci += [Locus([(150, 300 + i, 16), (300, 60, 16), (450, 400 + i, 16)]) for i in range(6)]    # hash 60: 18 times, rows 9 + 9
    loci += [Locus([(150, 500 + i, 16), (450, 500 + i, 16)], (0, 40, 110, 0, 40)) for i in range(2)]       # 10 times: in range whatever the rows
    db, mm, mc = build_db(loci, seed=12, split={50: 3, 60: 2}, absent={70: 5, 0: 3, 80: 0})
    mc2 = mc.copy()
    mc2["count"][np.isin(mc2["mer"], (100, 101, 102, 200, 201, 202, 300, 301, 302, 303, 304, 305, 400, 401, 402, 403, 404, 405))] = 5
    b = Built(db, mm, mc2, runs=[dict(mc_lower=4, mc_upper=11)])
    m = b.model(b.runs[0])
    assert sorted(mc2["count"][mc2["mer"] == 50]) == [3, 3, 3] and sorted(mc2["count"][mc2["mer"] == 60]) == [9, 9]
    assert m.count[50] == 9 and m.count[60] == 18 and m.drops["high"] == 18 and m.drops["low"] == 0
    assert key(50) in m.groups[key(100)].recs and key(400) in m.groups[key(300)].recs
    first_row = np.zeros(len(mc2), bool)
    first_row[np.unique(mc2["mer"], return_index=True)[1]] = True
    _differs(b, b.runs[0], Built(db, mm, mc2[first_row], runs=[]), b.runs[0])   # one row per hash: 50 is dropped, 60 is kept
    return b


def rule_sparse_reads():
    """reads with one kept shimmer, reads whose shimmers are all dropped, reads with no shimmer at all, between ordinary ones"""
    loci = _pairs_loci(2, 1000)
    loci.append(Locus([(300, 50, 16)]))                              # one kept shimmer a read
    loci.append(Locus([], (0, 40)))                                  # no shimmer at all
    loci.append(Locus([(200, 60, 16), (450, 61, 16)], (0,)))         # both occur once: below lower
    loci.append(Locus([(200, 62, 16), (450, 51, 16)], (0,)))         # one dropped, one kept ...
    loci.append(Locus([(100, 51, 16)], (0,)))                        # ... (51 occurs twice)
    loci += _pairs_loci(2, 2000)
    b = Built(*build_db(loci, seed=13), runs=[{}])
    m = b.model({})
    assert m.n_records == 4 * 3 * 2 and m.drops["low"] == 3 and m.drops["read"] >= 12 and len(b.db.rid) == 20
    assert not any(key(h) in m.groups for h in (50, 51, 60, 61, 62))
    return b


def rule_read_boundary():
    """the last shimmer of a read next to the first shimmer of the following read, 150 bases further on (and 350 bases back)"""
    loci = [Locus([(150, 100, 16), (300, 101, 16)]), Locus([(450, 102, 16), (600, 103, 16)])]
    b = Built(*build_db(loci, seed=14), runs=[{}])
    m = b.model({})
    assert m.drops["read"] == 5 and set(m.groups[key(101)].recs) == {key(100)} and m.n_records == 12
    one = Built(*build_db([Locus(loci[0].shimmers + loci[1].shimmers)], seed=14), runs=[{}])
    assert key(102) in one.model({}).groups[key(101)].recs
    _differs(b, {}, one, {})
    return b


def rule_same_key_twice():
    """the same key twice (four times) in a read: the forward and the reverse record of a pair meet in bucket (K, K)"""
    loci = [Locus([(150, 100, 16), (400, 100, 16)]), Locus([(150, 200, 16), (300, 200, 16), (450, 200, 16), (600, 200, 16)])]
    b = Built(*build_db(loci, seed=15), runs=[{}], env=dict(PGX_REPLAY_BIG="2", PGX_REPLAY_DUP="2"))
    m = b.model({})
    assert set(m.groups) == {key(100), key(200)} and all(g.key1s == [k0] for k0, g in m.groups.items())
    assert [len(g.recs[k0]) for k0, g in m.groups.items()] == [6, 18] and {d for _, d in m.groups[key(100)].recs[key(100)]} == {0, 1}
    return b


def rule_position_ties():
    """equal positions within a bucket: the sort is stable, ties stay in insertion order"""
    loci = [Locus([(200, 1000 + 2 * i, 16), (500, 1001 + 2 * i, 16)], (0, 0, 40, 0, 40)) for i in range(3)]
    b = Built(*build_db(loci, seed=16), runs=[{}, dict(bestn=1)])
    m = b.model({})
    pos = [p for p, _ in m.groups[key(1000)].recs[key(1001)]]
    assert pos == [200, 200, 160, 200, 160]
    return b


def rule_bucket_sizes():
    """buckets of 2, 3, ovlp_upper and ovlp_upper + 1 records at ovlp_upper = 5"""
    st = (0, 40, 110, 20, 60, 90)
    loci = [Locus([(200, 1000 + 2 * i, 16), (500, 1001 + 2 * i, 16)], st[:n]) for i, n in enumerate((2, 3, 5, 6))]
    b = Built(*build_db(loci, seed=17), runs=[dict(ovlp_upper=5), dict(ovlp_upper=6)])
    m = b.model({})
    assert [len(g.recs[g.key1s[0]]) for g in m.groups.values()] == [2, 2, 3, 3, 5, 5, 6, 6]
    assert (m.n_buckets(5), m.n_buckets(6)) == (4, 6)
    _differs(b, b.runs[0], b, b.runs[1])
    return b


def rule_chunks():
    """total_chunk 2, 3, 7 with every mychunk: consecutive hashes, so a pair's forward and reverse record have different owners"""
    loci = _pairs_loci(42, 1000)
    runs = [dict(total_chunk=t, mychunk=c) for t in (2, 3, 7) for c in range(1, t + 1)]
    b = Built(*build_db(loci, seed=18), runs=runs)
    whole = b.model({}).n_records
    for t in (2, 3, 7):
        ms = [b.model(kw) for kw in runs if kw["total_chunk"] == t]
        assert {int(x >> np.uint64(8)) % t for x in b.mm["x"]} == set(range(t))
        assert sum(m.n_records for m in ms) == whole and all(0 < m.n_records < whole and m.drops["chunk"] for m in ms)
        for m in ms:    # no chunk owns both records of a pair
            assert all(k1 not in m.groups or k0 not in m.groups[k1].recs for k0, g in m.groups.items() for k1 in g.recs)
    _differs(b, runs[0], b, runs[2])
    return b


# ---- seeded mixes ----------------------------------------------------------------------------------------------------------
def seeded_mix(seed):
    """random loci over a small key alphabet -- three hub keys that many loci hold, 500 others --, spacings 40 .. 400, random read
    starts (a read may begin after its locus's first shimmers), random thresholds between the hubs' multiplicities"""
    rng = np.random.default_rng(seed)
    alpha = _keys("mixed" if seed % 2 else "real", 503, rng)
    hubs, others = alpha[:3], alpha[3:]
    loci = []
    for _ in range(420):
        off, shim = int(rng.integers(60, 200)), []
        for _j in range(int(rng.integers(2, 7))):
            u = rng.random()
            k = hubs[0] if u < 0.22 else hubs[1] if u < 0.40 else hubs[2] if u < 0.50 else others[int(rng.integers(len(others)))]
            shim.append((off, *k))
            off += int(rng.integers(40, 401))
        starts = tuple(int(s) for s in rng.integers(0, 260, int(rng.integers(1, 6))))
        loci.append(Locus(shim, starts, read_len=1400, subs=3 if seed % 3 == 0 else 0))   # (every third seed: three substitutions a read)
    db, mm, mc = build_db(loci, seed=seed)
    cnt = Counter((mm["x"] >> np.uint64(8)).tolist())
    assert len({h for h, _ in hubs}) == 3
    c0, c1 = sorted((cnt[h] for h, _ in hubs), reverse=True)[:2]    # mc_upper drops the most frequent hub and keeps the second
    assert c0 > c1 + 1
    kw = dict(mc_lower=int(rng.integers(3, 9)), mc_upper=int(rng.integers(c1, c0)), bestn=(4, 2, 1)[seed % 3],
              ovlp_upper=int(rng.integers(20, 121)))
    b = Built(db, mm, mc, runs=[kw])
    m = b.model(kw)
    assert m.n_big() >= 1 and m.max_group() <= VISIT_WAVE_MAX, (m.n_big(), m.max_group())
    assert all(m.drops[r] > 0 for r in ("low", "high", "gap", "read")), m.drops
    return b


DESIGNS = {f"tables-{s}-{'trail' if t else 'notrail'}": functools.partial(table_sizes, s, t) for s in ("real", "wide", "mixed") for t in (1, 0)}
DESIGNS.update({"fan-in-trail": functools.partial(fan_in, 1), "fan-in-notrail": functools.partial(fan_in, 0),
                "beyond-a-wavefront": beyond_a_wavefront,
                "gap-99": functools.partial(rule_gap, 99), "gap-100": functools.partial(rule_gap, 100),
                "anchor-advances": rule_anchor_advances, "list-head": rule_list_head, "later-elements": rule_later_elements,
                "split-rows": rule_split_rows, "sparse-reads": rule_sparse_reads, "read-boundary": rule_read_boundary,
                "same-key-twice": rule_same_key_twice, "position-ties": rule_position_ties, "bucket-sizes": rule_bucket_sizes,
                "chunks": rule_chunks})
DESIGNS.update({f"mix-{s}": functools.partial(seeded_mix, s) for s in (101, 102, 103)})


@functools.lru_cache(maxsize=None)
def built(name) -> Built:
    return DESIGNS[name]()


@functools.lru_cache(maxsize=None)
def oracle_of(name, run):
    """the oracle's stream and counters for run `run` of a design: computed once, shared, never changed"""
    b = built(name)
    ov, st = b.oracle(b.runs[run])
    ov.setflags(write=False)
    return ov, st
