"""k_eval_big's WALK on one wavefront (pgx_replay.h): a row at a time, 64 partners per pass, the ballots of a pass in scalar registers, a
row of more than 64 remaining partners continued in a second pass, a duplicate inside a pass resolved within the wavefront.  The cases are
the smallest sets at which that can go wrong; every one first shows on the CPU, from the oracle's records laid over the oracle's buckets,
that its set really holds the shape it is named for, then compares the record SEQUENCE, n_align_needed, n_seen_skip and the stream
checksum with the oracle (shmr_overlap.c:52-180 over the same tables).  The sets are those of test_gpu_eval_big_lookup.py."""
import numpy as np
import pytest

import oracle_util as U
from peregrine_amd import _lib, formats, simreads
from peregrine_amd.shimmer import ResidentDB

pytestmark = pytest.mark.gpu

T_OVERLAP, T_CONTAINS, T_CONTAINED = 0, 1, 2
PASS = 64   # partners of a row per pass of the walk


class Shapes:
    """The oracle's buckets in walk layout (entries descending by position, stable) and, for every record of the oracle, its place in
    the walk: bucket, row, partner (entry indices) and type.  A record (row, partner) says that the walk of `row` went at least as far
    as `partner` and inserted the pair there."""

    def __init__(self, db, top, top_mc, want, mychunk, total, mc_upper, ovlp_upper):
        rl = np.zeros(int(db.rid.max()) + 1, np.uint32)
        rl[db.rid] = db.rlen
        recs = U.orc_pair_records(top, top_mc, rl, mychunk=mychunk, total=total, mc_upper=mc_upper)
        _, inv = np.unique(np.stack([recs["key0"], recs["key1"]], 1), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        pos = ((recs["y0"] & np.uint64(0xFFFFFFFF)) >> np.uint64(1)).astype(np.int64)
        order = np.lexsort((np.arange(len(recs)), -pos, inv))   # bucket, then position descending, then insertion order (sort_bucket)
        b = inv[order]
        start = np.r_[0, np.flatnonzero(np.diff(b)) + 1]
        self.size = np.diff(np.r_[start, len(b)])                # entries per bucket
        idx = np.arange(len(b)) - np.repeat(start, self.size)
        self.rid = [r for r in np.split((recs["y0"][order] >> np.uint64(32)).astype(np.int64), start[1:])]   # per bucket: the entries' reads
        walked = (self.size[b] > 2) & (self.size[b] <= ovlp_upper)
        where = {}
        for y, d, bb, ii in zip(recs["y0"][order][walked].tolist(), recs["dir"][order][walked].tolist(), b[walked].tolist(), idx[walked].tolist()):
            assert (y, d) not in where, "an entry belongs to one bucket"
            where[(y, d)] = (bb, ii)
        r0 = [where[k] for k in zip(want["y0"].tolist(), want["strand0"].tolist())]
        r1 = [where[k] for k in zip(want["y1"].tolist(), want["strand1"].tolist())]
        self.bucket = np.array([x[0] for x in r0])
        assert np.array_equal(self.bucket, np.array([x[0] for x in r1])), "both reads of a record sit in the record's bucket"
        self.row, self.par = np.array([x[1] for x in r0]), np.array([x[1] for x in r1])
        assert (self.par > self.row).all()
        self.type = want["ovlp_type"].astype(np.int64)
        self.n = self.size[self.bucket]                          # per record: entries of its bucket
        self.off = self.par - self.row - 1                       # per record: the partner's offset among its row's partners

    def repeats(self, times):
        """buckets (of a walked size) that hold some read at least `times` times: {bucket: [(read, entry indices)]}"""
        out = {}
        for bb in np.unique(self.bucket).tolist():
            rid = self.rid[bb]
            u, c = np.unique(rid, return_counts=True)
            if (c >= times).any():
                out[bb] = [(int(x), np.flatnonzero(rid == x)) for x in u[c >= times]]
        return out


class _Set:
    """a read set resident on the GPU, its index, and the oracle's answers (computed once per parameter set)"""

    def __init__(self, db):
        self.db, self.rdb = db, ResidentDB(db, 0)
        self.ix = self.rdb.index()
        self._want, self._shapes = {}, {}

    @staticmethod
    def okw(kw):
        return dict(mychunk=kw.get("mychunk", 1), total=kw.get("total_chunk", 1), mc_upper=kw.get("mc_upper", 240), bestn=kw.get("bestn", 4),
                    ovlp_upper=kw.get("ovlp_upper", 120))

    def want(self, kw):
        key = tuple(sorted(self.okw(kw).items()))
        if key not in self._want:
            self._want[key] = U.orc_overlap(self.db, self.ix.top, self.ix.top_mc, **self.okw(kw))
        return self._want[key]

    def shapes(self, kw):
        o = self.okw(kw)
        key = tuple(sorted(o.items()))
        if key not in self._shapes:
            self._shapes[key] = Shapes(self.db, self.ix.top, self.ix.top_mc, self.want(kw)[0], o["mychunk"], o["total"], o["mc_upper"], o["ovlp_upper"])
        return self._shapes[key]


@pytest.fixture(scope="module")
def family8():
    # one family of 8 exact copies at 24x, the multiplicity cut-off lifted by the caller: buckets of up to 138 entries, two of 65 and two of 128
    g = simreads.make_genome(1_200_000, 21, repeat_families=1, repeat_len=3000, repeat_copies=8, divergence=0.0)
    s = _Set(simreads.simulate_reads(g, seed=1, coverage=24, mean_len=9000, sd_len=1500))
    yield s
    s.rdb.close()


@pytest.fixture(scope="module")
def tandem():
    # tandem arrays put a read two and three times into a bucket
    g = simreads.make_genome(600_000, 9, repeat_families=2, repeat_len=4000, repeat_copies=6, tandem=60)
    s = _Set(simreads.simulate_reads(g, seed=43, coverage=30, mean_len=9000, sd_len=1500))
    yield s
    s.rdb.close()


def _run(s, monkeypatch, env, kw, min_records):
    want, ost = s.want(kw)
    assert len(want) > min_records
    monkeypatch.setenv("PGX_GPU_REPLAY", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, st = s.rdb.overlap(s.ix.top, s.ix.top_mc, **kw)
    print(env, kw, len(got), {k: st[k] for k in ("n_align_needed", "n_seen_skip", "rounds", "n_evaluations")})
    assert st["device_replay"] == 1 and formats.ovlp_fields_equal(got, want), (env, kw)
    assert st["n_align_needed"] == ost["n_align"] and st["n_seen_skip"] == ost["n_seen_skip"], (env, kw, st, ost)
    assert st["stream_checksum"] == formats.stream_checksum(want), (env, kw)
    return st


ALL_BIG = dict(PGX_REPLAY_BIG="2", PGX_REPLAY_DUP="2")   # every visited bucket, from 3 entries on, goes through k_eval_big
WIDE = dict(mc_upper=100000, ovlp_upper=128)             # the family's buckets are walked, up to 128 entries


def test_second_pass_holds_the_stop(family8, monkeypatch):
    """bestn 8, buckets of 65 to 128 entries: rows that insert a pair at partner offset 64 and beyond -- their first pass neither reached
    best-n nor ended the row, and the stop lies in the second"""
    kw = dict(WIDE, bestn=8)
    sh = family8.shapes(kw)
    far = (sh.n >= 65) & (sh.n <= 128) & (sh.off >= PASS)
    print("records inserted at offset >= 64:", int(far.sum()), "in", len(np.unique(sh.bucket[far])), "buckets; of type overlap", int((far & (sh.type == T_OVERLAP)).sum()))
    assert far.sum() >= 10 and (far & (sh.type == T_OVERLAP)).any()
    _run(family8, monkeypatch, ALL_BIG, kw, 5000)


def test_first_pass_reaches_bestn(family8, monkeypatch):
    """bestn 1: rows of more than 64 partners whose first pass inserts an overlap -- the row is complete, no second pass; and no record
    of such a row lies behind its first overlap"""
    kw = dict(WIDE, bestn=1)
    sh = family8.shapes(kw)
    early = (sh.n - sh.row - 1 > PASS) & (sh.off < PASS) & (sh.type == T_OVERLAP)
    print("rows of > 64 partners ended by an overlap of their first pass:", int(early.sum()))
    assert early.sum() >= 10
    _run(family8, monkeypatch, ALL_BIG, kw, 5000)


def test_stop_never_reached(family8, monkeypatch):
    """bestn 1000 > the 127 partners a row can have: no row ever reaches best-n, every one runs to its last partner or its containment"""
    kw = dict(WIDE, bestn=1000)
    sh = family8.shapes(kw)
    assert sh.size[np.unique(sh.bucket)].max() <= 128 < kw["bestn"]
    per_row = np.unique(np.stack([sh.bucket, sh.row], 1)[sh.type == T_OVERLAP], axis=0, return_counts=True)[1]
    print("most overlaps inserted by one row:", int(per_row.max()), "; records at offset >= 64:", int((sh.off >= PASS).sum()))
    assert per_row.max() > 8 and (sh.off >= PASS).sum() >= 10   # (more than any bestn in use would allow; rows with a second pass among them)
    _run(family8, monkeypatch, ALL_BIG, kw, 5000)


def _same_read_behind(sh, times=2):
    """per record (row, partner p1) of a bucket that holds p1's read again at p2 > p1: the offsets of p1 and of the nearest such p2 in the row"""
    out = []
    rep = sh.repeats(times)
    for i in np.flatnonzero(np.isin(sh.bucket, list(rep))).tolist():
        for _, at in rep[int(sh.bucket[i])]:
            later = at[at > sh.par[i]]
            if sh.par[i] in at and len(later):
                out.append((i, int(sh.off[i]), int(later[0] - sh.row[i] - 1)))
    return out


@pytest.mark.parametrize("bestn", [4, 1000])
def test_duplicate_within_a_pass(tandem, monkeypatch, bestn):
    """a row inserts a pair at partner p1 and the same read stands again at p2, both among the row's first 64 partners: p2 meets the pair in
    the pass that inserts it -- the row is cut in front of p2, and p2 finds the pair in the set in the next pass"""
    kw = dict(bestn=bestn)
    sh = tandem.shapes(kw)
    hits = [h for h in _same_read_behind(sh) if h[2] < PASS]
    print("insertions with the same read again within the first pass:", len(hits))
    assert len(hits) >= 10
    _run(tandem, monkeypatch, ALL_BIG, kw, 5000)


def test_duplicate_across_passes(tandem, monkeypatch):
    """a bucket of more than 64 entries: a row inserts a pair in its first pass and the same read stands again at offset 64 or beyond.  With
    bestn 1000 only a containment ends a row early, so the row's later pass looks at the second occurrence -- unless the row was ended or the
    occurrence flagged contained before -- and has to find the pair in the LDS set"""
    kw = dict(bestn=1000)
    sh = tandem.shapes(kw)
    hits = 0
    for i, o1, o2 in _same_read_behind(sh):
        if not o1 < PASS <= o2:
            continue
        here = sh.bucket == sh.bucket[i]
        row, p2 = sh.row[i], sh.row[i] + 1 + o2
        ended = (here & (sh.row == row) & (sh.type == T_CONTAINED) & (sh.off < o2)).any()
        flagged = (here & (((sh.type == T_CONTAINS) & (sh.par == p2) & (sh.row > row)) | ((sh.type == T_CONTAINED) & (sh.row == p2)))).any()
        hits += not ended and not flagged
    print("insertions of a first pass whose read is looked at again in a later pass of the row:", hits)
    assert hits >= 1
    _run(tandem, monkeypatch, ALL_BIG, kw, 5000)


def test_read_three_times(tandem, monkeypatch):
    """buckets that hold a read three times, and rows that insert the pair at its first occurrence"""
    kw = dict(bestn=8)
    sh = tandem.shapes(kw)
    rep = sh.repeats(3)
    hits = [h for h in _same_read_behind(sh, 3)]
    print("buckets holding a read three times:", len(rep), "; insertions at an occurrence with another behind it:", len(hits))
    assert len(rep) >= 3 and len(hits) >= 3
    _run(tandem, monkeypatch, ALL_BIG, kw, 5000)


def test_containment(family8, monkeypatch):
    """rows ended by a `contained` result, and partners flagged contained by a row that has rows below it (they skip the partner), both in
    buckets below and above 64 entries"""
    kw = dict(WIDE, bestn=4)
    sh = family8.shapes(kw)
    for name, sel in (("<= 64 entries", sh.n <= 64), ("> 64 entries", sh.n > 64)):
        ended, flagged = sel & (sh.type == T_CONTAINED), sel & (sh.type == T_CONTAINS) & (sh.row > 0)
        print(name, ": rows ended by a containment", int(ended.sum()), ", partners flagged above lower rows", int(flagged.sum()))
        assert ended.sum() >= 3 and flagged.sum() >= 3
    _run(family8, monkeypatch, ALL_BIG, kw, 5000)


BIG_WG = 512   # workgroups of a k_eval_big launch at the most (pgx_replay.h; no CU term), striding over the pass's list of big buckets


def test_a_workgroup_walks_many_buckets(family8, monkeypatch):
    """Every bucket of 3 .. 128 entries is dirty in the first pass, and under PGX_REPLAY_BIG=2 every one of them is on that pass's big
    list: more than two grids of them, so in every test of this file that uses ALL_BIG on family8 a workgroup of k_eval_big walks bucket
    after bucket on the same LDS (s_fact, s_vis / s_ins, the pair set).  Here the same under PGX_GRID_CAP = 3: three workgroups take
    them all."""
    kw = dict(WIDE, bestn=8)
    sh = family8.shapes(kw)
    walked = int(((sh.size > 2) & (sh.size <= kw["ovlp_upper"])).sum())
    print("buckets of 3 ..", kw["ovlp_upper"], "entries:", walked)
    assert walked > 2 * BIG_WG
    monkeypatch.setenv("PGX_GRID_CAP", "3")
    assert _lib.load().pgx_stride_grid(2**40, 32) == 3
    _run(family8, monkeypatch, ALL_BIG, kw, 5000)


def test_re_evaluation_with_default_thresholds(tandem, monkeypatch):
    """default thresholds, several sweeps: the walk runs over facts from settled and from pending memo entries"""
    st = _run(tandem, monkeypatch, dict(), dict(bestn=4), 5000)
    assert st["rounds"] > 1, st


@pytest.mark.parametrize("env", [dict(PGX_REPLAY_TIMING="1"), dict(PGX_REPLAY_WIN="64")], ids=["timing", "win64"])
def test_the_other_schedules(family8, monkeypatch, env):
    """the 128-entry case behind the narrow kernel (every kernel timed by itself) and from the window's list"""
    kw = dict(WIDE, bestn=8)
    sh = family8.shapes(kw)
    assert (sh.n == 128).any() and ((sh.n == 128) & (sh.off >= PASS)).any()
    _lib.timing_reset()
    _run(family8, monkeypatch, dict(ALL_BIG, **env), kw, 5000)
    if "PGX_REPLAY_TIMING" in env:
        assert _lib.timing("replay_big")[1] > 0
