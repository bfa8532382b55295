"""k_eval_big in three phases (pgx_replay.h): LOOK finds what the walk needs of every (row, partner) pair of a bucket and leaves a byte
per pair in LDS, WALK steps through the rows on LDS alone and notes what it visited and inserted in two 128-bit masks per row, COMMIT
registers the visited pairs as readers and writes the inserted ones as the bucket's item list.  The cases are the smallest sets at which
a phase can go wrong: buckets at the edges of the layout (64, 65 and 128 entries: the boundary between a row's two mask halves, the last
row and partner index), buckets that hold a read two and three times (rows cut at duplicates and continued alone), re-evaluations in
later sweeps (the "listed already?" test, memo hits with settled and pending requests), and the two other schedules of the kernel.
Every case: record SEQUENCE and the two counters against the oracle (shmr_overlap.c:52-180 over the same tables)."""
import numpy as np
import pytest

import oracle_util as U
from peregrine_amd import _lib, formats, simreads
from peregrine_amd.shimmer import ResidentDB

pytestmark = pytest.mark.gpu


class _Set:
    """a read set resident on the GPU, its index, and the oracle's answers (computed once per parameter set)"""

    def __init__(self, db):
        self.db, self.rdb = db, ResidentDB(db, 0)
        self.ix = self.rdb.index()
        self._want = {}

    def want(self, **okw):
        key = tuple(sorted(okw.items()))
        if key not in self._want:
            self._want[key] = U.orc_overlap(self.db, self.ix.top, self.ix.top_mc, **okw)
        return self._want[key]

    def bucket_sizes(self, mc_upper):
        """entries per bucket = records per (first shimmer, second shimmer) key in build_map's insertion sequence (the oracle, on the CPU)"""
        rl = np.zeros(int(self.db.rid.max()) + 1, np.uint32)
        rl[self.db.rid] = self.db.rlen
        recs = U.orc_pair_records(self.ix.top, self.ix.top_mc, rl, mc_upper=mc_upper)
        return np.unique(np.stack([recs["key0"], recs["key1"]], 1), axis=0, return_counts=True)[1]


def _family_set(copies, seed):
    # the recipe of test_device_visit_order_equals_oracle_and_host_visit: one family of exact copies, the multiplicity cut-off lifted by the caller
    g = simreads.make_genome(1_200_000, 21, repeat_families=1, repeat_len=3000, repeat_copies=copies, divergence=0.0)
    return _Set(simreads.simulate_reads(g, seed=seed, coverage=24, mean_len=9000, sd_len=1500))


@pytest.fixture(scope="module")
def family8():
    s = _family_set(8, 1)   # (8 copies at 24x: buckets of up to 138 entries, two of 65 and two of 128 among them)
    yield s
    s.rdb.close()


@pytest.fixture(scope="module")
def family5():
    s = _family_set(5, 7)   # (buckets of up to 71 entries, two of 64)
    yield s
    s.rdb.close()


@pytest.fixture(scope="module")
def tandem():
    # the genome of test_workgroup_evaluation_of_repeat_buckets_equals_oracle: tandem arrays put a read two and three times into a bucket
    g = simreads.make_genome(600_000, 9, repeat_families=2, repeat_len=4000, repeat_copies=6, tandem=60)
    s = _Set(simreads.simulate_reads(g, seed=43, coverage=30, mean_len=9000, sd_len=1500))
    yield s
    s.rdb.close()


def _run(s, monkeypatch, env, kw, min_records):
    okw = dict(mychunk=kw.get("mychunk", 1), total=kw.get("total_chunk", 1), mc_upper=kw.get("mc_upper", 240), bestn=kw.get("bestn", 4),
               ovlp_upper=kw.get("ovlp_upper", 120))
    want, ost = s.want(**okw)
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


@pytest.mark.parametrize("which,ovlp_upper,sizes", [("family8", 128, (65, 128)), ("family8", 65, (65,)), ("family5", 128, (64,))],
                         ids=["upper128-sizes65+128", "upper65-size65", "upper128-size64"])
def test_buckets_at_the_edges_of_the_layout(request, monkeypatch, which, ovlp_upper, sizes):
    """buckets of exactly 64, 65 and 128 = ovlp_upper entries (and of exactly ovlp_upper = 65), all through the workgroup kernel"""
    s = request.getfixturevalue(which)
    n = s.bucket_sizes(100000)
    print(which, "buckets", len(n), "largest", int(n.max()), {k: int((n == k).sum()) for k in (64, 65, 128)})
    for k in sizes:
        assert (n == k).any(), (which, k)
    if which == "family8":
        assert (n >= 65).any() and (n == ovlp_upper).any()
    _run(s, monkeypatch, ALL_BIG, dict(mc_upper=100000, ovlp_upper=ovlp_upper), 5000)


@pytest.mark.parametrize("bestn", [1, 4, 8])
def test_buckets_that_hold_a_read_twice_and_three_times(tandem, monkeypatch, bestn):
    """tandem arrays: a pair met again within the evaluation is found in the LDS set, a duplicate within a step cuts its row, the row is
    continued alone -- its masks are noted over several steps, its insertions numbered behind those of the rows above"""
    _run(tandem, monkeypatch, ALL_BIG, dict(bestn=bestn), 5000)


@pytest.mark.parametrize("kw", [dict(), dict(total_chunk=2, mychunk=2)], ids=["whole", "chunk2of2"])
def test_re_evaluations_in_later_sweeps(tandem, monkeypatch, kw):
    """the default thresholds: buckets are evaluated again (first_eval false: COMMIT's "listed already?" test) with the memo filled and
    requests both settled and pending"""
    st = _run(tandem, monkeypatch, dict(), kw, 5000)
    assert st["rounds"] > 1, st


def test_behind_the_narrow_kernel(tandem, monkeypatch):
    """PGX_REPLAY_TIMING=1: every kernel between events, k_eval_big behind the narrow kernel of its pass instead of beside it"""
    _lib.timing_reset()
    _run(tandem, monkeypatch, dict(ALL_BIG, PGX_REPLAY_TIMING="1"), dict(), 5000)
    assert _lib.timing("replay_big")[1] > 0


def test_small_windows(tandem, monkeypatch):
    """PGX_REPLAY_WIN=64: the dense rounds in windows of 64 buckets, k_eval_big from the list each window's narrow kernel notes"""
    _run(tandem, monkeypatch, dict(ALL_BIG, PGX_REPLAY_WIN="64"), dict(), 5000)
