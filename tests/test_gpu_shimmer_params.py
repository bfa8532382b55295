"""Everything after the index stage on lists made with other shimmer parameters than w = 80, k = 16, r = 6, two levels.

shmr_index takes -w -k -r -l and its lists go into shmr_overlap, shmr_dedup and shmr_map; what reads them depends on the parameters:
k sets the width of the hashes (the occupied bits the join's radix sort covers, the high term of khash's hash in both table levels of
the visit order, chunk ownership (x >> 8) % T, the keys of the count and first-insert tables), small w / r and one level make lists
so dense that the gap rule (pair only at >= 100 bases) decides nearly every record, and k = 12 / k = 28 make the keys crowded /
sparse.  Every row below runs index, overlap (every dispatch of the greedy walk, two chunkings), the one-call pipeline, and -- on
some rows -- the alignment kernels on the stream's own keys, shmr_map, the shimmer4py query helpers and the multi-rank record
scatter, all bit for bit against the CPU oracle computed here (pinned to the compiled reference at the same rows by
tests/test_oracle_vs_ref.py).  All comparisons are on integers and exact."""
import numpy as np
import pytest

import oracle_util as U
from peregrine_amd import _lib, formats, simreads
from peregrine_amd.shimmer import ResidentDB, ShimmerMap, map_reads_to_ref

pytestmark = pytest.mark.gpu

# (w, k, r, levels): (records of the oracle's stream for overlap chunk 1 of 1, for chunk 2 of 3 over the two-chunk lists)
ROWS = {
    (80, 16, 6, 2): (5672, 4172),   # the reference's defaults: the control
    (80, 20, 6, 2): (5674, 4095),
    (80, 28, 6, 2): (5197, 3201),   # 56-bit hashes: 64-bit join keys, sparse key population
    (48, 12, 4, 2): (6891, 6061),   # 24-bit hashes: high multiplicities, the mc_upper cut is active
    (64, 24, 3, 2): (7374, 6341),
    (80, 16, 2, 1): (6390, 5444),   # dense lists
    (40, 15, 2, 1): (154, 64),       # the densest: nearly every consecutive pair falls under the 100-base gap
    (128, 16, 3, 1): (6897, 5997),
    (32, 14, 12, 1): (6878, 6125),
    (255, 28, 2, 1): (6672, 5225),
    (100, 17, 5, 2): (5862, 4438),   # the first k at which kh32's high term is wider than at k = 16
}
K28, K12, W40, W64 = (80, 28, 6, 2), (48, 12, 4, 2), (40, 15, 2, 1), (64, 24, 3, 2)
SETTINGS = {K28: dict(bestn=2, mc_upper=30, ovlp_upper=60), K12: dict(mc_lower=1, mc_upper=1000), W40: dict(align_bandwidth=30)}
SETTING_RECORDS = {K28: 3814, K12: 6825, W40: 154}   # records of the oracle's stream, chunk 1 of 1, under the row's setting
GENOME_LEN = 300_000   # (the device form of the visit order engages at this size once PGX_EARLY_OUTER_MIN=1 lets the outer table start early)


def _id(row):
    return "w%d-k%d-r%d-l%d" % row


def _okw(kw):
    return dict(mychunk=kw.get("mychunk", 1), total=kw.get("total_chunk", 1), mc_lower=kw.get("mc_lower", 2), mc_upper=kw.get("mc_upper", 240),
                bestn=kw.get("bestn", 4), ovlp_upper=kw.get("ovlp_upper", 120), band=kw.get("align_bandwidth", 100))


class Work:
    """the module's read set, its one ResidentDB, and what the tests of a row share: computed once, never changed afterwards"""

    def __init__(self):
        self.g = simreads.make_genome(GENOME_LEN, 11, repeat_families=2, repeat_len=3000, repeat_copies=6, tandem=4)
        self.db = simreads.simulate_reads(self.g, coverage=14.0, seed=5, mean_len=8000, sd_len=900)
        self.rdb = None
        self._memo = {}

    def _once(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def sketch(self, db, w, k, keep=lambda rid: True):
        return np.concatenate([U.orc_sketch_seqdb(db.seqdb[int(o):int(o) + int(n)], w, k, int(r))
                               for r, n, o in zip(db.rid, db.rlen, db.roff) if keep(int(r))] or [np.zeros(0, formats.MM_DTYPE)])

    def oracle_l0(self, row):
        return self._once(("l0", row), lambda: self.sketch(self.db, row[0], row[1]))

    @staticmethod
    def reduce(l0, r, levels):
        for _ in range(levels):
            l0 = U.orc_reduce(l0, r)
        return l0

    def oracle_top(self, row):
        return self._once(("top", row), lambda: self.reduce(self.oracle_l0(row), row[2], row[3]))

    def gpu_index(self, row):
        w, k, r, lv = row
        return self._once(("ix", row), lambda: self.rdb.index(window=w, kmer=k, reduction=r, levels=lv))

    def gpu_index_halves(self, row):
        w, k, r, lv = row
        return self._once(("ix2", row), lambda: [self.rdb.index(total_chunk=2, mychunk=c, window=w, kmer=k, reduction=r, levels=lv) for c in (1, 2)])

    def lists(self, row, chunking):
        """the lists an overlap / map chunk reads: one index chunk's, or (chunk 2 of 3) the two files of a two-chunk index concatenated"""
        if chunking == "1of1":
            ix = self.gpu_index(row)
            return ix.top, ix.top_mc
        parts = self.gpu_index_halves(row)
        return np.concatenate([p.top for p in parts]), np.concatenate([p.top_mc for p in parts])

    def oracle_overlap(self, row, chunking, setting):
        kw = dict(SETTINGS[row]) if setting else {}
        if chunking == "2of3":
            kw.update(total_chunk=3, mychunk=2)
        mm, mc = self.lists(row, chunking)
        return self._once(("ov", row, chunking, setting), lambda: (kw,) + U.orc_overlap(self.db, mm, mc, **_okw(kw)))


@pytest.fixture(scope="module")
def work():
    wk = Work()
    wk.rdb = ResidentDB(wk.db, 0)
    yield wk
    wk.rdb.close()


def test_the_read_set_is_the_one_the_rows_were_counted_on(work):
    assert work.db.n_reads == 595 and work.db.n_bases == 4_757_187


@pytest.mark.parametrize("row", list(ROWS), ids=_id)
def test_index_vs_oracle(work, row):
    """L0, the top level and its count table: the general path (L0 requested), the fused path, and a two-chunk index"""
    w, k, r, lv = row
    db, rdb = work.db, work.rdb
    l0, top = work.oracle_l0(row), work.oracle_top(row)
    assert len(top) > 10_000
    a = rdb.index(window=w, kmer=k, reduction=r, levels=lv, want_l0=True)
    assert np.array_equal(a.l0, l0)
    assert np.array_equal(a.top, top)
    assert a.reads_literal == 0
    mc = formats.mc_as_sorted_pairs(U.orc_count(top))
    assert np.array_equal(formats.mc_as_sorted_pairs(a.top_mc), mc)
    assert np.array_equal(formats.mc_as_sorted_pairs(a.l0_mc), formats.mc_as_sorted_pairs(U.orc_count(l0)))
    f = work.gpu_index(row)
    assert np.array_equal(f.top, top) and np.array_equal(formats.mc_as_sorted_pairs(f.top_mc), mc)
    halves = work.gpu_index_halves(row)
    want = [work.reduce(work.sketch(db, w, k, lambda rid: rid % 2 == c % 2), r, lv) for c in (1, 2)]
    assert np.array_equal(np.concatenate([h.top for h in halves]), np.concatenate(want))
    for h, t in zip(halves, want):
        assert np.array_equal(formats.mc_as_sorted_pairs(h.top_mc), formats.mc_as_sorted_pairs(U.orc_count(t)))


DISPATCHES = [
    ("default", {}),
    ("device", dict(PGX_GPU_REPLAY="1", PGX_EARLY_OUTER_MIN="1")),                              # device walk, visit order on the device
    ("device-host-visit", dict(PGX_GPU_REPLAY="1", PGX_EARLY_OUTER_MIN="1", PGX_DEV_VISIT="0")),   # device walk, inner tables replayed by host threads
    ("host-threads", dict(PGX_GPU_REPLAY="0", PGX_PAR_MIN="0", PGX_THREADS="8")),                # the threaded host walk
]
OVERLAP_CASES = [(row, ch, False) for row in ROWS for ch in ("1of1", "2of3")] + [(row, "1of1", True) for row in SETTINGS]


@pytest.mark.parametrize("row,chunking,setting", OVERLAP_CASES, ids=["%s-%s%s" % (_id(c[0]), c[1], "-setting" if c[2] else "") for c in OVERLAP_CASES])
def test_overlap_vs_oracle_under_every_dispatch(work, monkeypatch, row, chunking, setting):
    """records, counters and checksum of the stage under the default dispatch, the device walk with the visit order built on the
    device and by host threads, and the threaded host walk.  The device form of the visit order must engage on EVERY row: a row
    on which only the default parameters reach the device tables is what this test is for."""
    kw, want, ost = work.oracle_overlap(row, chunking, setting)
    floor = (SETTING_RECORDS[row] if setting else ROWS[row][chunking == "2of3"]) // 2
    assert len(want) >= floor >= 25, (len(want), floor)
    mm, mc = work.lists(row, chunking)
    for name, env in DISPATCHES:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            got, st = work.rdb.overlap(mm, mc, **kw)
        msg = (name, kw, len(got), len(want), "device_replay %d device_visit %d" % (st["device_replay"], st["device_visit"]))
        assert formats.ovlp_fields_equal(got, want), msg
        assert st["n_records"] == len(want) and st["n_pair_records"] == ost["n_records"], (msg, st, ost)
        assert st["n_align_needed"] == ost["n_align"] and st["n_seen_skip"] == ost["n_seen_skip"], (msg, st, ost)
        assert st["stream_checksum"] == formats.stream_checksum(want), msg
        if name == "device":
            assert st["device_replay"] == 1 and st["device_visit"] >= 1 and st["n_buckets"] == ost["n_buckets"], (msg, st, ost)
            n_buckets = st["n_buckets"]
            print(f"{_id(row)} {chunking} {kw}: {len(want)} records, {st['n_pair_records']} pair records, {n_buckets} buckets, device_visit {st['device_visit']}")
        elif name == "device-host-visit":
            assert st["device_replay"] == 1 and st["device_visit"] == 0 and st["n_buckets"] == n_buckets, (msg, st, n_buckets)
        elif name == "host-threads":
            assert st["device_replay"] == 0, msg


@pytest.mark.parametrize("row", list(ROWS), ids=_id)
def test_one_call_pipeline_equals_the_two_stages(work, row):
    w, k, r, lv = row
    _, want, ost = work.oracle_overlap(row, "1of1", False)
    ix, ov, st = work.rdb.index_overlap(want_index_arrays=True, levels=lv, reduction=r, window=w, kmer=k)
    assert np.array_equal(ix.top, work.oracle_top(row))
    assert len(want) >= ROWS[row][0] // 2 and formats.ovlp_fields_equal(ov, want), (len(ov), len(want))
    assert st["n_pair_records"] == ost["n_records"] and st["n_align_needed"] == ost["n_align"] and st["n_seen_skip"] == ost["n_seen_skip"]


def _align_keys(db, ov, n_random, seed):
    """the alignment requests of a stream (read pair, offset of the query = difference of the two shimmer positions, strands), then random ones"""
    keys = np.zeros(len(ov) + n_random, _lib.ALIGN_KEY_DTYPE)
    k = keys[:len(ov)]
    k["rid0"] = ov["y0"] >> np.uint64(32); k["rid1"] = ov["y1"] >> np.uint64(32)
    k["q_off"] = (((ov["y0"] & np.uint64(0xFFFFFFFF)) >> np.uint64(1)) - ((ov["y1"] & np.uint64(0xFFFFFFFF)) >> np.uint64(1))).astype(np.uint32)
    k["dir0"] = ov["strand0"]; k["dir1"] = ov["strand1"]
    rng = np.random.default_rng(seed)
    r = keys[len(ov):]
    r["rid0"] = rng.integers(0, db.n_reads, n_random); r["rid1"] = rng.integers(0, db.n_reads, n_random)
    rl = db.rlen[r["rid0"]].astype(np.int64)
    r["q_off"] = np.where(rng.random(n_random) < 0.2, np.maximum(rl - rng.integers(0, 40, n_random), 0), rng.integers(0, rl))
    r["dir0"] = rng.integers(0, 2, n_random); r["dir1"] = rng.integers(0, 2, n_random)
    return keys


@pytest.mark.parametrize("row", [K28, W40], ids=_id)
def test_alignment_kernels_on_the_keys_of_the_stream(work, monkeypatch, row):
    """the grouped kernel on the 2-bit packs and the wavefront-per-candidate kernel on the requests these streams make: their q_off
    (the distance of the two reads' copies of the shimmer pair) is distributed differently from a k = 16 stream's"""
    db = work.db
    _, ov, _ = work.oracle_overlap(row, "1of1", False)
    keys = _align_keys(db, ov[:1500], 200, 17)
    assert len(keys) >= 200 + min(1500, ROWS[row][0] // 2)
    want = np.zeros(len(keys), _lib.MATCH_DTYPE)
    for i in range(len(keys)):
        a, b = int(keys["rid0"][i]), int(keys["rid1"][i])
        q = db.seqdb[int(db.roff[a]) + int(keys["q_off"][i]):int(db.roff[a]) + int(db.rlen[a])]
        t = db.seqdb[int(db.roff[b]):int(db.roff[b]) + int(db.rlen[b])]
        want[i] = U.orc_ovlp_match(q, int(keys["dir0"][i]), t, int(keys["dir1"][i]), 100)
    for env in (dict(PGX_ALIGN_SMALL="0", PGX_ALIGN_PACKED_MIN="0"), dict(PGX_ALIGN_SMALL="1000000000")):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            got = work.rdb.align(keys, 100)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (env, len(bad), keys[bad[:3]], got[bad[:3]], want[bad[:3]])


@pytest.mark.parametrize("row", [K28, K12, W64], ids=_id)
def test_map_vs_oracle(work, row):
    """shmr_map's text: the reads located on two exact 120 kb pieces of their genome, and on every 7th read as a contig; the whole
    map with the default bounds and chunk 2 of 3 with multiplicities 2 .. 30"""
    w, k, r, lv = row
    db = work.db
    ctg = simreads.simulate_reads(work.g[20_000:280_000], n_reads=2, seed=6, mean_len=120_000, sd_len=0, wrap=0, err=0.0)
    ctg_top = work.reduce(work.sketch(ctg, w, k), r, lv)
    mm, mc = work.lists(row, "1of1")
    rl, _ = db.by_rid()
    rid = (mm["y"] >> np.uint64(32)).astype(np.int64)
    for what, ref in (("contigs", ctg_top), ("every 7th read", mm[rid % 7 == 0])):
        for (c, T, lo, hi) in ((1, 1, 1, 240), (2, 3, 2, 30)):
            text, n = map_reads_to_ref(ref, mm, mc, rl, T, c, lo, hi)
            want, wn = U.orc_map_reads_to_ref(ref, mm, mc, rl, c, T, lo, hi)
            assert wn >= 250 and n == wn and text == want, (what, c, T, lo, hi, n, wn)


@pytest.mark.parametrize("row", [K28, K12, W64], ids=_id)
def test_query_helpers_vs_oracle(work, tmp_path, row):
    """build_shimmer_map4py over a three-chunk index written as files, then get_shimmer_hits / get_mmer_count / get_shimmers_for_read:
    300 keys of the list and three absent ones (a present hash with a wrong span, a hash with a bit above 2k, and 0), 50 reads"""
    w, k, r, lv = row
    db, rdb = work.db, work.rdb
    formats.write_seqdb(str(tmp_path / "sd"), db)
    sp = str(tmp_path / f"ix-L{lv}")
    parts = [rdb.index(total_chunk=3, mychunk=c, window=w, kmer=k, reduction=r, levels=lv) for c in (1, 2, 3)]
    for c, ix in zip((1, 2, 3), parts):
        formats.write_mmlist(f"{sp}-{c:02d}-of-03.dat", ix.top)
        formats.write_mm_count(f"{sp}-MC-{c:02d}-of-03.dat", ix.top_mc)
    mm = np.concatenate([p.top for p in parts])
    mcs = np.concatenate([p.top_mc for p in parts])
    rl, _ = db.by_rid()
    rng = np.random.default_rng(8)
    present = rng.choice(np.unique(mm["x"]), 300, replace=False)
    h0 = int(present[0]) >> 8
    assert (int(present[0]) & 0xFF) == k and h0 < (1 << 2 * k)
    hashes = [int(x) >> 8 for x in present] + [h0, h0 | 1 << (2 * k + 1), 0]
    spans = [int(x) & 0xFF for x in present] + [k + 1, k, 0]
    assert not np.isin(np.array([h0 << 8 | (k + 1), 0], np.uint64), mm["x"]).any()
    for (c, T) in ((1, 1), (2, 2)):
        m, o = ShimmerMap(str(tmp_path / "sd"), sp, c, T), U.OrcMap(mm, mcs, rl, c, T)
        assert np.array_equal(m.mmers, mm)
        nhit = 0
        for h, s in zip(hashes, spans):
            got, want = m.hits(h, s), o.hits(h, s)
            assert got.tobytes() == want.tobytes(), (c, T, h, s)
            assert m.mmer_count(h) == o.count(h), (c, T, h)
            nhit += len(want)
        assert nhit > 300, nhit
        for rd in rng.integers(0, db.n_reads, 50):
            assert m.read_range(int(rd)) == o.read_shimmers(int(rd))
        m.close(), o.close()


def test_record_scatter_with_56_bit_hashes(work, tmp_path):
    """the one-chunk-per-rank exchange at k = 28, three ranks played in turn (as tests/test_gpu_parallel.py does at k = 16): index
    chunk -> prepare -> scatter per rank, where the destination of a record is (x >> 8) % 3 of a 56-bit hash; the records regrouped
    per destination as the all-to-all delivers them, overlap stage per chunk; and the same chunks through the all-gather form."""
    import torch
    from peregrine_amd.parallel import REC_BYTES, scan_start
    N, (w, k, r, lv) = 3, K28
    db, rdb = work.db, work.rdb
    pre = str(tmp_path / "sd")
    formats.write_seqdb(pre, db)
    want = []
    for c in range(1, N + 1):
        U.orc_index_chunk(pre, str(tmp_path / "ix"), N, c, lv, r, 0, w, k)
    for c in range(1, N + 1):
        U.orc_overlap_chunk(pre, str(tmp_path / f"ix-L{lv}"), str(tmp_path / f"ov.{c}"), N, c)
        want.append(formats.read_ovlp(str(tmp_path / f"ov.{c}")))
    dev = torch.device("cuda", 0)
    tops, mcs = [], []
    for c in range(1, N + 1):
        _, d_top, n_top, d_mc, n_mc = rdb.index_dev(total_chunk=N, mychunk=c, levels=lv, reduction=r, window=w, kmer=k)
        tops.append(_lib.dev_tensor(d_top, n_top * 16, dev).clone()), mcs.append(_lib.dev_tensor(d_mc, n_mc * 16, dev).clone())
    counts_all = torch.cat(mcs)
    torch.cuda.synchronize()

    def prepare(t):
        _lib.stream_wait()
        return rdb.pairs_prepare_dev(t.data_ptr(), t.numel() // 16, counts_all.data_ptr(), counts_all.numel() // 16, 2, 240)

    firsts = [prepare(tops[rk]) for rk in range(N)]
    sends, counts = [], []
    for rk in range(N):
        prepare(tops[rk])
        d_send, cnt = rdb.pairs_scatter_dev(N, scan_start(firsts, rk))
        cnt = [int(x) for x in cnt]
        sends.append(_lib.dev_tensor(d_send, sum(cnt) * REC_BYTES, dev).clone()), counts.append(cnt)
    allmm = torch.cat(tops)
    for d in range(N):   # what rank d receives: source-major
        parts = []
        for rk in range(N):
            o = sum(counts[rk][:d]) * REC_BYTES
            parts.append(sends[rk][o:o + counts[rk][d] * REC_BYTES])
        recv = torch.cat(parts)
        torch.cuda.synchronize()
        _lib.stream_wait()
        ov, st = rdb.overlap_records_dev(recv.data_ptr(), recv.numel() // REC_BYTES, total_chunk=N, mychunk=d + 1)
        assert len(want[d]) > 1000 and formats.ovlp_fields_equal(ov, want[d]), f"chunk {d + 1} of {N}: {len(ov)} records, {len(want[d])} expected"
        ov2, _ = rdb.overlap_dev(allmm.data_ptr(), allmm.numel() // 16, counts_all.data_ptr(), counts_all.numel() // 16, total_chunk=N, mychunk=d + 1)
        assert formats.ovlp_fields_equal(ov2, want[d]), f"chunk {d + 1} of {N}, all-gather form"
