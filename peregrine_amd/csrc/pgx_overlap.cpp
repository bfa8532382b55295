// pgx_overlap.cpp -- the overlap stage: what main() of the reference's src/shmr_overlap.c:233-419 does for one chunk, as its driver
// (Stage) and the resident C entry points.  In the order a stage runs:
//   GPU : count table, keep flags, chain, pair records, sorts, bucket / first-key-group tables (the join, pgx_pairs.hip)
//   host: ONE thread replays klib's OUTER khash table from the distinct first keys; it starts during the join (PreOuter, pgx_host_tables.h)
//   GPU : the inner khash tables per group, the buckets placed in outer-slot order = the visit list (pgx_visit.hip)
//   GPU : the greedy best-n walk as a fixed point over the visit list, every ovlp_match in bulk batches (pgx_replay.hip, pgx_align.hip)
// Sets below 0.2 M pair records, and whatever the device tables' encodings do not hold, build the visit list (build_visit, pgx_host_tables.h)
// and walk it on the host (HostWalk, pgx_host_replay.h), with the alignments still on the GPU.  Either walk guesses the verdict of an
// alignment it has not seen, runs the alignments it asked for and repeats with the true results until nothing new is asked: ovlp_match is
// a pure function of its key, so the last pass equals the reference's sequential process and its record sequence.
#include <glob.h>
#include <sched.h>
#include <sys/mman.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <atomic>
#include <memory>
#include <mutex>
#include <optional>
#include <thread>

#include <fcntl.h>
#include <unistd.h>
#include <sys/stat.h>

#include <limits.h>

#include "pgx_internal.h"
#include "pgx_khash.h"

using namespace pgx;

namespace {

// The driver's knobs, read from the environment once per stage (tests change them between the calls of one process).
struct StageKnobs {
  int gpu_replay = -1;                       // PGX_GPU_REPLAY: 1 / 0 force the device / the host walk (unset: by the record count)
  bool dev_visit = true;                     // PGX_DEV_VISIT=0: the tables are downloaded, the inner tables replayed by host threads
  uint32_t visit_wave_max = VISIT_WAVE_MAX;  // PGX_VISIT_WAVE_MAX: largest group the device replays (tests: force the fall-back)
  unsigned threads = 0;                      // PGX_THREADS: host walk threads, over the 24-thread cap (0: unset)
  size_t par_min = 50000;                    // PGX_PAR_MIN: bucket entries below which one thread walks
  size_t block = 0;                          // PGX_BLOCK: buckets a worker takes at a time (0: ParReplay's default)
  unsigned local_world = 0;                  // LOCAL_WORLD_SIZE: ranks sharing this host's cores (0: unset)
  bool trace = false;                        // PGX_TRACE set
  int trace_level = 0;                       // ... and its value
  static StageKnobs from_env() {
    StageKnobs k;
    if (const char *e = getenv("PGX_GPU_REPLAY")) k.gpu_replay = atoi(e);
    if (const char *e = getenv("PGX_DEV_VISIT")) k.dev_visit = atoi(e) != 0;
    if (const char *e = getenv("PGX_VISIT_WAVE_MAX")) k.visit_wave_max = (uint32_t)std::min<long>(atol(e), VISIT_WAVE_MAX);
    if (const char *e = getenv("PGX_THREADS")) k.threads = (unsigned)std::max(1, atoi(e));
    if (const char *e = getenv("PGX_PAR_MIN")) k.par_min = (size_t)atoll(e);
    if (const char *e = getenv("PGX_BLOCK")) k.block = (size_t)std::max(1, atoi(e));
    if (const char *e = getenv("LOCAL_WORLD_SIZE")) k.local_world = (unsigned)std::max(1, atoi(e));
    if (const char *e = getenv("PGX_TRACE")) k.trace = true, k.trace_level = atoi(e);
    return k;
  }
};

#include "pgx_host_tables.h"   // maps, visit list + build_visit, thread team, pinned pools
#include "pgx_host_replay.h"   // Replay / ParReplay / HostWalk: the greedy walk on the host

// The greedy walk runs on the GPU (pgx_replay.hip) from 0.2 M pair records on, where it is as fast as or faster than the multi-threaded
// host walk and does not lean on the host cores, which the ranks of a multi-GPU job share (overlap stage, 30x sets: E. coli-size 10.2 vs
// 10.1 ms per step; 5 Mb 18.7 vs 19.7 ms; 20 Mb 44 vs 53 ms; 80 Mb 134 vs 217 ms; 150 Mb 0.23 vs 0.45 s; below that a sweep is bound
// by the latency of single bucket evaluations and kernel launches: 1 Mb 11.8 vs 9.8 ms, 0.3 Mb 10.9 vs 6.1 ms; tools/crossover.py).
constexpr size_t GPU_REPLAY_MIN = 200000;
// pair records from which the visit phase also packs the reads and clears the replay's tables while it waits for the outer table
constexpr size_t PREPARE_MIN = (size_t)2 << 20;

struct Scratch {   // the big host tables of a stage: torn down on the housekeeping thread once the results are out
  PairTables pt;
  Visit visit;
  PreOuter pre;   // the outer khash table, replayed by a host thread DURING the join (its destructor joins the thread)
};

// One overlap stage.  Owns what lives for the stage; overlap_stage() below calls the phases in order.
struct Stage {
  struct DropPre {   // (tables the visit phase cleared ahead of time for a device walk that then did not run: an exception, the host walk)
    const pgx_seqdb *db;
    ~DropPre() { replay_drop_precleared(db); }
  } drop_pre;
  pgx_seqdb *const db;
  const pgx_overlap_params *const p;
  RecordSink *const sink;
  OvOut &out;
  const StageKnobs k = StageKnobs::from_env();
  pgx_overlap_stats s;
  const double t0 = now_ms();
  double t1 = 0, gpu_ms = 0;
  MemTag mem_tag{"overlap.join"};
  Scratch *const scratch = new Scratch;
  DevicePairs dpairs;        // lives until the device walk has succeeded or its fall-back has fetched from it
  DevBuf<uint32_t> d_bids;   // the visit list on the device
  bool gpu_replay = k.gpu_replay != 0;   // (decided once the join has counted the records)
  std::optional<NodePin> pin;            // from the join's end on this thread and its helper threads stay on one memory node

  Stage(pgx_seqdb *db_, const pgx_overlap_params *p_, OvOut &out_, RecordSink *sink_) : drop_pre{db_}, db(db_), p(p_), sink(sink_), out(out_) {
    memset(&s, 0, sizeof(s));
  }
  Stage(const Stage &) = delete;
  Stage &operator=(const Stage &) = delete;
  ~Stage() {
    Scratch *z = scratch;
    defer_destroy([z] { delete z; });
  }

  void fetch_to_host() {   // the host walk reads the tables and the records (kept on the device in case the device walk ran)
    pairs_fetch_tables(dpairs, scratch->pt);
    pairs_fetch_records(dpairs, scratch->pt);
    dpairs = DevicePairs();
  }
  void trace_join(const char *visit_form) const {
    if (!k.trace) return;
    const PairTables &pt = scratch->pt;
    fprintf(stderr, "[pgx] GPU join: %zu records, %zu buckets, %zu key0 groups in %.2f ms; visit order (%llu buckets%s) in %.2f ms\n", pt.n_rec,
            pt.n_buckets, pt.n_groups, t1 - t0, (unsigned long long)s.n_buckets, visit_form, now_ms() - t1);
  }

  // count table, join, records; the record count decides between the device and the host walk
  void join(const StageInput &in) {
    PairTables &pt = scratch->pt;
    // the visit order on the device (pgx_visit.hip): the join's tables stay in HBM, the inner khash tables are replayed there, the
    // host only replays the outer one
    const bool dev_visit = gpu_replay && k.dev_visit;
    const unsigned jflags = PAIRS_ORD_TABLES | (gpu_replay ? PAIRS_LAZY_RECORDS : 0u) | (dev_visit ? PAIRS_DEV_TABLES : 0u);
    const EarlyFn early = [z = scratch](EarlyGroups &&g) { z->pre.start(std::move(g), z->pt.n_rec); };
    DevicePairs *keep = gpu_replay ? &dpairs : nullptr;
    if (in.records)
      dev_pairs_from_records(in.d_recs, in.n_recs, pt, keep, jflags, early, db);
    else
      dev_build_pairs(db->d_rlen.p, in.lists,
                      PairParams{(uint32_t)p->total_chunk, (uint32_t)p->mychunk, (uint32_t)p->mc_lower, (uint32_t)p->mc_upper,
                                 (uint32_t)db->rlen_by_rid.size()},
                      pt, jflags, keep, early, db);
    pgx::sync();
    s.n_pair_records = pt.n_rec;
    if (k.gpu_replay < 0) gpu_replay = pt.n_rec >= GPU_REPLAY_MIN;
    if (!gpu_replay) fetch_to_host();
    t1 = now_ms();
    gpu_ms += t1 - t0;
    pin.emplace();
    if (k.trace) fprintf(stderr, "[pgx]   pinned to a memory node at +%.2f ms after the join\n", now_ms() - t1);
  }

  // The visit list on the device from the join's tables in HBM: the GPU replays the inner tables while the host thread finishes the outer
  // one.  false: the outer table did not start, a group is too large for a wavefront, or the early keys are not the join's groups.
  bool place_on_device() {
    const PairTables &pt = scratch->pt;
    PreOuter &pre = scratch->pre;
    Visit &visit = scratch->visit;
    if (!(pre.started && pre.eg.n == dpairs.n_groups && dpairs.max_group_buckets <= k.visit_wave_max)) {
      if (k.trace)
        fprintf(stderr, "[pgx]   visit: host path (early outer table %s, largest group %u buckets)\n", pre.started ? "running" : "not started",
                dpairs.max_group_buckets);
      return false;
    }
    DevVisit dv;
    dev_visit_inner(dpairs, (uint32_t)p->ovlp_upper, dv);   // (enqueued: the GPU replays the inner tables ...
    if (pt.n_rec >= PREPARE_MIN) dev_align_prepare(db);     //  ... and packs the reads for the alignments ...
    if (pt.n_rec >= PREPARE_MIN) replay_preclear(db);       //  ... and clears the replay's tables (7-8 ms of a full-size chunk) ...
    pre.join();                                             //  ... while the outer table finishes here)
    const double tw = now_ms();
    bool ok = true;
    for (size_t i = 0; ok && i < dpairs.key_sample.size(); ++i) ok = pre.eg.keys[i * KEY_SAMPLE_STRIDE] == dpairs.key_sample[i];
    ok = ok && ((size_t)pre.eg.last_first == (size_t)dpairs.last_gfirst);
    if (!ok) {
      fprintf(stderr, "[pgx] note: the early outer-table keys do not match the join's group tables; the host builds the visit order\n");
      return false;
    }
    size_t nbv = 0, nev = 0;
    dev_visit_place(dpairs, dv, pre.table.slot, pre.table.nb, d_bids, &nbv, &nev);
    visit.n_buckets = nbv, visit.n_entries = nev, visit.on_device = true, visit.n_groups = 0;
    s.device_visit = 1 + dpairs.n_big_groups;   // (the tables stay until the device walk has succeeded: its fall-back, the host walk, fetches them)
    if (k.trace)
      fprintf(stderr, "[pgx]   visit on the device: waited %.2f ms for the outer table (host thread %.2f ms, %u slots), placed in %.2f ms\n", tw - t1,
              pre.ms, pre.table.nb, now_ms() - tw);
    return true;
  }

  // the device walk's visit list (bucket ids only): placed on the device, else built by the host's table replay (build_visit)
  void visit_order() {
    PairTables &pt = scratch->pt;
    Visit &visit = scratch->visit;
    bool placed = false;
    if (dpairs.tables) {
      placed = place_on_device();
      if (!placed) pairs_fetch_tables(dpairs, pt);
    }
    if (!placed) build_visit(pt, (uint32_t)p->ovlp_upper, visit, true, &scratch->pre);
    s.n_buckets = visit.n_buckets;
    trace_join(", ids only");
    if (k.trace_level >= 2 && visit.n_buckets && !visit.on_device && pt.on_host) {  // bucket sizes: a pass of the device walk lasts as long as its largest bucket
      std::vector<uint32_t> sz(visit.n_buckets);
      for (size_t i = 0; i < visit.n_buckets; ++i) sz[i] = pt.bstart[visit.bids[i] + 1] - pt.bstart[visit.bids[i]];
      std::sort(sz.begin(), sz.end());
      fprintf(stderr, "[pgx]   bucket sizes: median %u, 90 %% %u, 99 %% %u, 99.9 %% %u, max %u\n", sz[sz.size() / 2], sz[sz.size() * 9 / 10],
              sz[sz.size() * 99 / 100], sz[sz.size() * 999 / 1000], sz.back());
    }
    if (visit.on_device && !placed)
      dev_place_bids(visit.ids_all.data(), visit.ids_all.size(), visit.psrc.data(), visit.pcnt.data(), visit.pdst.data(), visit.n_groups,
                     visit.n_buckets, d_bids);
  }

  // false: dev_replay gave up (nothing was produced); the tables and the records are on the host for the host walk
  bool walk_device() {
    const Visit &visit = scratch->visit;
    const double r0 = now_ms();
    size_t nrec = 0;
    pgx_overlap_stats rs;
    memset(&rs, 0, sizeof(rs));
    const auto alloc_out = [this](size_t n) -> pgx_ovlp * {
      if (sink) {   // (the records go from the device to the sink: no host array)
        out_free(out.a), out.a = nullptr, out.n = n;
        return nullptr;
      }
      out.alloc(n);
      return out.a;
    };
    if (!dev_replay(db, dpairs, visit.on_device ? nullptr : visit.bids.data(), visit.on_device ? d_bids.p : nullptr, visit.n_buckets,
                    visit.n_entries, (uint32_t)(uint8_t)p->bestn, p->align_bandwidth, (uint32_t)p->ovlp_upper, alloc_out, sink, &nrec, &rs,
                    k.trace)) {
      fetch_to_host();
      return false;
    }
    s.n_align_needed = rs.n_align_needed, s.n_seen_skip = rs.n_seen_skip, s.n_align_gpu = rs.n_align_gpu, s.rounds = rs.rounds;
    s.n_evaluations = rs.n_evaluations, s.device_replay = 1;
    s.replay_attempts = rs.replay_attempts, s.stream_checksum = rs.stream_checksum;
    gpu_ms += now_ms() - r0;
    return true;
  }

  void walk_host() {
    Visit &visit = scratch->visit;
    build_visit(scratch->pt, (uint32_t)p->ovlp_upper, visit, false, &scratch->pre);
    s.n_buckets = visit.start.size() - 1;
    trace_join("");
    HostWalk{db, visit, p, k, t0, out, s, gpu_ms}.run();
  }

  void finish(pgx_overlap_stats *st) {
    const double tf0 = now_ms();
    timing_flush();
    if (k.trace) fprintf(stderr, "[pgx] stage total %.2f ms (timing flush %.2f ms)\n", now_ms() - t0, now_ms() - tf0);
    s.n_records = out.n;
    if (!s.device_replay)   // (the device walk adds its checksum up in k_emit; the host walk serves small sets)
      for (size_t i = 0; i < out.n; ++i) s.stream_checksum += record_checksum(out.a[i], i);
    s.gpu_ms = gpu_ms;
    s.host_ms = now_ms() - t0 - gpu_ms;
    if (st) *st = s;
  }
};

// what the resident entry points share: the stage's records as the caller's array
void stage_to_caller(pgx_seqdb *db, const StageInput &in, const pgx_overlap_params *p, pgx_ovlp **out, size_t *n_out, pgx_overlap_stats *stats) {
  OvOut v;
  overlap_stage(db, in, p, v, stats);
  *n_out = v.n;
  *out = v.release();
}

}  // namespace

namespace pgx {
void overlap_check_params(const pgx_overlap_params *p) {
  PGX_REQUIRE(p, PGX_EARG, "null params");
  PGX_REQUIRE(p->total_chunk > 0 && p->mychunk > 0 && p->mychunk <= p->total_chunk, PGX_EARG,
              "need 0 < mychunk <= total_chunk (shmr_overlap.c:328-329)");
  PGX_REQUIRE(p->align_bandwidth > 0 && p->align_bandwidth < (1 << 20), PGX_EARG, "bad align_bandwidth");
  PGX_REQUIRE(p->ovlp_upper >= 0 && p->mc_lower >= 0 && p->mc_upper >= 0, PGX_EARG, "negative bound");
}
void overlap_stage(pgx_seqdb *db, const StageInput &in, const pgx_overlap_params *p, OvOut &out, pgx_overlap_stats *st, RecordSink *sink) {
  dev_cache_age();
  Stage stage(db, p, out, sink);
  stage.join(in);
  bool walked = false;
  if (stage.gpu_replay && stage.dpairs.valid) {
    stage.visit_order();
    walked = stage.walk_device();
  }
  if (!walked) stage.walk_host();
  stage.finish(st);
}
}  // namespace pgx

extern "C" {

int pgx_khash_slot_order(const uint64_t *keys, size_t n, uint64_t *out) {
  return guarded([&] {
    PGX_REQUIRE((keys && out) || n == 0, PGX_EARG, "pgx_khash_slot_order: null argument");
    PGX_REQUIRE(n < (1ULL << 30), PGX_EARG, "pgx_khash_slot_order: too many keys");
    DistinctSlotTable t;
    for (size_t i = 0; i < n; ++i) {
      if (i + 8 < n) t.prefetch(keys[i + 8]);
      t.put_new(keys[i], (uint32_t)i);
    }
    size_t m = 0;
    for (uint32_t s0 = 0; s0 < t.nb; ++s0)
      if (t.is_used(s0)) out[m++] = keys[t.id_at(s0)];
  });
}

int pgx_khash_slot_order_ex(const uint64_t *keys, size_t n, int touch, uint64_t *out) {
  return guarded([&] {
    PGX_REQUIRE((keys && out) || n == 0, PGX_EARG, "pgx_khash_slot_order_ex: null argument");
    PGX_REQUIRE(n < (1ULL << 30), PGX_EARG, "pgx_khash_slot_order_ex: too many keys");
    if (n == 0) return;
    size_t m = 0;
    DistinctSlotTable t;
    for (size_t i = 0; i < n; ++i) {
      if (i + 8 < n) t.prefetch(keys[i + 8]);
      t.put_new(keys[i], (uint32_t)i);
    }
    if (touch) t.touch();
    for (uint32_t s0 = 0; s0 < t.nb; ++s0)
      if (t.is_used(s0)) out[m++] = keys[t.id_at(s0)];
    PGX_REQUIRE(m == n, PGX_ESTATE, "pgx_khash_slot_order_ex: %zu of %zu keys placed (are the keys distinct?)", m, n);
  });
}

int pgx_overlap_resident(pgx_seqdb *db, const pgx_mm128 *mmers, size_t n_mm, const pgx_mm_count *counts,
                         size_t n_counts, const pgx_overlap_params *p, pgx_ovlp **out, size_t *n_out,
                         pgx_overlap_stats *stats) {
  return guarded([&] {
    require_ready();
    PGX_REQUIRE(db && out && n_out && (n_mm == 0 || mmers) && (n_counts == 0 || counts), PGX_EARG,
                "pgx_overlap_resident: null argument");
    overlap_check_params(p);
    stage_to_caller(db, StageInput::host_lists(mmers, n_mm, counts, n_counts), p, out, n_out, stats);
  });
}

// index + overlap of ONE chunk with the shimmer list and the counts handed over in HBM (no download + upload between the
// stages); anything the fused index path does not cover falls back to the two-stage hand-over through host arrays
int pgx_index_overlap_resident(pgx_seqdb *db, const pgx_index_params *ip, const pgx_overlap_params *op, int want_index_arrays,
                               pgx_index_result *index_out, pgx_ovlp **out, size_t *n_out, pgx_overlap_stats *stats) {
  return guarded([&] {
    require_ready();
    PGX_REQUIRE(db && ip && op && index_out && out && n_out, PGX_EARG, "pgx_index_overlap_resident: null argument");
    PGX_REQUIRE(ip->total_chunk == 1 && ip->mychunk == 1, PGX_EARG,
                "pgx_index_overlap_resident is the single-index-chunk pipeline (other chunks' lists would be missing)");
    overlap_check_params(op);
    DeviceIndex dev;
    index_stage(db, ip, index_out, &dev, want_index_arrays != 0);
    // (not valid -- want_l0, ambiguous parameters ...: the general index path has already produced host arrays)
    const StageInput in = dev.valid ? StageInput::device_lists(dev.d_top, dev.n_top, dev.mc.p, dev.n_mc)
                                    : StageInput::host_lists(index_out->top, index_out->n_top, index_out->top_mc, index_out->n_top_mc);
    stage_to_caller(db, in, op, out, n_out, stats);
  });
}

// ---- multi-GPU hand-over on device pointers (include/pgx.h) -----------------------------------------------------
int pgx_overlap_resident_dev(pgx_seqdb *db, const pgx_mm128 *d_mmers, size_t n_mm, const pgx_mm_count *d_counts,
                             size_t n_counts, const pgx_overlap_params *p, pgx_ovlp **out, size_t *n_out,
                             pgx_overlap_stats *stats) {
  return guarded([&] {
    require_ready();
    PGX_REQUIRE(db && out && n_out && (n_mm == 0 || d_mmers) && (n_counts == 0 || d_counts), PGX_EARG,
                "pgx_overlap_resident_dev: null argument");
    overlap_check_params(p);
    stage_to_caller(db, StageInput::device_lists(d_mmers, n_mm, d_counts, n_counts), p, out, n_out, stats);
  });
}

int pgx_pairs_prepare_dev(pgx_seqdb *db, const pgx_mm128 *d_top, size_t n_top, const pgx_mm_count *d_counts_all,
                          size_t n_counts_all, int mc_lower, int mc_upper, int64_t *first_strict) {
  return guarded([&] {
    require_ready();
    PGX_REQUIRE(db && first_strict && (n_top == 0 || d_top) && (n_counts_all == 0 || d_counts_all) && mc_lower >= 0 && mc_upper >= 0,
                PGX_EARG, "pgx_pairs_prepare_dev: bad argument");
    *first_strict = dev_pairs_prepare(db, d_top, n_top, d_counts_all, n_counts_all, (uint32_t)mc_lower, (uint32_t)mc_upper);
  });
}

int pgx_pairs_scatter_dev(pgx_seqdb *db, int total_chunk, int64_t start, const pgx_pair_rec **d_send, uint64_t *send_counts) {
  return guarded([&] {
    require_ready();
    PGX_REQUIRE(db && d_send && send_counts && total_chunk > 0, PGX_EARG, "pgx_pairs_scatter_dev: bad argument");
    dev_pairs_scatter(db->d_rlen.p, (uint32_t)total_chunk, start, d_send, send_counts);
    timing_flush();
  });
}

int pgx_overlap_records_dev(pgx_seqdb *db, const pgx_pair_rec *d_records, size_t n_records, const pgx_overlap_params *p,
                            pgx_ovlp **out, size_t *n_out, pgx_overlap_stats *stats) {
  return guarded([&] {
    require_ready();
    PGX_REQUIRE(db && out && n_out && (n_records == 0 || d_records), PGX_EARG, "pgx_overlap_records_dev: null argument");
    overlap_check_params(p);
    stage_to_caller(db, StageInput::pair_records(d_records, n_records), p, out, n_out, stats);
  });
}

}  // extern "C"
