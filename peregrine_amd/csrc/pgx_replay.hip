// pgx_replay.hip -- the greedy best-n walk over the shimmer-pair buckets (shimmer_to_overlap + the seen-pair table of
// build_ovlp, src/shmr_overlap.c:52-228) on the GPU, one lane per bucket.
//
// The reference visits the buckets once, in order, sharing one seen-pair table.  A bucket's evaluation is a pure function of
// (a) which of the pairs it examines were inserted by EARLIER buckets (and with which type) and (b) the alignment results it
// looks up.  So the walk is solved as a fixed point (the same formulation as the host replay in pgx_overlap.cpp, which stays
// as the fallback), in phases separated by kernel boundaries -- no intra-kernel ordering is needed anywhere:
//
//   k_eval    every dirty bucket of a window re-runs shimmer_to_overlap against the pair table AS IT STANDS (read-only in
//             this kernel): pair present <=> owner < bucket.  It registers itself as a reader of every pair it examines
//             (lock-free push), guesses unknown alignments (accepted; type predicted from the geometry) and leaves the
//             list of pairs it would insert.
//   k_update  applies the evaluated buckets' lists to the table (compare-and-swap, lowest bucket wins), withdraws what a
//             bucket no longer inserts, and marks dirty every later reader of a pair whose state changed, the displaced
//             owner, and the bucket itself when an earlier bucket got in first.
//   ... repeated window by window until no bucket is dirty; then
//   k_file    files the alignments the lists still need in the memo table (insert-only) and numbers the requests,
//   dev_align the banded O(ND) kernel (pgx_align.hip) on the new requests,
//   k_settle  checks every guess against its result; a wrong guess makes the bucket dirty again
//   ... until a sweep files nothing or every guess was right; k_emit writes the ovlp_t records in bucket order.
//
// At the fixed point every bucket was last evaluated against a table that has not changed since in any way it could
// observe, and the owner of a pair is the lowest bucket inserting it: by induction over the bucket order that is the
// sequential walk.  Changes only ever propagate to LATER buckets, so the lowest unstable bucket rises monotonically.
#include <optional>

#include "pgx_replay.h"

namespace pgx {
using namespace rp;
namespace {
uint32_t pow2_at_least(size_t x) {
  size_t c = 1024;
  while (c < x) c <<= 1;
  return (uint32_t)c;
}
unsigned cdiv256(size_t n) { return (unsigned)((n + 255) / 256); }
int env_int(const char *name, int unset) { return getenv(name) ? atoi(getenv(name)) : unset; }
template <typename T>
void alloc_tagged(const char *tag, DevBuf<T> &buf, size_t n) { MemTag t(tag); buf.alloc(n); }   // booked under `tag` in the ledger

// ---- sizes ---------------------------------------------------------------------------------------------------------------------------
// Table sizes are multiples of the defaults below (pair and memo table: the power of two from the entries up).  Two things were found at
// full-size configs[3] (round 5, profiles/r05a_chunk_timeline_c4.txt):
//  * every one of the 8 chunks of a step ran two attempts in vain -- requests 1.72 x the entries, then the memo table -- and an
//    overflowing attempt costs a whole first sweep (the request / memo overflow is only seen when k_file runs): 205 of 1,103 ms;
//  * the open-addressing tables want a LOW load: with the pair table at 0.75 (64 M slots for 50 M read pairs) and the memo table at 0.71
//    the evaluations of a chunk took 73 ms longer than at 0.37 / 0.36 (linear probing: ~8 probes per miss instead of ~2).
// So a stage measures what it used per bucket entry (Usage) and the NEXT stage on the database (the chunks of a job are alike) sizes its
// tables by that (Mult::from): hash tables for a load of at most 0.4, arenas with 20 % to spare.  The first stage on a database starts from
// the defaults and, where they overflow, repeats with x 4 hash tables / x 2 arenas (Mult::grow).
constexpr size_t ITEMS_PER_ENTRY = 6, ITEMS_PER_BUCKET = 64, NODES_PER_ENTRY = 8, REQS_PER_ENTRY = 1;   // the arenas' defaults
constexpr size_t STATE_PER_BUCKET = 64;   // bytes: five flag bytes, five words, a wavefront slot and list entries, rounded up
constexpr double TABLE_LOAD = 0.4;

struct Usage {   // what a stage used per bucket entry (0: not known)
  double pairs = 0, reqs = 0, items = 0, nodes = 0;   // read pairs, requests (= memo entries), items, reader nodes
  void raise(const Usage &u) { pairs = std::max(pairs, u.pairs), reqs = std::max(reqs, u.reqs), items = std::max(items, u.items), nodes = std::max(nodes, u.nodes); }
};
struct Mult {    // an attempt's table sizes as multiples of the defaults
  double items = 1, nodes = 1, reqs = 1, pairs = 1, memo = 1;
  // (the arenas may also SHRINK to what the last stage used + 25-100 %: 8 reader nodes per entry are reserved by default and a c4 chunk links
  //  25 thousand of its 213 million; a stage that needs more than that repeats once and the next one knows)
  static Mult from(const Usage &learned, size_t ne, size_t nb) {
    Mult m;
    if (learned.pairs > 0) {
      const double items_default = (double)ITEMS_PER_ENTRY + (double)ITEMS_PER_BUCKET * (double)nb / ne;
      m.items = std::max(0.2, learned.items * 1.25 / items_default), m.nodes = std::max(0.02, learned.nodes * 2 / NODES_PER_ENTRY);
      m.reqs = std::max(1.0, learned.reqs * 1.2);
      m.pairs = std::max(1.0, learned.pairs / TABLE_LOAD), m.memo = std::max(1.0, learned.reqs / TABLE_LOAD);
    }
    if (getenv("PGX_REPLAY_PAIRS_X")) m.pairs = atof(getenv("PGX_REPLAY_PAIRS_X"));
    if (getenv("PGX_REPLAY_MEMO_X")) m.memo = atof(getenv("PGX_REPLAY_MEMO_X"));
    return m;
  }
  // unusual data (repeat-rich sets): the same walk again with larger tables.  Requests and memo entries are the same alignments: when the
  // request array was too small the memo table of the same size class is too, and k_file stopped before it could say so -- grow both
  void grow(uint32_t ov) {
    auto arena = [](double &m) { m = m < 1 ? 1.0 : m * 2; };   // (an arena that was shrunk to the last stage's use goes back to the default first)
    if (ov & OV_ITEMS) arena(items);
    if (ov & OV_NODES) arena(nodes);
    if (ov & OV_REQS) arena(reqs);
    if (ov & OV_PAIRS) pairs *= 4;
    if (ov & (OV_MEMO | OV_REQS)) memo *= 4;
  }
};

struct Sizes {   // of one attempt
  uint32_t pcap, mcap;                   // hot pair table, memo table (powers of two)
  uint32_t cshift = 0;                   // 2^cshift neighbouring hot slots share one reader list ...
  size_t ccap = 0;                       // ... so many of them (share_readers)
  uint32_t item_cap, rn_cap, req_cap;
  Sizes(size_t ne, size_t nb, const Mult &m) {
    const size_t top = 0x7FFFFFF0u;
    pcap = pow2_at_least((size_t)(ne * m.pairs)), mcap = pow2_at_least((size_t)(ne * m.memo));
    item_cap = (uint32_t)std::min((size_t)((ne * ITEMS_PER_ENTRY + nb * ITEMS_PER_BUCKET) * m.items) +
                                      (size_t)(nb / GPW + 2 + SPARSE_CAP + 8 + BIG_WG * BIG_NW) * ICH + (1u << 20), top);
    rn_cap = (uint32_t)std::min((size_t)(ne * NODES_PER_ENTRY * m.nodes) + (1u << 20), top);
    req_cap = (uint32_t)std::min((size_t)(ne * REQS_PER_ENTRY * m.reqs) + 65536, top);
  }
  // The hot table wants a load of <= 0.4 and the reader lists are 16 x as large per slot (34 GB for a full-size configs[3] chunk).  Where
  // that is more than a third of the free device memory, 2 (4, 8) neighbouring hot slots share one list: all sharing costs is that a change
  // of one pair also marks the other's later readers dirty -- a spurious re-evaluation, never a missed one (measured at c4: + 19 %
  // evaluations, + 1.3 % step time for 17 GB less).  PGX_REPLAY_COLD_SHIFT forces the shift (tests: 0 .. 3).  free_bytes: with the hot
  // table in place already -- that is the state round 5 measured the rule in, so the attempt asks only then.
  void share_readers(size_t free_bytes) {
    if (getenv("PGX_REPLAY_COLD_SHIFT")) cshift = (uint32_t)std::min(3, std::max(0, env_int("PGX_REPLAY_COLD_SHIFT", 0)));
    else
      while (cshift < 3 && ((size_t)pcap >> cshift) * sizeof(PCold) > free_bytes / 3) ++cshift;
    ccap = ((size_t)pcap >> cshift) + 1;
  }
};
// what dev_replay's fit check prices: the default sizes without their fixed parts, and 256 MiB for everything else
size_t default_need(size_t ne, size_t nb) {
  return (size_t)pow2_at_least(ne) * (sizeof(PHot) + sizeof(PCold) + sizeof(MSlot)) +
         ne * (ITEMS_PER_ENTRY * sizeof(Item) + NODES_PER_ENTRY * sizeof(RNode) + REQS_PER_ENTRY * (sizeof(pgx_align_key) + sizeof(pgx_match))) +
         nb * (ITEMS_PER_BUCKET * sizeof(Item) + STATE_PER_BUCKET) + (256u << 20);
}

// ---- the three hash tables -------------------------------------------------------------------------------------------------------------
// Round 6: the hot pair table, the reader lists and the memo (38.6 GB at full-size configs[3]) must start all zero, and clearing them takes
// 7-8 ms -- on a GPU that sits idle for ~18 ms of every chunk while the host finishes the outer khash table (pgx_overlap.cpp:
// Stage::visit_order).  So the stage allocates and clears tables of the sizes the LAST stage used inside that window (replay_preclear); the
// attempt takes them over when its own sizes come out the same (the chunks of a job are alike, the sizes are powers of two) and clears its
// own otherwise.
struct Tables {
  DevBuf<PHot> hot;     // (.n: the capacity)
  DevBuf<PCold> cold;
  DevBuf<MSlot> memo;
  bool hot_zero = false, cold_zero = false, memo_zero = false;   // cleared and not used since
  bool held() const { return hot.p != nullptr; }
  size_t bytes() const { return hot.n * sizeof(PHot) + cold.n * sizeof(PCold) + memo.n * sizeof(MSlot); }
  void alloc(size_t pcap, size_t ccap, size_t mcap) {   // every table that does not have its capacity yet (0: not this one, not now)
    if (pcap && hot.n != pcap) alloc_tagged("replay.pair_table_hot", hot, pcap), hot_zero = false;
    if (ccap && cold.n != ccap) alloc_tagged("replay.pair_table_readers", cold, ccap), cold_zero = false;
    if (mcap && memo.n != mcap) alloc_tagged("replay.memo_table", memo, mcap), memo_zero = false;
  }
  // (the reader lists must be cleared WHOLE: a registration takes its list position with an atomic and writes the entry a step later)
  void clear(hipStream_t s) {
    if (!hot_zero) PGX_HIP(hipMemsetAsync(hot.p, 0, hot.n * sizeof(PHot), s));
    if (!cold_zero) PGX_HIP(hipMemsetAsync(cold.p, 0, cold.n * sizeof(PCold), s));
    if (!memo_zero) PGX_HIP(hipMemsetAsync(memo.p, 0, memo.n * sizeof(MSlot), s));
    hot_zero = cold_zero = memo_zero = true;
  }
  void drop() { hot.release(), cold.release(), memo.release(), hot_zero = cold_zero = memo_zero = false; }
};
}  // namespace

// What the replay keeps between the stages of a job, with its read database (DbCaches): the chunks of a job are alike.
struct ReplayState {
  Tables pre;                              // cleared ahead of time (replay_preclear)
  size_t last_pcap = 0, last_ccap = 0, last_mcap = 0;   // what the last successful stage on the database used
  Usage learned;
  void forget() { pre.drop(), last_pcap = last_ccap = last_mcap = 0, learned = Usage(); }   // (not the handles below)
  // created on first use, freed with the database (which stays on the device it was made on)
  Counters *hc = nullptr;             // pinned mirror of the device counters
  unsigned long long *hs = nullptr;   // pinned mirror of the spread totals
  hipStream_t side_stream = nullptr;  // k_eval_big beside the narrow kernel of a pass
  hipEvent_t side_ev[2] = {nullptr, nullptr};
  void handles() {
    if (!hc) PGX_HIP(hipHostMalloc((void **)&hc, sizeof(Counters), hipHostMallocDefault));
    if (!hs) PGX_HIP(hipHostMalloc((void **)&hs, SPREAD * 8 * sizeof(unsigned long long), hipHostMallocDefault));
    if (!side_stream) PGX_HIP(hipStreamCreateWithFlags(&side_stream, hipStreamNonBlocking));
    for (auto &e : side_ev)
      if (!e) PGX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  ~ReplayState() {
    if (hc) (void)hipHostFree(hc);
    if (hs) (void)hipHostFree(hs);
    if (side_stream) (void)hipStreamDestroy(side_stream);
    for (auto &e : side_ev)
      if (e) (void)hipEventDestroy(e);
  }
};
void CacheFree::operator()(ReplayState *r) const { delete r; }

namespace {
// ---- one attempt -----------------------------------------------------------------------------------------------------------------------
// The schedule's constants.  Every one of them was an environment knob through round 3; tools/knob_sweep.sh (profiles/r04f_knob_sweep_c4s.txt)
// moved each over its plausible range on the repeat-rich 9-Gbase set: 391-405 ms per step whatever the setting (only k_eval_big behind
// instead of beside the narrow kernel is worse, 417 ms), so they are constants now -- those that were only ever on or off are gone, DESIGN.md
// section 4 keeps their numbers; PGX_REPLAY_WIN / _K stay because the parity tests randomise the schedule with them.
constexpr size_t WIN0 = 16384, WIN1 = 131072;   // the first pass ramps its window from WIN0 up to WIN1
// dense rounds only while more than 1 / DENSE_DEN of the buckets is dirty.  (Through round 4 also from 65,536 dirty buckets on: the second sweep of a
// full-size c4 chunk -- 275 k wrong guesses among 2.7 M buckets -- then went window by window, 41 passes each as long as its longest big bucket, 52 ms;
// as sparse passes from the list: 7.06 -> 6.97 s per step, + 0.3 % evaluations.)
constexpr size_t DENSE_DEN = 3;
constexpr size_t TAIL_MAX = 4000;   // tail mode (file_for_reader, look-ahead) once a sweep asks for at most this many alignments, or 1/256 of the first sweep's
constexpr uint32_t AHEAD = 24;      // tail mode: partners of a row filed ahead
// sparse passes per host round trip.  Round 2 measured 2 .. 8 within 1 % of each other and kept 4; with the GPU no longer waiting for the
// host elsewhere (round 3) the round trips and the k_file pass that precedes each one show: 8 instead of 4 = replay kernels 38.0 -> 35.5 ms
// and the step 113.4 -> 111.2 ms at c3, c4s 437 -> 429 ms, c5s 651 -> 639 (6), the E. coli-size set unchanged
constexpr int CHAIN = 8;
constexpr size_t BIG_BATCH = 100000;   // alignments from which a sweep is worth a round trip to know how many guesses were wrong

enum class Narrow { eval, rows };   // k_eval: 16 lanes per bucket; k_eval_rows<64, 16>: a wavefront per bucket, four rows per step
struct Walk {
  const pgx_seqdb *const db;
  ReplayState &rs;
  const size_t nb, ne;   // buckets; bucket entries (at least 1024: dev_replay)
  const int band;
  const bool trace;
  const hipStream_t s = ctx().stream;
  const double t0 = wall_ms();
  // the knobs, read per call
  const bool timed = env_int("PGX_REPLAY_TIMING", 0) != 0;   // "replay_*" in pgx_timing_get: every kernel between events of its own, k_eval_big BEHIND the narrow kernel
  const bool deep = env_int("PGX_TRACE", 0) >= 2; // wall times per dense iteration (synchronises after every launch)
  const size_t window = getenv("PGX_REPLAY_WIN") ? (size_t)atoll(getenv("PGX_REPLAY_WIN")) : (size_t)262144;
  // evaluate / update iterations per window of a dense round: 2 (through round 4: 3; at full-size c4 6.89 -> 6.81 s per step with 2 and 6.90 with 1,
  // c3 / c4s / c5s unchanged; the third iteration of a window mostly re-runs k_eval_big's longest bucket for a handful of dirty buckets that the
  // sparse passes behind the round pick up anyway)
  const int inner = env_int("PGX_REPLAY_K", 2);
  Sizes z;
  Tables tab;
  DevBuf<uint32_t> bid, words, dlist, blist, cblk;
  DevBuf<Item> items;
  DevBuf<RNode> rn;
  DevBuf<pgx_align_key> rq_key;
  DevBuf<pgx_match> rq_res;
  DevBuf<uint8_t> bytes;
  DevBuf<uint4> wcur;   // (one slot per wavefront of k_eval: GPW buckets each; list mode; k_eval_big)
  DevBuf<Counters> dc;
  DevBuf<unsigned long long> spread;
  R r;
  Counters *hc = nullptr;   // the counters as of the last fetch (rs.hc)
  bool use_big = false;     // k_setup marked a bucket for k_eval_big
  // what the host knows about the dirty set
  size_t n_dirty;                // as of the last fetch
  uint32_t d_lo = 0, d_hi;       // range holding the dirty buckets
  bool known = true;             // n_dirty / d_lo / d_hi are current
  bool have_list = false;        // the device holds a dirty list (a count has run since the last evaluations)
  // progress
  unsigned sweeps = 0, rounds_total = 0;
  size_t first_req = 0;     // requests [first_req, ...) belong to the running sweep
  size_t first_batch = 0;   // alignments the first sweep asked for
  double align_ms = 0;
  Walk(const pgx_seqdb *db_, size_t nb_, size_t ne_, int band_, bool trace_, const Mult &mult)
      : db(db_), rs(get_or_make(db_->caches.replay)), nb(nb_), ne(ne_), band(band_), trace(trace_), z(ne_, nb_, mult), n_dirty(nb_), d_hi((uint32_t)nb_) {
    memset(&r, 0, sizeof(r));
  }
  // -- setup: the tables (taken over or allocated), the arenas and the per-bucket state, cleared; k_setup
  void alloc_tables() {
    Tables &pre = rs.pre;
    const bool forced = getenv("PGX_REPLAY_COLD_SHIFT") != nullptr;
    const size_t pre_hold = pre.bytes();   // (what the pre-cleared tables hold was free memory when round 5 measured the rule of share_readers: counted as free here too)
    const bool take = pre.held() && pre.hot.n == z.pcap && pre.memo.n == z.mcap && !forced;   // (its reader lists: below, once the shift is known)
    if (take) tab.hot = std::move(pre.hot), tab.memo = std::move(pre.memo), tab.hot_zero = tab.memo_zero = true;
    tab.alloc(z.pcap, 0, 0);
    size_t free_b = 0, total_b = 0;
    const bool measured = !forced && hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    z.share_readers(measured ? free_b + dev_cache_free_bytes() + pre_hold : SIZE_MAX);   // (the last stage's tables are in the cache)
    if (take && pre.cold.n == z.ccap) tab.cold = std::move(pre.cold), tab.cold_zero = true;
    else pre.cold.release();
    tab.alloc(z.pcap, z.ccap, z.mcap);
    pre.drop();   // (whatever was not taken over goes back to the block cache)
    r.ph = tab.hot.p, r.pc = tab.cold.p, r.cshift = z.cshift, r.pmask = z.pcap - 1, r.mt = tab.memo.p, r.mmask = z.mcap - 1;
  }
  void alloc_state() {
    r.item_cap = z.item_cap, r.rn_cap = z.rn_cap, r.req_cap = z.req_cap;
    alloc_tagged("replay.items", items, r.item_cap), alloc_tagged("replay.reader_nodes", rn, r.rn_cap);
    alloc_tagged("replay.requests", rq_key, r.req_cap), alloc_tagged("replay.requests", rq_res, r.req_cap);
    r.items = items.p, r.rn = rn.p, r.rq_key = rq_key.p, r.rq_res = rq_res.p;
    bytes.alloc(nb * 5), words.alloc(nb * 5);
    r.dirty = bytes.p, r.evaluated = bytes.p + nb, r.parity = bytes.p + 2 * nb, r.bflags = bytes.p + 3 * nb, r.ever = bytes.p + 4 * nb;
    r.ihead = words.p, r.inum = words.p + nb, r.ohead = words.p + 2 * nb, r.lookups = words.p + 3 * nb, r.skips = words.p + 4 * nb;
    wcur.alloc(nb + 2 + SPARSE_CAP + 1 + (size_t)BIG_WG * BIG_NW);
    r.wcur = wcur.p, r.wlist0 = (uint32_t)(nb + 2), r.wbig0 = (uint32_t)(nb + 2 + SPARSE_CAP + 1);
    dlist.alloc(LIST_CAP), blist.alloc(LIST_CAP + 64), dc.alloc(1), spread.alloc(SPREAD * 8);
    r.dlist = dlist.p, r.blist = blist.p, r.c = dc.p, r.spread = spread.p;
  }
  void setup(const DevicePairs &dp, const uint32_t *visit_bids, const uint32_t *d_bids, uint32_t bestn) {
    rs.handles(), hc = rs.hc;
    r.nb = (uint32_t)nb;
    if (!d_bids) bid.alloc(nb), bid.upload(visit_bids, nb);   // (d_bids: the visit list was assembled on the device, dev_place_bids)
    r.bid = d_bids ? d_bids : bid.p, r.bstart = dp.bstart.p, r.y0 = dp.y0.p, r.dir = dp.dir.p, r.rlen = db->d_rlen.p;
    alloc_tables();
    alloc_state();
    // big buckets (>= big_min entries, no read twice) are evaluated by a workgroup each: k_eval_big beside every evaluation launch
    // (measured at C4 scale: the buckets that hold a read twice -- 7 k of 2.3 M, up to 128 entries, one partner at a time in the narrow
    // kernels -- were what every sparse pass waited for; big buckets WITHOUT a repeated read are rare (40 of 2.3 M beyond 48 entries:
    // the multiplicity cut-off removes the repeat families' shimmers) and stay with the narrow kernels by default)
    // (round 4: 48 -- with k_eval_big's walk a third shorter the long buckets WITHOUT a repeated read are better off there too: k_eval_rows 38 -> 22 ms
    //  per c4s step, hidden behind k_eval_big as it is: 360 -> 354 ms; from 24 entries on k_eval_big doubles, 411 ms.  Sixteen wavefronts = eight
    //  rows a step (-DPGX_BIG_NW=16): k_eval_big 56 -> 186 ms.)
    // (k_eval_big now looks a bucket's pairs up once and walks them on one wavefront, pgx_replay.h; swept again on c4s, profiles/eval_big_walk.txt:
    //  32 / 12, 48 / 6 and 32 / 6 within 1 ms of 48 / 12, 24 -> + 30 ms, 16 -> + 137 ms: a pass still waits for k_eval_big, so the thresholds stay)
    r.big_min = (uint32_t)std::max(0, env_int("PGX_REPLAY_BIG", 48));
    r.dup_min = (uint32_t)std::max(0, env_int("PGX_REPLAY_DUP", 12));
    r.predict = std::max(END_FUZZ * 2 - 8, 1), r.predict2 = END_FUZZ * 2 - 8;
    r.bestn = bestn, r.settled = 0;
    PGX_HIP(hipMemsetAsync(spread.p, 0, SPREAD * 8 * sizeof(unsigned long long), s));
    {
      std::optional<KernelTimer> tm;
      if (timed) tm.emplace("replay_misc", nb);
      const bool took = tab.hot_zero, took_cold = tab.cold_zero;
      tab.clear(s);
      if (trace && took) fprintf(stderr, "[pgx]   replay tables taken over pre-cleared (pair table%s, memo)\n", took_cold ? ", reader lists" : "");
      PGX_HIP(hipMemsetAsync(bytes.p, 0, nb * 5, s));
      PGX_HIP(hipMemsetAsync(words.p, 0, nb * 5 * sizeof(uint32_t), s));
      PGX_HIP(hipMemsetAsync(dc.p, 0, sizeof(Counters), s));
      hipLaunchKernelGGL(k_init_slots, dim3(cdiv256(wcur.n)), dim3(256), 0, s, wcur.p, (uint32_t)wcur.n, (uint32_t)(nb / GPW + 2), r.wlist0, dc.p);
      if (trace) setup_with_histogram();
      else hipLaunchKernelGGL(k_setup, dim3(cdiv256(nb)), dim3(256), 0, s, r, (uint32_t *)nullptr);
    }
    if (r.big_min || r.dup_min) {   // no big bucket in this set (uniform-random genomes): none of the ~100 passes of a step launches k_eval_big
      fetch(false);
      use_big = hc->nbig_total != 0;
    }
    cblk.alloc((nb + CB - 1) / CB * 3);
  }
  void setup_with_histogram() {
    DevBuf<uint32_t> hist(32);
    PGX_HIP(hipMemsetAsync(hist.p, 0, 32 * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_setup, dim3(cdiv256(nb)), dim3(256), 0, s, r, hist.p);
    uint32_t h[32];
    hist.download(h, 32);
    sync();
    fprintf(stderr, "[pgx]   buckets by entries / 8 (last class: >= 120):");
    for (int i = 0; i < 16; ++i) fprintf(stderr, " %u", h[i]);
    fprintf(stderr, "\n[pgx]   ... of those holding a read twice (one partner at a time):");
    for (int i = 0; i < 16; ++i) fprintf(stderr, " %u", h[16 + i]);
    fprintf(stderr, "\n");
  }
  // -- the host's view of the device: counters (and, with `totals`, the spread totals) to the pinned mirrors; synchronises
  void fetch(bool totals, bool counters = true) {
    if (counters) PGX_HIP(hipMemcpyAsync(hc, dc.p, sizeof(Counters), hipMemcpyDeviceToHost, s));
    if (totals) PGX_HIP(hipMemcpyAsync(rs.hs, spread.p, SPREAD * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    sync();
    if (totals) sum_totals();
  }
  void sum_totals() {
    const unsigned long long *hs = rs.hs;
    hc->evals = hc->lookups = hc->skips = 0;
    hc->records = 0;   // (re-used as the stream checksum k_emit adds up in word 7 of every line)
    for (uint32_t i = 0; i < SPREAD; ++i) hc->evals += hs[i * 8], hc->lookups += hs[i * 8 + 1], hc->skips += hs[i * 8 + 2], hc->records += hs[i * 8 + 7];
#ifdef PGX_BIG_STATS
    unsigned long long b3 = 0, b4 = 0, b5 = 0, b6 = 0, b7 = 0;
    for (uint32_t i = 0; i < SPREAD; ++i) b3 += hs[i * 8 + 3], b4 += hs[i * 8 + 4], b5 += hs[i * 8 + 5], b6 += hs[i * 8 + 6], b7 += hs[i * 8 + 7];
    fprintf(stderr, "[pgx]   k_eval_big so far: %u evaluations, %llu row passes, %llu rows committed; passes cut at a duplicate %llu, rows ended by a containment %llu, rows of more than one pass %llu; longest %u passes, %u evaluations of >= 64 passes (entries %u); %llu pairs looked up\n",
            hc->big_evals, b3, b4, b5, b6, b7, hc->big_max_passes, hc->big_long, hc->big_long_n, hc->big_pairs);
    {   // the phases (Counters): 10 ns ticks -> ms
      const unsigned long long *a = hc->big_cyc, *l = hc->big_cyc_long;
      const double sa = (double)(a[0] + a[1] + a[2]), sl = (double)(l[0] + l[1] + l[2]);
      fprintf(stderr, "[pgx]   k_eval_big phases, all evaluations: LOOK %.2f ms, WALK %.2f, COMMIT %.2f (%.0f / %.0f / %.0f %%); the longest evaluation of each of %u launches: LOOK %.2f ms, WALK %.2f, COMMIT %.2f (%.0f / %.0f / %.0f %%)\n",
              a[0] * 1e-5, a[1] * 1e-5, a[2] * 1e-5, sa ? 100 * a[0] / sa : 0, sa ? 100 * a[1] / sa : 0, sa ? 100 * a[2] / sa : 0, hc->big_launches,
              l[0] * 1e-5, l[1] * 1e-5, l[2] * 1e-5, sl ? 100 * l[0] / sl : 0, sl ? 100 * l[1] / sl : 0, sl ? 100 * l[2] / sl : 0);
    }
#endif
#ifdef PGX_SETTLE_STATS
    unsigned long long c3 = 0, c4 = 0, c5 = 0, c6 = 0;
    for (uint32_t i = 0; i < SPREAD; ++i) c3 += hs[i * 8 + 3], c4 += hs[i * 8 + 4], c5 += hs[i * 8 + 5], c6 += hs[i * 8 + 6];
    fprintf(stderr, "[pgx]   wrong guesses so far: type %llu, rejected short overlap %llu, rejected no match %llu, rejected other %llu\n", c3, c4, c5, c6);
#endif
  }
  void learn_dirty() { n_dirty = hc->ndirty, known = true, d_lo = n_dirty ? hc->min_dirty : 0, d_hi = n_dirty ? hc->max_dirty + 1 : 0; }   // (from the counters just fetched)
  uint32_t gave_up(uint32_t ov) {   // the attempt's result where it is not 0: the OV_* bits of what overflowed
    if (trace || !(ov & (OV_ITEMS | OV_NODES | OV_REQS | OV_PAIRS | OV_MEMO)))
      fprintf(stderr, "[pgx] note: the device replay gave up (code %u: items %u of %u, reader nodes %u of %u, requests %u of %u)\n", ov,
              hc->item_top, r.item_cap, hc->rnode_top, r.rn_cap, hc->nreq, r.req_cap);
    return ov;
  }
  // -- count + list of the dirty buckets of [lo, hi): no host round trip, ndirty, the range and the list stay on the device
  void count(uint32_t lo = 0, uint32_t hi = NONE) {
    hi = std::min<uint32_t>(hi, (uint32_t)nb);
    const uint32_t nbl = std::max<uint32_t>(1, (hi - lo + CB - 1) / CB);
    std::optional<KernelTimer> tm;
    if (timed) tm.emplace("replay_misc", 0);
    hipLaunchKernelGGL(k_count_a, dim3(nbl), dim3(256), 0, s, r, lo, hi, cblk.p);
    hipLaunchKernelGGL(k_count_b, dim3(nbl), dim3(256), 0, s, r, lo, hi, cblk.p, nbl);
  }
  void count_all() { count(), have_list = true; }
  // -- ONE evaluate / update pass, the only place that launches the evaluation kernels and k_update.  list == 0: over the buckets [lo, hi);
  // DEV_LIST_WIN: over the dirty ones among them, listed here first; DEV_LIST: over the list the last count left on the device.  `groups` buckets
  // at most, evaluated by `narrow`, the big ones among them by k_eval_big, a workgroup each.  A launch of k_eval_big lasts as long as its longest
  // bucket (~0.4 ms of dependent probes), whatever else the GPU could be doing: in list mode -- the count has noted the list's big buckets -- it runs
  // BESIDE the narrow kernel, on the second stream.  In range mode the narrow kernel notes them as it meets them, so k_eval_big comes behind it; so it
  // does where every kernel is timed by itself (PGX_REPLAY_TIMING: "replay_dense" = k_eval and the window's count, "replay_rows" = k_eval_rows,
  // "replay_big", "replay_update"; units: the buckets of a window, once) or walled (PGX_TRACE=2).
  void pass(uint32_t lo, uint32_t hi, uint32_t list, Narrow narrow, uint32_t groups, uint64_t units) {
    std::optional<KernelTimer> tm;
    if (timed) tm.emplace(narrow == Narrow::rows ? "replay_rows" : "replay_dense", units);
    const bool walled = deep && list != DEV_LIST;   // (the dense rounds' iterations)
    double td = 0, t_eval = 0;
    if (walled) sync(), td = wall_ms();
    // all but the very first evaluation of a window find only a part of its buckets dirty: they run from the window's
    // list (wavefronts full of live buckets) instead of over every bucket of the window
    if (list == DEV_LIST_WIN) count(lo, hi);
    const uint32_t a = list ? 0u : lo, b = list ? (uint32_t)nb : hi;   // (a list's entries are buckets of [0, nb))
    const uint32_t big_a = list == DEV_LIST_WIN ? LIST_CAP : list == DEV_LIST ? groups : lo;   // (list mode: the list entries this pass covers)
    const dim3 big_grid(grid_cap(std::min<uint32_t>(BIG_WG, groups))), big_block(64 * BIG_NW), grid(cdiv256((size_t)groups * GL));
    const bool side = use_big && list && !timed && !deep;
    if (side) {
      PGX_HIP(hipEventRecord(rs.side_ev[0], s));
      PGX_HIP(hipStreamWaitEvent(rs.side_stream, rs.side_ev[0], 0));
      hipLaunchKernelGGL(k_eval_big, big_grid, big_block, 0, rs.side_stream, r, big_a, b, list);
      PGX_HIP(hipEventRecord(rs.side_ev[1], rs.side_stream));
    }
    if (narrow == Narrow::rows) hipLaunchKernelGGL((k_eval_rows<64, 16>), dim3(cdiv256((size_t)groups * 64)), dim3(256), 0, s, r, a, b, list);
    else hipLaunchKernelGGL(k_eval, grid, dim3(256), 0, s, r, a, b, list);
    tm.reset();
    if (side) {
      PGX_HIP(hipStreamWaitEvent(s, rs.side_ev[1], 0));
    } else if (use_big) {
      if (timed) tm.emplace("replay_big", 0);
      hipLaunchKernelGGL(k_eval_big, big_grid, big_block, 0, s, r, big_a, b, list);
      tm.reset();
    }
    if (walled) sync(), t_eval = wall_ms() - td, td = wall_ms();
    if (timed) tm.emplace("replay_update", 0);
    hipLaunchKernelGGL(k_update, grid, dim3(256), 0, s, r, a, b, list);
    tm.reset();
    if (walled) sync(), fprintf(stderr, "[pgx]     iteration: eval %.3f ms, update %.3f ms\n", t_eval, wall_ms() - td);
  }
  // -- dense round: many of the buckets are dirty -- a group of 16 lanes each, window by window in bucket order (a window's buckets mostly
  // depend on earlier windows), `inner` evaluate / update iterations per window
  void dense_round(bool first_pass) {
    const size_t a_lo = d_lo & ~(size_t)63;  // (aligned: a bucket always belongs to the same wavefront slot)
    const size_t win = n_dirty > window / 4 ? window : (size_t)(d_hi - a_lo);
    // the very first pass ramps the window up (WIN0, 2 WIN0, ... window): with an empty pair table every bucket of a window
    // believes it owns all its pairs, and the early windows -- where nothing is "seen" yet -- re-evaluate nearly all of their
    // buckets; smaller windows there mean fewer wasted evaluations (2.20 M -> 1.7 M at 4.5 Gbases), later ones are launch-bound
    const size_t cap = first_pass ? std::min(WIN1, win) : win;
    size_t step = first_pass ? std::min(WIN0, cap) : win;
    for (size_t lo = a_lo, nxt; lo < d_hi; lo = nxt, step = std::min(step * 2, cap)) {
      nxt = lo + step;
      const uint32_t hi = (uint32_t)std::min<size_t>(d_hi, nxt), n = hi - (uint32_t)lo;
      for (int k = 0; k < inner; ++k) {
        const bool from_list = !(first_pass && k == 0) && n <= LIST_CAP;
        pass((uint32_t)lo, hi, from_list ? DEV_LIST_WIN : 0u, Narrow::eval, n, k == 0 ? n : 0);
      }
    }
    count_all();
  }
  // -- sparse chain: CHAIN passes straight from the list the last count left on the device -- the kernels read its length there,
  // so the host is not in the loop (a pass with nothing to do costs two empty launches); what a pass dirties is listed by
  // the count behind it.  A wavefront per bucket, four rows per step.
  void sparse_chain() {
    if (!have_list) count_all();
    const size_t est = known && n_dirty <= SPARSE_CAP / 4 ? std::max<size_t>(n_dirty * 4, 1024) : (size_t)SPARSE_CAP;
    const uint32_t groups = (uint32_t)std::min<size_t>(est, SPARSE_CAP);
    for (int c = 0; c < CHAIN; ++c) {
      pass(0, (uint32_t)nb, DEV_LIST, Narrow::rows, groups, 0);
      count_all();
    }
  }
  // -- file what the clean buckets need (always safe), then one round trip for everything: dirty count, range, requests
  uint32_t file_and_fetch(unsigned rounds) {
    {
      std::optional<KernelTimer> tm;
      if (timed) tm.emplace("replay_misc", 0);
      hipLaunchKernelGGL(k_file, dim3(cdiv256(nb)), dim3(256), 0, s, r, (uint32_t)nb);
    }
    fetch(trace);
    if (hc->overflow) return hc->overflow;
    learn_dirty();
    r.memo_used = hc->nreq != 0;
    if (trace)
      fprintf(stderr, "[pgx]   round %u: %zu dirty left in [%u, %u), %llu evaluations, t = +%.2f ms\n", rounds, n_dirty, d_lo, d_hi,
              (unsigned long long)hc->evals, wall_ms() - t0);
    return 0;
  }
  // -- the sweep's new requests aligned, every guess checked against its result: a wrong guess makes its bucket dirty again
  uint32_t align_and_settle(size_t nreq) {
    const double a0 = wall_ms();
    const size_t batch = nreq - first_req;
    if (sweeps == 1) first_batch = batch;
    r.tail = batch <= std::max(TAIL_MAX, first_batch / 256) ? AHEAD : 0u;   // (the NEXT sweep's k_file)
    dev_align(db, r.rq_key + first_req, batch, band, r.rq_res + first_req, sweeps > 2 ? 2 : sweeps > 1 ? 1 : 0);
    r.settled = (uint32_t)nreq, first_req = nreq;
    {
      std::optional<KernelTimer> tm;
      if (timed) tm.emplace("replay_misc", 0);
      hipLaunchKernelGGL(k_settle, dim3(cdiv256(nb)), dim3(256), 0, s, r);
    }
    count_all();
    if (batch > BIG_BATCH) {  // a big batch: worth a round trip to know how many guesses were wrong (dense or sparse next)
      fetch(false);
      if (hc->overflow) return hc->overflow;
      learn_dirty();
      if (trace) fprintf(stderr, "[pgx]   alignments + settle %.2f ms, %zu buckets guessed wrong\n", wall_ms() - a0, n_dirty);
    } else {
      known = false;  // (a small batch: the wrong guesses are handled by the sparse passes of the next round)
      n_dirty = std::min<size_t>(batch, SPARSE_CAP / 8);
      if (trace) fprintf(stderr, "[pgx]   %zu alignments + settle enqueued in %.2f ms\n", batch, wall_ms() - a0);
    }
    align_ms += wall_ms() - a0;
    return 0;
  }
  // -- the records, in bucket order; what the stage used, for the next one's sizes
  uint32_t emit(const std::function<pgx_ovlp *(size_t)> &alloc_out, RecordSink *sink, size_t *n_out, pgx_overlap_stats *st, Usage *usage) {
    const double e0 = wall_ms();
    DevBuf<uint32_t> off(nb + 1);
    exclusive_sum(r.inum, off.p, nb);
    uint32_t last_off = 0, last_num = 0;
    PGX_HIP(hipMemcpyAsync(&last_off, off.p + nb - 1, 4, hipMemcpyDeviceToHost, s));
    PGX_HIP(hipMemcpyAsync(&last_num, r.inum + nb - 1, 4, hipMemcpyDeviceToHost, s));
    // The attempt's LAST overflow check, in the round trip the record count needs anyway: neither k_count_pairs nor k_emit raises a bit, and
    // a sink must never take the records of an attempt that goes on to report an overflow (it cannot give them back: RecordSink::take).
    fetch(false);
    if (hc->overflow) return hc->overflow;
    const size_t nrec = (size_t)last_off + last_num;
    // (the table census for the next stage's sizes runs HERE, ahead of the record copy: a memory-bound kernel beside the copy's blit kernel
    //  crawls -- 40 ms instead of 0.5 for these 2 GB, profiles/r05e_chunk_timeline_c4.txt)
    DevBuf<unsigned long long> d_keys(1);
    PGX_HIP(hipMemsetAsync(d_keys.p, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_count_pairs, dim3((unsigned)std::min<size_t>(cdiv256(z.pcap), 4096)), dim3(256), 0, s, tab.hot.p, z.pcap, d_keys.p);
    results_wait();   // (pgx_results_async: the previous stage's record copy -- long finished -- gives its device buffer back first)
    pgx_ovlp *host = alloc_out(nrec);
    DevBuf<pgx_ovlp> d_out;
    alloc_tagged("replay.records_out", d_out, std::max<size_t>(nrec, 1));
    {
      std::optional<KernelTimer> tm;
      if (timed) tm.emplace("replay_emit", nrec);   // the records written and brought to the host (pinned destination)
      hipLaunchKernelGGL(k_emit, dim3(cdiv256(nb)), dim3(256), 0, s, r, off.p, d_out.p);
      // pgx_results_async: the copy runs on its own stream behind k_emit and this call returns without it -- the 2.9 GB of a human-scale
      // chunk (55 ms over PCIe) overlap the NEXT chunk's join and first sweep; the caller waits (pgx_results_wait) before it reads
      if (nrec && sink) sink->take(std::move(d_out), nrec);   // (served commands: device -> output file, pgx_served.cpp)
      else if (nrec && results_async() && !timed) results_copy_async(host, std::move(d_out), nrec);
      else if (nrec) PGX_HIP(hipMemcpyAsync(host, d_out.p, nrec * sizeof(pgx_ovlp), hipMemcpyDeviceToHost, s));
    }
    unsigned long long n_keys = 0;
    d_keys.download(&n_keys, 1);
    fetch(true, false);   // (the totals and the stream checksum; the counters have not moved since the check above)
    usage->pairs = (double)n_keys / ne, usage->reqs = (double)hc->nreq / ne, usage->items = (double)hc->item_top / ne, usage->nodes = (double)hc->rnode_top / ne;
    if (trace)
      fprintf(stderr, "[pgx]   tables: %llu read pairs in %u slots (load %.2f), %u alignments in %u memo slots (load %.2f), items %u of %u, reader nodes %u of %u, requests %u of %u\n",
              n_keys, z.pcap, (double)n_keys / z.pcap, hc->nreq, z.mcap, (double)hc->nreq / z.mcap, hc->item_top, r.item_cap, hc->rnode_top, r.rn_cap, hc->nreq, r.req_cap);
    rs.last_pcap = z.pcap, rs.last_mcap = z.mcap, rs.last_ccap = z.ccap;
    *n_out = nrec;
    if (st) {
      st->n_align_needed = hc->lookups, st->n_seen_skip = hc->skips, st->n_align_gpu = first_req, st->rounds = sweeps, st->n_evaluations = hc->evals;
#if !defined(PGX_BIG_STATS) && !defined(PGX_SETTLE_STATS)
      st->stream_checksum = hc->records;
#endif
    }
    if (trace)
      fprintf(stderr, "[pgx] device replay: %u sweeps, %u rounds, %llu evaluations, %zu records; emit %.2f ms; alignments %.2f ms; total %.2f ms\n",
              sweeps, rounds_total, (unsigned long long)hc->evals, nrec, wall_ms() - e0, align_ms, wall_ms() - t0);
    return 0;
  }
  // -- the fixed point as the head of this file describes it; 0, or the OV_* bits of what overflowed
  uint32_t run(const std::function<pgx_ovlp *(size_t)> &alloc_out, RecordSink *sink, size_t *n_out, pgx_overlap_stats *st, Usage *usage) {
    for (;;) {   // a sweep
      ++sweeps;
      const double p0 = wall_ms();
      unsigned rounds = 0;
      do {   // evaluate / update until no bucket is dirty
        ++rounds;
        if (known && n_dirty * DENSE_DEN > nb) dense_round(sweeps == 1 && rounds == 1);
        sparse_chain();
        if (const uint32_t ov = file_and_fetch(rounds)) return gave_up(ov);
        if (n_dirty && rounds > 20000) return gave_up(OV_PASSES);   // (cannot happen: the lowest unstable bucket rises every pass)
      } while (n_dirty);
      rounds_total += rounds;
      const size_t nreq = hc->nreq;
      if (trace)
        fprintf(stderr, "[pgx] device sweep %u: %u rounds, %llu evaluations so far, %.2f ms, %zu requests\n", sweeps, rounds,
                (unsigned long long)hc->evals, wall_ms() - p0, nreq - first_req);
      if (nreq == first_req) break;   // the sweep filed nothing: every alignment the lists need is known
      if (const uint32_t ov = align_and_settle(nreq)) return gave_up(ov);
      if (!n_dirty) break;            // every guess was right
    }
    const uint32_t ov = emit(alloc_out, sink, n_out, st, usage);
    return ov ? gave_up(ov) : 0;
  }
};

// the visit list on the device from the per-group slices the host's table replay left (pgx_overlap.cpp::build_visit, ids-only form)
__global__ void k_place_bids(const uint32_t *__restrict__ ids_all, const uint32_t *__restrict__ psrc, const uint32_t *__restrict__ pcnt,
                             const uint64_t *__restrict__ pdst, uint32_t n_groups, uint32_t *__restrict__ bid) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_groups) return;
  const uint32_t src = psrc[i], n = pcnt[i];
  const uint64_t dst = pdst[i];
  for (uint32_t k = 0; k < n; ++k) bid[dst + k] = ids_all[src + k];
}
}  // namespace
void dev_place_bids(const uint32_t *ids_all, size_t n_ids, const uint32_t *psrc, const uint32_t *pcnt, const uint64_t *pdst,
                    size_t n_groups, size_t nb, DevBuf<uint32_t> &bid) {
  bid.alloc(std::max<size_t>(nb, 1));
  if (!n_groups || !nb) return;
  DevBuf<uint32_t> d_ids(n_ids), d_src(n_groups), d_cnt(n_groups);
  DevBuf<uint64_t> d_dst(n_groups);
  d_ids.upload(ids_all, n_ids), d_src.upload(psrc, n_groups), d_cnt.upload(pcnt, n_groups), d_dst.upload(pdst, n_groups);
  hipLaunchKernelGGL(k_place_bids, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, ctx().stream, d_ids.p, d_src.p, d_cnt.p, d_dst.p,
                     (uint32_t)n_groups, bid.p);
  sync();   // (the upload sources are the caller's host arrays; the temporaries go back to the block cache)
}

void replay_drop_precleared(const pgx_seqdb *db) {   // (a stage that ended without a device replay: nothing cleared ahead of time outlives it)
  if (db->caches.replay) db->caches.replay->pre.drop();
}

// called by the stage's visit phase while the GPU would otherwise wait for the host's outer table: tables of the last stage's sizes, cleared, on ctx().stream
void replay_preclear(const pgx_seqdb *db) {
  ReplayState &rs = get_or_make(db->caches.replay);
  Tables &pre = rs.pre;
  if (!rs.last_pcap || pre.held() || env_int("PGX_REPLAY_PRECLEAR", 1) == 0) return;
  size_t free_b = 0, total_b = 0;
  const size_t need = rs.last_pcap * sizeof(PHot) + rs.last_ccap * sizeof(PCold) + rs.last_mcap * sizeof(MSlot);
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || need > free_b + dev_cache_free_bytes()) return;   // (no room ahead of time: the attempt decides)
  try {
    pre.alloc(rs.last_pcap, rs.last_ccap, rs.last_mcap);
    pre.clear(ctx().stream);
  } catch (const Fail &) {
    (void)hipGetLastError();
    pre.drop();
  }
}

bool dev_replay(const pgx_seqdb *db, const DevicePairs &dp, const uint32_t *visit_bids, const uint32_t *d_bids, size_t nb, size_t n_entries,
                uint32_t bestn, int band, uint32_t ovlp_upper, const std::function<pgx_ovlp *(size_t)> &alloc_out, RecordSink *sink,
                size_t *n_out, pgx_overlap_stats *st, bool trace) {
  *n_out = 0;
  ReplayState &rs = get_or_make(db->caches.replay);
  struct DropPre {   // (tables cleared ahead of time that no attempt took over do not outlive the stage)
    Tables &pre;
    ~DropPre() { pre.drop(); }
  } drop_pre{rs.pre};
  // what the encodings hold (anything else goes to the host replay)
  if (ovlp_upper > 128 || nb >= (1u << 29) - 2 || n_entries >= (1ULL << 31) || !dp.valid) return false;
  if (nb == 0) {
    alloc_out(0);
    return true;
  }
  const size_t ne = std::max<size_t>(n_entries, 1024);
  {  // the device tables must fit beside what is already resident (otherwise the host replay, which only needs host memory)
    const size_t need = default_need(ne, nb);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b) {
      rs.pre.drop();     // (tables cleared ahead of time are part of what `need` prices)
      dev_cache_trim();  // (blocks the cache holds for re-use count as used)
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || need > free_b) {
        fprintf(stderr, "[pgx] note: the device replay's tables (%.1f GB) do not fit the free device memory (%.1f GB); the host replay takes over\n",
                need / 1e9, free_b / 1e9);
        return false;
      }
    }
  }
  Mult mult = Mult::from(rs.learned, ne, nb);
  for (int attempt = 0; attempt < 4; ++attempt) {
    Usage usage;
    uint32_t ov;
    try {   // one attempt with these table sizes: 0, or the OV_* bits of what overflowed
      MemTag mem_tag("replay.other");
      Walk w(db, nb, ne, band, trace, mult);
      w.setup(dp, visit_bids, d_bids, bestn);
      ov = w.run(alloc_out, sink, n_out, st, &usage);
    } catch (const Fail &f) {
      //  tables sized by what an EARLIER stage used -- possibly another job's in a long-lived server -- may not fit where the
      // defaults would: once more with the defaults and the memory forgotten, else the host replay (which only needs host memory)
      if (f.code != PGX_ENOMEM && !(f.code == PGX_EHIP && strstr(pgx_last_error(), "hipMalloc"))) throw;   // (only a failed allocation)
      (void)hipGetLastError();
      const bool had_learned = rs.learned.pairs > 0;
      rs.forget();
      dev_cache_trim();
      if (!had_learned || attempt > 0) {
        fprintf(stderr, "[pgx] note: the device replay's tables could not be allocated (%s); the host replay takes over\n", pgx_last_error());
        return false;
      }
      mult = Mult();
      if (trace) fprintf(stderr, "[pgx]   the tables sized by the last stage's use do not fit (%s): once more with the default sizes\n", pgx_last_error());
      continue;
    }
    if (!ov) {
      rs.learned.raise(usage);
      if (st) st->replay_attempts = (uint32_t)attempt + 1;
      return true;
    }
    if (ov & (OV_QOFF | OV_PASSES)) break;  // not a matter of table sizes
    mult.grow(ov);
    if (trace) fprintf(stderr, "[pgx]   next attempt with items x %g, reader nodes x %g, requests x %g, pair table x %g, memo table x %g\n", mult.items, mult.nodes, mult.reqs, mult.pairs, mult.memo);
  }
  fprintf(stderr, "[pgx] note: the device replay's tables overflowed; the host replay takes over\n");
  return false;
}

}  // namespace pgx
