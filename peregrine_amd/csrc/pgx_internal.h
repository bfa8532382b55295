// pgx_internal.h -- shared declarations of libpgx.so (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/pgx.h"

// Every kernel of this library is written for 64-lane wavefronts (ballots as 64-bit masks, `threadIdx.x & 63` lane ids, DPP row
// patterns): refuse to build for a wave32 target instead of computing wrong scan starts there.
// (neither __AMDGCN_WAVEFRONT_SIZE nor a constexpr warpSize exists on ROCm 7 / gfx950; CDNA targets have no wave32 mode, so the
// guard is on the target itself)
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libpgx kernels assume 64-lane wavefronts and gfx950 instructions: build with --offload-arch=gfx950 only"
#endif

namespace pgx {

// ---------------------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------------------
void set_error(const char *fmt, ...);
struct Fail {
  int code;
  int64_t piece = -1;   // a refusal that names a piece of a consensus batch: the caller's number of it (PGX_REQUIRE_PIECE)
};
#define PGX_HIP(call)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      pgx::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      throw pgx::Fail{PGX_EHIP};                                                              \
    }                                                                                         \
  } while (0)
#define PGX_REQUIRE(cond, code, ...) \
  do {                               \
    if (!(cond)) {                   \
      pgx::set_error(__VA_ARGS__);   \
      throw pgx::Fail{code};         \
    }                                \
  } while (0)
// ... of a piece: the Fail carries the piece's number, so that a caller whose pieces are something else's (a contig's segments) can say so
#define PGX_REQUIRE_PIECE(cond, code, piece_no, ...) \
  do {                                               \
    if (!(cond)) {                                   \
      pgx::set_error(__VA_ARGS__);                   \
      throw pgx::Fail{code, (int64_t)(piece_no)};    \
    }                                                \
  } while (0)
// The epilogue of a C entry point: runs body (which returns nothing -- PGX_OK is answered -- or the code to answer); a Fail becomes its
// code, an allocation failure PGX_ENOMEM with a message.  No C++ exception of the library's own leaves an extern "C" function.
template <class F>
int guarded(F &&body) {
  try {
    if constexpr (std::is_void_v<decltype(body())>) body();
    else return body();
  } catch (const Fail &f) {
    return f.code;
  } catch (const std::bad_alloc &) {
    set_error("out of host memory");
    return PGX_ENOMEM;
  }
  return PGX_OK;
}
// The code a stage's builder answers for the Fail its passes threw: a HIP error that is the device running out of memory becomes
// PGX_ENOMEM with "<who>: no device memory for the <what> of <n> <units>" (whatever the builder read is untouched).
inline int build_fail_code(const Fail &f, const char *who, const char *what, uint64_t n, const char *units) {
  if (f.code != PGX_EHIP || hipGetLastError() != hipErrorOutOfMemory) return f.code;
  set_error("%s: no device memory for the %s of %llu %s", who, what, (unsigned long long)n, units);
  return PGX_ENOMEM;
}

// ---------------------------------------------------------------------------------------------------------
// context: one device, one stream
// ---------------------------------------------------------------------------------------------------------
struct Context {
  int device = -1;
  hipStream_t stream = nullptr;
  bool ready = false;
  int num_cu = 256;
};
Context &ctx();
void require_ready();
// The grid of a persistent kernel (a workgroup strides over the items: `for (i = blockIdx.x; i < n; i += gridDim.x)`).
// PGX_GRID_CAP: a test hook, read at every launch, that caps such a grid so that small inputs give a workgroup several items one
// after the other (1: one workgroup takes them all, in order).  Without it (or when it holds no positive integer) a grid is what it was.
inline uint32_t grid_cap(uint64_t grid) {
  const char *v = getenv("PGX_GRID_CAP");
  const long long c = v ? atoll(v) : 0;
  if (c > 0 && (uint64_t)c < grid) grid = (uint64_t)c;
  return (uint32_t)grid;
}
// min(n_items, per_cu workgroups for every CU), under the cap
inline uint32_t stride_grid(uint64_t n_items, uint32_t per_cu) {
  const uint64_t full = (uint64_t)ctx().num_cu * per_cu;
  return grid_cap(n_items < full ? n_items : full);
}
// Per-context device state that outlives a call (buffers handed out as library-owned views, side streams, pinned pools) registers a
// reset function: pgx_shutdown() runs them all BEFORE it returns the cached blocks to the driver, so nothing survives into the next
// pgx_init() (which may choose another device).  Use: static pgx::ShutdownHook h_([] { ... });
// What belongs to a read database (its packs, index plans, DbCaches) goes with the database instead: a database stays on the device
// it was made on.
void on_shutdown(void (*fn)());
struct ShutdownHook {
  explicit ShutdownHook(void (*fn)()) { on_shutdown(fn); }
};
// bumped by every index-stage call that rewrites the index workspaces ("ix.*"): consumers of zero-copy views of those
// workspaces (pgx_pairs_prepare_dev -> pgx_pairs_scatter_dev) compare it to detect that their input was overwritten
uint64_t &index_generation();
bool ws_contains(const void *p);    // p points into one of the named workspaces
bool index_owns(const void *p);     // p points into memory an index-stage call handed out as a library-owned view

// device buffer (RAII, grow-only reuse is up to the caller)
// Device blocks come from a size-class cache: hipMalloc / hipFree are synchronous and cost tens of microseconds each, and
// the stages allocate dozens of temporaries per call.  All work is enqueued on ONE stream, so handing a released block to
// the next user is stream-ordered and safe.  pgx_shutdown() returns everything to the driver.
void *dev_alloc(size_t bytes);
void dev_release(void *p);
void dev_cache_trim();
size_t dev_cache_free_bytes();   // what the cache holds for re-use (the driver counts it as used)
void dev_cache_age();   // a stage starts: cached blocks of 64 MiB and more that two whole stages did not ask for go back to the driver
// device blocks allocated while a MemTag is in scope (on this thread) are booked under its name in the ledger (pgx_mem_ledger)
struct MemTag {
  explicit MemTag(const char *t);
  ~MemTag();
  MemTag(const MemTag &) = delete;
  MemTag &operator=(const MemTag &) = delete;
  const char *prev;
};

template <typename T>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  explicit DevBuf(size_t count) { alloc(count); }
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = o.p, n = o.n;
      o.p = nullptr, o.n = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  void alloc(size_t count) {
    release();
    n = count;
    if (count) p = (T *)dev_alloc(count * sizeof(T));
  }
  void release() {
    if (p) dev_release(p);
    p = nullptr, n = 0;
  }
  void upload(const T *src, size_t count) {
    if (count) PGX_HIP(hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, ctx().stream));
  }
  void download(T *dst, size_t count) const {
    if (count) PGX_HIP(hipMemcpyAsync(dst, p, count * sizeof(T), hipMemcpyDeviceToHost, ctx().stream));
  }
};
inline void sync() { PGX_HIP(hipStreamSynchronize(ctx().stream)); }
// blocks of b for a items; LAUNCH: a thread per item, 256 to a block, on the `st` of the scope it is used in
static inline unsigned cdiv(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }
#define LAUNCH(kernel, n, ...) hipLaunchKernelGGL(kernel, dim3(pgx::cdiv((n), 256)), dim3(256), 0, st, __VA_ARGS__)

// The live objects of one kind that keep device state between calls and are handed to the caller (dedup streams, string graphs,
// unitigs).  T supplies `bool shut` and drop_device_state(), which releases what the object holds on the device (idempotent).  The
// shutdown rule: pgx_shutdown drops the device state of every member and marks it `shut` -- the caller still holds the handle, whose
// entry points then refuse it, and destroys it whenever it likes.  Use: LiveSet<T> g_set; ShutdownHook g_hook([] { g_set.shutdown(); });
// Members are made by live_build (below, behind the timers it flushes).
template <class T>
class LiveSet {
  std::mutex mu;
  std::vector<T *> live;

 public:
  void add(T *t) {
    std::lock_guard<std::mutex> lk(mu);
    live.push_back(t);
  }
  void shutdown() {
    std::lock_guard<std::mutex> lk(mu);
    for (T *t : live) t->drop_device_state(), t->shut = true;
  }
  bool contains(const T *t) {
    std::lock_guard<std::mutex> lk(mu);
    for (T *x : live)
      if (x == t) return true;
    return false;
  }
  // the end of t (a member or not): what is enqueued may still read its buffers, so the stream drains first
  void destroy(T *t) {
    {
      std::lock_guard<std::mutex> lk(mu);
      for (size_t i = 0; i < live.size(); ++i)
        if (live[i] == t) live.erase(live.begin() + i), i = live.size();
      if (!t->shut && ctx().ready) (void)hipStreamSynchronize(ctx().stream);
      t->drop_device_state();
    }
    delete t;
  }
};
inline double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// grow-only named device buffers that persist across calls (hipMalloc/hipFree are synchronous and slow)
void *ws_raw(const char *name, size_t bytes);
template <typename T>
T *ws(const char *name, size_t count) {
  return (T *)ws_raw(name, (count ? count : 1) * sizeof(T));
}

// ---------------------------------------------------------------------------------------------------------
// device-wide primitives (pgx_prims.hip, the one file that includes hipcub): sorts, selects, sums, reductions over device arrays
// ---------------------------------------------------------------------------------------------------------
// hipcub's two-call idiom (size query, workspace, run; one number back and a synchronisation where a count or total is returned), once
// per primitive and element type.  n == 0 is defined by each: no launch, no workspace, count or total 0, offs[0] = 0.  A count that does
// not fit hipcub's int is refused (PGX_EARG).  Nothing here synchronises unless it returns a number.
// tmp: the workspace, a block of the block cache grown with a quarter of slack.  A caller that runs several primitives in a row passes its
// own, so that the sequence allocates once; with none given a call uses one of its own and hands it back to the block cache on return,
// while its kernels are still enqueued -- which is safe on ctx().stream ONLY (the cache's next user comes behind them on that stream).
// A call on any other stream must pass a workspace that outlives the work.
struct PrimWs {
  DevBuf<uint8_t> buf;
  void *get(size_t bytes) {
    if (bytes > buf.n) buf.alloc(bytes + (bytes >> 2) + 256);
    return buf.p;
  }
};
#define PGX_PRIM_TAIL PrimWs *tmp = nullptr, hipStream_t st = ctx().stream
// stable radix sort by the key bits [begin_bit, end_bit), values carried along
void sort_pairs(const uint64_t *k_in, uint64_t *k_out, const uint32_t *v_in, uint32_t *v_out, size_t n, int begin_bit, int end_bit, PGX_PRIM_TAIL);
void sort_pairs(const uint32_t *k_in, uint32_t *k_out, const uint32_t *v_in, uint32_t *v_out, size_t n, int begin_bit, int end_bit, PGX_PRIM_TAIL);
void sort_pairs(const uint8_t *k_in, uint8_t *k_out, const uint32_t *v_in, uint32_t *v_out, size_t n, int begin_bit, int end_bit, PGX_PRIM_TAIL);
void sort_keys(const uint64_t *k_in, uint64_t *k_out, size_t n, int begin_bit, int end_bit, PGX_PRIM_TAIL);
// d[i] = i; out[i] = key[idx[i]]
void iota(uint32_t *d, size_t n, PGX_PRIM_TAIL);
void gather(const uint64_t *key, const uint32_t *idx, size_t n, uint64_t *out, PGX_PRIM_TAIL);
// order_out = the stable order of 0 .. n-1 by (keys[0], keys[1], ..), each key by its low `bits` bits: a chain of sort_pairs from the last
// key to the first, each key but the chain's first gathered behind the order so far.  first_out = keys[0] in that order (it may be
// keys[0] itself where there are more keys).  order_in: the order the chain starts from (equal keys keep its order; not order_out),
// nullptr: 0 .. n-1.  On ctx().stream only: the temporaries (an order, a key column or two) go back to the block cache on return.
struct SortKey {
  const uint64_t *key;
  int bits;
};
void sort_order(std::initializer_list<SortKey> keys, size_t n, const uint32_t *order_in, uint32_t *order_out, uint64_t *first_out, PrimWs *tmp = nullptr);
// list = the i < n, ascending, with flags[i] != 0; returns how many (_dev: leaves the number at d_num instead, no synchronisation)
uint32_t select_indices(const uint8_t *d_flags, size_t n, uint32_t *d_list, PGX_PRIM_TAIL);
uint32_t select_indices(const uint32_t *d_flags, size_t n, uint32_t *d_list, PGX_PRIM_TAIL);
uint64_t select_indices(const uint8_t *d_flags, size_t n, uint64_t *d_list, PGX_PRIM_TAIL);
void select_indices_dev(const uint8_t *d_flags, size_t n, uint32_t *d_list, uint32_t *d_num, PGX_PRIM_TAIL);
// ... with flags[i] != 0 and none of skip_bits set in it
uint32_t select_flagged(const uint32_t *d_flags, size_t n, uint32_t *d_list, uint32_t skip_bits = 0, PGX_PRIM_TAIL);
// out = the in[i] with flags[i] != 0, in order; returns how many
uint64_t select_values(const pgx_mm128 *d_in, const uint8_t *d_flags, size_t n, pgx_mm128 *d_out, PGX_PRIM_TAIL);
// out[i] = in[0] + .. + in[i - 1] (in == out scans in place)
void exclusive_sum(const uint32_t *d_in, uint32_t *d_out, size_t n, PGX_PRIM_TAIL);
void exclusive_sum(const uint64_t *d_in, uint64_t *d_out, size_t n, PGX_PRIM_TAIL);
// offs[0] = 0, offs[i + 1] = vals[0] + .. + vals[i] (n + 1 entries; vals == offs + 1 scans in place); scan_to_total returns offs[n]
void scan_offsets(const uint32_t *d_vals, uint32_t *d_offs, size_t n, PGX_PRIM_TAIL);
uint32_t scan_to_total(const uint32_t *d_vals, uint32_t *d_offs, size_t n, PGX_PRIM_TAIL);
uint64_t scan_to_total(const uint32_t *d_vals, uint64_t *d_offs, size_t n, PGX_PRIM_TAIL);
uint64_t scan_to_total(const uint64_t *d_vals, uint64_t *d_offs, size_t n, PGX_PRIM_TAIL);
// out[i] = max(in[0], .., in[i]) (in == out scans in place)
void running_max(const int32_t *d_in, int32_t *d_out, size_t n, PGX_PRIM_TAIL);
void running_max(const uint64_t *d_in, uint64_t *d_out, size_t n, PGX_PRIM_TAIL);
// *d_out = the sum / the maximum of in[0 .. n) (0 for none), left on the device
void reduce_sum(const uint32_t *d_in, uint32_t *d_out, size_t n, PGX_PRIM_TAIL);
void reduce_max(const uint32_t *d_in, uint32_t *d_out, size_t n, PGX_PRIM_TAIL);
// the runs of equal keys: uniq[r] = the run's key, sums[r] = the sum of its values / counts[r] = its length; return the number of runs
uint32_t sum_by_key(const uint64_t *d_keys, uint64_t *d_uniq, const uint32_t *d_vals, uint32_t *d_sums, size_t n, PGX_PRIM_TAIL);
uint64_t run_lengths(const uint64_t *d_in, uint64_t *d_uniq, uint32_t *d_counts, size_t n, PGX_PRIM_TAIL);
#undef PGX_PRIM_TAIL

// ---------------------------------------------------------------------------------------------------------
// per-kernel timing with HIP events on the library stream
// ---------------------------------------------------------------------------------------------------------
struct KernelTimer {
  KernelTimer(const char *name, uint64_t units);
  ~KernelTimer();
  const char *name;
  uint64_t units;
  hipEvent_t e0, e1;
};
void timing_flush();  // resolve pending events into the totals (synchronises the stream)

// The entry point that builds a member of a LiveSet, once.  In this order: `out` is checked and cleared; no device context is refused;
// pre() throws the stage's own refusals of its arguments and their state; build(obj, &n) fills a new T inside the stage's own MemTag and
// KernelTimer scopes, and keeps n -- the size of its input, in `units` -- current for the message of a device that ran out of memory
// (build_fail_code); the timers are flushed; the object joins the set and goes to *out.  After any failure the object is deleted.
template <class T, class Pre, class Build>
int live_build(const char *who, LiveSet<T> &set, T **out, Pre &&pre, Build &&build, const char *what, const char *units) {
  T *obj = nullptr;
  const int rc = guarded([&] {
    PGX_REQUIRE(out, PGX_EARG, "%s: null argument", who);
    *out = nullptr;
    PGX_REQUIRE(ctx().ready, PGX_ESTATE, "%s: no device context (pgx_init has not been called, or found no HIP device)", who);
    pre();
    int code = PGX_OK;
    uint64_t n = 0;
    try {
      obj = new T;
      build(obj, &n);
    } catch (const Fail &f) {
      code = build_fail_code(f, who, what, n, units);
    }
    timing_flush();
    if (code != PGX_OK) return code;
    set.add(obj);
    *out = obj;
    return (int)PGX_OK;
  });
  if (rc != PGX_OK) delete obj;
  return rc;
}

// ---------------------------------------------------------------------------------------------------------
// resident read database
// ---------------------------------------------------------------------------------------------------------
struct ReadDesc {
  uint64_t off;
  uint32_t len;
  uint32_t rid;
};
// What the library keeps between the stages of the job running on one read database: each part is built on first use by the file
// that owns its type and released with the database (two live databases each hold their own).
struct CountCache;    // the aggregated count table (pgx_pairs.hip)
struct ReplayState;   // the device replay's learned table sizes, the tables it cleared ahead of time, its pinned mirrors and second stream (pgx_replay.hip)
struct ServedCache;   // device copies of the list / count files index commands wrote, the assembled lists of the last prefix (pgx_served.cpp)
struct CacheFree {    // (each operator() is defined in the file that owns the type)
  void operator()(CountCache *) const;
  void operator()(ReplayState *) const;
  void operator()(ServedCache *) const;
};
struct DbCaches {
  std::unique_ptr<CountCache, CacheFree> counts;
  std::unique_ptr<ReplayState, CacheFree> replay;
  std::unique_ptr<ServedCache, CacheFree> served;
};
template <typename T>
T &get_or_make(std::unique_ptr<T, CacheFree> &part) {   // the part, built on first use (where T is complete)
  if (!part) part.reset(new T);
  return *part;
}
}  // namespace pgx

struct pgx_seqdb {
  pgx::DevBuf<uint8_t> d_seq;      // seqdb bytes + 1 KiB of zero padding
  bool borrowed = false;           // d_seq.p belongs to the caller (pgx_seqdb_adopt_dev): never released here
  ~pgx_seqdb() {
    if (borrowed) d_seq.p = nullptr, d_seq.n = 0;
  }
  // the packed alignment kernel's view of the reads (pgx_pack.hip): a cache of the immutable seqdb bytes, built on first use
  mutable pgx::DevBuf<uint32_t> d_pack;          // 2-bit packs of the seqdb, both strands
  mutable pgx::DevBuf<uint32_t> d_nflag;         // by rid: the read holds a byte that has no 2-bit code (an ambiguous base)
  mutable pgx::DevBuf<uint64_t> d_poff;          // by rid: dword index of the read's forward strand in d_pack (its reverse complement follows)
  mutable pgx::DevBuf<uint32_t> d_prank;         // by rid: the read's rank in the packs' layout (the alignment launches take their requests in this order)
  mutable pgx::DevBuf<uint64_t> d_locus_key;     // by rid, only until the packs are built: smallest top-level shimmer hash (pgx_pack.hip)
  mutable bool locus_key_filled = false, locus_ordered = false;   // (ordered: the packs' reads are laid out by locus key, not in file order)
  mutable bool packs_built = false, packs_failed = false;   // (failed: no HBM for them -- the byte-wise kernels serve this database)
  mutable uint32_t n_flagged_reads = 0;                     // reads marked in d_nflag (known once the packs are built)
  // the side store of a COMPACTED database (pgx_side.hip, pgx_seqdb_compact_bytes): the bytes of the flagged reads only, kept when d_seq goes
  pgx::DevBuf<uint8_t> d_side;      // [16 zero bytes | a slot per flagged read, ascending rid | 1 KiB of zero padding]
  pgx::DevBuf<uint32_t> d_side_rid; // the flagged rids, ascending
  pgx::DevBuf<uint64_t> d_side_off; // byte offset in d_side of each one's first base (congruent mod 16 to its seqdb offset)
  pgx::DevBuf<uint64_t> d_roff;    // indexed by rid
  pgx::DevBuf<uint32_t> d_rlen;    // indexed by rid
  std::vector<uint32_t> rid, rlen; // idx-file order
  std::vector<uint64_t> roff;
  std::vector<uint32_t> rlen_by_rid;
  uint32_t max_rlen = 0;  // longest read (chooses the 16-bit V ring of the alignment kernel)
  std::vector<uint64_t> roff_by_rid;
  size_t nbytes = 0;
  uint64_t bases = 0;
  // the read selections of the last index calls (rid % total == mychunk % total, idx order), one per (total, chunk): the steps of a resident
  // pipeline cycle through the job's chunks, and rebuilding + re-uploading a selection of 775 k reads costs 9.5 ms of host time per stage
  // (76 ms of a full-size configs[3] step through round 4, when only the LAST selection was kept)
  struct IndexPlan {
    int total = -1, chunk = -1;
    uint64_t bases = 0, last_use = 0;
    std::vector<pgx::ReadDesc> reads;
    // the fused index path's device half (dev_index_fused): the selection's descriptors and slab offsets, uploaded once per plan
    pgx::DevBuf<pgx::ReadDesc> d_reads;
    pgx::DevBuf<uint64_t> d_slab_off;
    uint64_t slab_total = 0, plan_bases = 0;
    int plan_w = 0, plan_k = 0;
    uint64_t plan_div = 0;   // 0: the device half is not built
    bool plan_ok = false;
  };
  std::vector<IndexPlan> plans;   // at most 32, least recently used replaced
  mutable pgx::DbCaches caches;   // (built on first use, like the packs)
};

namespace pgx {

// A database over bytes that a stage of the library made in place (pgx_fasta.hip): `bytes` holds nbytes of seqdb and 1 KiB of room behind
// them, and becomes the database's d_seq -- the constructor pgx_seqdb_upload_dev and pgx_seqdb_adopt_dev end in, without their copy.  After
// a failure the block is released.
int seqdb_take_dev(DevBuf<uint8_t> &&bytes, size_t nbytes, const uint32_t *rid, const uint32_t *rlen, const uint64_t *roff, uint32_t nreads,
                   pgx_seqdb **out);

// ---------------------------------------------------------------------------------------------------------
// device stages (pgx_kernels.hip).  All take/return device pointers and run on ctx().stream.
// ---------------------------------------------------------------------------------------------------------
// L0 minimizers of the given reads (device array of ReadDesc, in output order). Returns device list.
void dev_sketch(const pgx_seqdb *db, const std::vector<ReadDesc> &reads, int w, int k, DevBuf<pgx_mm128> &out,
                size_t &n_out, uint32_t *n_literal, bool hpc = false);   // hpc: mm_sketch's is_hpc = 1 (pgx_sketch_hpc.hip)
// fused index path: k_sketch_blk, or k_sketch_wave -> per-read reduce x levels in LDS; redo passes for the reads they flag; ordered
// gather.  Returns false (and leaves the outputs untouched) when the chunk needs the general path (other w/k ...).
// plan: the database's selection of `reads`, whose descriptors and slab offsets stay on the device with it (nullptr: uploaded for this call only)
bool dev_index_fused(const pgx_seqdb *db, const std::vector<ReadDesc> &reads, int w, int k, int rs, int levels,
                     const pgx_mm128 **d_top, size_t *n_top, pgx_seqdb::IndexPlan *plan = nullptr, uint32_t *n_second = nullptr);   // n_second: reads sketched run by run (ambiguous bases)
// one mm_reduce level over a device list
void dev_reduce(const pgx_mm128 *d_in, size_t n, int rs, DevBuf<pgx_mm128> &out, size_t &n_out);
// multiplicity of x>>8, sorted by mer
void dev_count(const pgx_mm128 *d_in, size_t n, int kmer_bits, DevBuf<pgx_mm_count> &out, size_t &n_out);
// ---- the index stage's launchers and helpers, shared by pgx_kernels.hip, pgx_sketch_fast.hip and pgx_sketch_n.hip -----------------------
// bytes: the byte view of a compacted database that d_reads' offsets count from (nullptr: the seqdb)
bool sketch_wave_eligible(const ReadDesc &rd, int w, int k);
void launch_sketch_wave(const pgx_seqdb *db, const ReadDesc *d_reads, const uint32_t *d_list, uint32_t n_list, int w, int k,
                        pgx_mm128 *d_slab, const uint64_t *d_slab_off, uint32_t *d_counts, uint32_t *d_flags, const uint8_t *bytes = nullptr);
// the bases of one batch of launch_sketch_general / launch_sketch_hpc (a longer read is a batch of its own).  PGX_SKETCH_BATCH: a test
// hook that shrinks it so that small inputs take several batches.
inline uint64_t sketch_batch_bases() {
  const char *v = getenv("PGX_SKETCH_BATCH");
  const long long b = v ? atoll(v) : (long long)(256ull << 20);
  return (uint64_t)(b < 1 ? 1 : b);
}
void launch_sketch_general(const pgx_seqdb *db, const ReadDesc *d_reads, const std::vector<uint32_t> &lens, const uint32_t *d_list, int w,
                           int k, pgx_mm128 *d_slab, const uint64_t *d_slab_off, uint32_t *d_counts, uint32_t *d_flags,
                           const uint8_t *bytes = nullptr);
void launch_sketch_hpc(const pgx_seqdb *db, const ReadDesc *d_reads, const std::vector<uint32_t> &lens, const uint32_t *d_list, int w, int k,
                       pgx_mm128 *d_slab, const uint64_t *d_slab_off, int off_by_list, uint32_t *d_counts, uint32_t *d_flags,
                       uint32_t *d_need);
bool sketch_blk_supported(int w, int k, int rs, int levels);
void launch_sketch_blk(const pgx_seqdb *db, const ReadDesc *d_reads, uint32_t n, int rs, int levels, pgx_mm128 *d_slab,
                       const uint64_t *d_slab_off, uint32_t *d_counts, uint32_t *d_flags);
void launch_sketch_fused_list(const pgx_seqdb *db, const ReadDesc *d_reads, const uint32_t *d_list, uint32_t n_list, int rs, int levels,
                              pgx_mm128 *d_slab, const uint64_t *d_slab_off, uint32_t *d_counts, uint32_t *d_flags,
                              uint32_t *d_need = nullptr, int off_by_list = 0);
// the listed reads (slots of d_reads, ascending) cut into runs of unambiguous bases (pgx_sketch_n.hip): their level-0 lists packed in
// list order, nl0[nl0_off[i] .. nl0_off[i+1]); reduced `levels` times per read: top[nl0_off[i] .. + cnt[i])
void dev_sketch_nreads(const pgx_seqdb *db, const ReadDesc *d_reads, const uint32_t *d_list, uint32_t nn, int w, int k,
                       DevBuf<pgx_mm128> &nl0, DevBuf<uint64_t> &nl0_off, uint64_t *n_total);
void dev_reduce_nreads(const DevBuf<pgx_mm128> &nl0, const DevBuf<uint64_t> &nl0_off, uint32_t nn, uint64_t total, int rs, int levels,
                       DevBuf<pgx_mm128> &top, DevBuf<uint32_t> &cnt);
void dev_scatter_counts(uint32_t *d_counts_by_slot, const uint32_t *d_list, uint32_t nn, const uint64_t *d_off, const uint32_t *d_cnt);
void dev_mark_slots(uint32_t *d_by_slot, const uint32_t *d_list, uint32_t nn, uint32_t v);
// banded O(ND) confirmation of n candidate alignments (keys on device)
void dev_align(const pgx_seqdb *db, const pgx_align_key *d_keys, size_t n, int band, pgx_match *d_out,
               int tail_batch = 0);   // tail_batch: 1 = the second request batch of a stage, 2 = a later one (mostly hard candidates: pgx_align.hip)
// alignments whose target starts at byte t_off of read rid1 (k_align1t), a wavefront each, on the bytes seq + off[rid]
void dev_align2(const pgx_seqdb *db, const uint8_t *seq, const uint64_t *off, const pgx_align_key2 *d_keys, size_t n, int band, pgx_match *d_out);
void dev_align_prepare(const pgx_seqdb *db);   // the database's 2-bit packs, ahead of the first large launch (no-op once they exist)
// the 2-bit packs of a read database (pgx_pack.hip: read by read, [forward strand | reverse complement] at dword d_poff[rid]; d_nflag
// marks the reads with bytes that have no 2-bit code): built on first use, kept with the database; nullptr: no HBM
const uint32_t *seq_packs(const pgx_seqdb *db);
bool seq_packs_valid(const pgx_seqdb *db);
// the locus key of the reads, gathered by the overlap stage's join before the first seq_packs() (no-ops once the packs exist)
uint64_t *seq_locus_key_buffer(const pgx_seqdb *db);
void locus_key_add_mm(const pgx_seqdb *db, const pgx_mm128 *d_mm, size_t n);
void locus_key_add_records(const pgx_seqdb *db, const uint64_t *d_key0, const uint64_t *d_y0, size_t n);

// ---- a compacted database (pgx_side.hip): the whole-seqdb bytes are gone, the packs serve what they can, and the byte-wise kernels read a
// BYTE VIEW -- the side store (flagged reads, as in the file) plus a scratch region into which k_unpack_reads rebuilds the bytes of the
// unflagged reads a call needs (shmr_utils.c:44-51 backwards).  seq + off[rid] is the read's first base, at an address congruent mod 16 to its
// seqdb offset (the tile loads of the sketch kernels take the same path as on the seqdb); off[] counts from the side store and wraps modulo
// 2^64 into the scratch region.  Only the entries of the reads the view was built for are valid.  The view's scratch goes back to the block
// cache with it (stream-ordered: kernels enqueued before that still read it safely).
inline bool seq_compacted(const pgx_seqdb *db) { return db->d_seq.p == nullptr && db->d_side.p != nullptr; }
struct ByteView {
  const uint8_t *seq = nullptr;
  const uint64_t *off = nullptr;   // by rid
  DevBuf<uint8_t> scratch;
};
void side_build(pgx_seqdb *db);    // the side store from the bytes (which must be there, the packs built, every read <= 65,535 bases)
uint64_t side_store_bytes(const pgx_seqdb *db);
// the view for both reads of the candidates keys[list[0 .. n)], and for the reads of the slots d_reads[list[0 .. n)]
void side_view_of_keys(const pgx_seqdb *db, const pgx_align_key *d_keys, const uint32_t *d_list, uint32_t n, ByteView &v);
void side_view_of_reads(const pgx_seqdb *db, const ReadDesc *d_reads, const uint32_t *d_list, uint32_t n, ByteView &v);
// the view for the reads d_rids[0 .. n) names (duplicates allowed), also on a database whose bytes were RELEASED: all of them from the packs
void side_view_of_rids(const pgx_seqdb *db, const uint32_t *d_rids, uint32_t n, ByteView &v);
// tr[i] = d_reads[list[i]] with its offset in the view, iota[i] = i
void side_translate_reads(const ByteView &v, const ReadDesc *d_reads, const uint32_t *d_list, uint32_t n, ReadDesc *tr, uint32_t *iota);

// Large host arrays.  Never value-initialised (they are about to be overwritten); from 16 MiB up they are pooled anonymous
// mappings advised to use transparent huge pages, which the allocator would not do for us (THP is in "madvise" mode on
// the target hosts): first-touch faults and the final munmap are ~500x fewer than with 4 KiB pages.
void *big_alloc(size_t bytes);            // never returns nullptr (throws std::bad_alloc); content arbitrary
void big_free(void *p, size_t bytes);
void *big_alloc_zero(size_t bytes);       // all-zero mapping (fresh, or one that big_free_zero cleared)
void big_free_zero(void *p, size_t bytes);
void big_pool_trim();                     // unmap everything pooled (pgx_shutdown)
void *out_alloc(size_t bytes);            // an array for the caller (pgx_free): malloc, or a pooled mapping when large
void out_free(void *p);
template <typename T>
struct HostArray {
  T *p = nullptr;
  size_t n = 0;
  HostArray() = default;
  explicit HostArray(size_t count) { alloc(count); }
  HostArray(const HostArray &) = delete;
  HostArray &operator=(const HostArray &) = delete;
  HostArray(HostArray &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
  HostArray &operator=(HostArray &&o) noexcept {
    if (this != &o) {
      clear();
      p = o.p, n = o.n;
      o.p = nullptr, o.n = 0;
    }
    return *this;
  }
  ~HostArray() { clear(); }
  void alloc(size_t count) {
    clear();
    p = (T *)big_alloc((count ? count : 1) * sizeof(T));
    n = count;
  }
  void clear() {
    if (p) big_free(p, (n ? n : 1) * sizeof(T));
    p = nullptr, n = 0;
  }
  T *data() { return p; }
  const T *data() const { return p; }
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
  T &operator[](size_t i) { return p[i]; }
  const T &operator[](size_t i) const { return p[i]; }
  T *begin() { return p; }
  T *end() { return p + n; }
  const T *begin() const { return p; }
  const T *end() const { return p + n; }
  const T &back() const { return p[n - 1]; }
};

// shimmer-pair join (pgx_pairs.hip): records sorted by (key0, key1, position desc, insertion order) plus the bucket /
// key0-group tables the host needs to replay the khash slot order on distinct keys
struct PairTables {
  size_t n_rec = 0;
  size_t n_groups = 0, n_buckets = 0;   // (always set; the arrays below only when the tables came to the host: PAIRS_DEV_TABLES)
  bool on_host = true;
  HostArray<uint64_t> y0;        // per record
  HostArray<uint8_t> dir;        // per record
  HostArray<uint64_t> bkey1;     // per bucket
  HostArray<uint32_t> bstart;    // nb+1 record offsets
  HostArray<uint32_t> bfirst;    // first insertion (record seq) of the bucket
  HostArray<uint64_t> gkey0;     // per key0 group
  HostArray<uint32_t> gstart;    // ng+1 record offsets
  HostArray<uint32_t> gfirst, glast;  // first / last insertion of the group
  HostArray<uint32_t> gbucket;   // ng+1: first bucket of the group
  HostArray<uint32_t> gord;      // groups in order of first insertion
  HostArray<uint32_t> bord;      // buckets ordered by (group, first insertion): group g's slice is [gbucket[g], gbucket[g+1])
  // PAIRS_ORD_TABLES: what the inner-table replay reads, already IN bord ORDER (sequential on the host instead of three gathers
  // per bucket): second key and size of bucket bord[i]; per group: is a put repeated after its last first-insertion (khash.h:298-306)
  HostArray<uint64_t> bkey1_ord;
  HostArray<uint32_t> bn_ord;
  HostArray<uint8_t> gtrail;
  HostArray<uint64_t> y1;        // per record, only with PAIRS_Y1
  HostArray<uint64_t> umer;      // aggregated multiplicities, sorted by mer: only with PAIRS_COUNTS
  HostArray<uint32_t> ucnt;
};
struct PairParams {
  uint32_t total, mychunk, lower, upper;  // bucket ownership (x>>8) % total == mychunk % total; multiplicity bounds
  uint32_t n_rid = 0;                     // entries of d_rlen (0: unknown, the list is not checked against the read database)
};
enum : unsigned {
  PAIRS_Y1 = 1,               // also return the second coordinate of every record (mp128_t.y1)
  PAIRS_INSERTION_ORDER = 2,  // records of a bucket in insertion order instead of position-descending
  PAIRS_COUNTS = 4,           // also return the aggregated multiplicity table
  PAIRS_ORD_TABLES = 16,      // bkey1_ord / bn_ord / gtrail instead of bkey1 / bfirst (the overlap stage's table replay)
  PAIRS_LAZY_RECORDS = 8,     // with `keep`: leave the sorted records (y0, dir) on the device only; pairs_fetch_records downloads them
  PAIRS_DEV_TABLES = 32,      // with `keep` + PAIRS_ORD_TABLES: leave the group / bucket tables on the device only (the visit order is
                              // built there, pgx_visit.hip); pairs_fetch_tables downloads them for the host paths
};
// what the join leaves in HBM for the device replay (pgx_replay.hip): the bucket-sorted records
struct DevicePairs {
  DevBuf<uint64_t> y0;       // per record: rid << 32 | lastPos << 1 | strand
  DevBuf<uint8_t> dir;       // per record
  DevBuf<uint32_t> bstart;   // n_buckets + 1 record offsets
  size_t n_rec = 0, n_buckets = 0;
  bool valid = false;
  // PAIRS_DEV_TABLES: the tables of PairTables (same names, same contents), left where the join computed them
  bool tables = false;
  size_t n_groups = 0;
  DevBuf<uint32_t> gstart, gbucket;   // n_groups + 1 each (end sentinels)
  DevBuf<uint32_t> gord, gfirst, glast, bord, bn_ord;
  DevBuf<uint64_t> gkey0, bkey1_ord;
  DevBuf<uint8_t> gtrail;
  uint32_t max_group_buckets = 0;     // most buckets a first-key group holds
  uint32_t n_big_groups = 0;          // groups with more than VISIT_LANE_MAX buckets
  DevBuf<uint32_t> big_groups;        // their indices
  std::vector<uint64_t> key_sample;   // gkey0[gord[i * KEY_SAMPLE_STRIDE]]: what the early outer-table keys are checked against
  uint32_t last_gfirst = 0;           // gfirst[gord[n_groups - 1]]
};
constexpr uint32_t VISIT_LANE_MAX = 48;     // buckets of a group one lane replays (a 64-slot table: pgx_visit.hip)
constexpr uint32_t VISIT_WAVE_MAX = 3153;   // ... a wavefront (a 4,096-slot table); larger groups: the host replay of the tables
constexpr uint32_t KEY_SAMPLE_STRIDE = 997;
void pairs_fetch_tables(const DevicePairs &dp, PairTables &out);   // (no-op when the tables are on the host already)
// the visit order on the device (pgx_visit.hip): inner tables of every first-key group replayed by a lane / a wavefront each
// (enqueued; runs while the host finishes the outer table), then the groups' visited buckets placed in outer-slot order
struct DevVisit {
  DevBuf<uint32_t> ids_all, gnb;
  DevBuf<unsigned long long> tot;
};
void dev_visit_inner(const DevicePairs &dp, uint32_t ovlp_upper, DevVisit &v);
// slots: the outer table as DistinctSlotTable leaves it (pinned host memory), ids = positions in first-insertion order
void dev_visit_place(const DevicePairs &dp, DevVisit &v, const uint64_t *slots, uint32_t n_slots, DevBuf<uint32_t> &bid, size_t *n_buckets,
                     size_t *n_entries);
// The distinct first keys of the records in the order of their first insertion -- what the host replays klib's OUTER table from
// (pgx_overlap.cpp) -- computed right after the records exist (a hash aggregation of first occurrences + an ordered select) and
// handed to `early` while the join's sorts are still to run: the outer-table replay, the longest sequential piece of host work
// of the stage, then overlaps the rest of the join.  keys[i] == gkey0[gord[i]] of the tables the join returns.
struct EarlyGroups {
  HostArray<uint64_t> keys;
  uint32_t n = 0;
  uint32_t last_first = 0;   // record index of the last key's first occurrence
};
using EarlyFn = std::function<void(EarlyGroups &&)>;
// the shimmer list and the count entries of a join, both as host arrays or both as device arrays (used in place)
struct Lists {
  const pgx_mm128 *mm = nullptr;
  size_t n_mm = 0;
  const pgx_mm_count *mc = nullptr;
  size_t n_mc = 0;
  bool on_device = false;
};
// d_rlen: read length by rid, on the device
void dev_build_pairs(const uint32_t *d_rlen, const Lists &lists, const PairParams &pp, PairTables &out, unsigned flags = 0,
                     DevicePairs *keep = nullptr,   // keep: the sorted records stay on the device too
                     const EarlyFn &early = nullptr,
                     const pgx_seqdb *db = nullptr);   // db: keeps the count table for the job's next chunk, and its packs' locus keys are
                                                       // gathered from the lists on the way (pgx_pack.hip); nullptr: the table is built uncached
// ---- multi-GPU hand-over: counts all-gathered, pair records routed to their owner chunk -------------------------
// prepare: aggregate ALL chunks' counts, flag the kept shimmers of THIS index chunk's list (both on the device); returns the index
// of the first shimmer with lower <= count < upper (-1: none).  scatter: the records of every adjacent kept pair from `start` on
// (the list position the global scan starts at, shmr_utils.c:311-320), grouped by destination chunk 1..T in scan order; *d_send
// stays valid until the next prepare.  from_records: the join of one overlap chunk over the records it received, in arrival order
// (= source chunk order, then scan order: the insertion order of build_map over the concatenated lists).
int64_t dev_pairs_prepare(const pgx_seqdb *db, const pgx_mm128 *d_mm, size_t n_mm, const pgx_mm_count *d_counts, size_t n_counts,
                          uint32_t lower, uint32_t upper);
void dev_pairs_scatter(const uint32_t *d_rlen, uint32_t T, int64_t start, const pgx_pair_rec **d_send, uint64_t *counts);
void dev_pairs_from_records(const pgx_pair_rec *d_rec, size_t n, PairTables &out, DevicePairs *keep_dev, unsigned flags = 0,
                            const EarlyFn &early = nullptr, const pgx_seqdb *locus_db = nullptr);
void pairs_fetch_records(const DevicePairs &dp, PairTables &out);  // the lazily kept records, to the host tables

// The greedy walk over the visit list (visit_bids: the join's bucket ids in visit order) on the GPU; the records go to the
// array alloc_out(n) returns, or -- sink != nullptr -- from the device to the sink, right behind k_emit.  false: the job does not fit the device tables' encodings or they overflowed -- nothing was
// produced and the caller runs the host replay.
struct RecordSink;
void dev_place_bids(const uint32_t *ids_all, size_t n_ids, const uint32_t *psrc, const uint32_t *pcnt, const uint64_t *pdst,
                    size_t n_groups, size_t nb, DevBuf<uint32_t> &bid);   // the visit list assembled on the device
bool dev_replay(const pgx_seqdb *db, const DevicePairs &dp, const uint32_t *visit_bids, const uint32_t *d_bids, size_t nb, size_t n_entries,
                uint32_t bestn, int band, uint32_t ovlp_upper, const std::function<pgx_ovlp *(size_t)> &alloc_out, RecordSink *sink,
                size_t *n_out, pgx_overlap_stats *st, bool trace);

// what the index stage leaves in HBM for a following overlap stage of the same process (pgx_index_overlap_resident)
struct DeviceIndex {
  const pgx_mm128 *d_top = nullptr;  // lives in the index workspace: valid until the next index call
  size_t n_top = 0;
  DevBuf<pgx_mm_count> mc;
  size_t n_mc = 0;
  bool valid = false;
};
// the index stage; keep != nullptr: leave the final list + counts on the device too; host_arrays == false: do not download them
void index_stage(pgx_seqdb *db, const pgx_index_params *p, pgx_index_result *out, DeviceIndex *keep, bool host_arrays);

// Records on their way to the host while the caller already works on the next chunk (pgx_results_async, include/pgx.h): the overlap
// stage's device replay hands its record buffer to a copy on a second stream and returns; results_wait() -- called by
// pgx_results_wait, by the next stage before it allocates its own buffer, by pgx_free of that array and by every entry point that
// reads the records itself -- waits for the copy and gives the device buffer back.
bool &results_async();
void results_wait();
void results_wait_if(const void *host);   // only if `host` is the array the pending copy writes
void results_copy_async(pgx_ovlp *host, DevBuf<pgx_ovlp> &&dev, size_t n);   // after what is enqueued on ctx().stream

// ---- file-level entry points of the overlap stage (pgx_served.cpp) over the stage itself (pgx_overlap.cpp) -------------------------------
struct OvOut {  // the stage's output: one malloc'd array handed to the caller as is (a == nullptr, n set: the records went to a RecordSink)
  pgx_ovlp *a = nullptr;
  size_t n = 0;
  void alloc(size_t count) {
    out_free(a);
    a = (pgx_ovlp *)out_alloc(count ? count * sizeof(pgx_ovlp) : 1);
    n = count;
  }
  pgx_ovlp *release() {
    pgx_ovlp *p = a;
    a = nullptr, n = 0;
    return p;
  }
  ~OvOut() { out_free(a); }
};
// what a stage runs on: the lists (host or device arrays), or -- a rank of a multi-GPU job -- the pair records this chunk received from
// all index chunks (device pointer, arrival order = insertion order; may be empty)
struct StageInput {
  bool records = false;
  Lists lists;
  const pgx_pair_rec *d_recs = nullptr;
  size_t n_recs = 0;
  static StageInput host_lists(const pgx_mm128 *mm, size_t n_mm, const pgx_mm_count *mc, size_t n_mc) {
    return StageInput{false, Lists{mm, n_mm, mc, n_mc, false}, nullptr, 0};
  }
  static StageInput device_lists(const pgx_mm128 *d_mm, size_t n_mm, const pgx_mm_count *d_mc, size_t n_mc) {
    return StageInput{false, Lists{d_mm, n_mm, d_mc, n_mc, true}, nullptr, 0};
  }
  static StageInput pair_records(const pgx_pair_rec *d_recs, size_t n) { return StageInput{true, Lists{}, d_recs, n}; }
};
void overlap_check_params(const pgx_overlap_params *p);
// the stage: the records go to `out`, or -- sink != nullptr and the walk ran on the device -- to the sink (out.a == nullptr, out.n set)
void overlap_stage(pgx_seqdb *db, const StageInput &in, const pgx_overlap_params *p, OvOut &out, pgx_overlap_stats *st, RecordSink *sink = nullptr);
// Where a stage's records go when they are not wanted as a host array (served commands: straight to the output file).  The device replay hands
// its record buffer over right behind k_emit -- take() returns at once, the transfer runs on the sink's own threads and streams -- and
// allocates no host array; the host replay (small sets, fall-back) delivers a host array that the caller writes itself.
struct RecordSink {
  virtual void take(DevBuf<pgx_ovlp> &&dev, size_t n) = 0;   // ordered behind what is enqueued on ctx().stream; at most once per stage (the attempt's last overflow check has passed)
  virtual ~RecordSink() {}
};
// Served jobs: an index command leaves with the database a device copy of every final-level list / count file it wrote (keyed by the
// file's absolute path, size and mtime); the job's overlap commands assemble their input from those copies instead of reading the files
// back (pgx_served.cpp).  d_payload (device) or h_payload (host): the file's entries, without the 8-byte count header; call AFTER the file
// is closed.  A copy that cannot be made (no HBM, a HIP error) is skipped: the files are complete, the copies are only a cache.
void list_stash_put(const pgx_seqdb *db, const std::string &path, const void *d_payload, const void *h_payload, size_t bytes);
void replay_drop_precleared(const pgx_seqdb *db);
void replay_preclear(const pgx_seqdb *db);   // tables of the last stage's sizes, allocated and cleared ahead of the replay (while the GPU waits for the host's outer table)

// pgx_overlap_stats::stream_checksum: the sum over the records of a 64-bit mix of every field (padding bytes excluded) and the record's
// position in the stream -- the same on the device (k_emit adds it up while it writes the records) and on the host
__host__ __device__ inline uint64_t checksum_mix(uint64_t h) {
  h ^= h >> 33, h *= 0xff51afd7ed558ccdULL, h ^= h >> 33, h *= 0xc4ceb9fe1a85ec53ULL, h ^= h >> 33;
  return h;
}
__host__ __device__ inline uint64_t record_checksum(const pgx_ovlp &o, uint64_t pos) {
  uint64_t h = checksum_mix(o.y0 + 0x9E3779B97F4A7C15ULL * (pos + 1));
  h = checksum_mix(h ^ o.y1);
  h = checksum_mix(h ^ ((uint64_t)o.rl0 | (uint64_t)o.rl1 << 32));
  h = checksum_mix(h ^ ((uint64_t)o.strand0 | (uint64_t)o.strand1 << 8 | (uint64_t)o.ovlp_type << 16));
  h = checksum_mix(h ^ ((uint64_t)(uint32_t)o.match.m_size | (uint64_t)(uint32_t)o.match.dist << 32));
  h = checksum_mix(h ^ ((uint64_t)(uint32_t)o.match.q_bgn | (uint64_t)(uint32_t)o.match.q_end << 32));
  h = checksum_mix(h ^ ((uint64_t)(uint32_t)o.match.t_bgn | (uint64_t)(uint32_t)o.match.t_end << 32));
  h = checksum_mix(h ^ ((uint64_t)(uint32_t)o.match.t_m_end | (uint64_t)(uint32_t)o.match.q_m_end << 32));
  return h;
}

// Runs fn on the library's housekeeping thread: tearing down GB-sized host tables (munmap, free) takes tens of
// milliseconds that the caller does not have to wait for.  At most a few jobs are queued; beyond that fn runs inline.
void defer_destroy(std::function<void()> fn);
void drain_deferred();  // waits until every queued job has run (pgx_shutdown)

// the contig layout from rows, however they were made (pgx_contigs.hip): a tiling path file's, or a built tiling's
using TileRowFn = std::function<void(const std::string &ctg, int64_t rid0, int64_t rid1, int64_t s, int64_t e, uint8_t strand0, uint8_t strand1, uint64_t line)>;
using TileRowFeed = std::function<void(const TileRowFn &add)>;
int contigs_from_rows(const char *who, const char *seqdb_prefix, const TileRowFeed &feed, const char *out_path, uint64_t *n_ctg, uint64_t *n_bases);
// ... up to the FASTA: the batches' contig bytes, kept until every batch is through (an error in a later batch must leave nothing
// written).  Batch b holds the contigs ctg0 .. ctg0 + off.size() - 2, contig ctg0 + c at text[off[c] .. off[c + 1]); names: the contigs'
// in order of first appearance.
struct ContigPieces {
  struct Piece {
    char *text = nullptr;   // out_alloc'd
    std::vector<uint64_t> off;
    size_t ctg0 = 0;
  };
  std::vector<Piece> pieces;
  std::vector<std::string> names;
  uint64_t bases = 0;
  ContigPieces() = default;
  ContigPieces(const ContigPieces &) = delete;
  ContigPieces &operator=(const ContigPieces &) = delete;
  ~ContigPieces();
};
void contig_pieces_from_rows(const char *who, const char *seqdb_prefix, const TileRowFeed &feed, ContigPieces &out);   // throws
// ... over a resident database in any state: pgx_contigs_resident's body (rows: s, e as the tiling path gives them, transformed in place;
// *text out_alloc'd, NUL-terminated; ctg_off: n_ctg + 1 entries).  Throws; the Fail of a refused row carries the row's index (Fail::piece).
void contigs_resident_rows(const char *who, pgx_seqdb *db, std::vector<pgx_tile_row> &rows, size_t n_ctg, char **text, uint64_t *ctg_off, uint64_t *text_len);

// host helpers (pgx_api.cpp)
int load_idx(const char *path, std::vector<uint32_t> &rid, std::vector<uint32_t> &rlen, std::vector<uint64_t> &roff);
bool read_file(const std::string &path, std::vector<uint8_t> &out);
template <typename T>
T *host_copy(const std::vector<T> &v) {
  T *p = (T *)malloc(v.size() ? v.size() * sizeof(T) : 1);
  if (v.size()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}
// The consensus call on rows and strings in device memory (pgx_cns.hip; include/pgx.h: pgx_cns_call_dev; piece_tlen and the results are the
// host's).  names: where the pieces are a selection of the caller's, the caller's number of each, which the refusals then name (or nullptr).
// d_text_out and d_off_out both given: the text and its n_piece + 1 offsets stay on the device instead (text, piece_off are not written).
void cns_call_dev(const char *who, const pgx_cns_aln *d_alns, size_t n_aln, const uint8_t *d_q, const uint8_t *d_t, size_t str_bytes, const uint32_t *piece_tlen,
                  size_t n_piece, uint32_t min_cov, char **text, uint64_t *piece_off, pgx_cns_stats *stats, const uint32_t *names, DevBuf<char> *d_text_out = nullptr,
                  DevBuf<uint64_t> *d_off_out = nullptr);
// falcon.align for n > 0 checked requests in device memory over a device pool with 16 bytes of padding behind it (pgx_cns_align.hip): the
// answers, without strings unless a request wants them.  max_band: the widest band among them.
struct FalnOut {
  DevBuf<pgx_faln_res> res;
  DevBuf<uint8_t> q_str, t_str;
  uint64_t str_bytes = 0;
};
void faln_dev(const char *who, const pgx_faln_req *d_reqs, size_t n, const uint8_t *d_seq, uint32_t max_band, FalnOut &out, pgx_faln_stats *stats);
// pgx_cns_pieces on pieces, reads and a pool that are on the device already (the pool with 16 bytes of padding behind its seq_bytes): the
// pieces' text stays there, piece p at text[off[p], off[p + 1]).  name_base: the caller's number of piece 0 (the refusals name name_base + p).
struct CnsPiecesDev {
  DevBuf<char> text;       // 16 bytes of room behind the last piece
  DevBuf<uint64_t> off;    // n_piece + 1
  DevBuf<uint8_t> used;    // per read: accepted
  uint64_t total = 0;
};
void cns_pieces_dev(const char *who, const pgx_cns_piece *d_pieces, uint32_t n_piece, const pgx_cns_read *d_reads, uint32_t n_read, const uint8_t *d_seq,
                    uint64_t seq_bytes, uint32_t min_cov, CnsPiecesDev &out, pgx_cns_pieces_stats *stats, uint32_t name_base);
// the line select of the device parsers of map text (pgx_cns_job.hip): flag[i] = text[i] is a newline
__global__ void k_par_newlines(const char *text, uint32_t n, uint8_t *flag);
// the merge of shmr_map's rows (pgx_mapmerge.hip): n > 0 rows (9 x u32, device) in the order of `LC_ALL=C sort -k 1 -g -k 2 -g` over their
// lines to d_out (not d_rows); the times are added to *ms
void map_merge_dev(const uint32_t *d_rows, uint32_t n, uint32_t *d_out, pgx_map_merge_stats *ms);
// n bytes of text as a NUL-terminated string of the caller's (pgx_free); src == nullptr: room for n bytes, still to be filled
inline char *caller_text(const char *src, size_t n) {
  char *t = (char *)malloc(n + 1);
  if (!t) throw std::bad_alloc();
  if (src && n) memcpy(t, src, n);
  t[n] = 0;
  return t;
}
}  // namespace pgx
