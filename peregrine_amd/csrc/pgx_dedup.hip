// pgx_dedup.hip -- SURVEY.md 8(f) row f2: what /root/reference/src/shmr_dedup.c:32-101 does (cat ovlp*.dat | shmr_dedup):
// the first record of every read pair wins, its coordinates are mapped to FALCON's preads.ovl text line.
// GPU: first-wins flags by a stable radix sort of (pair, stream index) + the coordinate transform of the kept records;
// host: text formatting only ("%09d %09d %d %0.1f %u %d %d %u %u %d %d %u %s\n", shmr_dedup.c:91-99).
// Note: on an EMPTY stream the reference formats one record from uninitialised stack memory (its while(!feof) loop runs
// once); this implementation writes nothing.
//
// The STREAMING form (pgx_dedup_open / _feed / _feed_dev / _close) takes the job's records piece by piece in bounded memory: the
// in-batch first-wins above makes a piece's pair keys distinct, a seen-pair set that lives in HBM for the stream's life (open
// addressing, one 64-bit word per slot) says which of them are new, and the text lines are written on the device too (k_line_len ->
// exclusive scan -> k_format) and leave through a pinned staging buffer.

#include "pgx_dedup_rows.h"

namespace pgx {
namespace {

__global__ void k_pair_keys(const pgx_ovlp *__restrict__ in, uint32_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ idx) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t r0 = (uint32_t)(in[i].y0 >> 32), r1 = (uint32_t)(in[i].y1 >> 32);
  key[i] = r0 < r1 ? ((uint64_t)r0 << 32 | r1) : ((uint64_t)r1 << 32 | r0);
  idx[i] = i;
}
__global__ void k_first_flags(const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sidx, uint32_t n,
                              uint8_t *__restrict__ keep) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  keep[sidx[i]] = (i == 0) || skey[i] != skey[i - 1];  // stable sort: the first of a run is the earliest in the stream
}
// coordinate transform of shmr_dedup.c:44-89 (unsigned 32-bit arithmetic exactly as written there)
__global__ void k_rows(const pgx_ovlp *__restrict__ in, const uint32_t *__restrict__ sel, uint32_t m, Row *__restrict__ out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const pgx_ovlp o = in[sel[j]];
  const uint32_t pos0 = (uint32_t)((o.y0 & 0xFFFFFFFFu) >> 1) + 1, pos1 = (uint32_t)((o.y1 & 0xFFFFFFFFu) >> 1) + 1;
  const uint32_t rlen0 = o.rl0, rlen1 = o.rl1;
  int32_t q_bgn = o.match.q_bgn, q_end = o.match.q_end, t_bgn = o.match.t_bgn, t_end = o.match.t_end;
  q_bgn -= t_bgn;
  t_bgn = 0;
  uint32_t a_bgn, a_end, b_bgn, b_end;
  if (o.strand0 == 0) {
    a_bgn = (uint32_t)((int32_t)(pos0 - pos1) + q_bgn);
    a_end = (uint32_t)((int32_t)(pos0 - pos1) + q_end);
  } else {
    a_bgn = (uint32_t)((int32_t)rlen0 - (int32_t)(pos0 - pos1) - q_end);
    a_end = (uint32_t)((int32_t)rlen0 - (int32_t)(pos0 - pos1) - q_bgn);
  }
  a_end = a_end >= rlen0 ? rlen0 : a_end;  // the "< 0" fixes of the reference are no-ops on unsigned values
  if (o.strand1 == 0) {
    b_bgn = (uint32_t)t_bgn;
    b_end = (uint32_t)t_end;
  } else {
    b_bgn = (uint32_t)((int32_t)rlen1 - t_end);
    b_end = (uint32_t)((int32_t)rlen1 - t_bgn);
  }
  b_end = b_end >= rlen1 ? rlen1 : b_end;
  Row r;
  r.rid0 = (uint32_t)(o.y0 >> 32), r.rid1 = (uint32_t)(o.y1 >> 32);
  r.m_size = o.match.m_size, r.dist = o.match.dist;
  r.a_bgn = a_bgn, r.a_end = a_end, r.rlen0 = rlen0;
  r.strand = o.strand0 == 0 ? o.strand1 : 1u - o.strand1;
  r.b_bgn = b_bgn, r.b_end = b_end, r.rlen1 = rlen1, r.type = o.ovlp_type;
  out[j] = r;
}

// ---------------------------------------------------------------------------------------------------------
// streaming form: the seen-pair set
// ---------------------------------------------------------------------------------------------------------
// One 64-bit word per slot: pair key + 1, 0 = empty; `mask + 1` slots, linear probing from a 64-bit mix of the key, load <= 1/2 (the
// host grows the table BEFORE a feed could pass it, so a probe always ends at an empty slot).  The one key whose word would be 0 --
// both read ids 2^32 - 1 -- has a word of its own behind the table (tab[mask + 1]).
// Returns true when the key was absent (and is now present).  A feed's candidates are distinct, so no two lanes ever race for one key
// and the answer does not depend on scheduling; they only race for SLOTS, which the compare-and-swap settles.
__device__ inline bool seen_claim(unsigned long long *__restrict__ tab, uint64_t mask, uint64_t key) {
  if (key == ~0ULL) return atomicExch(&tab[mask + 1], 1ULL) == 0;
  const unsigned long long want = key + 1;
  uint64_t s = checksum_mix(key) & mask;
  for (;;) {
    unsigned long long old = __atomic_load_n(&tab[s], __ATOMIC_RELAXED);
    if (old == 0) old = atomicCAS(&tab[s], 0ULL, want);
    if (old == 0) return true;
    if (old == want) return false;
    s = (s + 1) & mask;
  }
}
// read-only probe: is the key in the set (no feed inserts while this runs)
__device__ inline bool seen_has(const unsigned long long *__restrict__ tab, uint64_t mask, uint64_t key) {
  if (key == ~0ULL) return tab[mask + 1] != 0;
  const unsigned long long want = key + 1;
  for (uint64_t s = checksum_mix(key) & mask;; s = (s + 1) & mask) {
    const unsigned long long v = tab[s];
    if (v == want) return true;
    if (v == 0) return false;
  }
}
// heads of the runs of equal keys in the sorted batch (stable sort: the head is the pair's earliest record of the batch) that the set
// does not hold yet, and how many: EXACTLY the entries this feed adds, so the host grows the table only when it must
__global__ void k_run_heads(const uint64_t *__restrict__ skey, uint32_t n, const unsigned long long *__restrict__ tab, uint64_t mask,
                            uint8_t *__restrict__ head, uint32_t *__restrict__ n_new) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool h = i < n && (i == 0 || skey[i] != skey[i - 1]) && !seen_has(tab, mask, skey[i]);
  if (i < n) head[i] = h;
  const uint64_t b = __ballot(h);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(n_new, (uint32_t)__popcll(b));
}
// keep = run head AND the pair was not seen in an earlier feed (head[] already says so; the claim is what enters the key)
__global__ void k_seen_insert(const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sidx, const uint8_t *__restrict__ head,
                              uint32_t n, unsigned long long *__restrict__ tab, uint64_t mask, uint8_t *__restrict__ keep) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  keep[sidx[i]] = head[i] && seen_claim(tab, mask, skey[i]);
}
// every entry of the old table into the new (cleared) one
__global__ void k_seen_rehash(const unsigned long long *__restrict__ old_tab, uint64_t old_cap, unsigned long long *__restrict__ tab,
                              uint64_t mask) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > old_cap) return;
  const unsigned long long v = old_tab[i];
  if (i == old_cap) {
    tab[mask + 1] = v;
    return;
  }
  if (v) seen_claim(tab, mask, v - 1);
}

// ---------------------------------------------------------------------------------------------------------
// streaming form: the text lines, "%09d %09d %d %0.1f %u %d %d %u %u %d %d %u %s\n" as glibc prints them
// ---------------------------------------------------------------------------------------------------------
constexpr uint32_t FMT_MAXLINE = 148;  // longest line: 11 + 11 + 11 + 15 + 1 + 11 + 11 + 10 + 10 + 11 + 11 + 10 + 9 + 12 blanks + '\n' = 145
template <bool WRITE>
__device__ inline uint32_t format_row(const Row &r, char *dst) {  // m_size != 0
  LineOut<WRITE> o{dst, 0};
  o.rid((int32_t)r.rid0), o.ch(' ');
  o.rid((int32_t)r.rid1), o.ch(' ');
  o.i32((int32_t)(0u - (uint32_t)r.m_size)), o.ch(' ');
  o.f1(err_est_of(r.dist, r.m_size)), o.ch(' ');
  o.ch('0'), o.ch(' ');
  o.i32((int32_t)r.a_bgn), o.ch(' ');
  o.i32((int32_t)r.a_end), o.ch(' ');
  o.u32(r.rlen0), o.ch(' ');
  o.u32(r.strand), o.ch(' ');
  o.i32((int32_t)r.b_bgn), o.ch(' ');
  o.i32((int32_t)r.b_end), o.ch(' ');
  o.u32(r.rlen1), o.ch(' ');
  o.ch(r.type == 0 ? 'o' : 'c'), o.ch(r.type == 0 ? 'v' : 'o'), o.ch(r.type == 0 ? 'e' : 'n'), o.ch(r.type == 0 ? 'r' : 't');   // overlap / contains / contained
  o.ch(r.type == 0 ? 'l' : 'a'), o.ch(r.type == 0 ? 'a' : 'i'), o.ch(r.type == 0 ? 'p' : 'n');
  if (r.type != 0) o.ch(r.type == 1 ? 's' : 'e');
  if (r.type > 1) o.ch('d');
  o.ch('\n');
  return o.n;
}
// len[j] = bytes of row j's line, len[m] = 0 (so that the exclusive scan's last entry is the total).  Rows with m_size == 0 get no
// bytes here: their quotient is infinite or NaN, whose printed sign is the host FPU's -- the host formats and splices those in.
__global__ void k_line_len(const Row *__restrict__ rows, uint32_t m, uint64_t *__restrict__ len, uint32_t *__restrict__ n_special) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j > m) return;
  uint32_t l = 0;
  if (j < m) {
    const Row r = rows[j];
    if (r.m_size != 0) l = format_row<false>(r, nullptr);
    else atomicAdd(n_special, 1u);
  }
  len[j] = l;
}
// A workgroup formats a tile of rows into LDS at the offsets the scan gives (a lane per row), then streams the tile out (tile_out: the
// tile sits in LDS at the global address's offset within 16 bytes).
constexpr uint32_t FMT_TILE = 256;
__global__ __launch_bounds__(FMT_TILE) void k_format(const Row *__restrict__ rows, const uint64_t *__restrict__ off, uint32_t m,
                                                     char *__restrict__ text) {
  __shared__ __attribute__((aligned(16))) char tile[FMT_TILE * FMT_MAXLINE + 16];
  const uint32_t j0 = blockIdx.x * FMT_TILE, j = j0 + threadIdx.x, j1 = min(m, j0 + FMT_TILE);
  const uint64_t base = off[j0], end = off[j1];
  const uint32_t pad = (uint32_t)((uintptr_t)(text + base) & 15u);
  if (j < m) {
    const Row r = rows[j];
    if (r.m_size != 0) format_row<true>(r, tile + pad + (uint32_t)(off[j] - base));
  }
  __syncthreads();
  tile_out<FMT_TILE>(tile, text + base - pad, pad, pad + (uint32_t)(end - base));
}

// ---------------------------------------------------------------------------------------------------------
// graph mode: the reads the string graph's loader would call contained, and the lines it would keep
// ---------------------------------------------------------------------------------------------------------
// the read a printed line marks (ovlp_to_graph.py:683-698): none for a self pair or an `overlap` line, rid1 for `contains`, rid0 for
// `contained` -- every other type value, as the formatter prints it
__device__ inline bool row_marks(const Row &r, uint32_t *rid) {
  if (r.rid0 == r.rid1 || r.type == 0) return false;
  *rid = r.type == 1 ? r.rid1 : r.rid0;
  return true;
}
// one bit per read id; ids beyond the bitmap are unmarked (it is sized by the largest id that WAS marked)
__device__ inline bool bit_marked(const uint32_t *__restrict__ bits, uint32_t n_words, uint32_t rid) {
  const uint32_t w = rid >> 5;
  return w < n_words && ((bits[w] >> (rid & 31u)) & 1u);
}
__device__ inline bool row_kept(const Row &r, const uint32_t *__restrict__ bits, uint32_t n_words) {
  return r.type == 0 && r.rid0 != r.rid1 && !bit_marked(bits, n_words, r.rid0) && !bit_marked(bits, n_words, r.rid1);
}
// out[0] += rows that mark a read, out[1] = max(out[1], the largest id they mark): a wavefront reduces first, one atomic pair per wavefront
__global__ void k_mark_extent(const Row *__restrict__ rows, uint32_t m, uint32_t *__restrict__ out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t rid = 0;
  const bool mk = j < m && row_marks(rows[j], &rid);
  uint32_t v = mk ? rid : 0u;
  for (int d = 32; d; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
  const uint64_t b = __ballot(mk);
  if ((threadIdx.x & 63) == 0 && b) {
    atomicAdd(&out[0], (uint32_t)__popcll(b));
    atomicMax(&out[1], v);
  }
}
__global__ void k_mark(const Row *__restrict__ rows, uint32_t m, uint32_t *__restrict__ bits, uint32_t n_words) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t rid;
  if (j >= m || !row_marks(rows[j], &rid)) return;
  const uint32_t w = rid >> 5;
  if (w < n_words) atomicOr(&bits[w], 1u << (rid & 31u));   // (the host sized the bitmap for this feed's largest id before the launch)
}
__global__ void k_kept_flags(const Row *__restrict__ rows, uint32_t m, const uint32_t *__restrict__ bits, uint32_t n_words,
                             uint8_t *__restrict__ flag) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < m) flag[j] = row_kept(rows[j], bits, n_words);
}
__global__ void k_gather_rows(const Row *__restrict__ rows, const uint32_t *__restrict__ sel, uint32_t m, Row *__restrict__ out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < m) out[j] = rows[sel[j]];
}
__global__ void k_count_bits(const uint32_t *__restrict__ bits, uint32_t n_words, unsigned long long *__restrict__ total) {
  uint32_t c = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += gridDim.x * blockDim.x) c += (uint32_t)__popc(bits[i]);
  for (int d = 32; d; d >>= 1) c += (uint32_t)__shfl_xor((int)c, d);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(total, (unsigned long long)c);
}

// one line on the host (what pgx_dedup prints, PGX_DEDUP_HOST_TEXT=1, and the rows with m_size == 0)
static int host_line(const Row &r, char *line, size_t cap) {
  const double err_est = 100.0 - 100.0 * (double)r.dist / (double)r.m_size;
  return snprintf(line, cap, "%09d %09d %d %0.1f %u %d %d %u %u %d %d %u %s\n", (int)r.rid0, (int)r.rid1, -r.m_size, err_est, 0u,
                  (int)r.a_bgn, (int)r.a_end, r.rlen0, r.strand, (int)r.b_bgn, (int)r.b_end, r.rlen1,
                  r.type == 0 ? "overlap" : (r.type == 1 ? "contains" : "contained"));
}
}  // namespace
}  // namespace pgx

using namespace pgx;

// ---------------------------------------------------------------------------------------------------------
// the streaming entry points
// ---------------------------------------------------------------------------------------------------------
namespace pgx {
namespace {
constexpr uint64_t SEEN_MIN_CAP = 1ULL << 16;
LiveSet<pgx_dedup_stream> g_streams;   // the open ones
ShutdownHook g_streams_hook([] { g_streams.shutdown(); });

void seen_alloc(DevBuf<unsigned long long> &tab, uint64_t cap) {
  MemTag tag("dedup");
  try {
    tab.alloc(cap + 1);
  } catch (const Fail &) {
    (void)hipGetLastError();
    set_error("pgx_dedup: no device memory for a pair set of %llu slots", (unsigned long long)cap);
    throw Fail{PGX_ENOMEM};
  }
  PGX_HIP(hipMemsetAsync(tab.p, 0, (cap + 1) * sizeof(unsigned long long), ctx().stream));
}
// room for `more` new pairs at load <= 1/2
void seen_reserve(pgx_dedup_stream *s, uint64_t more) {
  uint64_t cap = s->cap;
  while ((s->n_unique + more) * 2 > cap) cap *= 2;
  if (cap == s->cap) return;
  DevBuf<unsigned long long> bigger;
  seen_alloc(bigger, cap);
  hipLaunchKernelGGL(k_seen_rehash, dim3(cdiv(s->cap + 1, 256)), dim3(256), 0, ctx().stream, s->tab.p, s->cap, bigger.p, cap - 1);
  PGX_HIP(hipGetLastError());
  s->tab = std::move(bigger);   // (the old table goes back to the block cache: one stream, so its next user comes after the rehash)
  s->cap = cap;
}

// The text the device wrote for m rows: `total` bytes, row j's line at off[j] -- none for the n_special rows with m_size == 0
struct DeviceLines {
  pgx_dedup_stream *s;
  const uint64_t *d_off;
  const char *d_text;
  uint64_t total;
  uint32_t n_special;
};
// The lines of m rows (m > 0) as the host's snprintf prints them; dev != nullptr: only those of the rows with m_size == 0, spliced into the
// device's text at their place.
std::string rows_to_host_text(const Row *d_rows, size_t m, const DeviceLines *dev = nullptr) {
  hipStream_t st = ctx().stream;
  std::vector<Row> rows(m);
  std::vector<uint64_t> off(dev ? m + 1 : 0);
  std::vector<char> dev_text(dev ? dev->total : 0);
  PGX_HIP(hipMemcpyAsync(rows.data(), d_rows, m * sizeof(Row), hipMemcpyDeviceToHost, st));
  if (dev) {
    PGX_HIP(hipMemcpyAsync(off.data(), dev->d_off, (m + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    text_download(dev->s->stage, dev->d_text, dev->total, dev_text.data());
  }
  pgx::sync();
  std::string out;
  out.reserve(dev ? dev->total + (size_t)dev->n_special * 64 : m * 96);
  char line[256];
  uint64_t done = 0;   // bytes of the device's text taken so far
  for (size_t j = 0; j < m; ++j) {
    if (dev && rows[j].m_size != 0) continue;
    if (dev) out.append(dev_text.data() + done, off[j] - done), done = off[j];
    out.append(line, (size_t)host_line(rows[j], line, sizeof(line)));
  }
  if (dev && dev->total > done) out.append(dev_text.data() + done, dev->total - done);
  return out;
}

// the text of m rows on the device (m > 0; d_m[1] is zero: it counts the rows the host formats)
void rows_to_text(pgx_dedup_stream *s, const Row *d_rows, uint32_t m, uint32_t *d_m, char **text, size_t *text_len) {
  static const bool host_text = getenv("PGX_DEDUP_HOST_TEXT") && atoi(getenv("PGX_DEDUP_HOST_TEXT")) != 0;   // diagnostic (=1): the lines by snprintf on the host
  hipStream_t st = ctx().stream;
  if (host_text) {
    const std::string out = rows_to_host_text(d_rows, m);
    *text = caller_text(out.data(), out.size()), *text_len = out.size();
    return;
  }
  uint64_t *d_off = ws<uint64_t>("dd.off", (size_t)m + 1);
  {
    uint64_t *d_len = ws<uint64_t>("dd.len", (size_t)m + 1);
    hipLaunchKernelGGL(k_line_len, dim3(cdiv((size_t)m + 1, 256)), dim3(256), 0, st, d_rows, m, d_len, d_m + 1);
    exclusive_sum(d_len, d_off, (size_t)m + 1);
  }
  uint64_t total = 0;
  uint32_t n_special = 0;
  PGX_HIP(hipMemcpyAsync(&total, d_off + m, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  PGX_HIP(hipMemcpyAsync(&n_special, d_m + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  pgx::sync();
  char *d_text = ws<char>("dd.text", total);
  hipLaunchKernelGGL(k_format, dim3(cdiv(m, FMT_TILE)), dim3(FMT_TILE), 0, st, d_rows, d_off, m, d_text);
  PGX_HIP(hipGetLastError());
  if (n_special == 0) return text_hand_out(s->stage, d_text, total, text, text_len);
  // rows with m_size == 0 (no real overlap record has one): the host's snprintf prints them, spliced in at their place
  const DeviceLines dev{s, d_off, d_text, total, n_special};
  const std::string out = rows_to_host_text(d_rows, m, &dev);
  *text = caller_text(out.data(), out.size()), *text_len = out.size();
}

// ---- graph mode -----------------------------------------------------------------------------------------------------------------------
constexpr uint64_t BITS_MIN_WORDS = 2;   // doubled up to the word of the largest marked id: 2^27 words = 512 MiB at most
constexpr uint64_t STORE_MIN_ROWS = 1ULL << 16;
constexpr uint32_t COMPACT_ROWS = 1u << 22;    // rows per piece of the final compaction (its scratch: 192 MiB)

template <typename T>
void graph_alloc(DevBuf<T> &buf, uint64_t count, const char *what) {
  MemTag tag("dedup");
  try {
    buf.alloc(count);
  } catch (const Fail &) {
    (void)hipGetLastError();
    set_error("pgx_dedup: no device memory for %s of %llu bytes", what, (unsigned long long)(count * sizeof(T)));
    throw Fail{PGX_ENOMEM};
  }
}
// the bitmap covers read id max_rid
void bits_reserve(pgx_dedup_stream *s, uint32_t max_rid) {
  uint64_t words = s->bits.n ? s->bits.n : BITS_MIN_WORDS;
  while (words * 32 <= (uint64_t)max_rid) words *= 2;
  if (words == s->bits.n) return;
  DevBuf<uint32_t> bigger;
  graph_alloc(bigger, words, "a read bitmap");
  hipStream_t st = ctx().stream;
  if (s->bits.n) PGX_HIP(hipMemcpyAsync(bigger.p, s->bits.p, s->bits.n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  PGX_HIP(hipMemsetAsync(bigger.p + s->bits.n, 0, (words - s->bits.n) * sizeof(uint32_t), st));
  s->bits = std::move(bigger);   // (one stream: the old words' next user comes after the copy)
}
// room for `more` rows behind the store's store_n
void store_reserve(pgx_dedup_stream *s, uint64_t more) {
  uint64_t cap = s->store.n ? s->store.n : STORE_MIN_ROWS;
  while (s->store_n + more > cap) cap *= 2;
  if (cap == s->store.n) return;
  DevBuf<Row> bigger;
  graph_alloc(bigger, cap, "a row store");
  if (s->store_n) PGX_HIP(hipMemcpyAsync(bigger.p, s->store.p, s->store_n * sizeof(Row), hipMemcpyDeviceToDevice, ctx().stream));
  s->store = std::move(bigger);
}
// sel[0 .. returned) = the j < m, ascending, whose row the graph's loader would keep under the bitmap as it is now
uint32_t select_kept(pgx_dedup_stream *s, const Row *d_rows, uint32_t m, uint32_t *sel) {
  hipStream_t st = ctx().stream;
  uint8_t *flag = ws<uint8_t>("dd.gflag", m);
  hipLaunchKernelGGL(k_kept_flags, dim3(cdiv(m, 256)), dim3(256), 0, st, d_rows, m, s->bits.p, (uint32_t)s->bits.n, flag);
  return select_indices(flag, m, sel);
}
// a feed's winner rows: their marks into the bitmap, then the rows that may still become lines behind the store.  A row whose read is
// marked ALREADY is dropped here, which only bounds the store: a mark that arrives later is seen by the final pass (graph_compact).
void graph_take(pgx_dedup_stream *s, const Row *d_rows, uint32_t m) {
  hipStream_t st = ctx().stream;
  uint32_t *d_g = ws<uint32_t>("dd.g", 2);   // [0]: rows that mark, [1]: the largest id they mark
  PGX_HIP(hipMemsetAsync(d_g, 0, 2 * sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_mark_extent, dim3(cdiv(m, 256)), dim3(256), 0, st, d_rows, m, d_g);
  uint32_t ext[2] = {0, 0};
  PGX_HIP(hipMemcpyAsync(ext, d_g, sizeof(ext), hipMemcpyDeviceToHost, st));
  pgx::sync();
  if (ext[0]) {
    bits_reserve(s, ext[1]);
    hipLaunchKernelGGL(k_mark, dim3(cdiv(m, 256)), dim3(256), 0, st, d_rows, m, s->bits.p, (uint32_t)s->bits.n);
  }
  uint32_t *sel = ws<uint32_t>("dd.gsel", m);
  const uint32_t k = select_kept(s, d_rows, m, sel);
  if (k == 0) return;
  store_reserve(s, k);
  hipLaunchKernelGGL(k_gather_rows, dim3(cdiv(k, 256)), dim3(256), 0, st, d_rows, sel, k, s->store.p + s->store_n);
  PGX_HIP(hipGetLastError());
  s->store_n += k;
}
uint64_t graph_count_marked(pgx_dedup_stream *s) {
  if (!s->bits.n) return 0;
  hipStream_t st = ctx().stream;
  unsigned long long *d_total = ws<unsigned long long>("dd.gtotal", 1), total = 0;
  PGX_HIP(hipMemsetAsync(d_total, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_count_bits, dim3(std::min<unsigned>(cdiv(s->bits.n, 256), 4096)), dim3(256), 0, st, s->bits.p, (uint32_t)s->bits.n, d_total);
  PGX_HIP(hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, st));
  pgx::sync();
  return total;
}

// The first record of every read pair of d_in[0 .. n) (n > 0) as rows, in stream order ("dd.rows"; returns how many): pair keys, stable
// sort, heads of the runs of equal keys, select, coordinate transform.  s != nullptr: only the pairs its seen-pair set does not hold yet,
// which enter it (d_new: a zero on the device, counts them) and are counted in its statistics; without a set the run heads alone decide.
uint32_t first_wins_rows(const pgx_ovlp *d_in, size_t n, pgx_dedup_stream *s, uint32_t *d_new, Row **d_rows) {
  hipStream_t st = ctx().stream;
  uint64_t *key = ws<uint64_t>("dd.key", n), *skey = ws<uint64_t>("dd.skey", n);
  uint32_t *idx = ws<uint32_t>("dd.idx", n), *sidx = ws<uint32_t>("dd.sidx", n), *sel = ws<uint32_t>("dd.sel", n);
  uint8_t *keep = ws<uint8_t>("dd.keep", n);
  PrimWs tmp;
  hipLaunchKernelGGL(k_pair_keys, dim3(cdiv(n, 256)), dim3(256), 0, st, d_in, (uint32_t)n, key, idx);
  sort_pairs(key, skey, idx, sidx, n, 0, 64, &tmp);
  if (s) {
    uint8_t *head = ws<uint8_t>("dd.head", n);
    hipLaunchKernelGGL(k_run_heads, dim3(cdiv(n, 256)), dim3(256), 0, st, skey, (uint32_t)n, s->tab.p, s->cap - 1, head, d_new);
    uint32_t n_new = 0;
    PGX_HIP(hipMemcpyAsync(&n_new, d_new, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    pgx::sync();
    seen_reserve(s, n_new);
    hipLaunchKernelGGL(k_seen_insert, dim3(cdiv(n, 256)), dim3(256), 0, st, skey, sidx, head, (uint32_t)n, s->tab.p, s->cap - 1, keep);
  } else {
    hipLaunchKernelGGL(k_first_flags, dim3(cdiv(n, 256)), dim3(256), 0, st, skey, sidx, (uint32_t)n, keep);
  }
  const uint32_t m = select_indices(keep, n, sel, &tmp);
  if (s) s->n_records += n, s->n_unique += m;   // (the set holds them from here on, whatever happens to the rows and the text)
  *d_rows = ws<Row>("dd.rows", m);
  if (m) hipLaunchKernelGGL(k_rows, dim3(cdiv(m, 256)), dim3(256), 0, st, d_in, sel, m, *d_rows);
  return m;
}

// one feed over records that are on the device
void feed_device(pgx_dedup_stream *s, const pgx_ovlp *d_in, size_t n, char **text, size_t *text_len) {
  KernelTimer tm("dedup", n);
  uint32_t *d_m = ws<uint32_t>("dd.m", 2);   // [0]: the pairs that are new; [1]: rows the host formats
  PGX_HIP(hipMemsetAsync(d_m, 0, 2 * sizeof(uint32_t), ctx().stream));
  Row *d_rows = nullptr;
  const uint32_t m = first_wins_rows(d_in, n, s, d_m, &d_rows);
  if (m && s->graph) graph_take(s, d_rows, m);   // the lines wait for the end of the stream (pgx_dedup_drain)
  if (m == 0 || s->graph) text_hand_out(s->stage, nullptr, 0, text, text_len);
  else rows_to_text(s, d_rows, m, d_m, text, text_len);
}

// text_call for a stream's entry points: after an error the stream that body left in `blame`, if any, has failed
template <class F>
int stream_text_call(char **text, size_t *text_len, int *done, F &&body) {
  pgx_dedup_stream *blame = nullptr;
  const int rc = text_call(text, text_len, done, [&] { return body(blame); });
  if (rc != PGX_OK && blame) blame->failed = true;
  return rc;
}
int feed_any(pgx_dedup_stream *s, const pgx_ovlp *recs, size_t n, char **text, size_t *text_len, bool on_device, const char *who) {
  return stream_text_call(text, text_len, nullptr, [&](pgx_dedup_stream *&blame) {
    blame = s;
    PGX_REQUIRE(s && text && text_len && (n == 0 || recs), PGX_EARG, "%s: null argument", who);
    PGX_REQUIRE(!s->shut, PGX_ESTATE, "%s: pgx_shutdown ran while the stream was open (close it)", who);
    PGX_REQUIRE(!s->failed, PGX_ESTATE, "%s: the stream returned an error before (close it)", who);
    if (s->draining) {   // (refused, not an error of the stream: the drain goes on)
      set_error("%s: the stream is being drained (pgx_dedup_drain ran)", who);
      blame = nullptr;
      return (int)PGX_ESTATE;
    }
    require_ready();
    PGX_REQUIRE(n < (1ULL << 31), PGX_EARG, "too many records for one feed");
    if (n == 0) {
      text_hand_out(s->stage, nullptr, 0, text, text_len);
      return (int)PGX_OK;
    }
    const pgx_ovlp *d_in = recs;
    if (!on_device) {
      pgx_ovlp *up = ws<pgx_ovlp>("dd.in", n);
      PGX_HIP(hipMemcpyAsync(up, recs, n * sizeof(pgx_ovlp), hipMemcpyHostToDevice, ctx().stream));
      d_in = up;
    }
    feed_device(s, d_in, n, text, text_len);
    timing_flush();   // (synchronises: the caller's records are no longer read when the feed returns)
    return (int)PGX_OK;
  });
}
}  // namespace

// the end of the stream: one stable pass over the store against the FINAL bitmap, piece by piece and in place (a piece's kept rows go
// to a scratch buffer and from there to the store's front, which the pass has read already)
void graph_compact(pgx_dedup_stream *s) {
  hipStream_t st = ctx().stream;
  const uint64_t n = s->store_n;
  uint64_t kept = 0;
  if (n) {
    const uint32_t piece = (uint32_t)std::min<uint64_t>(n, COMPACT_ROWS);
    DevBuf<Row> scratch;
    graph_alloc(scratch, piece, "the compaction's scratch");
    uint32_t *sel = ws<uint32_t>("dd.gsel", piece);
    for (uint64_t at = 0; at < n; at += piece) {
      const uint32_t m = (uint32_t)std::min<uint64_t>(piece, n - at);
      const uint32_t k = select_kept(s, s->store.p + at, m, sel);
      if (k == 0) continue;
      if (kept == at && k == m) {   // nothing dropped so far: the rows are in place
        kept += k;
        continue;
      }
      hipLaunchKernelGGL(k_gather_rows, dim3(cdiv(k, 256)), dim3(256), 0, st, s->store.p + at, sel, k, scratch.p);
      PGX_HIP(hipMemcpyAsync(s->store.p + kept, scratch.p, (size_t)k * sizeof(Row), hipMemcpyDeviceToDevice, st));
      kept += k;
    }
    PGX_HIP(hipGetLastError());
  }
  s->store_n = kept;
  s->draining = true;
}
}  // namespace pgx

extern "C" int pgx_dedup(const pgx_ovlp *recs, size_t n, char **text, size_t *text_len, uint64_t *n_unique) {
  return guarded([&] {
    require_ready();
    PGX_REQUIRE(text && text_len && (n == 0 || recs), PGX_EARG, "pgx_dedup: null argument");
    PGX_REQUIRE(n < (1ULL << 31), PGX_EARG, "too many records for one call");
    std::string out;
    uint64_t m = 0;
    if (n) {
      KernelTimer tm("dedup", n);
      pgx_ovlp *d_in = ws<pgx_ovlp>("dd.in", n);
      PGX_HIP(hipMemcpyAsync(d_in, recs, n * sizeof(pgx_ovlp), hipMemcpyHostToDevice, ctx().stream));
      Row *d_rows = nullptr;
      m = first_wins_rows(d_in, n, nullptr, nullptr, &d_rows);
      out = rows_to_host_text(d_rows, m);
    }
    *text = caller_text(out.data(), out.size());
    *text_len = out.size();
    if (n_unique) *n_unique = m;
    timing_flush();
  });
}

static int open_any(uint64_t expected_pairs, pgx_dedup_stream **out, bool graph, const char *who) {
  pgx_dedup_stream *s = nullptr;
  const int rc = guarded([&] {
    PGX_REQUIRE(out, PGX_EARG, "%s: null argument", who);
    *out = nullptr;
    PGX_REQUIRE(ctx().ready, PGX_ESTATE, "%s: no device context (pgx_init has not been called, or found no HIP device)", who);
    PGX_REQUIRE(expected_pairs < (1ULL << 40), PGX_ENOMEM, "%s: no device holds a set of %llu pairs", who, (unsigned long long)expected_pairs);
    uint64_t cap = SEEN_MIN_CAP;
    while (cap < 2 * expected_pairs) cap *= 2;
    s = new pgx_dedup_stream;
    s->graph = graph;
    seen_alloc(s->tab, cap);
    s->cap = cap;
    pgx::sync();
    g_streams.add(s);
    *out = s;
  });
  if (rc) delete s;
  return rc;
}

extern "C" int pgx_dedup_open(uint64_t expected_pairs, pgx_dedup_stream **out) { return open_any(expected_pairs, out, false, "pgx_dedup_open"); }

extern "C" int pgx_dedup_open_graph(uint64_t expected_pairs, pgx_dedup_stream **out) {
  return open_any(expected_pairs, out, true, "pgx_dedup_open_graph");
}

extern "C" int pgx_dedup_feed(pgx_dedup_stream *s, const pgx_ovlp *recs, size_t n, char **text, size_t *text_len) {
  return feed_any(s, recs, n, text, text_len, false, "pgx_dedup_feed");
}

extern "C" int pgx_dedup_feed_dev(pgx_dedup_stream *s, const pgx_ovlp *d_recs, size_t n, char **text, size_t *text_len) {
  return feed_any(s, d_recs, n, text, text_len, true, "pgx_dedup_feed_dev");
}

// what both graph-mode calls ask of their stream (the device context first: without one no stream can exist)
static void require_graph_stream(const pgx_dedup_stream *s, const char *who) {
  PGX_REQUIRE(ctx().ready, PGX_ESTATE, "%s: no device context (pgx_init has not been called, or found no HIP device)", who);
  PGX_REQUIRE(s, PGX_EARG, "%s: null argument", who);
  PGX_REQUIRE(!s->shut, PGX_ESTATE, "%s: pgx_shutdown ran while the stream was open (close it)", who);
  PGX_REQUIRE(!s->failed, PGX_ESTATE, "%s: the stream returned an error before (close it)", who);
  PGX_REQUIRE(s->graph, PGX_ESTATE, "%s: not a graph-mode stream (pgx_dedup_open_graph)", who);
}

// the next lines of a graph-mode stream, at most max_lines of them; the first call settles which lines there are
static void drain_lines(pgx_dedup_stream *s, uint64_t max_lines, char **text, size_t *text_len, int *done) {
  KernelTimer tm("dedup", std::min<uint64_t>(max_lines, s->store_n - s->drained));
  if (!s->draining) graph_compact(s);
  const uint32_t m = (uint32_t)text_lines(max_lines, s->store_n - s->drained);
  if (m == 0) text_hand_out(s->stage, nullptr, 0, text, text_len);
  else {
    uint32_t *d_m = ws<uint32_t>("dd.m", 2);
    PGX_HIP(hipMemsetAsync(d_m, 0, 2 * sizeof(uint32_t), ctx().stream));
    rows_to_text(s, s->store.p + s->drained, m, d_m, text, text_len);
  }
  s->drained += m;
  if (s->drained == s->store_n) {
    *done = 1;
    s->store.release();   // (the counters stay for pgx_dedup_graph_stats)
    s->released = true;
  }
}

extern "C" int pgx_dedup_drain(pgx_dedup_stream *s, uint64_t max_lines, char **text, size_t *text_len, int *done) {
  return stream_text_call(text, text_len, done, [&](pgx_dedup_stream *&blame) {
    require_graph_stream(s, "pgx_dedup_drain");
    PGX_REQUIRE(text && text_len && done && max_lines, PGX_EARG, "pgx_dedup_drain: null argument or max_lines == 0");
    blame = s;   // the checks passed: an error from here on is the stream's
    drain_lines(s, max_lines, text, text_len, done);
    timing_flush();
    return (int)PGX_OK;
  });
}

extern "C" int pgx_dedup_graph_stats(pgx_dedup_stream *s, uint64_t *n_contained_reads, uint64_t *n_lines_kept, uint64_t *n_lines_total) {
  return guarded([&] {
    require_graph_stream(s, "pgx_dedup_graph_stats");
    if (n_contained_reads) *n_contained_reads = graph_count_marked(s);
    if (n_lines_kept) *n_lines_kept = s->store_n;
    if (n_lines_total) *n_lines_total = s->n_unique;
  });
}

extern "C" int pgx_dedup_close(pgx_dedup_stream *s, uint64_t *n_records, uint64_t *n_unique) {
  if (!s) {
    set_error("pgx_dedup_close: null argument");
    return PGX_EARG;
  }
  if (n_records) *n_records = s->n_records;
  if (n_unique) *n_unique = s->n_unique;
  g_streams.destroy(s);
  return PGX_OK;
}
