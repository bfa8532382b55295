// pgx_reads.hip -- FASTA/FASTQ texts, in pieces and from several files, to one resident pgx_seqdb on the GPU.
// The grammar is the whole reader loop of the reference's kseq reader, its '+' branch included, as predicates of a byte or a line, prefix
// sums and one successor function over the lines that hold a header marker; the records are the chain from line 0 under that function,
// marked by pointer doubling (k_rd_chase).  Passes on carry + piece:
//   marks  : k_fa_first, k_fa_marks (pgx_fasta_k.h), the line starts (select), k_rd_fm (a line's first marker byte)
//   lines  : k_rd_lines (kept length K, stop / non-empty / marker / suspicious flags), PS = scan of K, the four flag lists (select)
//   chain  : k_rd_succ (successor, verdict and stop line of every line with a marker), k_rd_chase x (ceil(log2(lines)) + 1), k_rd_verdict
//   tables : record of every line (scan), k_rd_seq (sequence-line flags), then the sequence-line / record / name tables, the gather and the
//            encode of pgx_fasta_k.h, the encode straight into the builder's store
// A record is committed only when its whole parse lies inside the bytes seen; the text from the first uncommitted header byte on is carried.
#include <sys/stat.h>
#include <zlib.h>

#include <algorithm>
#include <string>

#include "pgx_fasta_k.h"

struct pgx_seqdb_builder {
  bool shut = false;
  pgx::DevBuf<uint8_t> store;   // the database's bytes so far and room behind them ("seqdb.bytes")
  uint64_t used = 0;
  pgx::DevBuf<uint8_t> carry;   // the current file's text from its first uncommitted header byte on ("reads")
  uint64_t carry_len = 0;
  uint64_t file_len = 0;        // bytes fed of the current file
  bool file_dead = false;       // the current file's records have ended (a record the reader calls truncated)
  std::vector<uint64_t> roff{0};   // records so far + 1
  std::vector<char> names;
  void drop_device_state() {
    store.release(), carry.release();
    carry_len = 0;
  }
};

namespace pgx {
namespace {

LiveSet<pgx_seqdb_builder> g_builders;
ShutdownHook g_builders_hook([] { g_builders.shutdown(); });

enum : uint8_t { RD_NONE = 0, RD_EMIT = 1, RD_BAD = 2, RD_MORE = 3, RD_REFUSE = 4 };

__device__ __forceinline__ uint64_t rd_line_end(const uint8_t *__restrict__ b, uint64_t n, const uint64_t *__restrict__ start, uint32_t n_lines, uint32_t j) {
  return j + 1 < n_lines ? start[j + 1] - 1 : (b[n - 1] == '\n' ? n - 1 : n);
}
// the first entry >= v of an ascending list, or none
__device__ __forceinline__ uint32_t rd_next_in(const uint32_t *__restrict__ list, uint32_t cnt, uint32_t v, uint32_t none) {
  uint32_t lo = 0, hi = cnt;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (list[mid] >= v) hi = mid;
    else lo = mid + 1;
  }
  return lo < cnt ? list[lo] : none;
}

// fm[j] = the smallest marker byte of line j (starts as NONE).  Quality strings are full of '@' and '>': of a wavefront's 64 bytes only
// the markers with no earlier marker of the same line among them (none between them and the last '\n' in front) look their line up.
__global__ __launch_bounds__(TPB) void k_rd_fm(const uint8_t *__restrict__ b, uint64_t n, uint64_t m0, const uint64_t *__restrict__ start, uint32_t n_lines,
                                               unsigned long long *__restrict__ fm) {
  const uint64_t base = (uint64_t)blockIdx.x * TILE;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t below = (1ull << lane) - 1;
  for (uint32_t it = 0; it < TILE / TPB; ++it) {
    const uint64_t i = base + it * TPB + threadIdx.x;
    const uint32_t c = i < n && i >= m0 ? b[i] : 0;
    const bool mk = fa_marker(c);
    const uint64_t mks = __ballot(mk) & below, nls = __ballot(c == '\n') & below;
    // (the nearest earlier marker of the wavefront is of this line unless a '\n' lies between: compare the highest set bits)
    if (!mk || (mks && (!nls || (63 - __builtin_clzll(mks)) > (63 - __builtin_clzll(nls))))) continue;
    const uint64_t u = upper_bound<uint64_t>(start, 0, n_lines, i);   // (>= 1: start[0] == m0 <= i)
    if (u) atomicMin(fm + (u - 1), (unsigned long long)i);
  }
}

// per line: K = its length less one trailing '\r'; stop: it starts with '>', '+' or '@'; full: it is not empty; susp: it is empty behind a
// line that is empty, "\r" or ends "\r\r" -- the only lines at which the reader's strip of the accumulated quality string can take a byte
// that K did not
__global__ void k_rd_lines(const uint8_t *__restrict__ b, uint64_t n, const uint64_t *__restrict__ start, uint32_t n_lines,
                           const unsigned long long *__restrict__ fm, uint64_t *__restrict__ K, uint8_t *__restrict__ stop, uint8_t *__restrict__ full,
                           uint8_t *__restrict__ has_fm, uint8_t *__restrict__ susp) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_lines) return;
  const uint64_t s = start[j], e = rd_line_end(b, n, start, n_lines, j), len = e - s;
  K[j] = len - (len && b[e - 1] == '\r' ? 1 : 0);
  const uint32_t c = len ? b[s] : 0;
  stop[j] = c == '>' || c == '+' || c == '@';
  full[j] = len != 0;
  has_fm[j] = fm[j] != NONE;
  bool sp = false;
  if (!len && j) {
    const uint64_t ps = start[j - 1], pl = s - 1 - ps;   // (line j - 1 has its '\n')
    sp = pl == 0 || (b[s - 2] == '\r' && (pl == 1 || b[s - 3] == '\r'));
  }
  susp[j] = sp;
}

struct RdLists {
  const uint32_t *stops, *full, *marked, *susp;
  uint32_t n_stops, n_full, n_marked, n_susp;
};

// The successor function.  For a line j with a marker (its header sits at fm[j]): J[j] = the line of the next header (n_lines: none),
// st[j] = RD_EMIT (the record is complete: its sequence lines are the non-empty lines in (j, kk[j])), RD_BAD (the reader calls it
// truncated: the file's records end in front of it), RD_MORE (its parse does not end inside the bytes seen; only without `final`),
// RD_REFUSE (kk[j]: the empty quality line at which the reader's sum is no prefix sum) or RD_NONE (a marker that starts no record).
__global__ void k_rd_succ(const uint8_t *__restrict__ b, uint64_t n, const uint64_t *__restrict__ start, uint32_t n_lines,
                          const unsigned long long *__restrict__ fm, const uint64_t *__restrict__ PS, RdLists ls, uint32_t final, uint32_t eof_seen,
                          uint32_t *__restrict__ J, uint8_t *__restrict__ st, uint32_t *__restrict__ kk) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j > n_lines) return;
  const uint32_t L = n_lines;
  uint32_t nxt = L, k_out = L;
  uint8_t verdict = RD_NONE;
  const bool last_term = b[n - 1] == '\n';
  const uint8_t short_of = final ? RD_BAD : RD_MORE;
  do {
    if (j == L || fm[j] == NONE) break;
    if (final && eof_seen && fm[j] == n - 1) break;
    if (!final && j + 1 == L && !last_term) { verdict = RD_MORE; break; }
    const uint32_t k = rd_next_in(ls.stops, ls.n_stops, j + 1, L);
    if (k == L) { verdict = final ? RD_EMIT : RD_MORE; break; }
    k_out = k;
    if (b[start[k]] != '+') { verdict = RD_EMIT, nxt = k; break; }
    if (k + 1 == L && !last_term) { verdict = short_of; break; }
    uint64_t slen = PS[k] - PS[j + 1];
    {
      const uint32_t f = rd_next_in(ls.full, ls.n_full, j + 1, L);
      if (f < k && start[f + 1] - 1 - start[f] == 1 && b[start[f]] == '\r') ++slen;
    }
    const uint32_t q0 = k + 1;
    if (q0 >= L) { verdict = final ? (slen == 0 ? RD_EMIT : RD_BAD) : RD_MORE; break; }
    uint32_t f = rd_next_in(ls.full, ls.n_full, q0, L);
    if (f < L && !(rd_line_end(b, n, start, L, f) - start[f] == 1 && b[start[f]] == '\r')) f = L;   // f: the lone "\r" that is the block's first non-empty line
    uint32_t lo = q0, hi = L;   // the smallest m whose lines q0 .. m keep slen bytes or more
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (PS[mid + 1] - PS[q0] + (f <= mid ? 1 : 0) >= slen) hi = mid;
      else lo = mid + 1;
    }
    const uint32_t m = lo;
    if (m == L) { verdict = short_of; break; }
    if (!final && m + 1 == L && !last_term) { verdict = RD_MORE; break; }
    const uint32_t sp = rd_next_in(ls.susp, ls.n_susp, q0 + 1, L);
    if (sp <= m) {   // the reader's own sum over these lines, a line at a time
      uint64_t ln = 0, tail = 0;   // of the accumulated string: its length, its trailing '\r's
      bool refused = false;
      for (uint32_t t = q0; t <= m && !refused; ++t) {
        const uint64_t s = start[t], e = rd_line_end(b, n, start, L, t);
        uint64_t cr = 0;
        while (cr < e - s && b[e - 1 - cr] == '\r') ++cr;
        tail = cr == e - s ? tail + cr : cr;
        ln += e - s;
        if (ln > 1 && tail) {
          if (e == s) refused = true, k_out = t;
          else --ln, --tail;
        }
      }
      if (refused) { verdict = RD_REFUSE; break; }
    }
    if (PS[m + 1] - PS[q0] + (f <= m ? 1 : 0) != slen) { verdict = RD_BAD; break; }
    verdict = RD_EMIT, nxt = rd_next_in(ls.marked, ls.n_marked, m + 1, L);
  } while (false);
  J[j] = nxt, st[j] = verdict, kk[j] = k_out;
}

// a round of the pointer doubling: every marked line marks the line it points at, and every line then points twice as far
__global__ void k_rd_chase(const uint32_t *__restrict__ J, uint32_t *__restrict__ Jn, uint8_t *mark, uint32_t n_nodes) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_nodes) return;
  const uint32_t t = J[j];
  if (mark[j]) mark[t] = 1;
  Jn[j] = J[t];
}

// is_rec: a line of the chain whose record is complete; acc[0..2]: the smallest header byte of a chain line that is RD_BAD / RD_MORE, the
// smallest refused line's byte
__global__ void k_rd_verdict(const uint8_t *__restrict__ mark, const uint8_t *__restrict__ st, const uint32_t *__restrict__ kk,
                             const unsigned long long *__restrict__ fm, const uint64_t *__restrict__ start, uint32_t n_lines, uint32_t *__restrict__ is_rec,
                             unsigned long long *acc) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_lines) return;
  const uint8_t v = mark[j] ? st[j] : (uint8_t)RD_NONE;
  is_rec[j] = v == RD_EMIT;
  if (v == RD_BAD) atomicMin(acc, fm[j]);
  if (v == RD_MORE) atomicMin(acc + 1, fm[j]);
  if (v == RD_REFUSE) atomicMin(acc + 2, (unsigned long long)start[kk[j]]);
}

// is_seq: a non-empty line between the header line of a record (the last one at or before it: rec_incl) and that record's stop line
__global__ void k_rd_seq(const uint8_t *__restrict__ full, const uint32_t *__restrict__ rec_incl, const uint32_t *__restrict__ hl,
                         const uint32_t *__restrict__ kk, uint32_t n_lines, uint8_t *__restrict__ is_seq) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_lines) return;
  const uint32_t r = rec_incl[t + 1];
  bool sq = false;
  if (r && full[t]) {
    const uint32_t j = hl[r - 1];
    sq = t > j && t < kk[j];
  }
  is_seq[t] = sq;
}

// room for `more` bytes and the 1 KiB tail behind the bytes in use: doubles and copies
void store_reserve(pgx_seqdb_builder *b, uint64_t more) {
  const uint64_t need = b->used + more + 1024;
  if (need <= b->store.n) return;
  MemTag mem_tag("seqdb.bytes");
  DevBuf<uint8_t> grown(std::max<uint64_t>(need, 2 * (uint64_t)b->store.n));
  if (b->used) PGX_HIP(hipMemcpyAsync(grown.p, b->store.p, b->used, hipMemcpyDeviceToDevice, ctx().stream));
  pgx::sync();
  b->store = std::move(grown);
}

// the grammar on d (n >= 1 bytes: carry + piece), the complete records of its chain into the store; answers the byte from which the text
// is carried (n: nothing is), or NONE: the file's records have ended
uint64_t reads_passes(pgx_seqdb_builder *bd, const uint8_t *d, uint64_t n, bool final, uint32_t eof_seen, uint64_t file_off) {
  hipStream_t st = ctx().stream;
  PrimWs tmp;
  DevBuf<unsigned long long> acc(6);   // m0, line starts, (k_fa_marks' '+'), RD_BAD, RD_MORE, RD_REFUSE
  unsigned long long h_acc[6] = {NONE, 0, NONE, NONE, NONE, NONE};
  acc.upload(h_acc, 6);
  pgx::sync();
  hipLaunchKernelGGL(k_fa_first, dim3(cdiv(n, TILE)), dim3(TPB), 0, st, d, n, acc.p);
  acc.download(h_acc, 1);
  pgx::sync();
  const uint64_t m0 = h_acc[0];
  if (m0 == NONE) return n;   // (the reader skips to the next marker)
  DevBuf<uint64_t> start;
  uint64_t n_lines64 = 0;
  {
    DevBuf<uint8_t> ls(n);
    hipLaunchKernelGGL(k_fa_marks, dim3(cdiv(n, TILE)), dim3(TPB), 0, st, d, n, m0, ls.p, acc.p + 1);
    acc.download(h_acc, 2);
    pgx::sync();
    n_lines64 = h_acc[1];
    PGX_REQUIRE(n_lines64 < (1ull << 31), PGX_EINVAL, "pgx_seqdb_builder_feed: %llu lines in one piece and its carry (2^31 and more are not read here)",
                (unsigned long long)n_lines64);
    start.alloc(n_lines64 + 1);
    uint64_t got = 0;
    for (uint64_t at = 0; at < n; at += 1ull << 30) {   // (the select takes at most 2^30 flags a call)
      const uint64_t len = std::min<uint64_t>(n - at, 1ull << 30);
      PGX_REQUIRE(got <= n_lines64, PGX_EHIP, "pgx_seqdb_builder_feed: the line starts were counted as %llu and selected as more", (unsigned long long)n_lines64);
      const uint64_t c = select_indices(ls.p + at, len, start.p + got, &tmp);
      if (c && at) hipLaunchKernelGGL(k_fa_add_base, dim3(cdiv(c, 256)), dim3(256), 0, st, start.p + got, c, at);
      got += c;
    }
    PGX_REQUIRE(got == n_lines64, PGX_EHIP, "pgx_seqdb_builder_feed: the line starts were counted as %llu and selected as %llu", (unsigned long long)n_lines64,
                (unsigned long long)got);
  }
  const uint32_t L = (uint32_t)n_lines64;
  // lines
  DevBuf<unsigned long long> fm((size_t)L + 1);
  PGX_HIP(hipMemsetAsync(fm.p, 0xff, ((size_t)L + 1) * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_rd_fm, dim3(cdiv(n, TILE)), dim3(TPB), 0, st, d, n, m0, start.p, L, fm.p);
  DevBuf<uint64_t> PS((size_t)L + 2);
  DevBuf<uint8_t> f_stop((size_t)L + 1), f_full((size_t)L + 1), f_fm((size_t)L + 1), f_susp((size_t)L + 1);
  LAUNCH(k_rd_lines, L, d, n, start.p, L, fm.p, PS.p + 1, f_stop.p, f_full.p, f_fm.p, f_susp.p);
  scan_to_total(PS.p + 1, PS.p, L, &tmp);
  DevBuf<uint32_t> l_stop((size_t)L + 1), l_full((size_t)L + 1), l_fm((size_t)L + 1), l_susp((size_t)L + 1);
  RdLists lists;
  lists.stops = l_stop.p, lists.full = l_full.p, lists.marked = l_fm.p, lists.susp = l_susp.p;
  lists.n_stops = select_indices(f_stop.p, L, l_stop.p, &tmp);
  lists.n_full = select_indices(f_full.p, L, l_full.p, &tmp);
  lists.n_marked = select_indices(f_fm.p, L, l_fm.p, &tmp);
  lists.n_susp = select_indices(f_susp.p, L, l_susp.p, &tmp);
  f_stop.release(), f_fm.release(), f_susp.release();
  // chain
  DevBuf<uint32_t> J((size_t)L + 1), Jn((size_t)L + 1), kk((size_t)L + 1);
  DevBuf<uint8_t> verdict((size_t)L + 1), mark((size_t)L + 1);
  LAUNCH(k_rd_succ, (size_t)L + 1, d, n, start.p, L, fm.p, PS.p, lists, final ? 1u : 0u, eof_seen, J.p, verdict.p, kk.p);
  PGX_HIP(hipMemsetAsync(mark.p, 0, (size_t)L + 1, st));
  PGX_HIP(hipMemsetAsync(mark.p, 1, 1, st));
  uint32_t rounds = 1;
  while ((1ull << (rounds - 1)) < (uint64_t)L + 1) ++rounds;
  for (uint32_t r = 0; r < rounds; ++r) {
    LAUNCH(k_rd_chase, (size_t)L + 1, J.p, Jn.p, mark.p, L + 1);
    std::swap(J.p, Jn.p);
  }
  DevBuf<uint32_t> is_rec((size_t)L + 1), rec_incl((size_t)L + 2);
  LAUNCH(k_rd_verdict, L, mark.p, verdict.p, kk.p, fm.p, start.p, L, is_rec.p, acc.p + 3);
  acc.download(h_acc, 6);
  const uint32_t n_rec = scan_to_total(is_rec.p, rec_incl.p, L, &tmp);   // (synchronises)
  PGX_REQUIRE(h_acc[5] == NONE, PGX_EINVAL,
              "pgx_seqdb_builder_feed: the empty quality line at byte offset %llu of the file follows a '\\r' that the reader would strip from an earlier line "
              "(not evaluated here: use shmr_mkseqdb)", (unsigned long long)(file_off + h_acc[5]));
  const uint64_t carry_from = h_acc[3] != NONE || final ? NONE : (h_acc[4] != NONE ? (uint64_t)h_acc[4] : n);
  J.release(), Jn.release(), mark.release(), verdict.release(), PS.release();
  l_stop.release(), l_full.release(), l_fm.release(), l_susp.release();
  if (!n_rec) return carry_from;
  PGX_REQUIRE(bd->roff.size() - 1 + (uint64_t)n_rec < (1ull << 32), PGX_EINVAL, "pgx_seqdb_builder_feed: %llu records (2^32 and more do not fit the idx)",
              (unsigned long long)(bd->roff.size() - 1 + (uint64_t)n_rec));
  // tables
  DevBuf<uint32_t> hl((size_t)n_rec + 1), sl((size_t)L + 1);
  DevBuf<uint8_t> is_seq((size_t)L + 1);
  const uint32_t n_hl = select_indices(is_rec.p, L, hl.p, &tmp);
  PGX_REQUIRE(n_hl == n_rec, PGX_EHIP, "pgx_seqdb_builder_feed: %u record headers scanned, %u selected", n_rec, n_hl);
  LAUNCH(k_rd_seq, L, f_full.p, rec_incl.p, hl.p, kk.p, L, is_seq.p);
  const uint32_t n_sl = select_indices(is_seq.p, L, sl.p, &tmp);
  is_rec.release(), is_seq.release(), f_full.release(), kk.release();
  DevBuf<uint64_t> l_start((size_t)n_sl + 1), l_kept((size_t)n_sl + 1), pool_off((size_t)n_sl + 2);
  DevBuf<uint32_t> l_rec((size_t)n_sl + 1);
  if (n_sl) LAUNCH(k_fa_seq_lines, n_sl, d, n, start.p, (uint64_t)L, sl.p, n_sl, rec_incl.p, final ? eof_seen : 0u, l_start.p, l_kept.p, l_rec.p);
  const uint64_t pool_size = scan_to_total(l_kept.p, pool_off.p, n_sl, &tmp);
  if (!n_sl) PGX_HIP(hipMemsetAsync(pool_off.p, 0, sizeof(uint64_t), st));
  DevBuf<uint64_t> hdr_off((size_t)n_rec + 1), name_len1((size_t)n_rec + 1), name_off((size_t)n_rec + 2), roff((size_t)n_rec + 1);
  // (the headers sit at fm, not at the line starts: a header behind a quality block may stand in the middle of a line)
  LAUNCH(k_fa_records, (size_t)n_rec + 1, d, n, (const uint64_t *)fm.p, hl.p, n_rec, l_rec.p, n_sl, pool_off.p, hdr_off.p, name_len1.p, roff.p);
  const uint64_t names_size = scan_to_total(name_len1.p, name_off.p, n_rec, &tmp);
  DevBuf<char> names(names_size + 1);
  LAUNCH(k_fa_names, n_rec, d, hdr_off.p, name_off.p, n_rec, names.p);
  std::vector<uint64_t> h_roff((size_t)n_rec + 1);
  std::vector<char> h_names(names_size);
  roff.download(h_roff.data(), (size_t)n_rec + 1);
  names.download(h_names.data(), names_size);
  pgx::sync();
  for (uint32_t r = 0; r < n_rec; ++r)
    PGX_REQUIRE(h_roff[r + 1] - h_roff[r] < (1ull << 32), PGX_EINVAL, "pgx_seqdb_builder_feed: record %llu has %llu bases (2^32 and more do not fit the idx)",
                (unsigned long long)(bd->roff.size() - 1 + r), (unsigned long long)(h_roff[r + 1] - h_roff[r]));
  start.release(), sl.release(), hl.release(), rec_incl.release(), fm.release();
  // gather, and encode behind the bytes in use
  DevBuf<uint8_t> pool(pool_size + 1);
  if (pool_size) hipLaunchKernelGGL(k_fa_gather, dim3(cdiv(n, TILE)), dim3(TPB), 0, st, d, n, l_start.p, l_kept.p, pool_off.p, n_sl, pool.p, pool_size);
  store_reserve(bd, pool_size);
  if (pool_size) hipLaunchKernelGGL(k_fa_encode, dim3(cdiv(pool_size, TILE)), dim3(TPB), 0, st, pool.p, pool_size, roff.p, n_rec, bd->store.p + bd->used);
  PGX_HIP(hipGetLastError());
  pgx::sync();
  // commit
  const uint64_t base = bd->used;
  for (uint32_t r = 1; r <= n_rec; ++r) bd->roff.push_back(base + h_roff[r]);
  bd->names.insert(bd->names.end(), h_names.begin(), h_names.end());
  bd->used = base + pool_size;
  return carry_from;
}

void require_builder(const pgx_seqdb_builder *b, const char *who) {
  PGX_REQUIRE(b, PGX_EARG, "%s: null argument", who);
  PGX_REQUIRE(!b->shut && ctx().ready, PGX_ESTATE, "%s: pgx_shutdown ran while the builder was open (close it)", who);
}

void builder_feed(pgx_seqdb_builder *b, const char *text, size_t len, int on_device, int ends_file) {
  hipStream_t st = ctx().stream;
  const uint64_t file_len = b->file_len + len, n = b->carry_len + len;
  if (!b->file_dead && n) {
    MemTag mem_tag("reads");
    DevBuf<uint8_t> copy;
    const uint8_t *d = (const uint8_t *)text;
    if (b->carry_len || !on_device) {
      KernelTimer tm_up("reads.upload", len);
      copy.alloc(n + 1);
      if (b->carry_len) PGX_HIP(hipMemcpyAsync(copy.p, b->carry.p, b->carry_len, hipMemcpyDeviceToDevice, st));
      if (len) PGX_HIP(hipMemcpyAsync(copy.p + b->carry_len, text, len, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
      d = copy.p;
    }
    KernelTimer tm("reads", n);
    const uint64_t from = reads_passes(b, d, n, ends_file != 0, file_len % KS_BUF != 0, file_len - n);
    DevBuf<uint8_t> carry;
    const uint64_t keep = from == NONE ? 0 : n - from;
    if (keep) {
      carry.alloc(keep);
      PGX_HIP(hipMemcpyAsync(carry.p, d + from, keep, hipMemcpyDeviceToDevice, st));
    }
    pgx::sync();   // (the caller's text and the copy are free behind this)
    b->carry = std::move(carry), b->carry_len = keep;
    b->file_dead = from == NONE;
  }
  b->file_len = file_len;
  if (ends_file) {
    b->carry.release();
    b->carry_len = 0, b->file_len = 0, b->file_dead = false;
  }
}

int builder_feed_entry(pgx_seqdb_builder *b, const char *text, size_t len, int on_device, int ends_file) {
  int code = PGX_OK;
  try {
    builder_feed(b, text, len, on_device, ends_file);
  } catch (const Fail &f) {
    code = build_fail_code(f, "pgx_seqdb_builder_feed", "tables, pool and database", b->carry_len + len, "bytes of text");
  }
  timing_flush();
  return code;
}

int builder_finish(pgx_seqdb_builder *b, pgx_seqdb **out, char **names, size_t *names_len, uint64_t *n_reads, uint64_t *n_bases) {
  const size_t n_rec = b->roff.size() - 1;
  PGX_REQUIRE(n_rec, PGX_EINVAL, "pgx_seqdb_builder_finish: no record in the texts fed");
  store_reserve(b, 0);
  if ((uint64_t)b->store.n - (b->used + 1024) > (uint64_t)b->store.n / 8) {   // too much slack: one exact copy
    MemTag mem_tag("seqdb.bytes");
    DevBuf<uint8_t> exact(b->used + 1024);
    if (b->used) PGX_HIP(hipMemcpyAsync(exact.p, b->store.p, b->used, hipMemcpyDeviceToDevice, ctx().stream));
    pgx::sync();
    b->store = std::move(exact);
  }
  PGX_HIP(hipMemsetAsync(b->store.p + b->used, 0, 1024, ctx().stream));
  std::vector<uint32_t> rid(n_rec), rlen(n_rec);
  for (size_t r = 0; r < n_rec; ++r) rid[r] = (uint32_t)r, rlen[r] = (uint32_t)(b->roff[r + 1] - b->roff[r]);
  char *nm = (char *)malloc(b->names.size() + 1);
  if (!nm) throw std::bad_alloc();
  memcpy(nm, b->names.data(), b->names.size());
  nm[b->names.size()] = 0;
  const uint64_t bases = b->used;
  const int rc = seqdb_take_dev(std::move(b->store), (size_t)bases, rid.data(), rlen.data(), b->roff.data(), (uint32_t)n_rec, out);
  const size_t nl = b->names.size();
  b->used = 0, b->roff.assign(1, 0), b->names.clear();
  b->carry.release();
  b->carry_len = 0, b->file_len = 0, b->file_dead = false;
  if (rc != PGX_OK) {
    free(nm);
    return rc;
  }
  *names = nm, *names_len = nl;
  if (n_reads) *n_reads = n_rec;
  if (n_bases) *n_bases = bases;
  return PGX_OK;
}

}  // namespace
}  // namespace pgx

using namespace pgx;

extern "C" int pgx_seqdb_builder_open(uint64_t reserve_bases, pgx_seqdb_builder **out) {
  return live_build("pgx_seqdb_builder_open", g_builders, out, [] {}, [&](pgx_seqdb_builder *b, uint64_t *n) {
    *n = reserve_bases;
    MemTag mem_tag("seqdb.bytes");
    b->store.alloc(reserve_bases + 1024);
  }, "database", "bases reserved");
}

extern "C" int pgx_seqdb_builder_feed(pgx_seqdb_builder *b, const char *text, size_t len, int on_device, int ends_file) {
  return guarded([&]() -> int {
    require_ready();
    require_builder(b, "pgx_seqdb_builder_feed");
    PGX_REQUIRE(text || len == 0, PGX_EARG, "pgx_seqdb_builder_feed: null argument");
    return builder_feed_entry(b, text, len, on_device, ends_file);
  });
}

extern "C" int pgx_seqdb_builder_finish(pgx_seqdb_builder *b, pgx_seqdb **out, char **names, size_t *names_len, uint64_t *n_reads, uint64_t *n_bases) {
  return guarded([&]() -> int {
    require_ready();
    require_builder(b, "pgx_seqdb_builder_finish");
    PGX_REQUIRE(out && names && names_len, PGX_EARG, "pgx_seqdb_builder_finish: null argument");
    *out = nullptr, *names = nullptr, *names_len = 0;
    return builder_finish(b, out, names, names_len, n_reads, n_bases);
  });
}

extern "C" void pgx_seqdb_builder_close(pgx_seqdb_builder *b) {
  if (b) g_builders.destroy(b);
}

extern "C" int pgx_seqdb_from_files(const char *seq_dataset_path, pgx_seqdb **out, char **names, size_t *names_len, uint64_t *n_reads, uint64_t *n_bases) {
  pgx_seqdb_builder *b = nullptr;
  uint8_t *pinned = nullptr;
  FILE *lst = nullptr;
  const int rc = guarded([&]() -> int {
    require_ready();
    PGX_REQUIRE(seq_dataset_path && out && names && names_len, PGX_EARG, "pgx_seqdb_from_files: null argument");
    *out = nullptr, *names = nullptr, *names_len = 0;
    lst = fopen(seq_dataset_path, "r");
    PGX_REQUIRE(lst, PGX_EIO, "file '%s' open error", seq_dataset_path);
    const size_t PIECE = getenv("PGX_FROM_READS_PIECE") ? (size_t)atoll(getenv("PGX_FROM_READS_PIECE")) : ((size_t)256 << 20);
    PGX_REQUIRE(PIECE >= 1, PGX_EARG, "pgx_seqdb_from_files: PGX_FROM_READS_PIECE must be 1 or more");
    char fn[8192];
    uint64_t on_disk = 0;   // (half of it is reserved: the bases of four-line FASTQ in plain files; anything else grows the store)
    while (fscanf(lst, "%8191s", fn) == 1) {
      struct stat sb;
      if (stat(fn, &sb) == 0) on_disk += (uint64_t)sb.st_size;
    }
    rewind(lst);
    int code = pgx_seqdb_builder_open(on_disk / 2, &b);
    if (code != PGX_OK) return code;
    PGX_HIP(hipHostMalloc((void **)&pinned, PIECE, hipHostMallocDefault));
    while (fscanf(lst, "%8191s", fn) == 1) {
      gzFile gz = gzopen(fn, "r");   // (reads plain and gzip files alike; inflation stays on this thread, a file after the other)
      PGX_REQUIRE(gz, PGX_EIO, "file '%s' open error", fn);
      gzbuffer(gz, 1 << 20);
      bool eof = false;
      while (!eof && code == PGX_OK) {
        size_t have = 0;
        while (!eof && have < PIECE) {
          const int got = gzread(gz, pinned + have, (unsigned)std::min<size_t>(PIECE - have, (size_t)1 << 30));
          if (got <= 0) eof = true;
          else have += (size_t)got;
        }
        code = builder_feed_entry(b, (const char *)pinned, have, 0, eof ? 1 : 0);
      }
      gzclose(gz);
      if (code != PGX_OK) return code;
    }
    return builder_finish(b, out, names, names_len, n_reads, n_bases);
  });
  if (lst) fclose(lst);
  if (pinned) (void)hipHostFree(pinned);
  pgx_seqdb_builder_close(b);
  return rc;
}

extern "C" int pgx_seqdb_read_lengths(const pgx_seqdb *db, uint32_t *rlen_by_rid, size_t cap) {
  return guarded([&]() -> int {
    PGX_REQUIRE(db && (rlen_by_rid || cap == 0), PGX_EARG, "pgx_seqdb_read_lengths: null argument");
    PGX_REQUIRE(cap >= db->rlen_by_rid.size(), PGX_EARG, "pgx_seqdb_read_lengths: room for %zu lengths, the database has %zu", cap, db->rlen_by_rid.size());
    std::copy(db->rlen_by_rid.begin(), db->rlen_by_rid.end(), rlen_by_rid);
    return PGX_OK;
  });
}
