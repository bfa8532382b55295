// pgx_text.h -- everything about device text, once: the fields of a line that is read (is_blank, parse_int), the pieces of a line as
// glibc prints them (LineOut), the stream-out of a tile of
// text from LDS (tile_out), the pinned staging that device text leaves through (TextStage), the host side of an entry point that hands
// text out (text_call, text_hand_out), and the piece scheme whole (k_piece_len, k_piece_format, TextPlan, plan_text, text_next).
// The stages that write their text on the device tile it in one of two ways:
//   * tiles of lines: a workgroup formats 256 lines into LDS behind a pad to the global address's phase (k_format of pgx_dedup.hip,
//     k_sg_format of pgx_sgraph.hip).  The two kernels are their stages' own; they share LineOut, tile_out and the host side.
//   * tiles of bytes over pieces: a workgroup serves TEXT_TILE bytes of the file and finds the pieces that touch them by searching the
//     pieces' offsets (pgx_unitigs.hip, pgx_ctgpaths.hip, pgx_tiling.hip).  A stage supplies a piece source; the kernels, the layout and
//     the hand-out are here.
#pragma once
#include <algorithm>

#include "pgx_internal.h"

namespace pgx {
// ---- reading text: the fields of a line as Python's split() cuts them ----------------------------------------------------------------------
__host__ __device__ inline bool is_blank(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 28 && c <= 31); }
// an optional '-' and 1 .. 18 digits
__host__ __device__ inline bool parse_int(const char *p, uint32_t n, int64_t *out) {
  const bool neg = n && p[0] == '-';
  uint32_t i = neg;
  if (i >= n || n - i > 18) return false;
  int64_t v = 0;
  for (; i < n; ++i) {
    if (p[i] < '0' || p[i] > '9') return false;
    v = v * 10 + (p[i] - '0');
  }
  *out = neg ? -v : v;
  return true;
}

// ---- text: "%d", "%09d", "%u", "%0.1f" as glibc prints them -------------------------------------------------------------------------------
__device__ inline uint32_t div10(uint32_t v) { return __umulhi(v, 0xCCCCCCCDu) >> 3; }
__device__ inline uint64_t div10(uint64_t v) { return __umul64hi(v, 0xCCCCCCCCCCCCCCCDULL) >> 3; }
__device__ inline uint32_t ndigits(uint32_t v) {
  return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 : v < 10000000u ? 7 : v < 100000000u ? 8
         : v < 1000000000u ? 9 : 10;
}
__device__ inline uint32_t ndigits(uint64_t v, uint32_t nd = 1) {  // nd: what the first digit counts as (with it a sign, a fraction)
  for (uint64_t t = div10(v); t; t = div10(t)) ++nd;
  return nd;
}
// WRITE == false: only counts (a stage's length kernel and its format kernel share one definition of a line)
template <bool WRITE>
struct LineOut {
  char *p;
  uint32_t n;
  __device__ void ch(char c) {
    if (WRITE) p[n] = c;
    ++n;
  }
  __device__ void u32(uint32_t v, uint32_t min_digits = 1) {
    const uint32_t nd = max(ndigits(v), min_digits);
    if (WRITE)
      for (uint32_t k = nd; k-- > 0;) {
        const uint32_t q = div10(v);
        p[n + k] = (char)('0' + (v - q * 10u));
        v = q;
      }
    n += nd;
  }
  __device__ void u64(uint64_t v) {
    const uint32_t nd = ndigits(v);
    if (WRITE)
      for (uint32_t k = nd; k-- > 0;) {
        const uint64_t q = div10(v);
        p[n + k] = (char)('0' + (uint32_t)(v - q * 10u));
        v = q;
      }
    n += nd;
  }
  __device__ void i32(int32_t v) {  // %d
    if (v < 0) ch('-'), u32(0u - (uint32_t)v);
    else u32((uint32_t)v);
  }
  __device__ void i64(int64_t v) {  // %d of an int64
    if (v < 0) ch('-'), u64(0ULL - (uint64_t)v);
    else u64((uint64_t)v);
  }
  __device__ void i64(int64_t v, uint32_t width) {  // %<width>d: blanks in front, the sign counts
    const bool neg = v < 0;
    const uint64_t a = neg ? 0ULL - (uint64_t)v : (uint64_t)v;
    for (uint32_t nd = ndigits(a, neg ? 2 : 1); nd < width; ++nd) ch(' ');
    if (neg) ch('-');
    u64(a);
  }
  __device__ void rid(int32_t v) {  // %09d: zero padding to width 9, the sign counts
    if (v < 0) ch('-'), u32(0u - (uint32_t)v, 8);
    else u32((uint32_t)v, 9);
  }
  __device__ void node(uint32_t r, uint32_t end) {  // a node's name, "%09d:E" or "%09d:B"
    rid((int32_t)r), ch(':'), ch(end ? 'E' : 'B');
  }
  // %0.1f of a finite double: the EXACT binary value M * 2^e rounded to one decimal, ties to even, in integer arithmetic
  __device__ void f1(double x) {
    const uint64_t bits = (uint64_t)__double_as_longlong(x);
    if (bits >> 63) ch('-');  // also for a value that rounds to 0.0: "-0.0"
    const uint32_t ex = (uint32_t)(bits >> 52) & 0x7FFu;
    uint64_t M = bits & ((1ULL << 52) - 1);
    int e = -1074;
    if (ex) M |= 1ULL << 52, e = (int)ex - 1075;
    const uint64_t m10 = M * 10u;  // < 2^57; tenths = m10 * 2^e
    uint64_t t;
    if (e >= 0) {
      t = m10 << min(e, 6);  // (not reached: |err_est| < 2^38, so e <= -15)
    } else if (-e >= 58) {
      t = 0;  // m10 < 2^57 <= half a unit
    } else {
      const int s = -e;
      t = m10 >> s;
      const uint64_t rem = m10 & ((1ULL << s) - 1), half = 1ULL << (s - 1);
      if (rem > half || (rem == half && (t & 1))) ++t;
    }
    const uint64_t whole = div10(t);
    u64(whole);
    ch('.');
    ch((char)('0' + (uint32_t)(t - whole * 10u)));
  }
};

// The stream-out of a format kernel: a workgroup of THREADS threads has formatted a tile of text into LDS and now writes it to global
// memory with 16-byte stores.  The contract:
//   * g is 16-byte aligned, and so is tile;
//   * g[k] corresponds to tile[k] for k in [lo, hi) -- the tile sits in LDS at the global address's offset within 16 bytes, so the
//     aligned chunks line up on both sides;
//   * bytes outside [lo, hi) are not touched: the head and tail bytes that share a 16-byte chunk with the neighbouring tiles go out
//     byte by byte;
//   * the caller has passed its barrier (the whole tile is written).
template <uint32_t THREADS>
__device__ inline void tile_out(const char *tile, char *g, uint32_t lo, uint32_t hi) {
  const uint32_t body_lo = min(hi, (lo + 15u) & ~15u), body_hi = max(body_lo, hi & ~15u);
  for (uint32_t k = lo + threadIdx.x; k < body_lo; k += THREADS) g[k] = tile[k];
  for (uint32_t k = body_lo + threadIdx.x * 16u; k < body_hi; k += THREADS * 16u)
    *reinterpret_cast<uint4 *>(g + k) = *reinterpret_cast<const uint4 *>(tile + k);
  for (uint32_t k = body_hi + threadIdx.x; k < hi; k += THREADS) g[k] = tile[k];
}

// ---- the host side of an entry point that hands text out ---------------------------------------------------------------------------------
// Device text on its way to host memory: two pinned buffers, the copy of one piece runs while the host moves the last.  Owned by whoever
// hands out text (a dedup stream, a string graph, the unitigs); made at the first download.
struct TextStage {
  char *pin[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  void drop();   // frees the buffers and events (idempotent)
};
void text_download(TextStage &ts, const char *d_text, size_t total, char *dst);
// `total` bytes of device text as the caller's text (pgx_free), through ts; total == 0: the empty text, and nothing is downloaded
void text_hand_out(TextStage &ts, const char *d_text, size_t total, char **text, size_t *text_len);

// lines per call at most (the longest, dedup's: < 2.4 GB of text)
constexpr uint64_t TEXT_MAX_LINES = 1ULL << 24;
inline uint64_t text_lines(uint64_t max_lines, uint64_t left) { return std::min<uint64_t>({max_lines, left, TEXT_MAX_LINES}); }

// The epilogue of the entry points that hand out text: guarded(), and after an error the call's text is freed (*text was cleared before
// anything could throw: what it holds now is this call's own allocation).  done: nullptr where the entry point has none.
template <class F>
int text_call(char **text, size_t *text_len, int *done, F &&body) {
  if (text) *text = nullptr;   // the outputs first: the caller's variables may hold anything, and the error paths free only what
  if (text_len) *text_len = 0;  // this call put there
  if (done) *done = 0;
  const int rc = guarded(body);
  if (rc != PGX_OK) {
    if (text && *text) free(*text), *text = nullptr;
    if (text_len) *text_len = 0;
  }
  return rc;
}

// ---- tiles of bytes over pieces -------------------------------------------------------------------------------------------------------
// A text is a sequence of pieces: piece j occupies the bytes [poff[j], poff[j + 1]) of the whole file.  A line starts at the first byte
// of some piece (a line is one piece or several).  No piece is longer than its source's bound.
// A piece source is a trivially copyable struct that goes to the kernels by value and supplies
//   uint32_t n                                                       the number of pieces
//   static constexpr uint32_t MAX                                    an upper bound of a piece's length, a multiple of 16
//   template <bool WRITE> __device__ uint32_t piece(j, dst) const    prints piece j through LineOut<WRITE>, returns its length
constexpr uint32_t TEXT_TILE = 8192, TEXT_THREADS = 256;
template <class Src>
__global__ void k_piece_len(Src src, uint32_t *__restrict__ len) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < src.n) len[j] = src.template piece<false>(j, nullptr);
}
template <class Index>
__global__ void k_line_off(const Index *__restrict__ first_piece, const uint64_t *__restrict__ poff, uint32_t n_lines, uint64_t *__restrict__ line_off) {
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l <= n_lines) line_off[l] = poff[first_piece[l]];
}
// A workgroup per tile of TEXT_TILE output bytes: text[t * TEXT_TILE ..) holds the characters base + t * TEXT_TILE .. of the whole file.
// The pieces that cover the tile are found by binary search of the pieces' offsets (as k_stitch finds its segments); each is formatted
// whole into LDS, which has Src::MAX bytes of margin on either side for the pieces that straddle the tile's ends, and the tile streams
// out (tile_out from its byte 0: text is 16-byte aligned, TEXT_TILE and Src::MAX are multiples of 16).
template <class Src>
__global__ __launch_bounds__(TEXT_THREADS) void k_piece_format(Src src, const uint64_t *__restrict__ poff, uint64_t base, uint64_t total, char *__restrict__ text) {
  static_assert(Src::MAX % 16 == 0, "the margin keeps the tile 16-byte aligned in LDS");
  __shared__ __attribute__((aligned(16))) char tile[Src::MAX + TEXT_TILE + Src::MAX];
  const uint64_t t0 = (uint64_t)blockIdx.x * TEXT_TILE, lo = base + t0, hi = base + min(total, t0 + TEXT_TILE);
  // the last piece that starts at or before lo (poff[0 .. n] ascending, poff[n] > lo)
  uint32_t a = 0, b = src.n;
  while (a < b) {
    const uint32_t mid = a + ((b - a) >> 1);
    if (poff[mid + 1] <= lo) a = mid + 1;
    else b = mid;
  }
  for (uint32_t j = a + threadIdx.x; j < src.n; j += TEXT_THREADS) {
    const uint64_t at = poff[j];
    if (at >= hi) break;
    src.template piece<true>(j, tile + Src::MAX + (int64_t)(at - lo));   // (at - lo > -Src::MAX: the piece reaches past lo)
  }
  __syncthreads();
  tile_out<TEXT_THREADS>(tile + Src::MAX, text + t0, 0, (uint32_t)(hi - lo));
}

// a text whose pieces and lines are laid out: where each starts in the whole file, and how many lines have been handed out
struct TextPlan {
  DevBuf<uint64_t> poff, line_off;   // pieces + 1; lines + 1, or none where every piece is a line
  uint64_t n_lines = 0, cursor = 0;
  const uint64_t *line_offs() const { return line_off.p ? line_off.p : poff.p; }
  void release() { poff.release(), line_off.release(); }
};
// lays a text out: the lengths of its pieces, their scan, the lines' offsets.  d_first_piece: lines + 1 entries, the first piece of each
// line and the number of pieces behind the last; a typed nullptr where every piece is a line.  No piece: no launch, poff[0] = 0.
template <class Src, class Index>
void plan_text(const Src &src, const Index *d_first_piece, uint64_t n_lines, TextPlan *plan, PrimWs *tmp) {
  hipStream_t st = ctx().stream;
  plan->n_lines = n_lines, plan->cursor = 0;
  plan->poff.alloc((size_t)src.n + 1);
  DevBuf<uint32_t> plen(src.n);
  if (src.n) LAUNCH(k_piece_len<Src>, src.n, src, plen.p);
  (void)scan_to_total(plen.p, plan->poff.p, src.n, tmp);
  if (d_first_piece) {
    plan->line_off.alloc(n_lines + 1);
    LAUNCH(k_line_off<Index>, n_lines + 1, d_first_piece, plan->poff.p, (uint32_t)n_lines, plan->line_off.p);
  }
  PGX_HIP(hipGetLastError());
}
// what a stage calls its timers (the stage's total, its text), its MemTag and the workspace its text is formatted into
struct TextNames {
  const char *stage, *text, *tag, *ws;
};
// The body of an entry point that hands out the next lines of a planned text, [cursor, cursor + max_lines), inside text_call: two offsets
// come down, the tiles between them are formatted and handed out through `stage`; *done when the last line has left.
template <class Src>
void text_next(const char *who, TextPlan &plan, const Src &src, TextStage &stage, const TextNames &names, uint64_t max_lines, char **text, size_t *text_len, int *done) {
  PGX_REQUIRE(text && text_len && done && max_lines, PGX_EARG, "%s: null argument or max_lines == 0", who);
  hipStream_t st = ctx().stream;
  const uint64_t nl = text_lines(max_lines, plan.n_lines - plan.cursor);
  if (nl == 0) {
    text_hand_out(stage, nullptr, 0, text, text_len);
  } else {
    KernelTimer tm(names.stage, nl), tm_text(names.text, nl);
    MemTag tag(names.tag);
    uint64_t range[2];
    PGX_HIP(hipMemcpyAsync(&range[0], plan.line_offs() + plan.cursor, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    PGX_HIP(hipMemcpyAsync(&range[1], plan.line_offs() + plan.cursor + nl, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    pgx::sync();
    const uint64_t total = range[1] - range[0];
    char *d_text = ws<char>(names.ws, total + 16);
    hipLaunchKernelGGL(k_piece_format<Src>, dim3(cdiv(total, TEXT_TILE)), dim3(TEXT_THREADS), 0, st, src, plan.poff.p, range[0], total, d_text);
    PGX_HIP(hipGetLastError());
    text_hand_out(stage, d_text, total, text, text_len);
  }
  plan.cursor += nl;
  if (plan.cursor == plan.n_lines) *done = 1;
  timing_flush();
}
}  // namespace pgx
