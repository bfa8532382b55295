// pgx_text.h -- everything about device text, once: the pieces of a line as glibc prints them (LineOut), the stream-out of a tile of
// text from LDS (tile_out), the pinned staging that device text leaves through (TextStage), and the host side of an entry point that
// hands text out (text_call, text_hand_out).  Used by the stages that write their text on the device: pgx_dedup.hip, pgx_sgraph.hip,
// pgx_unitigs.hip.
#pragma once
#include <algorithm>

#include "pgx_internal.h"

namespace pgx {
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
}  // namespace pgx
