// pgx_dedup_rows.h -- what pgx_dedup.hip shares with the stages that read a graph-mode stream's rows in HBM (pgx_sgraph.hip): the row,
// the stream, the pieces of a text line as glibc prints them, and the pinned staging that device text leaves through.
#pragma once
#include "pgx_internal.h"

namespace pgx {
// a line of the dedup text before it is printed (shmr_dedup.c:44-89: the coordinates already transformed)
struct Row {
  uint32_t rid0, rid1;
  int32_t m_size, dist;
  uint32_t a_bgn, a_end, rlen0, strand, b_bgn, b_end, rlen1, type;
};

// ---- text: "%d", "%09d", "%u", "%0.1f" as glibc prints them -------------------------------------------------------------------------------
__device__ inline uint32_t div10(uint32_t v) { return __umulhi(v, 0xCCCCCCCDu) >> 3; }
__device__ inline uint64_t div10(uint64_t v) { return __umul64hi(v, 0xCCCCCCCCCCCCCCCDULL) >> 3; }
__device__ inline uint32_t ndigits(uint32_t v) {
  return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 : v < 10000000u ? 7 : v < 100000000u ? 8
         : v < 1000000000u ? 9 : 10;
}
// WRITE == false: only counts (k_line_len and k_format share one definition of a line)
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
    uint32_t nd = 1;
    for (uint64_t t = div10(v); t; t = div10(t)) ++nd;
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
  __device__ void rid(int32_t v) {  // %09d: zero padding to width 9, the sign counts
    if (v < 0) ch('-'), u32(0u - (uint32_t)v, 8);
    else u32((uint32_t)v, 9);
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
// the three IEEE double operations of shmr_dedup.c:89-90 in that order, never contracted
__device__ inline double err_est_of(int32_t dist, int32_t m_size) {
#pragma clang fp contract(off)
  const double p = 100.0 * (double)dist;
  const double q = p / (double)m_size;
  return 100.0 - q;
}

// Device text on its way to host memory: two pinned buffers, the copy of one piece runs while the host moves the last.  Owned by whoever
// hands out text (a dedup stream, a string graph); made at the first download.
struct TextStage {
  char *pin[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  void drop();   // frees the buffers and events (idempotent)
};
void text_download(TextStage &ts, const char *d_text, size_t total, char *dst);
}  // namespace pgx

struct pgx_dedup_stream {
  pgx::DevBuf<unsigned long long> tab;   // the seen-pair set: cap slots + the word of the all-ones key; owned by the stream (MemTag "dedup")
  uint64_t cap = 0;
  uint64_t n_records = 0, n_unique = 0;
  bool failed = false;              // an entry point returned an error: only pgx_dedup_close is accepted
  bool shut = false;                // pgx_shutdown ran while the stream was open: its device state is gone
  pgx::TextStage stage;             // text staging (pinned), made at the first feed that has text
  // graph mode (pgx_dedup_open_graph): the lines wait in HBM as rows until the end of the stream says which reads are contained
  bool graph = false;
  bool draining = false;            // the first pgx_dedup_drain ran: the store holds exactly the kept lines' rows, no feed is accepted
  pgx::DevBuf<uint32_t> bits;            // contained reads, one bit per read id (MemTag "dedup"); bits.n words, a power of two
  pgx::DevBuf<pgx::Row> store;           // rows of the `overlap` lines between two unmarked reads, in stream order; store.n is the capacity
  uint64_t store_n = 0, drained = 0;   // rows held; rows handed out as text
  bool released = false;            // the last line was handed out and the store went back: nothing left for pgx_sgraph_build
};

namespace pgx {
// the end of a graph-mode stream: the store compacted against the final bitmap (sets s->draining; from then on feeds are refused)
void graph_compact(pgx_dedup_stream *s);
// a live graph's edge records on the device, in creation order with their final types (pgx_sgraph.hip; `who` names the caller in the
// error a freed context gives); what reads them runs on ctx().stream, behind the build
const pgx_sgraph_edge *sgraph_device_edges(const pgx_sgraph *g, const char *who, uint64_t *n);
}  // namespace pgx
