// pgx_gedges.h -- the G edges of a set of edge records, once, for the stages that walk the string graph (pgx_unitigs.hip, pgx_gfa.hip,
// pgx_tiling.hip): which records are G edges, their node keys, and the two sorted lists an edge or a node's edges are looked up in.
// G edges are numbered gi = 0 .. m-1 in record order (gsel[gi]: the record).  A node is its key (rid << 1) | end.
//   by_w   (wkey, gi) ascending                (a node's in-edges)
//   by_vw  (vkey, wkey, gi) ascending          (a node's out-edges; equal neighbours are duplicates; find_vw looks an edge up here)
// Both orders are stable: within equal keys the edges ascend by record index.
#pragma once
#include "pgx_dedup_rows.h"

namespace pgx {
constexpr uint32_t NONE = 0xFFFFFFFFu;

__device__ inline uint64_t vkey(const pgx_sgraph_edge &e) { return (uint64_t)e.v_rid << 1 | (e.v_end & 1u); }
__device__ inline uint64_t wkey(const pgx_sgraph_edge &e) { return (uint64_t)e.w_rid << 1 | (e.w_end & 1u); }
// the first i in [lo, hi] for which before(i) does not hold (it holds on a prefix of [lo, hi))
template <class Before>
__device__ inline uint32_t bisect(uint32_t lo, uint32_t hi, Before before) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (before(mid)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// the first i in [0, n] with a[i] >= x (a ascending)
__device__ inline uint32_t lower_bound(const uint64_t *__restrict__ a, uint32_t n, uint64_t x) {
  return bisect(0, n, [&](uint32_t i) { return a[i] < x; });
}
__device__ inline uint32_t lower_bound(const uint32_t *__restrict__ a, uint32_t n, uint32_t x) {
  return bisect(0, n, [&](uint32_t i) { return a[i] < x; });
}
// the last i in [0, n) with a[i] <= x (a ascending, a[0] <= x)
__device__ inline uint32_t last_le(const uint64_t *__restrict__ a, uint32_t n, uint64_t x) {
  const uint32_t lo = bisect(0, n, [&](uint32_t i) { return a[i] <= x; });
  return lo ? lo - 1 : 0;
}
// where edge (v, w) stands in by_vw (the first of its duplicates), NONE: no G edge joins the two
__device__ inline uint32_t find_vw(const uint64_t *__restrict__ sv, const uint64_t *__restrict__ sw, uint32_t m, uint64_t v, uint64_t w) {
  const uint32_t lo = bisect(0, m, [&](uint32_t i) { return sv[i] < v || (sv[i] == v && sw[i] < w); });
  return lo < m && sv[lo] == v && sw[lo] == w ? lo : NONE;
}

template <uint8_t TYPE>
__global__ void k_ge_flags(const pgx_sgraph_edge *__restrict__ edges, uint32_t n, uint8_t *__restrict__ flag) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) flag[e] = edges[e].type == TYPE;
}
// A stage's rule is a trivially copyable functor that goes to the kernel by value (as a piece source of pgx_text.h does): rule(e) says
// that G edge e breaks it, and err[0] = min(err[0], the record index of such an edge).  NoRule: err is not touched.
struct NoRule {
  __device__ bool operator()(const pgx_sgraph_edge &) const { return false; }
};
template <class Rule>
__global__ void k_ge_keys(const pgx_sgraph_edge *__restrict__ edges, const uint32_t *__restrict__ gsel, uint32_t m, uint64_t *__restrict__ vk,
                          uint64_t *__restrict__ wk, uint32_t *__restrict__ ids, Rule rule, uint32_t *__restrict__ err) {
  const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
  if (gi >= m) return;
  const pgx_sgraph_edge e = edges[gsel[gi]];
  vk[gi] = vkey(e), wk[gi] = wkey(e), ids[gi] = gi;
  if (rule(e)) atomicMin(err, gsel[gi]);
}
// by_vw's second key; DUPS: err[0] = min(err[0], the record index of an edge whose (v, w) an earlier edge has)
template <bool DUPS>
__global__ void k_ge_second(const uint64_t *__restrict__ sv, const uint32_t *__restrict__ out_e, const uint64_t *__restrict__ wk, const uint32_t *__restrict__ gsel,
                            uint32_t m, uint64_t *__restrict__ sw, uint32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint64_t w = wk[out_e[i]];
  sw[i] = w;
  if (DUPS && i && sv[i] == sv[i - 1] && w == wk[out_e[i - 1]]) atomicMin(err, gsel[out_e[i]]);   // (stable sorts: i is the later of the two)
}

// What a stage has asked for so far, on ctx().stream; nothing synchronises but select().  A stage releases the parts it is done with.
struct GEdges {
  const pgx_sgraph_edge *rec = nullptr;
  uint32_t m = 0;                 // G edges
  DevBuf<uint32_t> gsel;          // their record indices, ascending
  DevBuf<uint64_t> vk, wk;        // their keys, by G index
  DevBuf<uint32_t> ids;           // 0 .. m-1: what a sort by one of the keys carries along
  DevBuf<uint64_t> swk;           // by_w: the w keys sorted ...
  DevBuf<uint32_t> in_e;          // ... and the G index of every entry
  DevBuf<uint64_t> sv, sw;        // by_vw: the keys sorted ...
  DevBuf<uint32_t> out_e;         // ... and the G index of every entry

  void select(const pgx_sgraph_edge *edges, uint32_t n, PrimWs *tmp) {
    hipStream_t st = ctx().stream;
    rec = edges, m = 0;
    gsel.alloc(n);
    if (n == 0) return;
    DevBuf<uint8_t> flag(n);
    LAUNCH(k_ge_flags<PGX_SGRAPH_G>, n, edges, n, flag.p);
    m = select_indices(flag.p, n, gsel.p, tmp);
  }
  // err: see k_ge_keys
  template <class Rule>
  void keys(Rule rule, uint32_t *err) {
    hipStream_t st = ctx().stream;
    vk.alloc(m), wk.alloc(m), ids.alloc(m);
    if (m) LAUNCH(k_ge_keys<Rule>, m, rec, gsel.p, m, vk.p, wk.p, ids.p, rule, err);
  }
  void by_w(PrimWs *tmp) {
    swk.alloc(m), in_e.alloc(m);
    sort_pairs(wk.p, swk.p, ids.p, in_e.p, m, 0, 33, tmp);
  }
  // behind by_w(): a stable sort of the in-lists by v.  dup_err: nullptr, or see k_ge_second
  void by_vw(uint32_t *dup_err, PrimWs *tmp) {
    hipStream_t st = ctx().stream;
    sv.alloc(m), out_e.alloc(m);
    sort_order({{vk.p, 33}}, m, in_e.p, out_e.p, sv.p, tmp);
    sw.alloc(m);
    if (m && dup_err) LAUNCH(k_ge_second<true>, m, sv.p, out_e.p, wk.p, gsel.p, m, sw.p, dup_err);
    else if (m) LAUNCH(k_ge_second<false>, m, sv.p, out_e.p, wk.p, gsel.p, m, sw.p, dup_err);
  }
  void release_lists() { ids.release(), swk.release(), in_e.release(), sv.release(), sw.release(), out_e.release(); }
};
}  // namespace pgx
