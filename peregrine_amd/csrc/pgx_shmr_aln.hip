// pgx_shmr_aln.hip -- shmr_aln (src/shmr_align.c:21-160, direction 0) for a batch of list pairs: the shared shimmers of two lists chained
// into co-linear runs, chain for chain and element for element what the reference's serial walk leaves (the rule: DESIGN.md section 4.9).
//
//   index    one stable sort of (list, x >> 8) over the pool of side 0: list l's occurrences of a hash lie together in skey / sidx
//            [off0[l], off0[l + 1]), in ascending position of the list.  Pairs that share a list 0 share its index.
//   bound    k_aln_bound: per pair the sum over list 1 of the occurrence counts of the hashes the skip rule lets through -- at least its
//            candidates, so at least its chains and its chain elements.  A scan of the bounds gives every pair its slice of the state and
//            element arrays.
//   walk     k_aln_walk: a wavefront per pair.  64 shimmers of list 1 are looked up at once (a lane each, binary search); the ones the
//            skip rule keeps are then taken in order.  Per candidate the lanes stride over the chains opened so far, a wavefront
//            reduction takes the minimum of (diff, chain) -- the first chain among the smallest diff -- and lane 0 appends.  The first
//            lds_cap chains keep their state in LDS, the others in the pair's slice (PGX_SHMR_ALN_LDS shrinks the first, a test hook).
//            Elements are (idx0, idx1, the chain's previous element).
//   unroll   k_aln_lens, k_aln_unroll: the linked elements as CSR -- chains per pair, elements per chain, idx0[], idx1[].
// Nothing is decided by the order in which atomics land: there are none.
#include <algorithm>

#include "pgx_internal.h"

namespace pgx {
namespace {

constexpr uint32_t ALN_MAX_SMALL = 4800;   // MAX_SMALL_ALNS (src/shmr_align.c:19)
constexpr uint32_t ALN_LDS_CHAINS = 1024;  // chains whose state a wavefront keeps in LDS (5 words each: 20 KiB a block)
constexpr uint32_t ALN_NONE = 0xFFFFFFFFu;

using AlnPair = pgx_shmr_aln_pair;

__device__ __forceinline__ uint32_t mm_pos(uint64_t y) { return (uint32_t)(y & 0xFFFFFFFFull) >> 1; }
__device__ __forceinline__ uint32_t abs_diff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }   // of two values below 2^31

// list_of[i] = the list that holds element order[i] of the pool (the second, stable sort's key)
__global__ void k_aln_list_of(const uint64_t *__restrict__ off, uint32_t n_lists, const uint32_t *__restrict__ order, uint64_t n,
                              uint32_t *__restrict__ list_of) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t g = order[i];
  uint32_t lo = 0, hi = n_lists;   // the last l with off[l] <= g (off[n_lists] = n > g; empty lists before it share its offset)
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= g) lo = mid;
    else hi = mid;
  }
  list_of[i] = lo;
}
__global__ void k_aln_hash_key(const pgx_mm128 *__restrict__ mm, uint64_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ val) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  key[i] = mm[i].x >> 8;
  val[i] = (uint32_t)i;
}
// after both sorts: the hash and the position IN ITS LIST of the element at every sorted place
__global__ void k_aln_sorted(const pgx_mm128 *__restrict__ mm, const uint32_t *__restrict__ order, const uint32_t *__restrict__ list_sorted,
                             const uint64_t *__restrict__ off, uint64_t n, uint64_t *__restrict__ skey, uint32_t *__restrict__ sidx) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t g = order[i];
  skey[i] = mm[g].x >> 8;
  sidx[i] = (uint32_t)(g - off[list_sorted[i]]);
}

// the occurrences of hash h in the sorted keys [0, n): first place and count
__device__ __forceinline__ void aln_lookup(const uint64_t *__restrict__ skey, uint32_t n, uint64_t h, uint32_t &first, uint32_t &cnt) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (skey[mid] < h) lo = mid + 1;
    else hi = mid;
  }
  first = lo;
  hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (skey[mid] <= h) lo = mid + 1;
    else hi = mid;
  }
  cnt = lo - first;
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
  for (int d = 32; d; d >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
    v += (uint64_t)hi << 32 | lo;
  }
  return v;
}
__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
  for (int d = 32; d; d >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
    const uint64_t o = (uint64_t)hi << 32 | lo;
    v = o < v ? o : v;
  }
  return v;
}

// bound[p] = the occurrences in list 0 of the shimmers of list 1 that the skip rule keeps (a wavefront per pair)
__global__ __launch_bounds__(64) void k_aln_bound(const AlnPair *__restrict__ pairs, uint32_t n_pairs, const uint64_t *__restrict__ off0,
                                                  const uint64_t *__restrict__ off1, const pgx_mm128 *__restrict__ mm1,
                                                  const uint64_t *__restrict__ skey, uint32_t max_repeat, uint64_t *__restrict__ bound) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t p = blockIdx.x; p < n_pairs; p += gridDim.x) {
    const AlnPair pr = pairs[p];
    const uint64_t b0 = off0[pr.list0], b1 = off1[pr.list1];
    const uint32_t n0 = (uint32_t)(off0[pr.list0 + 1] - b0), n1 = (uint32_t)(off1[pr.list1 + 1] - b1);
    uint64_t sum = 0;
    if (n0)
      for (uint32_t s = lane; s < n1; s += 64) {
        uint32_t first, cnt;
        aln_lookup(skey + b0, n0, mm1[b1 + s].x >> 8, first, cnt);
        if (cnt && cnt <= max_repeat) sum += cnt;
      }
    sum = wave_sum(sum);
    if (lane == 0) bound[p] = sum;
  }
}

// The walk.  Per pair: its chains' state at st[cbase ..] / tail[cbase ..] (of the first lds_cap chains only when the pair is done),
// its elements at e_idx0 / e_idx1 / e_prev [cbase ..] (a candidate is at most one chain and exactly one element: one base serves both),
// n_chain[p], stopped[p] = the walk ended at the small-chain count.
__global__ __launch_bounds__(64) void k_aln_walk(const AlnPair *__restrict__ pairs, uint32_t n_pairs, const uint64_t *__restrict__ off0,
                                                 const uint64_t *__restrict__ off1, const pgx_mm128 *__restrict__ mm0,
                                                 const pgx_mm128 *__restrict__ mm1, const uint64_t *__restrict__ skey,
                                                 const uint32_t *__restrict__ sidx, const uint64_t *__restrict__ base, uint32_t max_diff,
                                                 uint32_t max_dist, uint32_t max_repeat, uint32_t lds_cap, uint4 *st, uint32_t *tail,
                                                 uint32_t *e_idx0, uint32_t *e_idx1, uint32_t *e_prev, uint32_t *__restrict__ n_chain,
                                                 uint32_t *__restrict__ stopped) {
  __shared__ uint32_t s_i0[ALN_LDS_CHAINS], s_p0[ALN_LDS_CHAINS], s_d[ALN_LDS_CHAINS], s_len[ALN_LDS_CHAINS], s_tail[ALN_LDS_CHAINS];
  const uint32_t lane = threadIdx.x;
  for (uint32_t p = blockIdx.x; p < n_pairs; p += gridDim.x) {
    const AlnPair pr = pairs[p];
    const uint64_t b0 = off0[pr.list0], b1 = off1[pr.list1], cb = base[p];
    const uint32_t n0 = (uint32_t)(off0[pr.list0 + 1] - b0), n1 = (uint32_t)(off1[pr.list1 + 1] - b1);
    const uint32_t cap = (uint32_t)(base[p + 1] - cb);   // the pair's slice: chains and elements stay below it
    const uint64_t *key0 = skey + b0;
    const uint32_t *idx0 = sidx + b0;
    uint4 *g_st = st + cb;
    uint32_t *g_tail = tail + cb, *g_e0 = e_idx0 + cb, *g_e1 = e_idx1 + cb, *g_ep = e_prev + cb;
    uint32_t nch = 0, nel = 0, small = 0, last_small = 0;
    bool stop = false;
    for (uint32_t s0 = 0; s0 < n1 && n0 && !stop; s0 += 64) {
      // 64 lookups at once; a kept shimmer's first occurrence is fetched with it
      const uint32_t sl = s0 + lane;
      uint32_t first = 0, cnt = 0, f_i0 = 0;
      uint64_t y1 = 0, f_y0 = 0;
      if (sl < n1) {
        const pgx_mm128 m = mm1[b1 + sl];
        y1 = m.y;
        aln_lookup(key0, n0, m.x >> 8, first, cnt);
        if (cnt > max_repeat) cnt = 0;
        if (cnt) f_i0 = idx0[first], f_y0 = mm0[b0 + f_i0].y;
      }
      unsigned long long todo = __ballot(cnt != 0);
      while (todo && !stop) {
        const int j = __ffsll(todo) - 1;
        todo &= todo - 1;
        const uint32_t s = s0 + (uint32_t)j;
        const uint32_t c_first = __shfl(first, j, 64), c_cnt = __shfl(cnt, j, 64);
        const uint64_t c_y1 = (uint64_t)__shfl((uint32_t)(y1 >> 32), j, 64) << 32 | __shfl((uint32_t)y1, j, 64);
        const uint32_t pos1 = mm_pos(c_y1);
        for (uint32_t i = 0; i < c_cnt; ++i) {
          uint32_t i0;
          uint64_t y0;
          if (i == 0) {
            i0 = __shfl(f_i0, j, 64);
            y0 = (uint64_t)__shfl((uint32_t)(f_y0 >> 32), j, 64) << 32 | __shfl((uint32_t)f_y0, j, 64);
          } else {
            i0 = idx0[c_first + i];
            y0 = mm0[b0 + i0].y;
          }
          if ((y0 & 1) != (c_y1 & 1)) continue;
          const uint32_t pos0 = mm_pos(y0), delta0 = abs_diff(pos0, pos1);
          // the scan: every chain opened so far, the smallest (diff, chain) among those that qualify
          uint64_t best = ~0ull;
          for (uint32_t c = lane; c < nch; c += 64) {
            uint32_t li0, lp0, ld;
            if (c < lds_cap) li0 = s_i0[c], lp0 = s_p0[c], ld = s_d[c];
            else {
              const uint4 v = g_st[c];
              li0 = v.x, lp0 = v.y, ld = v.z;
            }
            const uint32_t diff = abs_diff(delta0, ld);
            if (i0 >= li0 && abs_diff(pos0, lp0) < max_dist && diff < max_diff) {
              const uint64_t k = (uint64_t)diff << 32 | c;
              best = k < best ? k : best;
            }
          }
          if (__ballot(best != ~0ull)) best = wave_min(best);
          last_small = small;   // counted before this scan's append
          if (nel < cap) {      // (the bound holds: this only keeps a wrong bound from writing past the slice)
            uint32_t c, len, prev;
            if (best != ~0ull) {
              c = (uint32_t)best;
              len = (c < lds_cap ? s_len[c] : g_st[c].w) + 1;
              prev = c < lds_cap ? s_tail[c] : g_tail[c];
              if (len == 3) --small;
            } else {
              c = nch++, len = 1, prev = ALN_NONE;
              ++small;
            }
            if (lane == 0) {
              if (c < lds_cap) s_i0[c] = i0, s_p0[c] = pos0, s_d[c] = delta0, s_len[c] = len, s_tail[c] = nel;
              else g_st[c] = make_uint4(i0, pos0, delta0, len), g_tail[c] = nel;
              g_e0[nel] = i0, g_e1[nel] = s, g_ep[nel] = prev;
            }
            ++nel;
            __syncthreads();   // one wavefront: the append is in LDS / on its way to memory before the next scan reads
          }
        }
        if (last_small > ALN_MAX_SMALL) stop = true;   // after the shimmer, as the reference tests it
      }
    }
    // the head of the state joins the rest for the unroll
    const uint32_t head = nch < lds_cap ? nch : lds_cap;
    for (uint32_t c = lane; c < head; c += 64) g_st[c] = make_uint4(s_i0[c], s_p0[c], s_d[c], s_len[c]), g_tail[c] = s_tail[c];
    if (lane == 0) n_chain[p] = nch, stopped[p] = stop ? 1u : 0u;
    __syncthreads();   // the next pair's appends come behind this pair's reads of LDS
  }
}

// len_out[pair_off[p] + c] = the length of pair p's chain c (a wavefront per pair)
__global__ __launch_bounds__(64) void k_aln_lens(uint32_t n_pairs, const uint64_t *__restrict__ base, const uint64_t *__restrict__ pair_off,
                                                 const uint4 *__restrict__ st, uint32_t *__restrict__ len_out) {
  for (uint32_t p = blockIdx.x; p < n_pairs; p += gridDim.x) {
    const uint64_t o = pair_off[p];
    const uint32_t nch = (uint32_t)(pair_off[p + 1] - o);
    for (uint32_t c = threadIdx.x; c < nch; c += 64) len_out[o + c] = st[base[p] + c].w;
  }
}
// a lane per chain walks it back from its tail into its place of idx0[] / idx1[]
__global__ __launch_bounds__(64) void k_aln_unroll(uint32_t n_pairs, const uint64_t *__restrict__ base, const uint64_t *__restrict__ pair_off,
                                                   const uint64_t *__restrict__ chain_off, const uint32_t *__restrict__ tail,
                                                   const uint32_t *__restrict__ e_idx0, const uint32_t *__restrict__ e_idx1,
                                                   const uint32_t *__restrict__ e_prev, uint32_t *__restrict__ out0, uint32_t *__restrict__ out1) {
  for (uint32_t p = blockIdx.x; p < n_pairs; p += gridDim.x) {
    const uint64_t o = pair_off[p], cb = base[p];
    const uint32_t nch = (uint32_t)(pair_off[p + 1] - o), cap = (uint32_t)(base[p + 1] - cb);
    for (uint32_t c = threadIdx.x; c < nch; c += 64) {
      const uint64_t a = chain_off[o + c];
      uint64_t k = chain_off[o + c + 1];
      uint32_t e = tail[cb + c];
      while (k > a && e < cap) {   // (e < cap: ALN_NONE ends a chain; nothing is read past the slice)
        --k;
        out0[k] = e_idx0[cb + e], out1[k] = e_idx1[cb + e];
        e = e_prev[cb + e];
      }
    }
  }
}

uint32_t lds_chains() {   // PGX_SHMR_ALN_LDS: a test hook that shrinks the LDS head of the chain state so that small inputs reach the slice
  const char *v = getenv("PGX_SHMR_ALN_LDS");
  const long c = v ? atol(v) : (long)ALN_LDS_CHAINS;
  return (uint32_t)std::min<long>(std::max<long>(c, 0), (long)ALN_LDS_CHAINS);
}

// the four arrays for the caller; after a failure none is left
struct AlnOut {
  uint64_t *pair_off = nullptr, *chain_off = nullptr;
  uint32_t *idx0 = nullptr, *idx1 = nullptr;
  void alloc(size_t n_pairs, size_t n_chains, size_t n_elems) {
    pair_off = (uint64_t *)out_alloc((n_pairs + 1) * sizeof(uint64_t));
    chain_off = (uint64_t *)out_alloc((n_chains + 1) * sizeof(uint64_t));
    idx0 = (uint32_t *)out_alloc(n_elems ? n_elems * sizeof(uint32_t) : 1);
    idx1 = (uint32_t *)out_alloc(n_elems ? n_elems * sizeof(uint32_t) : 1);
  }
  void release() { pair_off = chain_off = nullptr, idx0 = idx1 = nullptr; }
  ~AlnOut() { out_free(pair_off), out_free(chain_off), out_free(idx0), out_free(idx1); }
};

void shmr_aln_dev(const char *who, const pgx_mm128 *mm0, const uint64_t *off0, size_t n_lists0, const pgx_mm128 *mm1, const uint64_t *off1,
                  size_t n_lists1, const pgx_shmr_aln_pair *pairs, size_t n_pairs, uint32_t max_diff, uint32_t max_dist, uint32_t max_repeat,
                  AlnOut &out, pgx_shmr_aln_stats &stats) {
  hipStream_t st = ctx().stream;
  const uint64_t n0 = off0[n_lists0], n1 = off1[n_lists1];
  const uint32_t np = (uint32_t)n_pairs, grid = stride_grid(n_pairs, 8);   // one grid for the four persistent kernels
  PrimWs ws;
  const double t0 = wall_ms();
  DevBuf<pgx_mm128> d_mm0(n0 ? n0 : 1), d_mm1(n1 ? n1 : 1);
  DevBuf<uint64_t> d_off0(n_lists0 + 1), d_off1(n_lists1 + 1);
  DevBuf<AlnPair> d_pairs(n_pairs);
  d_mm0.upload(mm0, n0), d_mm1.upload(mm1, n1);
  d_off0.upload(off0, n_lists0 + 1), d_off1.upload(off1, n_lists1 + 1);
  d_pairs.upload(pairs, n_pairs);
  // ---- the index of side 0: stable by hash, then stable by list
  DevBuf<uint64_t> skey(n0 ? n0 : 1);
  DevBuf<uint32_t> sidx(n0 ? n0 : 1);
  if (n0) {
    DevBuf<uint64_t> key(n0), key_s(n0);
    DevBuf<uint32_t> val(n0), by_hash(n0), list_in(n0), list_s(n0), order(n0);
    LAUNCH(k_aln_hash_key, n0, d_mm0.p, n0, key.p, val.p);
    sort_pairs(key.p, key_s.p, val.p, by_hash.p, n0, 0, 56, &ws);
    LAUNCH(k_aln_list_of, n0, d_off0.p, (uint32_t)n_lists0, by_hash.p, n0, list_in.p);
    int bits = 1;
    while (bits < 32 && (1ull << bits) < n_lists0) ++bits;
    sort_pairs(list_in.p, list_s.p, by_hash.p, order.p, n0, 0, bits, &ws);
    LAUNCH(k_aln_sorted, n0, d_mm0.p, order.p, list_s.p, d_off0.p, n0, skey.p, sidx.p);
  }
  sync();
  const double t1 = wall_ms();
  // ---- bounds and slices
  DevBuf<uint64_t> bound(n_pairs), base(n_pairs + 1);
  hipLaunchKernelGGL(k_aln_bound, dim3(grid), dim3(64), 0, st, d_pairs.p, np, d_off0.p, d_off1.p, d_mm1.p, skey.p, max_repeat, bound.p);
  const uint64_t total = scan_to_total(bound.p, base.p, n_pairs, &ws);
  PGX_REQUIRE(total < (1ull << 32), PGX_ENOMEM, "%s: no device memory for the chain state of %llu candidates", who, (unsigned long long)total);
  stats.n_candidates = total;
  const size_t ne = total ? total : 1;
  DevBuf<uint4> state(ne);
  DevBuf<uint32_t> tail(ne), e0(ne), e1(ne), ep(ne), n_chain(n_pairs), stopped(n_pairs), n_stopped(1);
  // ---- the walk
  hipLaunchKernelGGL(k_aln_walk, dim3(grid), dim3(64), 0, st, d_pairs.p, np, d_off0.p, d_off1.p, d_mm0.p, d_mm1.p, skey.p, sidx.p, base.p, max_diff, max_dist,
                     max_repeat, lds_chains(), state.p, tail.p, e0.p, e1.p, ep.p, n_chain.p, stopped.p);
  sync();
  const double t2 = wall_ms();
  // ---- CSR
  DevBuf<uint64_t> pair_off(n_pairs + 1);
  const uint64_t n_chains = scan_to_total(n_chain.p, pair_off.p, n_pairs, &ws);
  DevBuf<uint32_t> len(n_chains ? n_chains : 1);
  DevBuf<uint64_t> chain_off(n_chains + 1);
  hipLaunchKernelGGL(k_aln_lens, dim3(grid), dim3(64), 0, st, np, base.p, pair_off.p, state.p, len.p);
  const uint64_t n_elems = scan_to_total(len.p, chain_off.p, n_chains, &ws);
  PGX_REQUIRE(n_elems <= total, PGX_EHIP, "%s: %llu chain elements from %llu candidates", who, (unsigned long long)n_elems, (unsigned long long)total);
  DevBuf<uint32_t> o0(n_elems ? n_elems : 1), o1(n_elems ? n_elems : 1);
  hipLaunchKernelGGL(k_aln_unroll, dim3(grid), dim3(64), 0, st, np, base.p, pair_off.p, chain_off.p, tail.p, e0.p, e1.p, ep.p, o0.p, o1.p);
  reduce_sum(stopped.p, n_stopped.p, n_pairs, &ws);
  out.alloc(n_pairs, n_chains, n_elems);
  uint32_t h_stopped = 0;
  pair_off.download(out.pair_off, n_pairs + 1);
  chain_off.download(out.chain_off, n_chains + 1);
  o0.download(out.idx0, n_elems), o1.download(out.idx1, n_elems);
  n_stopped.download(&h_stopped, 1);
  sync();
  const double t3 = wall_ms();
  stats.n_chains = n_chains, stats.n_elems = n_elems, stats.n_stopped = h_stopped;
  stats.index_ms = t1 - t0, stats.walk_ms = t2 - t1, stats.unroll_ms = t3 - t2, stats.gpu_ms = t3 - t0;
}

}  // namespace
}  // namespace pgx

using namespace pgx;

extern "C" int pgx_shmr_aln_batch(const pgx_mm128 *mm0, const uint64_t *off0, size_t n_lists0, const pgx_mm128 *mm1, const uint64_t *off1, size_t n_lists1,
                                  const pgx_shmr_aln_pair *pairs, size_t n_pairs, uint8_t direction, uint32_t max_diff, uint32_t max_dist, uint32_t max_repeat,
                                  uint64_t **pair_off, uint64_t **chain_off, uint32_t **idx0, uint32_t **idx1, pgx_shmr_aln_stats *stats) {
  return guarded([&]() -> int {
    const char *who = "pgx_shmr_aln_batch";
    PGX_REQUIRE(ctx().ready, PGX_ESTATE, "%s: no device context (pgx_init has not been called, or found no HIP device)", who);
    PGX_REQUIRE(pair_off && chain_off && idx0 && idx1 && off0 && off1 && (n_pairs == 0 || pairs), PGX_EARG, "%s: null argument", who);
    PGX_REQUIRE((off0[n_lists0] == off0[0] || mm0) && (off1[n_lists1] == off1[0] || mm1), PGX_EARG, "%s: null argument", who);
    PGX_REQUIRE(direction == 0, PGX_EARG,
                "%s: direction %u is refused: the reference's reversed walk starts by reading mmers1->a[n], one past the list "
                "(src/shmr_align.c:65-69), so it has no answer to reproduce; only direction 0 is offered",
                who, (unsigned)direction);
    PGX_REQUIRE(n_pairs < (1ull << 31) && n_lists0 < (1ull << 32) && n_lists1 < (1ull << 32), PGX_EARG, "%s: too many pairs or lists for one call", who);
    for (int side = 0; side < 2; ++side) {
      const uint64_t *off = side ? off1 : off0;
      const size_t nl = side ? n_lists1 : n_lists0;
      PGX_REQUIRE(off[0] == 0, PGX_EARG, "%s: the offsets of side %d do not start at 0", who, side);
      for (size_t l = 0; l < nl; ++l) {
        PGX_REQUIRE(off[l] <= off[l + 1], PGX_EARG, "%s: the offsets of side %d decrease at list %zu", who, side, l);
        PGX_REQUIRE(off[l + 1] - off[l] < (1ull << 31), PGX_EARG, "%s: list %zu of side %d has 2^31 entries or more", who, l, side);
      }
      PGX_REQUIRE(off[nl] < (1ull << 31), PGX_EARG, "%s: the lists of side %d hold 2^31 entries or more together", who, side);
    }
    for (size_t p = 0; p < n_pairs; ++p)
      PGX_REQUIRE(pairs[p].list0 < n_lists0 && pairs[p].list1 < n_lists1, PGX_EARG, "%s: pair %zu (%u, %u) names a list out of range (%zu, %zu lists)", who, p,
                  pairs[p].list0, pairs[p].list1, n_lists0, n_lists1);
    pgx_shmr_aln_stats s = {};
    s.n_pairs = n_pairs, s.n_lists0 = n_lists0;
    AlnOut out;
    if (n_pairs == 0) {
      out.alloc(0, 0, 0);
      out.pair_off[0] = out.chain_off[0] = 0;
    } else {
      MemTag mem_tag("shmr_aln");
      try {
        shmr_aln_dev(who, mm0, off0, n_lists0, mm1, off1, n_lists1, pairs, n_pairs, max_diff, max_dist, max_repeat, out, s);
      } catch (const Fail &f) {
        return build_fail_code(f, who, "chain state", s.n_candidates, "candidates");
      }
    }
    *pair_off = out.pair_off, *chain_off = out.chain_off, *idx0 = out.idx0, *idx1 = out.idx1;
    out.release();
    if (stats) *stats = s;
    return PGX_OK;
  });
}
