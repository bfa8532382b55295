// pgx_sgraph.hip -- the string graph: what generate_string_graph of the reference (py/scripts/ovlp_to_graph.py:658-905) does with
// disable_chimer_bridge_removal=True and lfc=False, on the rows a graph-mode dedup stream keeps in HBM (pgx_dedup.hip), down to the
// sg_edges_list text; with PGX_SGRAPH_CHIMER_ORDERED also the chimer bridge step (mark_chimer_edges, :127-195) between the transitive
// reduction and the first spur pass, with bfs_nodes' pool popped smallest (rid, end) first.  What the kernels rely on ("string graph"):
//   * the stream's pairs are unique, so the loader's overlap_set rejects nothing and no add_edge meets an edge that exists;
//   * a row that passes the filter and its geometry case adds exactly two edges, 2k and 2k + 1, each other's reverse (e ^ 1);
//   * nodes are (rid, end) numbered in creation order -- only the spur pass depends on the numbering;
//   * mark_tr_edges works node by node on state it resets after every node: a node's pass is independent of every other's;
//   * out-lists are in (length, creation) order from the first stable sort on; in-lists stay in creation order;
//   * every pass reduces an edge together with its reverse, so `reduced` is symmetric and an edge's type is the pass that reduced it first.
// Device layout: edge records in creation order; node_of[2e] / node_of[2e + 1] = dense ids of e's in- / out-node; out-lists
// (out_off / out_e / out_w / out_len) sorted by (node, length, edge), in-lists (in_off / in_e) by (node, edge); type[e] (0 = G).
// No result depends on the order in which atomics land: they only count (degrees, statistics), claim hash slots whose layout no answer
// depends on, or take a minimum.

#include "pgx_dedup_rows.h"

using pgx::Row;
typedef pgx_sgraph_edge Edge;

namespace pgx {
namespace {

constexpr uint32_t FUZZ = 500;
constexpr uint32_t DEG_CAP = 256;      // most out-edges of a node whose transitive reduction runs from LDS
constexpr uint32_t TAB_SLOTS = 512;    // its neighbour table (open addressing, load <= 1/2)
constexpr uint32_t NO_ROW = 0xFFFFFFFFu;
enum : uint8_t { T_G = PGX_SGRAPH_G, T_TR = PGX_SGRAPH_TR, T_S = PGX_SGRAPH_S, T_R = PGX_SGRAPH_R, T_C = PGX_SGRAPH_C };

// ---------------------------------------------------------------------------------------------------------
// rows -> edges
// ---------------------------------------------------------------------------------------------------------
// the identity of a row in tenths, as `%0.1f` prints it (LineOut::f1's rounding: the exact binary value, ties to even); x is finite
__device__ inline int64_t idt_tenths(double x) {
  const uint64_t bits = (uint64_t)__double_as_longlong(x);
  const uint32_t ex = (uint32_t)(bits >> 52) & 0x7FFu;
  uint64_t M = bits & ((1ULL << 52) - 1);
  int e = -1074;
  if (ex) M |= 1ULL << 52, e = (int)ex - 1075;
  const uint64_t m10 = M * 10u;
  uint64_t t;
  if (e >= 0) {
    t = m10 << min(e, 6);
  } else if (-e >= 58) {
    t = 0;
  } else {
    const int s = -e;
    t = m10 >> s;
    const uint64_t rem = m10 & ((1ULL << s) - 1), half = 1ULL << (s - 1);
    if (rem > half || (rem == half && (t & 1))) ++t;
  }
  return (bits >> 63) ? -(int64_t)t : (int64_t)t;
}
__device__ inline void set_edge(Edge &e, uint32_t v_rid, uint8_t v_end, uint32_t w_rid, uint8_t w_end, uint32_t rid, int32_t sp, int32_t tp) {
  e.v_rid = v_rid, e.v_end = v_end, e.w_rid = w_rid, e.w_end = w_end, e.label_rid = rid, e.sp = sp, e.tp = tp;
}
// the four geometry cases of ovlp_to_graph.py:768-841, each with its own skip test; false: the row adds nothing
__device__ inline bool row_geometry(const Row &r, Edge &e0, Edge &e1) {
  const uint32_t f = r.rid0, g = r.rid1;
  const int32_t f_b = (int32_t)r.a_bgn, f_e = (int32_t)r.a_end, f_l = (int32_t)r.rlen0, g_l = (int32_t)r.rlen1;   // (lengths < 2^31: checked)
  int32_t g_b = (int32_t)r.b_bgn, g_e = (int32_t)r.b_end;
  if (r.strand == 1) {
    const int32_t t = g_b;
    g_b = g_e, g_e = t;
  }
  constexpr uint8_t B = 0, E = 1;
  if (f_b > 0) {
    if (g_b < g_e) {
      if (g_e == g_l) return false;
      set_edge(e0, g, B, f, B, f, f_b, 0), set_edge(e1, f, E, g, E, g, g_e, g_l);
    } else {
      if (g_e == 0) return false;
      set_edge(e0, g, E, f, B, f, f_b, 0), set_edge(e1, f, E, g, B, g, g_e, 0);
    }
  } else {
    if (g_b < g_e) {
      if (g_b == 0 || f_e == f_l) return false;
      set_edge(e0, f, B, g, B, g, g_b, 0), set_edge(e1, g, E, f, E, f, f_e, f_l);
    } else {
      if (g_b == g_l || f_e == f_l) return false;
      set_edge(e0, f, B, g, E, g, g_b, g_l), set_edge(e1, g, B, f, E, f, f_e, f_l);
    }
  }
  return true;
}
__device__ inline uint32_t edge_len(const Edge &e) { return (uint32_t)llabs((long long)e.sp - (long long)e.tp); }

// flag[j]: row j passes the load filter and its geometry case.  cnt[0] += rows past the filter; cnt[1] = min(cnt[1], the first row that
// cannot be built: m_size == 0 -- its identity prints as nan or inf -- or a read length of 2^31 and more)
__global__ void k_sg_filter(const Row *__restrict__ rows, uint32_t n, int64_t min_len, double min_idt, uint8_t *__restrict__ flag,
                            uint32_t *__restrict__ cnt) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  bool pass = false, ok = false;
  if (j < n) {
    const Row r = rows[j];
    if (r.m_size == 0 || (r.rlen0 | r.rlen1) >> 31) {
      atomicMin(&cnt[1], j);
    } else {
      const int64_t t = idt_tenths(err_est_of(r.dist, r.m_size));
      pass = !((double)t / 10.0 < min_idt) && (int64_t)r.rlen0 >= min_len && (int64_t)r.rlen1 >= min_len;
      Edge e0, e1;
      ok = pass && row_geometry(r, e0, e1);
    }
    flag[j] = ok;
  }
  const uint64_t b = __ballot(pass);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&cnt[0], (uint32_t)__popcll(b));
}
// the two edges of every selected row, and the four node keys ((rid << 1) | end) in the order add_edge meets them
__global__ void k_sg_edges(const Row *__restrict__ rows, const uint32_t *__restrict__ sel, uint32_t m, Edge *__restrict__ edges,
                           uint64_t *__restrict__ nkey, uint32_t *__restrict__ npos) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const Row r = rows[sel[j]];
  Edge e0 = {}, e1 = {};
  row_geometry(r, e0, e1);
  e0.score = e1.score = -(int64_t)(int32_t)(0u - (uint32_t)r.m_size);   // the line prints -m_size as an int, the loader negates the number it reads
  e0.idt_tenths = e1.idt_tenths = idt_tenths(err_est_of(r.dist, r.m_size));
  edges[2 * (size_t)j] = e0, edges[2 * (size_t)j + 1] = e1;
  const uint64_t k[4] = {(uint64_t)e0.v_rid << 1 | e0.v_end, (uint64_t)e0.w_rid << 1 | e0.w_end, (uint64_t)e1.v_rid << 1 | e1.v_end,
                         (uint64_t)e1.w_rid << 1 | e1.w_end};
  for (uint32_t q = 0; q < 4; ++q) nkey[4 * (size_t)j + q] = k[q], npos[4 * (size_t)j + q] = 4 * j + q;
}

// ---------------------------------------------------------------------------------------------------------
// nodes in creation order, adjacency
// ---------------------------------------------------------------------------------------------------------
// the sorted (key, position) list: a run's head is the key's first position (stable sort); first[p] = 1 at those positions, head[i] = index
// of the head of i's run once the running maximum has passed over it
__global__ void k_sg_heads(const uint64_t *__restrict__ skey, const uint32_t *__restrict__ spos, uint32_t n, uint32_t *__restrict__ first,
                           int32_t *__restrict__ head) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool h = i == 0 || skey[i] != skey[i - 1];
  first[spos[i]] = h;
  head[i] = h ? (int32_t)i : 0;
}
__global__ void k_sg_node_ids(const uint32_t *__restrict__ spos, const int32_t *__restrict__ head, const uint32_t *__restrict__ rank, uint32_t n,
                              uint32_t *__restrict__ node_of) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) node_of[spos[i]] = rank[spos[head[i]]];
}
__global__ void k_sg_degrees(const uint32_t *__restrict__ node_of, const Edge *__restrict__ edges, uint32_t n_e, uint32_t *__restrict__ outdeg,
                             uint32_t *__restrict__ indeg, uint64_t *__restrict__ okey, uint32_t *__restrict__ ikey, uint32_t *__restrict__ iota) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_e) return;
  const uint32_t v = node_of[2 * (size_t)e], w = node_of[2 * (size_t)e + 1];
  atomicAdd(&outdeg[v], 1u), atomicAdd(&indeg[w], 1u);
  okey[e] = (uint64_t)v << 32 | edge_len(edges[e]);
  ikey[e] = w, iota[e] = e;
}
__global__ void k_sg_out_lists(const uint32_t *__restrict__ out_e, const uint64_t *__restrict__ skey, const uint32_t *__restrict__ node_of, uint32_t n_e,
                               uint32_t *__restrict__ out_w, uint32_t *__restrict__ out_len, uint64_t *__restrict__ vw_key, uint32_t *__restrict__ vw_pos) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_e) return;
  const uint32_t w = node_of[2 * (size_t)out_e[k] + 1];
  out_w[k] = w, out_len[k] = (uint32_t)skey[k];
  if (vw_key) vw_key[k] = (skey[k] & 0xFFFFFFFF00000000ULL) | w, vw_pos[k] = k;
}
__global__ void k_sg_big_flags(const uint32_t *__restrict__ out_off, uint32_t n_nodes, uint32_t cap, uint8_t *__restrict__ flag) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n_nodes) flag[v] = out_off[v + 1] - out_off[v] > cap;
}

// ---------------------------------------------------------------------------------------------------------
// transitive reduction: the hot path.  One wavefront (a workgroup of 64) per node v with out-list w_0 .. w_{d-1}.
//   marks    all neighbours in play (0); 1 = eliminated
//   loop 1   i in order: unless w_i is eliminated, every e2 of w_i's out-list with len(e2) + len_i < max_len (a prefix: the list is sorted)
//            eliminates its end if that is a neighbour.  Sequential in i -- an earlier i decides whether a later w_i is read -- and
//            parallel inside: the lanes take w_i's out-list.
//   loop 2   every i, eliminated or not: the end of w_i's first out-edge, and of every e2 shorter than FUZZ.  Order-free: a lane per i.
//   then     an eliminated neighbour's edge and its reverse are reduced.
// Where the marks live and how "is x a neighbour, and which" is answered is the policy: NbLds (d <= cap: marks and a hash table of the
// neighbours in LDS) or NbGlobal (any d: the marks are the node's own slice of an array in HBM, the lookup a binary search of the edge
// list sorted by (v, w)).  Both run the same passes.
// ---------------------------------------------------------------------------------------------------------
struct NbLds {
  uint32_t *tkey;   // TAB_SLOTS node ids, ~0 = empty
  uint16_t *tval;   // the neighbour's index in v's out-list
  uint8_t *mark;    // DEG_CAP
  __device__ void build(const uint32_t *__restrict__ nb, uint32_t d, uint32_t lane) {
    for (uint32_t s = lane; s < TAB_SLOTS; s += 64) tkey[s] = ~0u;
    for (uint32_t i = lane; i < d; i += 64) mark[i] = 0;
    __syncthreads();
    for (uint32_t i = lane; i < d; i += 64) {
      const uint32_t key = nb[i];
      for (uint32_t s = (key * 0x9E3779B1u) >> 23;; s = (s + 1) & (TAB_SLOTS - 1))   // (top 9 bits: TAB_SLOTS == 512)
        if (atomicCAS(&tkey[s], ~0u, key) == ~0u) {
          tval[s] = (uint16_t)i;
          break;
        }
    }
    __syncthreads();
  }
  __device__ int find(uint32_t x) const {
    for (uint32_t s = (x * 0x9E3779B1u) >> 23;; s = (s + 1) & (TAB_SLOTS - 1)) {
      const uint32_t k = tkey[s];
      if (k == x) return tval[s];
      if (k == ~0u) return -1;
    }
  }
  __device__ bool gone(uint32_t i) const { return mark[i] != 0; }
  __device__ void eliminate(uint32_t i) { mark[i] = 1; }
};
static_assert(TAB_SLOTS == 512, "the table's hash takes the top 9 bits");
struct NbGlobal {
  const uint64_t *vw_key;   // every edge's (v << 32 | w), ascending
  const uint32_t *vw_pos;   // its position in the out-lists
  uint32_t n_e, v, base;    // base: out_off[v]
  uint32_t *mark;           // v's slice of the per-edge marks (zero before the launch)
  __device__ void build(const uint32_t *, uint32_t, uint32_t) {}
  __device__ int find(uint32_t x) const {
    const uint64_t want = (uint64_t)v << 32 | x;
    uint32_t lo = 0, hi = n_e;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (vw_key[mid] < want) lo = mid + 1;
      else hi = mid;
    }
    return lo < n_e && vw_key[lo] == want ? (int)(vw_pos[lo] - base) : -1;
  }
  // (device-scope accesses: what a lane wrote before the barrier is what every lane reads after it, whatever the vector cache holds)
  __device__ bool gone(uint32_t i) const { return __hip_atomic_load(&mark[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0; }
  __device__ void eliminate(uint32_t i) { __hip_atomic_store(&mark[i], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
template <class Nb>
__device__ inline void tr_node(Nb &nb, uint32_t o, uint32_t d, uint32_t lane, const uint32_t *__restrict__ out_off, const uint32_t *__restrict__ out_e,
                               const uint32_t *__restrict__ out_w, const uint32_t *__restrict__ out_len, uint8_t *__restrict__ type) {
  nb.build(out_w + o, d, lane);
  const uint64_t max_len = (uint64_t)out_len[o + d - 1] + FUZZ;
  for (uint32_t i = 0; i < d; ++i) {
    if (nb.gone(i)) continue;   // (uniform: every lane reads the same mark, behind the barrier that ended the last round)
    const uint32_t w = out_w[o + i], wo = out_off[w], wd = out_off[w + 1] - wo;
    const uint64_t len_i = out_len[o + i];
    for (uint32_t k0 = 0; k0 < wd; k0 += 64) {
      const uint32_t k = k0 + lane;
      const bool in = k < wd && (uint64_t)out_len[wo + k] + len_i < max_len;
      if (in) {
        const int j = nb.find(out_w[wo + k]);
        if (j >= 0) nb.eliminate((uint32_t)j);
      }
      if (__ballot(in) != ~0ULL) break;   // the prefix ended in this chunk
    }
    __syncthreads();
  }
  for (uint32_t i = lane; i < d; i += 64) {
    const uint32_t w = out_w[o + i], wo = out_off[w], wd = out_off[w + 1] - wo;
    for (uint32_t k = 0; k < wd && (k == 0 || out_len[wo + k] < FUZZ); ++k) {
      const int j = nb.find(out_w[wo + k]);
      if (j >= 0) nb.eliminate((uint32_t)j);
    }
  }
  __syncthreads();
  for (uint32_t i = lane; i < d; i += 64)
    if (nb.gone(i)) {
      const uint32_t e = out_e[o + i];
      type[e] = T_TR, type[e ^ 1u] = T_TR;   // (other nodes' passes may store the same value to the same bytes)
    }
  __syncthreads();   // the tables are reused by the workgroup's next node
}
// every node with 1 .. cap out-edges, a workgroup per node, grid-stride
__global__ __launch_bounds__(64) void k_sg_tr_lds(uint32_t n_nodes, uint32_t cap, const uint32_t *__restrict__ out_off, const uint32_t *__restrict__ out_e,
                                                  const uint32_t *__restrict__ out_w, const uint32_t *__restrict__ out_len, uint8_t *__restrict__ type) {
  __shared__ uint32_t tkey[TAB_SLOTS];
  __shared__ uint16_t tval[TAB_SLOTS];
  __shared__ uint8_t mark[DEG_CAP];
  NbLds nb{tkey, tval, mark};
  for (uint32_t v = blockIdx.x; v < n_nodes; v += gridDim.x) {
    const uint32_t o = out_off[v], d = out_off[v + 1] - o;
    if (d == 0 || d > cap) continue;
    tr_node(nb, o, d, threadIdx.x, out_off, out_e, out_w, out_len, type);
  }
}
// the listed nodes (more than cap out-edges)
__global__ __launch_bounds__(64) void k_sg_tr_global(const uint32_t *__restrict__ list, uint32_t n_list, const uint32_t *__restrict__ out_off,
                                                     const uint32_t *__restrict__ out_e, const uint32_t *__restrict__ out_w, const uint32_t *__restrict__ out_len,
                                                     const uint64_t *__restrict__ vw_key, const uint32_t *__restrict__ vw_pos, uint32_t n_e,
                                                     uint32_t *__restrict__ marks, uint8_t *__restrict__ type) {
  for (uint32_t q = blockIdx.x; q < n_list; q += gridDim.x) {
    const uint32_t v = list[q], o = out_off[v], d = out_off[v + 1] - o;
    NbGlobal nb{vw_key, vw_pos, n_e, v, o, marks + o};
    tr_node(nb, o, d, threadIdx.x, out_off, out_e, out_w, out_len, type);
  }
}

// ---------------------------------------------------------------------------------------------------------
// chimer bridge step (mark_chimer_edges, :127-195; PGX_SGRAPH_CHIMER_ORDERED).  It reads the marks as the transitive reduction left them
// (only to find the candidates) and adjacency in any state; what it decides goes to a byte per candidate, and a kernel of its own marks
// the chosen nodes' edges afterwards.  So a candidate's answer depends on no other candidate's, and the candidates run side by side:
// one wavefront (a workgroup of 64) per candidate n.
//   test 1   O = the heads of n's out-edges, T = the heads of the out-edges of the tails of n's in-edges, without n: O and T disjoint
//   test 2   the union of flow(v, n) over O and the union over T are disjoint.  flow(s, n) is bfs_nodes with depth 5: A = pool = {s};
//            at most 4 times the pool's smallest (rid as unsigned, end) leaves it and every head w != n of its out-edges that is not in
//            A enters A, and the pool too if w has out-edges.  The pop order is this library's: the script pops from a set of objects.
// One table node -> (generation << 2 | sides) serves both tests: side 1 = reached from O, side 2 = from T, generation = the flow that
// saw the node last, so "w is in A" is "w's generation is this flow's" and the two unions meet where a node has both sides.  The pool
// holds ranks in the (rid, end) order (krank), so a pop is a minimum.  Where the table lives is the policy: ChLds (a hash table of
// CH_SLOTS in LDS; a candidate whose flows outgrow it is handed on) or ChGlobal (any size: the workgroup's own slice of an array in
// HBM with an entry per node, valid where its upper half is the candidate's tag).
// ---------------------------------------------------------------------------------------------------------
// an edge's mark where other lanes or workgroups of the same kernel may be storing to it
__device__ inline uint8_t type_now(const uint8_t *type, uint32_t e) { return __hip_atomic_load(&type[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void type_set(uint8_t *type, uint32_t e, uint8_t t) { __hip_atomic_store(&type[e], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
constexpr uint32_t CH_SLOTS = 2048;           // ChLds: open addressing
constexpr uint32_t CH_NODES = CH_SLOTS / 2;   // the most nodes it takes (load <= 1/2), and the pool's size: a flow's pool is part of its A
enum : uint8_t { CH_CHOSEN = 1, CH_PAST1 = 2, CH_OVER = 4 };
enum { FL_OK = 0, FL_MEET = 1, FL_FULL = 2 };

// node keys (rid << 1 | end) by dense id (every edge of a node stores the same value), and the identity list for the sort by key
__global__ void k_sg_node_keys(const uint32_t *__restrict__ node_of, const Edge *__restrict__ edges, uint32_t n_e, uint64_t *__restrict__ nkey,
                               uint32_t *__restrict__ iota) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_e) return;
  const Edge ed = edges[e];
  const uint32_t v = node_of[2 * (size_t)e], w = node_of[2 * (size_t)e + 1];
  nkey[v] = (uint64_t)ed.v_rid << 1 | ed.v_end, iota[v] = v;
  nkey[w] = (uint64_t)ed.w_rid << 1 | ed.w_end, iota[w] = w;
}
__global__ void k_sg_kranks(const uint32_t *__restrict__ by_rank, uint32_t n_nodes, uint32_t *__restrict__ krank) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_nodes) krank[by_rank[i]] = i;
}
// multi[v]: bit 0 = at least 2 unreduced out-edges, bit 1 = at least 2 unreduced in-edges
__global__ void k_sg_multi(uint32_t n_nodes, const uint32_t *__restrict__ out_off, const uint32_t *__restrict__ out_e, const uint32_t *__restrict__ in_off,
                           const uint32_t *__restrict__ in_e, const uint8_t *__restrict__ type, uint8_t *__restrict__ multi) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_nodes) return;
  uint32_t lo = 0, li = 0;   // (whole lists, no early exit: the counts are read after the loops)
  for (uint32_t k = out_off[v]; k < out_off[v + 1]; ++k) lo += type[out_e[k]] == T_G;
  for (uint32_t k = in_off[v]; k < in_off[v + 1]; ++k) li += type[in_e[k]] == T_G;
  multi[v] = (uint8_t)((lo >= 2) | (li >= 2) << 1);
}
// a candidate: an unreduced in-edge from a node with 2 and more unreduced out-edges, and an unreduced out-edge into a node with 2 and more
// unreduced in-edges (:129-154)
__global__ void k_sg_chimer_cands(uint32_t n_nodes, const uint32_t *__restrict__ out_off, const uint32_t *__restrict__ out_e, const uint32_t *__restrict__ out_w,
                                  const uint32_t *__restrict__ in_off, const uint32_t *__restrict__ in_e, const uint32_t *__restrict__ node_of,
                                  const uint8_t *__restrict__ type, const uint8_t *__restrict__ multi, uint8_t *__restrict__ flag) {
  const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_nodes) return;
  uint32_t a = 0, b = 0;
  for (uint32_t k = in_off[n]; k < in_off[n + 1]; ++k) a += type[in_e[k]] == T_G && (multi[node_of[2 * (size_t)in_e[k]]] & 1);
  for (uint32_t k = out_off[n]; k < out_off[n + 1]; ++k) b += type[out_e[k]] == T_G && (multi[out_w[k]] & 2);
  flag[n] = a != 0 && b != 0;
}

struct ChLds {
  uint32_t *tkey;   // CH_SLOTS node ids, ~0 = empty
  uint32_t *tval;   // generation << 2 | sides
  uint32_t *pool;   // CH_NODES
  uint32_t lim;     // the most nodes the table may take (PGX_SGRAPH_CHIMER_LDS; <= CH_NODES)
  uint32_t cnt;     // nodes in it (the same in every lane)
  __device__ void reset(uint32_t lane) {
    for (uint32_t s = lane; s < CH_SLOTS; s += 64) tkey[s] = ~0u;
    cnt = 0;
    __syncthreads();
  }
  __device__ bool room(uint32_t need) const { return cnt + need <= lim; }
  __device__ void grew(uint32_t k) { cnt += k; }
  __device__ static uint32_t home(uint32_t x) { return (x * 0x9E3779B1u) >> 21; }   // (top 11 bits: CH_SLOTS == 2048)
  __device__ uint32_t claim(uint32_t x, bool &fresh) {   // x's slot, made if there is none (room() said there is space)
    for (uint32_t s = home(x);; s = (s + 1) & (CH_SLOTS - 1)) {
      const uint32_t k = atomicCAS(&tkey[s], ~0u, x);
      if (k == ~0u || k == x) {
        fresh = k == ~0u;
        return s;
      }
    }
  }
  __device__ bool has(uint32_t x) const {
    for (uint32_t s = home(x);; s = (s + 1) & (CH_SLOTS - 1)) {
      const uint32_t k = tkey[s];
      if (k == x) return true;
      if (k == ~0u) return false;
    }
  }
  __device__ uint32_t get(uint32_t s) const { return tval[s]; }
  __device__ void set(uint32_t s, uint32_t v) { tval[s] = v; }
  __device__ uint32_t pool_get(uint32_t i) const { return pool[i]; }
  __device__ void pool_set(uint32_t i, uint32_t v) { pool[i] = v; }
};
static_assert(CH_SLOTS == 2048, "the table's hash takes the top 11 bits");
struct ChGlobal {
  uint64_t *tab;    // an entry per node: tag << 32 | generation << 2 | sides (zero before the launch; a tag is never 0)
  uint32_t *pool;   // 4 * the largest out-degree + 1
  uint64_t tag;     // the candidate's, in the upper half
  // (device-scope accesses, as NbGlobal's: what a lane wrote before the barrier is what every lane reads after it)
  __device__ uint64_t ld(uint32_t x) const { return __hip_atomic_load(&tab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ void reset(uint32_t) {}
  __device__ bool room(uint32_t) const { return true; }
  __device__ void grew(uint32_t) {}
  __device__ uint32_t claim(uint32_t x, bool &fresh) {   // (the caller sets a fresh entry at once)
    fresh = (ld(x) & 0xFFFFFFFF00000000ULL) != tag;
    return x;
  }
  __device__ bool has(uint32_t x) const { return (ld(x) & 0xFFFFFFFF00000000ULL) == tag; }
  __device__ uint32_t get(uint32_t s) const { return (uint32_t)ld(s); }
  __device__ void set(uint32_t s, uint32_t v) { __hip_atomic_store(&tab[s], tag | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ uint32_t pool_get(uint32_t i) const { return __hip_atomic_load(&pool[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ void pool_set(uint32_t i, uint32_t v) { __hip_atomic_store(&pool[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
struct ChGraph {   // what the tests read: adjacency in any state, and the (rid, end) order
  const uint32_t *out_off, *out_w, *in_off, *in_e, *node_of, *krank, *by_rank;
};
// one step of a flow: the active lanes' nodes (all different: a node's out-edges have different heads) enter A unless they are in it,
// and the pool if they have out-edges (the start node: always)
template <class Tab>
__device__ inline int flow_add(Tab &tab, const ChGraph &G, bool active, uint32_t w, uint32_t side, uint32_t gen, bool start, uint32_t &pool_n, uint32_t lane) {
  if (!tab.room((uint32_t)__popcll(__ballot(active)))) return FL_FULL;
  bool fresh = false, push = false, meet = false;
  if (active) {
    const uint32_t s = tab.claim(w, fresh), v = fresh ? 0u : tab.get(s);
    if (fresh || (v >> 2) != gen) {
      const uint32_t nv = gen << 2 | (v & 3u) | side;
      tab.set(s, nv);
      meet = (nv & 3u) == 3u;
      push = start || G.out_off[w + 1] != G.out_off[w];
    }
  }
  tab.grew((uint32_t)__popcll(__ballot(fresh)));
  const uint64_t pb = __ballot(push);
  if (push) tab.pool_set(pool_n + (uint32_t)__popcll(pb & ((1ULL << lane) - 1)), G.krank[w]);
  pool_n += (uint32_t)__popcll(pb);
  __syncthreads();
  return __ballot(meet) ? FL_MEET : FL_OK;
}
// the pool's smallest rank leaves it; ~0: the pool is empty.  (The ranks in a pool are all different, so one lane holds the minimum.)
template <class Tab>
__device__ inline uint32_t pool_pop(Tab &tab, uint32_t pool_n, uint32_t lane) {
  uint32_t best = ~0u, at = 0;
  for (uint32_t i = lane; i < pool_n; i += 64) {
    const uint32_t r = tab.pool_get(i);
    if (r < best) best = r, at = i;
  }
  uint32_t mn = best;
  for (int s = 32; s; s >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, s));
  if (mn != ~0u && best == mn) tab.pool_set(at, ~0u);
  __syncthreads();
  return mn;
}
// flow(s, n) into the table as generation gen of `side`; FL_MEET as soon as a node has both sides (the answer is then known)
template <class Tab>
__device__ inline int flow(Tab &tab, const ChGraph &G, uint32_t s, uint32_t n, uint32_t side, uint32_t gen, uint32_t lane) {
  uint32_t pool_n = 0;
  int r = flow_add(tab, G, lane == 0, s, side, gen, true, pool_n, lane);
  for (int pop = 0; pop < 4 && r == FL_OK; ++pop) {
    const uint32_t mn = pool_pop(tab, pool_n, lane);
    if (mn == ~0u) break;
    const uint32_t p = G.by_rank[mn], po = G.out_off[p], pd = G.out_off[p + 1] - po;
    for (uint32_t k0 = 0; k0 < pd && r == FL_OK; k0 += 64) {
      const uint32_t k = k0 + lane, w = k < pd ? G.out_w[po + k] : n;
      r = flow_add(tab, G, w != n, w, side, gen, false, pool_n, lane);
    }
  }
  return r;
}
// the two tests of candidate n: CH_PAST1 / CH_CHOSEN, or CH_OVER alone where the table is full (every branch is wave-uniform)
template <class Tab>
__device__ inline uint8_t chimer_node(Tab &tab, const ChGraph &G, uint32_t n, uint32_t lane) {
  tab.reset(lane);
  const uint32_t no = G.out_off[n], nd = G.out_off[n + 1] - no, io = G.in_off[n], id = G.in_off[n + 1] - io;
  for (uint32_t k0 = 0; k0 < nd; k0 += 64) {   // O, as side 1 of generation 0 (no flow's)
    const uint32_t k = k0 + lane;
    if (!tab.room((uint32_t)__popcll(__ballot(k < nd)))) return CH_OVER;
    bool fresh = false;
    if (k < nd) tab.set(tab.claim(G.out_w[no + k], fresh), 1u);
    tab.grew((uint32_t)__popcll(__ballot(fresh)));
  }
  __syncthreads();
  for (uint32_t i = 0; i < id; ++i) {   // test 1: no member of T is in the table
    const uint32_t u = G.node_of[2 * (size_t)G.in_e[io + i]], uo = G.out_off[u], ud = G.out_off[u + 1] - uo;
    bool hit = false;
    for (uint32_t k = lane; k < ud; k += 64) {
      const uint32_t w = G.out_w[uo + k];
      hit |= w != n && tab.has(w);
    }
    if (__ballot(hit)) return 0;
  }
  uint32_t gen = 0;   // (at most one flow per edge: below 2^30)
  for (uint32_t k = 0; k < nd; ++k) {
    const int r = flow(tab, G, G.out_w[no + k], n, 1u, ++gen, lane);
    if (r != FL_OK) return r == FL_FULL ? CH_OVER : CH_PAST1;
  }
  for (uint32_t i = 0; i < id; ++i) {
    const uint32_t u = G.node_of[2 * (size_t)G.in_e[io + i]], uo = G.out_off[u], ud = G.out_off[u + 1] - uo;
    for (uint32_t k = 0; k < ud; ++k) {
      const uint32_t w = G.out_w[uo + k];
      if (w == n) continue;
      const int r = flow(tab, G, w, n, 2u, ++gen, lane);   // (a member of T that two tails share runs twice, to the same end)
      if (r != FL_OK) return r == FL_FULL ? CH_OVER : CH_PAST1;
    }
  }
  return CH_PAST1 | CH_CHOSEN;
}
// every candidate, a workgroup per candidate, grid-stride
__global__ __launch_bounds__(64) void k_sg_chimer_lds(const uint32_t *__restrict__ cand, uint32_t n_cand, uint32_t lim, ChGraph G, uint8_t *__restrict__ res) {
  __shared__ uint32_t tkey[CH_SLOTS], tval[CH_SLOTS], pool[CH_NODES];
  ChLds tab{tkey, tval, pool, lim, 0};
  for (uint32_t q = blockIdx.x; q < n_cand; q += gridDim.x) {
    const uint8_t r = chimer_node(tab, G, cand[q], threadIdx.x);
    if (threadIdx.x == 0) res[q] = r;
    __syncthreads();   // the tables are reused by the workgroup's next candidate
  }
}
// the listed candidates (their flows outgrew the LDS table), on the workgroup's slices of tabs and pools
__global__ __launch_bounds__(64) void k_sg_chimer_global(const uint32_t *__restrict__ cand, const uint32_t *__restrict__ list, uint32_t n_list, ChGraph G,
                                                         uint64_t *__restrict__ tabs, uint32_t n_nodes, uint32_t *__restrict__ pools, uint32_t pool_size,
                                                         uint8_t *__restrict__ res) {
  for (uint32_t j = blockIdx.x; j < n_list; j += gridDim.x) {
    const uint32_t q = list[j];
    ChGlobal tab{tabs + (size_t)blockIdx.x * n_nodes, pools + (size_t)blockIdx.x * pool_size, (uint64_t)(q + 1) << 32};
    const uint8_t r = chimer_node(tab, G, cand[q], threadIdx.x);
    if (threadIdx.x == 0) res[q] = r;
    __syncthreads();
  }
}
// flag[q] = res[q] has `bit`; cnt[0] += the candidates past test 1 (bit == CH_CHOSEN only: the last call)
__global__ void k_sg_chimer_flags(const uint8_t *__restrict__ res, uint32_t n, uint8_t bit, uint8_t *__restrict__ flag, uint32_t *__restrict__ cnt) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  const uint8_t r = q < n ? res[q] : 0;
  if (q < n) flag[q] = (r & bit) != 0;
  const uint64_t b = __ballot(bit == CH_CHOSEN && (r & CH_PAST1));
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(cnt, (uint32_t)__popcll(b));
}
// the chosen nodes' keys, and their edges that the reduction left unreduced become C, each with its reverse (:173-193; a thread per node.
// An edge reads G or, where another chosen node got there first, C: both end as C.  TR stays.)
__global__ void k_sg_chimer_mark(const uint32_t *__restrict__ cand, const uint32_t *__restrict__ chosen, uint32_t n_chosen, const uint64_t *__restrict__ nkey,
                                 const uint32_t *__restrict__ out_off, const uint32_t *__restrict__ out_e, const uint32_t *__restrict__ in_off,
                                 const uint32_t *__restrict__ in_e, uint8_t *type, uint64_t *__restrict__ ckey) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_chosen) return;
  const uint32_t n = cand[chosen[j]];
  ckey[j] = nkey[n];
  for (uint32_t k = out_off[n]; k < out_off[n + 1]; ++k)
    if (type_now(type, out_e[k]) != T_TR) type_set(type, out_e[k], T_C), type_set(type, out_e[k] ^ 1u, T_C);
  for (uint32_t k = in_off[n]; k < in_off[n + 1]; ++k)
    if (type_now(type, in_e[k]) != T_TR) type_set(type, in_e[k], T_C), type_set(type, in_e[k] ^ 1u, T_C);
}

// ---------------------------------------------------------------------------------------------------------
// spur pass, best overlap
// ---------------------------------------------------------------------------------------------------------
// a node the spur pass can act on: an out-edge into a node without out-edges, or an in-edge from a node without in-edges (the degrees
// never change: the passes only reduce)
__global__ void k_sg_spur_flags(uint32_t n_nodes, const uint32_t *__restrict__ out_off, const uint32_t *__restrict__ out_w, const uint32_t *__restrict__ in_off,
                                const uint32_t *__restrict__ in_e, const uint32_t *__restrict__ node_of, uint8_t *__restrict__ flag) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_nodes) return;
  bool c = false;
  for (uint32_t k = out_off[v]; k < out_off[v + 1] && !c; ++k) c = out_off[out_w[k] + 1] == out_off[out_w[k]];
  for (uint32_t k = in_off[v]; k < in_off[v + 1] && !c; ++k) {
    const uint32_t u = node_of[2 * (size_t)in_e[k]];
    c = in_off[u + 1] == in_off[u];
  }
  flag[v] = c;
}
// one side of mark_spur_edge at node v: with more than one unreduced edge in the list, every unreduced one whose far node is a dead end
// goes, with its reverse.  far_off: the far node's degree table (out-degrees for the out side, in-degrees for the in side).
__device__ inline void spur_side(const uint32_t *__restrict__ lst, uint32_t d, uint32_t far_slot, const uint32_t *__restrict__ node_of,
                                 const uint32_t *__restrict__ far_off, uint8_t *type, uint32_t lane) {
  uint32_t live = 0;
  for (uint32_t k = lane; k < d; k += 64) live += type_now(type, lst[k]) == T_G;
  for (int s = 32; s; s >>= 1) live += (uint32_t)__shfl_xor((int)live, s);
  __syncthreads();
  if (live > 1)
    for (uint32_t k = lane; k < d; k += 64) {
      const uint32_t e = lst[k], far = node_of[2 * (size_t)e + far_slot];
      if (far_off[far + 1] == far_off[far] && type_now(type, e) == T_G) type_set(type, e, T_S), type_set(type, e ^ 1u, T_S);
    }
  __syncthreads();
}
// mark_spur_edge over the candidate nodes in creation order, ONE workgroup of one wavefront: a node's counts see what every earlier
// node reduced
__global__ __launch_bounds__(64) void k_sg_spur(const uint32_t *__restrict__ cand, uint32_t n_cand, const uint32_t *__restrict__ out_off,
                                                const uint32_t *__restrict__ out_e, const uint32_t *__restrict__ in_off, const uint32_t *__restrict__ in_e,
                                                const uint32_t *__restrict__ node_of, uint8_t *type) {
  for (uint32_t c = 0; c < n_cand; ++c) {
    const uint32_t v = cand[c];
    spur_side(out_e + out_off[v], out_off[v + 1] - out_off[v], 1, node_of, out_off, type, threadIdx.x);
    spur_side(in_e + in_off[v], in_off[v + 1] - in_off[v], 0, node_of, in_off, type, threadIdx.x);
  }
}
// per node the best unreduced out-edge and in-edge: the largest m_size, the first of equals in the list's own order
__device__ inline void best_of(const uint32_t *__restrict__ lst, uint32_t d, const Edge *__restrict__ edges, const uint8_t *__restrict__ type,
                               uint8_t *__restrict__ best) {
  uint32_t pick = ~0u;
  int64_t top = 0;
  for (uint32_t k = 0; k < d; ++k) {
    const uint32_t e = lst[k];
    if (type[e] != T_G) continue;
    const int64_t s = edges[e].score;
    if (pick == ~0u || s > top) pick = e, top = s;
  }
  if (pick != ~0u) best[pick] = 1;
}
__global__ void k_sg_best(uint32_t n_nodes, const uint32_t *__restrict__ out_off, const uint32_t *__restrict__ out_e, const uint32_t *__restrict__ in_off,
                          const uint32_t *__restrict__ in_e, const Edge *__restrict__ edges, const uint8_t *__restrict__ type, uint8_t *__restrict__ best) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_nodes) return;
  best_of(out_e + out_off[v], out_off[v + 1] - out_off[v], edges, type, best);
  best_of(in_e + in_off[v], in_off[v + 1] - in_off[v], edges, type, best);
}
// an unreduced pair goes unless both of its edges are best edges (a thread per pair)
__global__ void k_sg_not_best(uint32_t n_pairs, const uint8_t *__restrict__ best, uint8_t *__restrict__ type) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  if (type[2 * (size_t)p] == T_G && !(best[2 * (size_t)p] && best[2 * (size_t)p + 1])) type[2 * (size_t)p] = T_R, type[2 * (size_t)p + 1] = T_R;
}
__global__ void k_sg_finish(Edge *__restrict__ edges, const uint8_t *__restrict__ type, uint32_t n_e, uint32_t *__restrict__ by_type) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  const uint8_t t = e < n_e ? type[e] : 0xFF;
  if (e < n_e) edges[e].type = t;
  for (uint8_t q = 0; q < 5; ++q) {   // (by_type[4]: the C edges)
    const uint64_t b = __ballot(t == q);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&by_type[q], (uint32_t)__popcll(b));
  }
}

// ---------------------------------------------------------------------------------------------------------
// the text: '%s %s %s %5d %5d %5d %5.2f %s' (ovlp_to_graph.py:901), a line per edge
// ---------------------------------------------------------------------------------------------------------
constexpr uint32_t SG_MAXLINE = 112;   // 13 + 13 + 11 + 11 + 11 + 20 + 17 + 2 + 7 blanks + '\n' = 106
template <bool WRITE>
__device__ inline uint32_t format_edge(const Edge &e, char *dst) {
  LineOut<WRITE> o{dst, 0};
  o.node(e.v_rid, e.v_end), o.ch(' ');
  o.node(e.w_rid, e.w_end), o.ch(' ');
  o.rid((int32_t)e.label_rid), o.ch(' ');
  o.i64(e.sp, 5), o.ch(' ');
  o.i64(e.tp, 5), o.ch(' ');
  o.i64(e.score, 5), o.ch(' ');
  {   // %5.2f of the number the line's `%0.1f` text parses to: the tenths with one more 0
    const bool neg = e.idt_tenths < 0;
    const uint64_t a = neg ? 0ULL - (uint64_t)e.idt_tenths : (uint64_t)e.idt_tenths, whole = div10(a);
    for (uint32_t nd = ndigits(whole, neg ? 5 : 4); nd < 5; ++nd) o.ch(' ');
    if (neg) o.ch('-');
    o.u64(whole), o.ch('.'), o.ch((char)('0' + (uint32_t)(a - whole * 10u))), o.ch('0');
  }
  o.ch(' ');
  if (e.type == T_G) o.ch('G');
  else if (e.type == T_TR) o.ch('T'), o.ch('R');
  else o.ch(e.type == T_S ? 'S' : e.type == T_R ? 'R' : 'C');
  o.ch('\n');
  return o.n;
}
__global__ void k_sg_line_len(const Edge *__restrict__ edges, uint32_t m, uint64_t *__restrict__ len) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j > m) return;
  len[j] = j < m ? format_edge<false>(edges[j], nullptr) : 0;   // len[m] = 0: the exclusive scan's last entry is the total
}
// as k_format of pgx_dedup.hip: a workgroup formats a tile of lines into LDS at the scan's offsets, then streams the tile out (tile_out)
constexpr uint32_t SG_TILE = 256;
__global__ __launch_bounds__(SG_TILE) void k_sg_format(const Edge *__restrict__ edges, const uint64_t *__restrict__ off, uint32_t m, char *__restrict__ text) {
  __shared__ __attribute__((aligned(16))) char tile[SG_TILE * SG_MAXLINE + 16];
  const uint32_t j0 = blockIdx.x * SG_TILE, j = j0 + threadIdx.x, j1 = min(m, j0 + SG_TILE);
  const uint64_t base = off[j0], end = off[j1];
  const uint32_t pad = (uint32_t)((uintptr_t)(text + base) & 15u);
  if (j < m) format_edge<true>(edges[j], tile + pad + (uint32_t)(off[j] - base));
  __syncthreads();
  tile_out<SG_TILE>(tile, text + base - pad, pad, pad + (uint32_t)(end - base));
}
}  // namespace
}  // namespace pgx

using namespace pgx;

struct pgx_sgraph {
  DevBuf<Edge> edges;            // creation order, types final (MemTag "sgraph")
  pgx_sgraph_stats_t st = {};
  pgx_sgraph_chimer_stats_t ch = {};   // zeros without PGX_SGRAPH_CHIMER_ORDERED
  std::vector<uint64_t> chimers;       // the chosen nodes' keys (rid << 1 | end) in creation order
  uint64_t cursor = 0;           // edges handed out as text
  TextStage stage;
  bool shut = false;             // pgx_shutdown ran: the device state is gone
  void drop_device_state() {
    edges.release();
    stage.drop();
  }
};

namespace pgx {
namespace {
LiveSet<pgx_sgraph> g_graphs;
ShutdownHook g_graphs_hook([] { g_graphs.shutdown(); });

uint32_t deg_cap() {   // PGX_SGRAPH_DEG_MAX: a test hook that shrinks the LDS path so that small graphs reach the other one
  const char *v = getenv("PGX_SGRAPH_DEG_MAX");
  const long c = v ? atol(v) : (long)DEG_CAP;
  return (uint32_t)std::min<long>(std::max<long>(c, 0), (long)DEG_CAP);
}

uint32_t chimer_lds() {   // PGX_SGRAPH_CHIMER_LDS: a test hook that shrinks the LDS table of the chimer bridge step, as PGX_SGRAPH_DEG_MAX does
  const char *v = getenv("PGX_SGRAPH_CHIMER_LDS");
  const long c = v ? atol(v) : (long)CH_NODES;
  return (uint32_t)std::min<long>(std::max<long>(c, 0), (long)CH_NODES);
}

// the chimer bridge step on the marks the transitive reduction left in `type`; fills g->ch and g->chimers.  The host learns three
// counts (candidates, candidates beyond the LDS table, chosen nodes) and the chosen nodes' keys: no round trip per candidate.
void chimer_pass(pgx_sgraph *g, uint32_t n_nodes, uint32_t n_e, uint32_t max_deg, const Edge *edges, const uint32_t *node_of, const uint32_t *out_off,
                 const uint32_t *out_e, const uint32_t *out_w, const uint32_t *in_off, const uint32_t *in_e, uint8_t *type, uint32_t *d_past1, PrimWs *tmp) {
  hipStream_t st = ctx().stream;
  DevBuf<uint8_t> multi(n_nodes), flag(n_nodes);
  DevBuf<uint32_t> cand(n_nodes);
  LAUNCH(k_sg_multi, n_nodes, n_nodes, out_off, out_e, in_off, in_e, type, multi.p);
  LAUNCH(k_sg_chimer_cands, n_nodes, n_nodes, out_off, out_e, out_w, in_off, in_e, node_of, type, multi.p, flag.p);
  const uint32_t n_cand = select_indices(flag.p, n_nodes, cand.p, tmp);
  g->ch.candidates = n_cand;
  if (n_cand == 0) return;
  multi.release();
  // ---- the (rid, end) order: by_rank[i] = the node with the i-th smallest key, krank its inverse
  DevBuf<uint64_t> nkey(n_nodes), nkey_s(n_nodes);
  DevBuf<uint32_t> iota(n_nodes), by_rank(n_nodes), krank(n_nodes);
  LAUNCH(k_sg_node_keys, n_e, node_of, edges, n_e, nkey.p, iota.p);
  sort_pairs(nkey.p, nkey_s.p, iota.p, by_rank.p, n_nodes, 0, 33, tmp);
  LAUNCH(k_sg_kranks, n_nodes, by_rank.p, n_nodes, krank.p);
  nkey_s.release(), iota.release();
  // ---- the tests
  const ChGraph G{out_off, out_w, in_off, in_e, node_of, krank.p, by_rank.p};
  DevBuf<uint8_t> res(n_cand);
  DevBuf<uint32_t> list(n_cand);
  hipLaunchKernelGGL(k_sg_chimer_lds, dim3(stride_grid(n_cand, 32)), dim3(64), 0, st, cand.p, n_cand, chimer_lds(), G, res.p);
  LAUNCH(k_sg_chimer_flags, n_cand, res.p, n_cand, (uint8_t)CH_OVER, flag.p, d_past1);
  const uint32_t n_over = select_indices(flag.p, n_cand, list.p, tmp);
  if (n_over) {   // a table with an entry per node for each workgroup: as many workgroups as 1 GiB of tables allows
    const uint32_t wgs = grid_cap(std::min<uint64_t>({(uint64_t)n_over, 64, std::max<uint64_t>(1, (1ULL << 27) / n_nodes)}));   // (the slices below and the launch: this one value)
    const uint32_t pool_size = 4 * max_deg + 1;
    DevBuf<uint64_t> tabs((size_t)wgs * n_nodes);
    DevBuf<uint32_t> pools((size_t)wgs * pool_size);
    PGX_HIP(hipMemsetAsync(tabs.p, 0, (size_t)wgs * n_nodes * sizeof(uint64_t), st));
    hipLaunchKernelGGL(k_sg_chimer_global, dim3(wgs), dim3(64), 0, st, cand.p, list.p, n_over, G, tabs.p, n_nodes, pools.p, pool_size, res.p);
    PGX_HIP(hipGetLastError());
    pgx::sync();   // (the tables go back behind the kernel)
  }
  // ---- the chosen nodes in creation order, their edges
  LAUNCH(k_sg_chimer_flags, n_cand, res.p, n_cand, (uint8_t)CH_CHOSEN, flag.p, d_past1);
  const uint32_t n_chosen = select_indices(flag.p, n_cand, list.p, tmp);
  g->ch.chosen = n_chosen;
  if (n_chosen == 0) return;
  DevBuf<uint64_t> ckey(n_chosen);
  LAUNCH(k_sg_chimer_mark, n_chosen, cand.p, list.p, n_chosen, nkey.p, out_off, out_e, in_off, in_e, type, ckey.p);
  PGX_HIP(hipGetLastError());
  g->chimers.resize(n_chosen);
  ckey.download(g->chimers.data(), n_chosen);
  pgx::sync();
}

// the passes over n_rows rows at d_rows; fills g
void build_graph(const Row *d_rows, uint32_t n_rows, int64_t min_len, double min_idt, bool chimer, pgx_sgraph *g) {
  hipStream_t st = ctx().stream;
  MemTag tag("sgraph");
  PrimWs tmp;
  g->st.rows_in = n_rows;
  if (n_rows == 0) return;
  // ---- filter and geometry (the parts are timed one by one as well: "sgraph_edges", "_adj", "_tr", "_chimer", "_spur", "_best")
  std::unique_ptr<KernelTimer> part(new KernelTimer("sgraph_edges", n_rows));
  DevBuf<uint32_t> cnt(12);   // [0] rows past the filter, [1] first row that cannot be built, [2] largest out-degree, [4 .. 9) edges by type, [9] candidates past test 1
  PGX_HIP(hipMemsetAsync(cnt.p, 0, 12 * sizeof(uint32_t), st));
  PGX_HIP(hipMemsetAsync(cnt.p + 1, 0xFF, sizeof(uint32_t), st));
  DevBuf<uint8_t> flag(n_rows);
  DevBuf<uint32_t> sel(n_rows);
  LAUNCH(k_sg_filter, n_rows, d_rows, n_rows, min_len, min_idt, flag.p, cnt.p);
  const uint32_t m = select_indices(flag.p, n_rows, sel.p, &tmp);
  uint32_t h_cnt[2];
  cnt.download(h_cnt, 2);
  pgx::sync();
  PGX_REQUIRE(h_cnt[1] == NO_ROW, PGX_EINVAL,
              "pgx_sgraph_build: kept row %u has m_size == 0 (its identity prints as nan or inf) or a read length of 2^31 and more", h_cnt[1]);
  g->st.rows_pass = h_cnt[0];
  PGX_REQUIRE((uint64_t)m * 4 <= (uint64_t)INT32_MAX, PGX_EINVAL, "pgx_sgraph_build: %u rows make edges: more than one device-wide sort takes (2^29 - 1)", m);
  if (m == 0) return;
  flag.release();
  const uint32_t n_e = 2 * m, n_k = 4 * m;
  g->edges.alloc(n_e);
  Edge *edges = g->edges.p;
  // ---- node ids in creation order
  DevBuf<uint32_t> node_of(n_k);
  uint32_t n_nodes = 0;
  {
    DevBuf<uint64_t> nkey(n_k), skey(n_k);
    DevBuf<uint32_t> npos(n_k), spos(n_k), first(n_k), rank((size_t)n_k + 1);
    DevBuf<int32_t> head(n_k);
    LAUNCH(k_sg_edges, m, d_rows, sel.p, m, edges, nkey.p, npos.p);
    sort_pairs(nkey.p, skey.p, npos.p, spos.p, n_k, 0, 33, &tmp);
    LAUNCH(k_sg_heads, n_k, skey.p, spos.p, n_k, first.p, head.p);
    n_nodes = scan_to_total(first.p, rank.p, n_k, &tmp);
    running_max(head.p, head.p, n_k, &tmp);
    LAUNCH(k_sg_node_ids, n_k, spos.p, head.p, rank.p, n_k, node_of.p);
  }
  sel.release();
  part.reset(), part.reset(new KernelTimer("sgraph_adj", n_e));
  // ---- adjacency: out-lists by (node, length, edge), in-lists by (node, edge)
  DevBuf<uint32_t> out_off((size_t)n_nodes + 1), in_off((size_t)n_nodes + 1), out_e(n_e), in_e(n_e), out_w(n_e), out_len(n_e);
  DevBuf<uint64_t> vw_key;
  DevBuf<uint32_t> vw_pos;
  const uint32_t cap = deg_cap();
  uint32_t max_deg = 0;
  {
    DevBuf<uint32_t> outdeg(n_nodes), indeg(n_nodes), ikey(n_e), ikey_s(n_e), iota(n_e);
    DevBuf<uint64_t> okey(n_e), okey_s(n_e);
    PGX_HIP(hipMemsetAsync(outdeg.p, 0, (size_t)n_nodes * sizeof(uint32_t), st));
    PGX_HIP(hipMemsetAsync(indeg.p, 0, (size_t)n_nodes * sizeof(uint32_t), st));
    LAUNCH(k_sg_degrees, n_e, node_of.p, edges, n_e, outdeg.p, indeg.p, okey.p, ikey.p, iota.p);
    scan_offsets(outdeg.p, out_off.p, n_nodes, &tmp);
    scan_offsets(indeg.p, in_off.p, n_nodes, &tmp);
    reduce_max(outdeg.p, cnt.p + 2, n_nodes, &tmp);
    sort_pairs(okey.p, okey_s.p, iota.p, out_e.p, n_e, 0, 64, &tmp);
    sort_pairs(ikey.p, ikey_s.p, iota.p, in_e.p, n_e, 0, 32, &tmp);
    PGX_HIP(hipMemcpyAsync(&max_deg, cnt.p + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    pgx::sync();
    if (max_deg > cap) {   // the nodes beyond the LDS tables look their neighbours up in the edge list sorted by (v, w)
      DevBuf<uint64_t> raw(n_e);
      DevBuf<uint32_t> raw_pos(n_e);
      vw_key.alloc(n_e), vw_pos.alloc(n_e);
      LAUNCH(k_sg_out_lists, n_e, out_e.p, okey_s.p, node_of.p, n_e, out_w.p, out_len.p, raw.p, raw_pos.p);
      sort_pairs(raw.p, vw_key.p, raw_pos.p, vw_pos.p, n_e, 0, 64, &tmp);
    } else {
      LAUNCH(k_sg_out_lists, n_e, out_e.p, okey_s.p, node_of.p, n_e, out_w.p, out_len.p, (uint64_t *)nullptr, (uint32_t *)nullptr);
    }
  }
  // ---- transitive reduction
  part.reset(), part.reset(new KernelTimer("sgraph_tr", n_e));
  DevBuf<uint8_t> type(n_e), best(n_e), nflag(n_nodes);
  PGX_HIP(hipMemsetAsync(type.p, 0, n_e, st));
  hipLaunchKernelGGL(k_sg_tr_lds, dim3(stride_grid(n_nodes, 32)), dim3(64), 0, st, n_nodes, cap, out_off.p, out_e.p, out_w.p,
                     out_len.p, type.p);
  if (max_deg > cap) {
    DevBuf<uint32_t> big(n_nodes), marks(n_e);
    LAUNCH(k_sg_big_flags, n_nodes, out_off.p, n_nodes, cap, nflag.p);
    const uint32_t n_big = select_indices(nflag.p, n_nodes, big.p, &tmp);
    PGX_HIP(hipMemsetAsync(marks.p, 0, (size_t)n_e * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_sg_tr_global, dim3(stride_grid(n_big, 32)), dim3(64), 0, st, big.p, n_big, out_off.p, out_e.p, out_w.p,
                       out_len.p, vw_key.p, vw_pos.p, n_e, marks.p, type.p);
    PGX_HIP(hipGetLastError());
    pgx::sync();   // (big and marks go back to the block cache behind the kernel anyway: one stream)
  }
  vw_key.release(), vw_pos.release();
  // ---- chimer bridge step
  if (chimer) {
    part.reset(), part.reset(new KernelTimer("sgraph_chimer", n_e));
    chimer_pass(g, n_nodes, n_e, max_deg, edges, node_of.p, out_off.p, out_e.p, out_w.p, in_off.p, in_e.p, type.p, cnt.p + 9, &tmp);
  }
  // ---- spur, best overlap, spur
  part.reset(), part.reset(new KernelTimer("sgraph_spur", n_e));
  DevBuf<uint32_t> cand(n_nodes);
  LAUNCH(k_sg_spur_flags, n_nodes, n_nodes, out_off.p, out_w.p, in_off.p, in_e.p, node_of.p, nflag.p);
  const uint32_t n_cand = select_indices(nflag.p, n_nodes, cand.p, &tmp);
  if (n_cand) hipLaunchKernelGGL(k_sg_spur, dim3(1), dim3(64), 0, st, cand.p, n_cand, out_off.p, out_e.p, in_off.p, in_e.p, node_of.p, type.p);
  part.reset(), part.reset(new KernelTimer("sgraph_best", n_e));
  PGX_HIP(hipMemsetAsync(best.p, 0, n_e, st));
  LAUNCH(k_sg_best, n_nodes, n_nodes, out_off.p, out_e.p, in_off.p, in_e.p, edges, type.p, best.p);
  LAUNCH(k_sg_not_best, m, m, best.p, type.p);
  part.reset(), part.reset(new KernelTimer("sgraph_spur", n_e));
  if (n_cand) hipLaunchKernelGGL(k_sg_spur, dim3(1), dim3(64), 0, st, cand.p, n_cand, out_off.p, out_e.p, in_off.p, in_e.p, node_of.p, type.p);
  part.reset();
  LAUNCH(k_sg_finish, n_e, edges, type.p, n_e, cnt.p + 4);
  PGX_HIP(hipGetLastError());
  uint32_t by_type[6];   // ([5]: the candidates past test 1)
  PGX_HIP(hipMemcpyAsync(by_type, cnt.p + 4, sizeof(by_type), hipMemcpyDeviceToHost, st));
  pgx::sync();
  g->st.edges = n_e, g->st.nodes = n_nodes, g->st.max_out_degree = max_deg, g->st.spur_candidates = n_cand;
  g->st.n_g = by_type[T_G], g->st.n_tr = by_type[T_TR], g->st.n_s = by_type[T_S], g->st.n_r = by_type[T_R];
  g->ch.c_edges = by_type[T_C], g->ch.past_test1 = by_type[5];
}

void require_graph(const pgx_sgraph *g, const char *who) {
  PGX_REQUIRE(g, PGX_EARG, "%s: null argument", who);
  PGX_REQUIRE(!g->shut && ctx().ready, PGX_ESTATE, "%s: pgx_shutdown ran while the graph was alive (free it)", who);
}
}  // namespace
const pgx_sgraph_edge *sgraph_device_edges(const pgx_sgraph *g, const char *who, uint64_t *n) {
  require_graph(g, who);
  *n = g->st.edges;
  return g->edges.p;
}
}  // namespace pgx

extern "C" int pgx_sgraph_build(pgx_dedup_stream *s, int64_t min_len, double min_idt, uint32_t flags, pgx_sgraph **out) {
  auto pre = [&] {
    PGX_REQUIRE(s, PGX_EARG, "pgx_sgraph_build: null argument");
    PGX_REQUIRE(!s->shut, PGX_ESTATE, "pgx_sgraph_build: pgx_shutdown ran while the stream was open (close it)");
    PGX_REQUIRE(!s->failed, PGX_ESTATE, "pgx_sgraph_build: the stream returned an error before (close it)");
    PGX_REQUIRE(s->graph, PGX_ESTATE, "pgx_sgraph_build: not a graph-mode stream (pgx_dedup_open_graph)");
    PGX_REQUIRE(!s->released, PGX_ESTATE, "pgx_sgraph_build: the stream's last line was drained: its rows are gone");
    PGX_REQUIRE(!(flags & PGX_SGRAPH_CHIMER_BRIDGE), PGX_EINVAL,
                "pgx_sgraph_build: the chimer bridge step as the script runs it is not offered (it pops from a set of objects: the script's own output "
                "changes with the hash seed); PGX_SGRAPH_CHIMER_ORDERED runs the step with a stated pop order, or run ovlp_to_graph.py with "
                "--disable_chimer_bridge_removal to compare");
    PGX_REQUIRE(!(flags & PGX_SGRAPH_LFC), PGX_EINVAL, "pgx_sgraph_build: --lfc is not offered (pg_run.py leaves it off)");
    PGX_REQUIRE((flags & ~PGX_SGRAPH_CHIMER_ORDERED) == 0, PGX_EINVAL, "pgx_sgraph_build: unknown flag bits 0x%x", flags & ~PGX_SGRAPH_CHIMER_ORDERED);
    PGX_REQUIRE(!(min_idt != min_idt), PGX_EARG, "pgx_sgraph_build: min_idt is not a number");
  };
  // (after a failure the stream is untouched: pgx_dedup_drain still has its rows)
  return live_build("pgx_sgraph_build", g_graphs, out, pre, [&](pgx_sgraph *g, uint64_t *n) {
    KernelTimer tm("sgraph", *n = s->store_n);
    if (!s->draining) graph_compact(s), *n = s->store_n;
    PGX_REQUIRE(s->store_n <= (uint64_t)INT32_MAX, PGX_EINVAL, "pgx_sgraph_build: %llu kept rows, more than 2^31 - 1", (unsigned long long)s->store_n);
    build_graph(s->store.p, (uint32_t)s->store_n, min_len, min_idt, (flags & PGX_SGRAPH_CHIMER_ORDERED) != 0, g);
  }, "graph", "rows");
}

extern "C" int pgx_sgraph_stats(const pgx_sgraph *g, pgx_sgraph_stats_t *out) {
  return guarded([&] {
    PGX_REQUIRE(g && out, PGX_EARG, "pgx_sgraph_stats: null argument");
    *out = g->st;
  });
}

extern "C" int pgx_sgraph_chimer_stats(const pgx_sgraph *g, pgx_sgraph_chimer_stats_t *out) {
  return guarded([&] {
    PGX_REQUIRE(g && out, PGX_EARG, "pgx_sgraph_chimer_stats: null argument");
    *out = g->ch;
  });
}

// the chimers_nodes file (:854-856): a chosen node's name, then its reverse end's; formatted on the host from the keys the build kept
extern "C" int pgx_sgraph_chimer_nodes(const pgx_sgraph *g, char **text, size_t *len) {
  return text_call(text, len, nullptr, [&] {
    PGX_REQUIRE(g && text && len, PGX_EARG, "pgx_sgraph_chimer_nodes: null argument");
    std::string s;
    char line[32];
    for (const uint64_t key : g->chimers)
      for (const uint64_t k : {key, key ^ 1u}) {
        snprintf(line, sizeof line, "%09d:%c\n", (int)(int32_t)(uint32_t)(k >> 1), (k & 1) ? 'E' : 'B');
        s += line;
      }
    *text = caller_text(s.data(), s.size());
    *len = s.size();
  });
}

extern "C" int pgx_sgraph_edges(const pgx_sgraph *g, uint64_t first, uint64_t n, pgx_sgraph_edge *out) {
  return guarded([&] {
    require_graph(g, "pgx_sgraph_edges");
    PGX_REQUIRE(first <= g->st.edges && n <= g->st.edges - first && (n == 0 || out), PGX_EARG, "pgx_sgraph_edges: edges %llu .. + %llu of %llu",
                (unsigned long long)first, (unsigned long long)n, (unsigned long long)g->st.edges);
    if (n == 0) return;
    PGX_HIP(hipMemcpyAsync(out, g->edges.p + first, n * sizeof(Edge), hipMemcpyDeviceToHost, ctx().stream));
    pgx::sync();
  });
}

extern "C" int pgx_sgraph_text(pgx_sgraph *g, uint64_t max_lines, char **text, size_t *text_len, int *done) {
  return text_call(text, text_len, done, [&] {
    require_graph(g, "pgx_sgraph_text");
    PGX_REQUIRE(text && text_len && done && max_lines, PGX_EARG, "pgx_sgraph_text: null argument or max_lines == 0");
    hipStream_t st = ctx().stream;
    const uint32_t m = (uint32_t)text_lines(max_lines, g->st.edges - g->cursor);
    if (m == 0) {
      text_hand_out(g->stage, nullptr, 0, text, text_len);
    } else {
      KernelTimer tm("sgraph", m), tm_text("sgraph_text", m);
      const Edge *edges = g->edges.p + g->cursor;
      uint64_t *d_off = ws<uint64_t>("sg.off", (size_t)m + 1), *d_len = ws<uint64_t>("sg.len", (size_t)m + 1);
      LAUNCH(k_sg_line_len, (size_t)m + 1, edges, m, d_len);
      exclusive_sum(d_len, d_off, (size_t)m + 1);
      uint64_t total = 0;
      PGX_HIP(hipMemcpyAsync(&total, d_off + m, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
      pgx::sync();
      char *d_text = ws<char>("sg.text", total);
      hipLaunchKernelGGL(k_sg_format, dim3(cdiv(m, SG_TILE)), dim3(SG_TILE), 0, st, edges, d_off, m, d_text);
      PGX_HIP(hipGetLastError());
      text_hand_out(g->stage, d_text, total, text, text_len);
    }
    g->cursor += m;
    if (g->cursor == g->st.edges) *done = 1;
    timing_flush();
  });
}

extern "C" int pgx_sgraph_free(pgx_sgraph *g) {
  if (g) g_graphs.destroy(g);
  return PGX_OK;
}
