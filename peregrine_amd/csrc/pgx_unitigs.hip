// pgx_unitigs.hip -- phase 1 of unitig construction (py/scripts/ovlp_to_graph.py: identify_simple_paths, :1033-1144, and the utg_data
// line of :1478-1487): the maximal simple paths of the string graph's G edges, as a table, a path array and text.  The rule (DESIGN.md,
// "unitigs"), over the edges in creation order, G edges only:
//   * a node is simple when its G in-degree and out-degree are both 1;
//   * every edge that leaves a non-simple node starts a linear unitig, which follows the single out-edge of every simple node it reaches;
//   * what no such start reaches lies on rings of simple nodes: a ring is one circular unitig, cut at the tail of its edge with the
//     smallest creation index;
//   * unitigs are numbered by the creation index of their first edge; `via` is the path's second node.
// Device layout.  G edges are numbered gi = 0 .. m-1 in creation order (gsel[gi]: the creation index).  A node is its key
// (rid << 1) | end; there are no node ids: degrees and the single in- / out-edge of a node are ranges of the two sorted edge lists
// of pgx_gedges.h
//   by_w   (wkey, gi) ascending                (in-lists)
//   by_vw  (vkey, wkey, gi) ascending          (out-lists; equal neighbours are duplicates; the reverse of an edge is looked up here)
// found by binary search.  pred[gi] / succ[gi]: the edge before / after gi on its path, where the node between them is simple.
// List ranking (the hot path) is pointer doubling over pred: after round r an edge knows the 2^r edges before it -- their number, the sums
// of length and score, the earliest of them, the smallest index among them -- or has reached the first edge of its path.  What still has
// a pointer after ceil(log2 m) rounds lies on a ring, and has by then seen the whole ring: the edge that is the ring's minimum loses its
// pred, and a second ranking settles the rings like paths.
// No result depends on the order in which atomics land: they take a minimum (the first offending edge) or count.

#include <atomic>

#include "pgx_gedges.h"

typedef pgx_sgraph_edge Edge;

namespace pgx {
namespace {
// ---------------------------------------------------------------------------------------------------------
// edges -> keys, sorted lists, checks, links
// ---------------------------------------------------------------------------------------------------------
// the unitigs' rule on a G edge: it joins two reads
struct TwoReads {
  __device__ bool operator()(const Edge &e) const { return e.v_rid == e.w_rid; }
};
// is a node simple; lo_out / lo_in: where its out-list / in-list starts
__device__ inline bool node_simple(uint64_t x, const uint64_t *__restrict__ sv, const uint64_t *__restrict__ swk, uint32_t m, uint32_t &lo_out, uint32_t &lo_in) {
  lo_out = lower_bound(sv, m, x), lo_in = lower_bound(swk, m, x);
  return lower_bound(sv, m, x + 1) - lo_out == 1 && lower_bound(swk, m, x + 1) - lo_in == 1;
}
// pred / succ of every edge; err[2] = min(err[2], creation index of an edge whose reverse is missing)
__global__ void k_ut_links(const uint64_t *__restrict__ vk, const uint64_t *__restrict__ wk, const uint64_t *__restrict__ sv, const uint64_t *__restrict__ sw,
                           const uint32_t *__restrict__ out_e, const uint64_t *__restrict__ swk, const uint32_t *__restrict__ in_e,
                           const uint32_t *__restrict__ gsel, uint32_t m, uint32_t *__restrict__ pred, uint32_t *__restrict__ succ, uint32_t *__restrict__ err) {
  const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
  if (gi >= m) return;
  const uint64_t v = vk[gi], w = wk[gi];
  if (find_vw(sv, sw, m, w ^ 1u, v ^ 1u) == NONE) atomicMin(&err[2], gsel[gi]);   // the reverse (w ^ 1, v ^ 1)
  uint32_t lo_out, lo_in;
  succ[gi] = node_simple(w, sv, swk, m, lo_out, lo_in) ? out_e[lo_out] : NONE;
  pred[gi] = node_simple(v, sv, swk, m, lo_out, lo_in) ? in_e[lo_in] : NONE;
}

// ---------------------------------------------------------------------------------------------------------
// list ranking
// ---------------------------------------------------------------------------------------------------------
// what an edge knows of the `cnt` edges that end with it: h the earliest of them, p the edge before h (NONE: h starts the path), mn their
// smallest index, the sums of their lengths and scores
struct alignas(16) Rank {
  uint32_t p, cnt, h, mn;
  int64_t len, score;
};
__device__ inline void count_active(bool a, uint32_t *active) {
  const uint64_t b = __ballot(a);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(active, (uint32_t)__popcll(b));
}
__global__ void k_ut_rank_init(const Edge *__restrict__ edges, const uint32_t *__restrict__ gsel, const uint32_t *__restrict__ pred, uint32_t m,
                               Rank *__restrict__ out, uint32_t *__restrict__ active) {
  const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
  bool a = false;
  if (gi < m) {
    const Edge e = edges[gsel[gi]];
    const int64_t d = (int64_t)e.sp - (int64_t)e.tp;
    out[gi] = Rank{pred[gi], 1u, gi, gi, d < 0 ? -d : d, e.score};
    a = pred[gi] != NONE;
  }
  count_active(a, active);
}
// one doubling round: in -> out (two buffers: a round reads only what the last one wrote)
__global__ void k_ut_rank_jump(const Rank *__restrict__ in, Rank *__restrict__ out, uint32_t m, uint32_t *__restrict__ active) {
  const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
  bool a = false;
  if (gi < m) {
    Rank s = in[gi];
    if (s.p != NONE) {
      const Rank q = in[s.p];
      s.cnt += q.cnt, s.len += q.len, s.score += q.score, s.h = q.h, s.mn = min(s.mn, q.mn), s.p = q.p;
      a = s.p != NONE;
    }
    out[gi] = s;
  }
  count_active(a, active);
}
// after the full number of rounds: an edge that still has a pointer lies on a ring and mn is the ring's smallest index; that edge is the cut
__global__ void k_ut_cut(const Rank *__restrict__ r, uint32_t m, uint32_t *__restrict__ pred, uint8_t *__restrict__ circ) {
  const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
  if (gi < m && r[gi].p != NONE && r[gi].mn == gi) pred[gi] = NONE, circ[gi] = 1;
}

// ---------------------------------------------------------------------------------------------------------
// assembly
// ---------------------------------------------------------------------------------------------------------
__global__ void k_ut_first_flags(const uint32_t *__restrict__ pred, uint32_t m, uint8_t *__restrict__ flag) {
  const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
  if (gi < m) flag[gi] = pred[gi] == NONE;
}
// the unitig's number at its first edge, and what the first edge says of the unitig
__global__ void k_ut_heads(const uint32_t *__restrict__ firsts, uint32_t n_u, const uint64_t *__restrict__ vk, const uint64_t *__restrict__ wk,
                           const uint8_t *__restrict__ circ, uint32_t *__restrict__ uid_of, pgx_unitig *__restrict__ tab, uint32_t *__restrict__ n_circ) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  bool c = false;
  if (u < n_u) {
    const uint32_t gi = firsts[u];
    uid_of[gi] = u;
    c = circ[gi] != 0;
    pgx_unitig &t = tab[u];
    t.s_rid = (uint32_t)(vk[gi] >> 1), t.s_end = (uint8_t)(vk[gi] & 1), t.via_rid = (uint32_t)(wk[gi] >> 1), t.via_end = (uint8_t)(wk[gi] & 1), t.circular = c;
  }
  count_active(c, n_circ);
}
// ... and what the last edge says: the one without a successor, or whose successor is a ring's cut
__global__ void k_ut_tails(const Rank *__restrict__ r, const uint32_t *__restrict__ succ, const uint8_t *__restrict__ circ, const uint64_t *__restrict__ wk,
                           const uint32_t *__restrict__ uid_of, uint32_t m, uint32_t n_u, pgx_unitig *__restrict__ tab, uint32_t *__restrict__ n_edges,
                           uint32_t *__restrict__ broken) {
  const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
  if (gi >= m) return;
  const uint32_t s = succ[gi];
  if (s != NONE && !circ[s]) return;
  const Rank k = r[gi];
  const uint32_t u = uid_of[k.h];
  if (u >= n_u) {   // (never: h is a first edge.  Checked because the index goes into a store)
    atomicAdd(broken, 1u);
    return;
  }
  pgx_unitig &t = tab[u];
  t.t_rid = (uint32_t)(wk[gi] >> 1), t.t_end = (uint8_t)(wk[gi] & 1), t.n_edges = k.cnt, t.length = k.len, t.score = k.score;
  n_edges[u] = k.cnt;
}
__global__ void k_ut_scatter(const Rank *__restrict__ r, const uint32_t *__restrict__ uid_of, const uint64_t *__restrict__ off, const uint32_t *__restrict__ gsel,
                             const uint64_t *__restrict__ wk, uint32_t m, uint32_t n_u, uint32_t *__restrict__ paths, uint32_t *__restrict__ slot_u,
                             uint64_t *__restrict__ slot_w, uint32_t *__restrict__ broken) {
  const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
  if (gi >= m) return;
  const uint32_t u = uid_of[r[gi].h];
  const uint64_t slot = u < n_u ? off[u] + (r[gi].cnt - 1) : m;
  if (slot >= off[min(u, n_u - 1) + 1] || u >= n_u) {   // (never, as above)
    atomicAdd(broken, 1u);
    return;
  }
  paths[slot] = gsel[gi], slot_u[slot] = u, slot_w[slot] = wk[gi];
}
__global__ void k_ut_firsts(const uint64_t *__restrict__ off, uint32_t n_u, pgx_unitig *__restrict__ tab) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u < n_u) tab[u].first = off[u];
}

// ---------------------------------------------------------------------------------------------------------
// the text: 's via t simple length score n0~n1~...~nk', a line per unitig.  A line is cut into pieces, one per path slot: the node the
// slot's edge enters and what follows it ('~', or '\n' behind the line's last); the first slot's piece starts with the line's head and
// the path's first node.  The piece source of pgx_text.h's piece scheme, which lays the text out and formats it.
// ---------------------------------------------------------------------------------------------------------
struct SlotPieces {
  const uint32_t *__restrict__ slot_u;
  const uint64_t *__restrict__ slot_w;
  const pgx_unitig *__restrict__ tab;
  uint32_t n;                                  // path slots
  static constexpr uint32_t MAX = 128;   // 5 names of <= 13, " simple ", two numbers of <= 20, 4 blanks, 2 separators = 119
  template <bool WRITE>
  __device__ uint32_t piece(uint32_t j, char *dst) const {
    LineOut<WRITE> o{dst, 0};
    const uint32_t u = slot_u[j];
    const uint64_t slot = j, w = slot_w[j], first = tab[u].first;
    const uint32_t n_edges = tab[u].n_edges;
    if (slot == first) {
      const pgx_unitig t = tab[u];
      o.node(t.s_rid, t.s_end), o.ch(' '), o.node(t.via_rid, t.via_end), o.ch(' '), o.node(t.t_rid, t.t_end);
      for (const char *c = " simple "; *c; ++c) o.ch(*c);
      o.i64(t.length), o.ch(' '), o.i64(t.score), o.ch(' ');
      o.node(t.s_rid, t.s_end), o.ch('~');
    }
    o.node((uint32_t)(w >> 1), (uint32_t)(w & 1));
    o.ch(slot == first + n_edges - 1 ? '\n' : '~');
    return o.n;
  }
};
}  // namespace
}  // namespace pgx

using namespace pgx;

struct pgx_unitigs {
  DevBuf<pgx_unitig> tab;        // the unitigs in order (MemTag "unitigs", as all of these)
  DevBuf<uint32_t> paths;        // creation indices, unitig after unitig
  DevBuf<uint32_t> slot_u;       // per path slot: its unitig
  DevBuf<uint64_t> slot_w;       // ... and the key of the node its edge enters
  TextPlan text;                 // a piece per path slot, a line per unitig
  pgx_unitigs_stats_t st = {};
  uint64_t serial = 0;           // of this object among all unitigs ever built (> 0): an address may come again, a serial does not
  TextStage stage;
  bool shut = false;
  void drop_device_state() {
    tab.release(), paths.release(), slot_u.release(), slot_w.release(), text.release();
    stage.drop();
  }
};

namespace pgx {
namespace {
LiveSet<pgx_unitigs> g_ut;
ShutdownHook g_ut_hook([] { g_ut.shutdown(); });
std::atomic<uint64_t> g_ut_serials{0};
SlotPieces slot_pieces(const pgx_unitigs *u) { return SlotPieces{u->slot_u.p, u->slot_w.p, u->tab.p, (uint32_t)u->st.g_edges}; }

// pointer doubling over pred until every edge has reached the start of its path, max_rounds at the most; returns the edges that still
// have a pointer.  The answer is in *cur.
uint32_t rank_edges(const Edge *d_edges, const uint32_t *gsel, const uint32_t *pred, uint32_t m, uint32_t max_rounds, Rank **cur, Rank **other, uint32_t *d_active) {
  hipStream_t st = ctx().stream;
  uint32_t active = 0;
  auto counted = [&](auto &&launch) {
    PGX_HIP(hipMemsetAsync(d_active, 0, sizeof(uint32_t), st));
    launch();
    PGX_HIP(hipGetLastError());
    PGX_HIP(hipMemcpyAsync(&active, d_active, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    pgx::sync();
  };
  counted([&] { LAUNCH(k_ut_rank_init, m, d_edges, gsel, pred, m, *cur, d_active); });
  for (uint32_t round = 0; active && round < max_rounds; ++round) {
    counted([&] { LAUNCH(k_ut_rank_jump, m, *cur, *other, m, d_active); });
    std::swap(*cur, *other);
  }
  return active;
}

// the unitigs of the n edge records at d_edges; fills u
void build_unitigs(const Edge *d_edges, uint64_t n64, pgx_unitigs *u) {
  hipStream_t st = ctx().stream;
  MemTag tag("unitigs");
  PrimWs tmp;
  PGX_REQUIRE(n64 <= (uint64_t)INT32_MAX, PGX_EINVAL, "pgx_unitigs: %llu edge records, more than 2^31 - 1", (unsigned long long)n64);
  const uint32_t n = (uint32_t)n64;
  if (n == 0) return;
  // ---- G edges, keys, the two sorted lists, the checks, pred / succ
  std::unique_ptr<KernelTimer> part(new KernelTimer("unitigs_links", n));
  GEdges g;
  g.select(d_edges, n, &tmp);
  const uint32_t m = g.m;
  u->st.g_edges = m;
  if (m == 0) return;
  DevBuf<uint32_t> cnt(8);   // [0 .. 3) first offending edge of each rule, [4] edges with a pointer, [5] circular unitigs, [6] longest, [7] edges that found no place
  PGX_HIP(hipMemsetAsync(cnt.p, 0xFF, 4 * sizeof(uint32_t), st));
  PGX_HIP(hipMemsetAsync(cnt.p + 4, 0, 4 * sizeof(uint32_t), st));
  DevBuf<uint32_t> pred(m), succ(m);
  g.keys(TwoReads{}, cnt.p);
  g.by_w(&tmp);
  g.by_vw(cnt.p + 1, &tmp);
  LAUNCH(k_ut_links, m, g.vk.p, g.wk.p, g.sv.p, g.sw.p, g.out_e.p, g.swk.p, g.in_e.p, g.gsel.p, m, pred.p, succ.p, cnt.p);
  PGX_HIP(hipGetLastError());
  {
    uint32_t err[3];
    cnt.download(err, 3);
    pgx::sync();
    PGX_REQUIRE(err[0] == NONE, PGX_EINVAL, "pgx_unitigs: G edge %u joins the two ends of one read (v_rid == w_rid)", err[0]);
    PGX_REQUIRE(err[1] == NONE, PGX_EINVAL, "pgx_unitigs: G edge %u repeats the (v, w) of an earlier G edge", err[1]);
    PGX_REQUIRE(err[2] == NONE, PGX_EINVAL, "pgx_unitigs: G edge %u has no reverse (rev w, rev v) among the G edges", err[2]);
  }
  g.release_lists();
  // ---- list ranking
  part.reset(), part.reset(new KernelTimer("unitigs_rank", m));
  DevBuf<Rank> ra(m), rb(m);
  DevBuf<uint8_t> circ(m);
  PGX_HIP(hipMemsetAsync(circ.p, 0, m, st));
  Rank *cur = ra.p, *other = rb.p;
  uint32_t full = 0;
  while (full < 31 && (1u << full) < m) ++full;   // 2^full >= m: no path is longer
  if (rank_edges(d_edges, g.gsel.p, pred.p, m, full, &cur, &other, cnt.p + 4)) {
    LAUNCH(k_ut_cut, m, cur, m, pred.p, circ.p);
    const uint32_t left = rank_edges(d_edges, g.gsel.p, pred.p, m, full, &cur, &other, cnt.p + 4);
    PGX_REQUIRE(left == 0, PGX_EHIP, "pgx_unitigs: %u edges are not ranked (a bug)", left);
  }
  // ---- assembly
  part.reset(), part.reset(new KernelTimer("unitigs_paths", m));
  uint32_t n_u = 0;
  DevBuf<uint32_t> uid_of(m), firsts(m);
  {
    DevBuf<uint8_t> flag(m);
    LAUNCH(k_ut_first_flags, m, pred.p, m, flag.p);
    n_u = select_indices(flag.p, m, firsts.p, &tmp);
  }
  u->tab.alloc(n_u), u->paths.alloc(m), u->slot_u.alloc(m), u->slot_w.alloc(m);
  DevBuf<uint32_t> n_edges(n_u);
  PGX_HIP(hipMemsetAsync(uid_of.p, 0xFF, (size_t)m * sizeof(uint32_t), st));
  PGX_HIP(hipMemsetAsync(n_edges.p, 0, (size_t)n_u * sizeof(uint32_t), st));
  DevBuf<uint64_t> off((size_t)n_u + 1);
  PGX_HIP(hipMemsetAsync(u->tab.p, 0, (size_t)n_u * sizeof(pgx_unitig), st));
  LAUNCH(k_ut_heads, n_u, firsts.p, n_u, g.vk.p, g.wk.p, circ.p, uid_of.p, u->tab.p, cnt.p + 5);
  LAUNCH(k_ut_tails, m, cur, succ.p, circ.p, g.wk.p, uid_of.p, m, n_u, u->tab.p, n_edges.p, cnt.p + 7);
  reduce_max(n_edges.p, cnt.p + 6, n_u, &tmp);
  const uint64_t total_edges = scan_to_total(n_edges.p, off.p, n_u, &tmp);
  PGX_REQUIRE(total_edges == m, PGX_EHIP, "pgx_unitigs: the unitigs hold %llu of %u edges (a bug)", (unsigned long long)total_edges, m);
  LAUNCH(k_ut_firsts, n_u, off.p, n_u, u->tab.p);
  LAUNCH(k_ut_scatter, m, cur, uid_of.p, off.p, g.gsel.p, g.wk.p, m, n_u, u->paths.p, u->slot_u.p, u->slot_w.p, cnt.p + 7);
  // ---- where the text of every piece and line starts
  part.reset(), part.reset(new KernelTimer("unitigs_text", m));
  plan_text(slot_pieces(u), off.p, n_u, &u->text, &tmp);
  uint32_t h[3];
  PGX_HIP(hipMemcpyAsync(h, cnt.p + 5, sizeof(h), hipMemcpyDeviceToHost, st));
  pgx::sync();
  part.reset();
  PGX_REQUIRE(h[2] == 0, PGX_EHIP, "pgx_unitigs: %u edges found no place in a path (a bug)", h[2]);
  u->st.unitigs = n_u, u->st.circular = h[0], u->st.longest_edges = h[1];
}

void require_unitigs(const pgx_unitigs *u, const char *who) {
  PGX_REQUIRE(u, PGX_EARG, "%s: null argument", who);
  PGX_REQUIRE(!u->shut && ctx().ready, PGX_ESTATE, "%s: pgx_shutdown ran while the unitigs were alive (free them)", who);
}

}  // namespace
UnitigsView unitigs_device_view(const pgx_unitigs *u, const char *who) {
  require_unitigs(u, who);
  return UnitigsView{u->tab.p, u->paths.p, u->slot_u.p, u->slot_w.p, u->st.unitigs, u->st.g_edges, u->serial};
}
bool unitigs_live(const pgx_unitigs *u, uint64_t serial) { return u && g_ut.contains(u) && u->serial == serial && !u->shut && ctx().ready; }
namespace {

// the common part of the two builders: edges() answers the device edge records once the context is known to be up
template <class EdgesFn>
int build_entry(const char *who, pgx_unitigs **out, EdgesFn &&edges) {
  return live_build(who, g_ut, out, [] {}, [&](pgx_unitigs *u, uint64_t *n) {
    MemTag tag("unitigs");
    DevBuf<Edge> own;
    const Edge *d_edges = edges(own, n);
    KernelTimer tm("unitigs", *n);
    u->serial = ++g_ut_serials;
    build_unitigs(d_edges, *n, u);
  }, "unitigs", "edges");
}
}  // namespace
}  // namespace pgx

extern "C" int pgx_sgraph_unitigs(pgx_sgraph *g, pgx_unitigs **out) {
  return build_entry("pgx_sgraph_unitigs", out, [&](DevBuf<Edge> &, uint64_t *n) { return sgraph_device_edges(g, "pgx_sgraph_unitigs", n); });
}

extern "C" int pgx_unitigs_build(const pgx_sgraph_edge *edges, uint64_t n, pgx_unitigs **out) {
  return build_entry("pgx_unitigs_build", out, [&](DevBuf<Edge> &own, uint64_t *n_out) -> const Edge * {
    PGX_REQUIRE(edges || n == 0, PGX_EARG, "pgx_unitigs_build: null argument");
    PGX_REQUIRE(n <= (uint64_t)INT32_MAX, PGX_EINVAL, "pgx_unitigs_build: %llu edge records, more than 2^31 - 1", (unsigned long long)n);
    *n_out = n;
    if (n == 0) return nullptr;
    own.alloc(n);
    own.upload(edges, n);
    return own.p;
  });
}

extern "C" int pgx_unitigs_stats(const pgx_unitigs *u, pgx_unitigs_stats_t *out) {
  return guarded([&] {
    PGX_REQUIRE(out, PGX_EARG, "pgx_unitigs_stats: null argument");
    require_unitigs(u, "pgx_unitigs_stats");
    *out = u->st;
  });
}

extern "C" int pgx_unitigs_table(const pgx_unitigs *u, uint64_t first, uint64_t n, pgx_unitig *out) {
  return guarded([&] {
    require_unitigs(u, "pgx_unitigs_table");
    PGX_REQUIRE(first <= u->st.unitigs && n <= u->st.unitigs - first && (n == 0 || out), PGX_EARG, "pgx_unitigs_table: unitigs %llu .. + %llu of %llu",
                (unsigned long long)first, (unsigned long long)n, (unsigned long long)u->st.unitigs);
    if (n == 0) return;
    PGX_HIP(hipMemcpyAsync(out, u->tab.p + first, n * sizeof(pgx_unitig), hipMemcpyDeviceToHost, ctx().stream));
    pgx::sync();
  });
}

extern "C" int pgx_unitigs_paths(const pgx_unitigs *u, uint64_t first, uint64_t n, uint32_t *edge_index) {
  return guarded([&] {
    require_unitigs(u, "pgx_unitigs_paths");
    PGX_REQUIRE(first <= u->st.g_edges && n <= u->st.g_edges - first && (n == 0 || edge_index), PGX_EARG, "pgx_unitigs_paths: path entries %llu .. + %llu of %llu",
                (unsigned long long)first, (unsigned long long)n, (unsigned long long)u->st.g_edges);
    if (n == 0) return;
    PGX_HIP(hipMemcpyAsync(edge_index, u->paths.p + first, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx().stream));
    pgx::sync();
  });
}

extern "C" int pgx_unitigs_text(pgx_unitigs *u, uint64_t max_lines, char **text, size_t *text_len, int *done) {
  return text_call(text, text_len, done, [&] {
    require_unitigs(u, "pgx_unitigs_text");
    text_next("pgx_unitigs_text", u->text, slot_pieces(u), u->stage, TextNames{"unitigs", "unitigs_text", "unitigs", "ut.text"}, max_lines, text, text_len, done);
  });
}

extern "C" int pgx_unitigs_free(pgx_unitigs *u) {
  if (u) g_ut.destroy(u);
  return PGX_OK;
}
