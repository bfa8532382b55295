// pgx_ctgpaths.hip -- the phases py/scripts/ovlp_to_graph.py runs after identify_simple_paths (:1147-1555), on the unitigs of pgx_unitigs.hip:
// the unitig graph, the two spur passes, duplicate short paths, compound paths, repeat bridges, the contig walks and the greedy claim, and
// the two files they end in, utg_data and ctg_paths.  The rule is the script's algorithm with every unordered container given an order
// (DESIGN.md 4.5e): a node is its key (rid << 1) | end, a unitig its index, sets pop their smallest element, a node's edges iterate in
// ascending unitig index.
// The split (as 4.5d's): what is a pass over all G edges or all unitigs, and all text, runs on the device --
//   * the nodes of the unitig graph (the distinct s / t keys, sorted: a node's id is its rank), each unitig's two node ids, the in- and
//     out-lists (two stable sorts: ascending unitig index within a node) and their offsets;
//   * the dual of every unitig (the one that starts (t ^ 1, tail of the last edge ^ 1)), looked up in the out-lists;
//   * best_in of every node: the tail of the G edge entering it with the largest creation index (atomicMax on the index: the order the
//     atomics land in does not matter; the one winner of a node then writes the tail);
//   * both texts: a line is cut into pieces (a path slot of a simple unitig, or one `s~via~t` of a compound line or a contig line), the
//     pieces' lengths are scanned, and a workgroup formats a tile of 8 KiB of the file.  The simple lines read the unitigs' own slot
//     arrays: nothing of them is copied.
//   * the contig walks: a lane per start edge follows the single out-edge of every node it passes (k_cp_walk); its node set is what it
//     has claimed in a per-node owner array, and the walks that share a stretch settle in rounds.
// The serial cascades over the unitig TABLE run on the host, once, on arrays brought down behind one synchronisation: the spur passes, the
// bundle search and its filters, the repeat bridges and the claim (host_us reports them), and the few walks no start node reaches.  No
// launch and no round trip per unitig, contig or bundle.

#include <map>
#include <set>
#include <unordered_map>
#include <unordered_set>

#include "pgx_gedges.h"

namespace pgx {
namespace {
constexpr uint64_t NA = ~0ULL;   // the via of a compound unitig
enum : uint32_t { T_SIMPLE, T_SPUR2, T_DUP, T_CONTAINED, T_BRIDGE, T_COMPOUND, N_TYPES };

// ---------------------------------------------------------------------------------------------------------
// the unitig graph
// ---------------------------------------------------------------------------------------------------------
__global__ void k_cp_keys(const pgx_unitig *__restrict__ tab, const uint64_t *__restrict__ slot_w, uint32_t n_u, uint64_t *__restrict__ st_keys,
                          uint64_t *__restrict__ last_tail) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_u) return;
  const pgx_unitig t = tab[u];
  const uint64_t s = (uint64_t)t.s_rid << 1 | t.s_end;
  st_keys[2 * (size_t)u] = s, st_keys[2 * (size_t)u + 1] = (uint64_t)t.t_rid << 1 | t.t_end;
  last_tail[u] = t.n_edges > 1 ? slot_w[t.first + t.n_edges - 2] : s;
}
__global__ void k_cp_node_ids(const pgx_unitig *__restrict__ tab, const uint64_t *__restrict__ nodes, uint32_t n_nodes, uint32_t n_u, uint32_t *__restrict__ s_node,
                              uint32_t *__restrict__ t_node, uint32_t *__restrict__ iota) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_u) return;
  const pgx_unitig t = tab[u];
  s_node[u] = lower_bound(nodes, n_nodes, (uint64_t)t.s_rid << 1 | t.s_end);   // (present: the nodes are these keys)
  t_node[u] = lower_bound(nodes, n_nodes, (uint64_t)t.t_rid << 1 | t.t_end);
  iota[u] = u;
}
__global__ void k_cp_offsets(const uint32_t *__restrict__ sorted_s, const uint32_t *__restrict__ sorted_t, uint32_t n_u, uint32_t n_nodes, uint32_t *__restrict__ out_off,
                             uint32_t *__restrict__ in_off) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x > n_nodes) return;
  out_off[x] = lower_bound(sorted_s, n_u, x), in_off[x] = lower_bound(sorted_t, n_u, x);
}
// dual[u]: the unitig that leaves t ^ 1 through (tail of u's last edge) ^ 1; a ring has none.  err[0] = min(err[0], u without one)
__global__ void k_cp_duals(const pgx_unitig *__restrict__ tab, const uint64_t *__restrict__ last_tail, const uint64_t *__restrict__ nodes, uint32_t n_nodes,
                           const uint32_t *__restrict__ out_off, const uint32_t *__restrict__ out_list, uint32_t n_u, uint32_t *__restrict__ dual, uint32_t *__restrict__ err) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_u) return;
  const pgx_unitig t = tab[u];
  uint32_t d = NONE;
  if (!t.circular) {
    const uint64_t rs = ((uint64_t)t.t_rid << 1 | t.t_end) ^ 1u, rvia = last_tail[u] ^ 1u;
    const uint32_t x = lower_bound(nodes, n_nodes, rs);
    if (x < n_nodes && nodes[x] == rs)
      for (uint32_t k = out_off[x]; k < out_off[x + 1] && d == NONE; ++k) {
        const pgx_unitig c = tab[out_list[k]];
        if (((uint64_t)c.via_rid << 1 | c.via_end) == rvia) d = out_list[k];
      }
    if (d == NONE) atomicMin(&err[0], u);
  }
  dual[u] = d;
}
// best[x] = 1 + the largest creation index among the G edges that enter node x
__global__ void k_cp_best(const uint64_t *__restrict__ slot_w, const uint32_t *__restrict__ paths, uint32_t m, const uint64_t *__restrict__ nodes, uint32_t n_nodes,
                          uint32_t *__restrict__ best) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const uint64_t w = slot_w[j];
  const uint32_t x = lower_bound(nodes, n_nodes, w);
  if (x < n_nodes && nodes[x] == w) atomicMax(&best[x], paths[j] + 1u);
}
// ... and the tail of that edge (one slot per node wins)
__global__ void k_cp_best_tail(const uint64_t *__restrict__ slot_w, const uint32_t *__restrict__ slot_u, const uint32_t *__restrict__ paths, const pgx_unitig *__restrict__ tab,
                               uint32_t m, const uint64_t *__restrict__ nodes, uint32_t n_nodes, const uint32_t *__restrict__ best, uint64_t *__restrict__ best_tail) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const uint64_t w = slot_w[j];
  const uint32_t x = lower_bound(nodes, n_nodes, w);
  if (!(x < n_nodes && nodes[x] == w) || best[x] != paths[j] + 1u) return;
  const pgx_unitig t = tab[slot_u[j]];
  best_tail[x] = j == t.first ? ((uint64_t)t.s_rid << 1 | t.s_end) : slot_w[j - 1];
}

// ---------------------------------------------------------------------------------------------------------
// the contig walks (construct_c_path_from_utgs), a lane per start edge
// ---------------------------------------------------------------------------------------------------------
struct WalkG {   // the unitig graph as the cascades left it
  const uint32_t *eS, *eT, *type;         // per entry: tail and head node, final type
  const int64_t *len;
  const uint64_t *via, *last_tail;
  const uint32_t *sub_off, *sub;          // per compound entry (index - n_u): its bundle
  uint32_t n_u;
  const uint64_t *key, *best_tail;        // per node
  const uint32_t *in_deg, *out_deg, *single_out, *rev;
};
// may a walk that arrives through u go on through its head t, and what u then adds to path_length (the best_in test of :1317-1332)
__global__ void k_cp_edge_pass(WalkG g, const uint8_t *__restrict__ alive, uint32_t n_all, uint8_t *__restrict__ pass, int64_t *__restrict__ contrib) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_all) return;
  bool ok = alive[u] != 0;
  int64_t ln = g.len[u];
  const uint32_t t = g.eT[u];
  if (ok && g.in_deg[t] > 1) {
    const uint64_t b = g.best_tail[t];
    if (g.type[u] == T_SIMPLE) {
      ok = b == g.last_tail[u];
    } else if (g.type[u] == T_COMPOUND) {
      bool found = false;
      for (uint32_t k = g.sub_off[u - g.n_u]; k < g.sub_off[u - g.n_u + 1]; ++k) {
        const uint32_t x = g.sub[k];
        if (g.via[x] != g.key[t]) continue;
        ln = g.len[x];   // (the script's loop overwrites length and score: those of the last such sub-unitig count)
        if (g.key[g.eT[x]] == g.via[x] && g.last_tail[x] == b) found = true;
      }
      ok = found;
    }
  }
  pass[u] = ok, contrib[u] = ln;
}
// One round of the walks not made yet.  A walk goes on through t while t has out-degree 1, neither t nor rev t is in its node set and
// the edge it came by passes.  The node set is the start node and what the walk has claimed in owner[] (compare-and-swap from NONE: a
// claim is never overwritten, so a walk always finds its own).  A walk that meets another's claim is left for the next round, with
// nothing of it recorded; num[0] counts those, num[1] walks longer than there are edges (never).
__global__ void k_cp_walk(WalkG g, const uint8_t *__restrict__ pass, const int64_t *__restrict__ contrib, const uint32_t *__restrict__ w_edge, uint32_t K, uint32_t n_alive,
                          uint32_t *__restrict__ owner, uint8_t *__restrict__ state, uint32_t *__restrict__ cnt, int64_t *__restrict__ plen, uint32_t *__restrict__ num) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K || state[k]) return;
  uint32_t u = w_edge[k], t = g.eT[u], n = 0;
  const uint32_t s0 = g.eS[u];
  int64_t pl = 0;
  while (g.out_deg[t] == 1) {
    if (t == s0 || owner[t] == k) break;
    const uint32_t r = g.rev[t];
    if (r != NONE && (r == s0 || owner[r] == k)) break;
    if (!pass[u]) break;
    const uint32_t was = atomicCAS(&owner[t], NONE, k);
    if (was == k) break;   // in the node set after all (what the load above must have said)
    if (was != NONE) {     // another walk's: wait for it
      atomicAdd(&num[0], 1u);
      return;
    }
    ++n, pl += contrib[u];
    u = g.single_out[t];
    if (n > n_alive || u == NONE) {
      atomicAdd(&num[1], 1u);
      return;
    }
    t = g.eT[u];
  }
  cnt[k] = n + 1, plen[k] = pl + g.len[u], state[k] = 1;
}
// the edges of a made walk: cnt[k] of them from its start edge on, each the single out-edge of the last one's head
__global__ void k_cp_walk_paths(WalkG g, const uint32_t *__restrict__ w_edge, const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ off, uint32_t K,
                                uint32_t *__restrict__ paths) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  uint32_t u = w_edge[k];
  const uint64_t o = off[k];
  for (uint32_t i = 0, n = cnt[k]; i < n; ++i) {
    if (u == NONE) return;   // (never: cnt counted these steps)
    paths[o + i] = u;
    if (i + 1 < n) u = g.single_out[g.eT[u]];
  }
}

// ---------------------------------------------------------------------------------------------------------
// the texts.  utg_data: a line per entry of the table, `s via t type length score path`; the simple unitigs' lines are the unitigs' own
// (a piece per path slot) with the type replaced, a compound line lists `s~via~t` of its bundle, a piece each, joined by '|'.  ctg_paths:
// `id type s~via~t end length score s~via~t|...`, a piece per listed unitig.  The first piece of a line carries the line's head.
// ---------------------------------------------------------------------------------------------------------
struct Ent {   // an entry of the table: simple unitigs, then compound ones
  uint64_t s, via, t;
  int64_t len, score;
  uint32_t type, pad;
};
struct Head {   // the head of a line that is made of `s~via~t` pieces
  uint32_t kind, id;   // kind 0: a compound line of utg_data (u0 the entry); 1 / 2: the F / R line of contig id; 3: a ring's line
  uint32_t u0, circular;
  uint64_t end;
  int64_t len, score;
};
struct Piece {
  uint32_t u, head, last;   // the entry; its line's Head if it starts the line (NONE otherwise); whether it ends the line
};
template <bool WRITE>
__device__ inline void put(LineOut<WRITE> &o, const char *s) {
  for (; *s; ++s) o.ch(*s);
}
template <bool WRITE>
__device__ inline void put_node(LineOut<WRITE> &o, uint64_t key) {
  if (key == NA) o.ch('N'), o.ch('A');
  else o.node((uint32_t)(key >> 1), (uint32_t)(key & 1));
}
template <bool WRITE>
__device__ inline void put_type(LineOut<WRITE> &o, uint32_t type) {
  put(o, type == T_SIMPLE ? "simple" : type == T_SPUR2 ? "spur:2" : type == T_DUP ? "simple_dup" : type == T_CONTAINED ? "contained" : type == T_BRIDGE ? "repeat_bridge" : "compound");
}
template <bool WRITE>
__device__ inline void put_triple(LineOut<WRITE> &o, const Ent &e) {
  put_node(o, e.s), o.ch('~'), put_node(o, e.via), o.ch('~'), put_node(o, e.t);
}
template <bool WRITE>
__device__ inline void put_entry_head(LineOut<WRITE> &o, const Ent &e) {   // "s via t type length score "
  put_node(o, e.s), o.ch(' '), put_node(o, e.via), o.ch(' '), put_node(o, e.t), o.ch(' '), put_type(o, e.type), o.ch(' ');
  o.i64(e.len), o.ch(' '), o.i64(e.score), o.ch(' ');
}
// the piece source of both texts (pgx_text.h's piece scheme lays them out and formats them)
struct TextSrc {
  const Ent *ent;
  const pgx_unitig *tab;        // the slot pieces (utg_data's simple lines): pieces [0, m_slots)
  const uint32_t *slot_u;
  const uint64_t *slot_w;
  uint32_t m_slots;
  const Piece *triples;         // the triple pieces: pieces [m_slots, n)
  const Head *head;
  uint32_t n;
  static constexpr uint32_t MAX = 256;   // a contig line's head (id 10, type 12, a triple 41, a name 13, two numbers of <= 20, 6 blanks) + a triple + 1 = 161
  template <bool WRITE>
  __device__ uint32_t piece(uint32_t j, char *dst) const {
    LineOut<WRITE> o{dst, 0};
    if (j < m_slots) {
      const uint32_t u = slot_u[j];
      const uint64_t first = tab[u].first;
      if (j == first) put_entry_head(o, ent[u]), put_node(o, ent[u].s), o.ch('~');
      put_node(o, slot_w[j]);
      o.ch(j == first + tab[u].n_edges - 1 ? '\n' : '~');
      return o.n;
    }
    const Piece p = triples[j - m_slots];
    if (p.head != NONE) {
      const Head h = head[p.head];
      if (h.kind == 0) {
        put_entry_head(o, ent[h.u0]);
      } else {
        if (h.kind == 3) o.i64((int64_t)h.id, 6);
        else o.u32(h.id, 6), o.ch(h.kind == 1 ? 'F' : 'R');
        put(o, h.circular ? " ctg_circular " : " ctg_linear ");
        put_triple(o, ent[h.u0]), o.ch(' '), put_node(o, h.end), o.ch(' '), o.i64(h.len), o.ch(' '), o.i64(h.score), o.ch(' ');
      }
    }
    put_triple(o, ent[p.u]);
    o.ch(p.last ? '\n' : '|');
    return o.n;
  }
};
// the first piece of every line of utg_data: a simple unitig's first slot, a compound line's first triple piece, and the end
__global__ void k_cp_utg_line_piece(const pgx_unitig *__restrict__ tab, uint32_t n_u, const uint32_t *__restrict__ sub_off, uint32_t n_c, uint32_t m_slots,
                                    uint32_t *__restrict__ line_piece) {
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l > n_u + n_c) return;
  line_piece[l] = l < n_u ? (uint32_t)tab[l].first : m_slots + sub_off[l - n_u];
}
}  // namespace
}  // namespace pgx

using namespace pgx;

struct pgx_ctg_paths {
  pgx_unitigs *u = nullptr;      // the unitigs whose slot arrays the simple lines of utg_data are read from
  uint64_t u_serial = 0;         // ... and their serial: the address alone may belong to later unitigs
  bool owns_u = false;           // ... made by pgx_ctg_paths_build, and freed with this
  DevBuf<Ent> ent;               // the table (MemTag "ctg_paths", as all of these)
  DevBuf<Piece> utg_piece, ctg_piece;
  DevBuf<Head> utg_head, ctg_head;
  TextPlan utg, ctg;
  uint32_t m_slots = 0, n_utg_pieces = 0, n_ctg_pieces = 0;
  std::vector<pgx_ctg_unitig> table;
  std::vector<uint64_t> row_off;
  std::vector<uint32_t> row_u;
  pgx_ctg_paths_stats_t st = {};
  TextStage stage;
  bool shut = false;
  void drop_device_state() {
    ent.release(), utg_piece.release(), ctg_piece.release(), utg_head.release(), ctg_head.release(), utg.release(), ctg.release();
    stage.drop();
  }
};

namespace pgx {
namespace {
LiveSet<pgx_ctg_paths> g_cp;
ShutdownHook g_cp_hook([] { g_cp.shutdown(); });

// ---------------------------------------------------------------------------------------------------------
// the host cascades
// ---------------------------------------------------------------------------------------------------------
// a set of small integers that pops its smallest element
struct MinSet {
  std::set<uint32_t> s;
  void add(uint32_t x) { s.insert(x); }
  bool pop(uint32_t *x) {
    if (s.empty()) return false;
    *x = *s.begin();
    s.erase(s.begin());
    return true;
  }
};

struct Cascade {
  // per entry (simple unitigs, then compound ones)
  std::vector<uint32_t> S, T, type, dual, n_edges;   // S / T: node ids
  std::vector<uint64_t> via, last_tail;              // keys
  std::vector<int64_t> len, score;
  std::vector<uint8_t> alive;
  std::vector<std::vector<uint32_t>> sub;            // per compound entry (index - n_u): its bundle
  // per node (ascending key)
  std::vector<uint64_t> key, best_tail;
  std::vector<uint32_t> rev;                          // the node of key ^ 1 (NONE: none)
  std::vector<std::vector<uint32_t>> out, in;
  std::vector<uint32_t> in_deg, out_deg;
  std::vector<uint32_t> stamp;                        // ego sets: stamp[x] == gen
  uint32_t gen = 0, n_u = 0;
  uint64_t spur_rounds = 0;

  void add_edge(uint32_t u) {
    out[S[u]].push_back(u), in[T[u]].push_back(u);
    ++out_deg[S[u]], ++in_deg[T[u]];
    alive[u] = 1;
  }
  void remove_edge(uint32_t u) {
    alive[u] = 0;
    --out_deg[S[u]], --in_deg[T[u]];
  }
  // the nodes within `radius` directed hops of n in the graph as it stands: stamped with the answered generation, and listed
  uint32_t ego(uint32_t n, uint32_t radius, std::vector<uint32_t> *list) {
    ++gen;
    list->assign(1, n);
    stamp[n] = gen;
    size_t a = 0;
    for (uint32_t hop = 0; hop < radius && a < list->size(); ++hop) {
      const size_t b = list->size();
      for (; a < b; ++a)
        for (uint32_t u : out[(*list)[a]])
          if (alive[u] && stamp[T[u]] != gen) stamp[T[u]] = gen, list->push_back(T[u]);
    }
    return gen;
  }

  void spurs(int64_t spur_len) {
    MinSet cands;
    for (uint32_t x = 0; x < key.size(); ++x)
      if (in_deg[x] == 0) cands.add(x);
    std::vector<uint32_t> eg, front, nxt, hops;
    std::unordered_map<uint32_t, uint32_t> pred;
    uint32_t n;
    while (cands.pop(&n)) {
      if (in_deg[n] != 0) continue;
      const uint32_t g = ego(n, 10, &eg);
      std::sort(eg.begin(), eg.end());
      for (uint32_t b : eg) {
        if (in_deg[b] <= 1) continue;
        bool external = false;
        for (uint32_t u : in[b])
          if (alive[u] && stamp[S[u]] != g) external = true;
        if (!external) continue;
        // fewest hops from n to b: forward search, neighbours in edge order, the first discoverer is the predecessor
        pred.clear(), pred[n] = NONE;
        front.assign(1, n);
        while (!pred.count(b)) {
          nxt.clear();
          for (uint32_t x : front)
            for (uint32_t u : out[x])
              if (alive[u] && !pred.count(T[u])) pred[T[u]] = x, nxt.push_back(T[u]);
          front.swap(nxt);
          PGX_REQUIRE(!front.empty(), PGX_EINVAL, "pgx_ctg_paths: node %llu is not reached from %llu (a bug)", (unsigned long long)key[b], (unsigned long long)key[n]);
        }
        hops.clear();
        for (uint32_t x = b; pred[x] != NONE; x = pred[x]) hops.push_back(x);
        std::reverse(hops.begin(), hops.end());   // the heads of the hops; the first tail is n
        int64_t total = 0;
        uint32_t a = n;
        for (uint32_t c : hops) {
          for (uint32_t u : out[a])
            if (alive[u] && T[u] == c) total += len[u];
          a = c;
        }
        if (total >= spur_len) continue;
        a = n;
        for (uint32_t c : hops) {
          for (uint32_t u : out[a]) {
            if (!alive[u] || T[u] != c) continue;
            const uint32_t d = dual[u];
            remove_edge(u);
            if (d != NONE && alive[d]) {   // (otherwise the script's second remove_edge raises into its `except: pass`: no type is set)
              remove_edge(d);
              type[u] = type[d] = T_SPUR2;
            }
          }
          if (in_deg[c] == 0) cands.add(c);
          a = c;
        }
        ++spur_rounds;
        break;
      }
    }
  }

  void dups() {
    std::map<std::pair<uint32_t, uint32_t>, std::vector<uint32_t>> groups;
    for (uint32_t u = 0; u < n_u; ++u)
      if (n_edges[u] <= 2 && type[u] == T_SIMPLE) groups[{S[u], T[u]}].push_back(u);
    for (auto &g : groups) {
      std::vector<uint32_t> &us = g.second;
      std::stable_sort(us.begin(), us.end(), [&](uint32_t a, uint32_t b) { return via[a] < via[b]; });
      for (size_t k = 1; k < us.size(); ++k) {
        PGX_REQUIRE(alive[us[k]], PGX_EINVAL, "pgx_ctg_paths: unitig %u is a second short loop at one node (the script's remove_edge raises)", us[k]);
        remove_edge(us[k]);
        type[us[k]] = T_DUP;
      }
    }
  }

  struct Bundle {
    uint32_t s, t;
    int64_t len, score;
    std::vector<uint32_t> edges;   // ascending
  };
  // find_bundle(start, 48, 16, 500000); false: no bundle
  bool find_bundle(uint32_t start, Bundle *out_b) {
    std::vector<uint32_t> loc_list;
    const uint32_t g = ego(start, 48, &loc_list);
    auto in_loc = [&](uint32_t x) { return stamp[x] == g; };
    std::set<uint32_t> tips, b_edges;
    std::unordered_set<uint32_t> b_nodes{start};
    std::unordered_map<uint32_t, std::pair<int64_t, int64_t>> to{{start, {0, 0}}};
    auto rev_in_nodes = [&](uint32_t x) { return rev[x] != NONE && b_nodes.count(rev[x]); };
    // the in-edge of v with the largest positive score among those whose tail is settled; strict: false in *ok when a tail is not
    auto best_in_edge = [&](uint32_t v, bool strict, bool *ok) {
      uint32_t best = NONE;
      int64_t mx = 0;
      *ok = true;
      for (uint32_t u : in[v]) {
        if (!alive[u] || !in_loc(S[u])) continue;
        if (!to.count(S[u])) {
          if (strict) {
            *ok = false;
            return NONE;
          }
          continue;
        }
        if (score[u] > mx) mx = score[u], best = u;
      }
      return best;
    };
    auto settle = [&](uint32_t v, uint32_t best) {
      PGX_REQUIRE(best != NONE, PGX_EINVAL, "pgx_ctg_paths: no in-edge of node %llu in a bundle has a positive score (the script raises)", (unsigned long long)key[v]);
      to[v] = {to[S[best]].first + len[best], to[S[best]].second + score[best]};
    };
    for (uint32_t u : out[start])
      if (alive[u] && in_loc(T[u]) && !rev_in_nodes(T[u])) b_edges.insert(u), tips.insert(T[u]);
    b_nodes.insert(tips.begin(), tips.end());
    uint32_t depth = 1;
    bool ok;
    for (;;) {
      if (tips.size() > 4) return false;
      if (tips.size() == 1) {
        const uint32_t end = *tips.begin();
        if (!to.count(end)) settle(end, best_in_edge(end, false, &ok));
        out_b->s = start, out_b->t = end, out_b->len = to[end].first, out_b->score = to[end].second;
        out_b->edges.assign(b_edges.begin(), b_edges.end());
        return true;
      }
      ++depth;
      if (depth > 10 && (double)b_edges.size() / depth > 16.0) return false;
      if (depth > 48) return false;
      bool updated = false, loop = false;
      const std::vector<uint32_t> tips_list(tips.begin(), tips.end());
      for (uint32_t v : tips_list) {
        bool has_out = false;
        for (uint32_t u : out[v])
          if (alive[u] && in_loc(T[u])) has_out = true;
        if (!has_out) continue;
        const uint32_t best = best_in_edge(v, true, &ok);
        if (ok) {
          settle(v, best);
          if (to[v].first > 500000) return false;
          bool v_up = false;
          for (uint32_t u : out[v]) {
            if (!alive[u] || !in_loc(T[u])) continue;
            if (to.count(T[u])) {
              loop = true;
              break;
            }
            if (!b_edges.count(u) && !rev_in_nodes(T[u])) tips.insert(T[u]), b_edges.insert(u), updated = v_up = true;
          }
          if (v_up) {
            tips.erase(v);
            if (tips.size() == 1) break;
          }
        }
        if (loop) break;
      }
      if (loop || !updated) return false;
      b_nodes.insert(tips.begin(), tips.end());
    }
  }

  uint32_t dual_of(uint32_t u, const char *what) {
    PGX_REQUIRE(dual[u] != NONE, PGX_EINVAL, "pgx_ctg_paths: unitig %u of %s has no dual", u, what);
    return dual[u];
  }

  void compounds() {
    std::vector<Bundle> found;
    for (uint32_t p = 0; p < key.size(); ++p)
      if (out_deg[p] > 1) {
        Bundle b;
        if (find_bundle(p, &b)) found.push_back(std::move(b));
      }
    std::stable_sort(found.begin(), found.end(), [](const Bundle &a, const Bundle &b) { return a.edges.size() > b.edges.size(); });
    // the script's dictionaries keyed (s, "NA", t): insertion order, a second insertion of a key replaces the value in place
    typedef std::pair<uint32_t, uint32_t> K;
    std::vector<K> order1;
    std::map<K, Bundle> cp1;
    auto put1 = [&](Bundle b) {
      const K k{b.s, b.t};
      if (!cp1.count(k)) order1.push_back(k);
      cp1[k] = std::move(b);
    };
    std::unordered_set<uint32_t> e2c;
    for (Bundle &b : found) {
      bool overlapped = false;
      for (uint32_t u : b.edges) {
        if (e2c.count(u) || e2c.count(dual_of(u, "a bundle"))) {
          overlapped = true;
          break;
        }
      }
      if (overlapped) continue;
      PGX_REQUIRE(rev[b.s] != NONE && rev[b.t] != NONE, PGX_EINVAL, "pgx_ctg_paths: the bundle at node %llu has no reverse", (unsigned long long)key[b.s]);
      Bundle r{rev[b.t], rev[b.s], b.len, b.score, {}};
      for (uint32_t u : b.edges) r.edges.push_back(dual[u]), e2c.insert(u), e2c.insert(dual[u]);
      put1(b), put1(std::move(r));
    }
    auto has = [&](const std::map<K, Bundle> &m, uint32_t s, uint32_t t) { return rev[s] != NONE && rev[t] != NONE && m.count(K{rev[t], rev[s]}) != 0; };
    std::vector<K> order2, order3;
    std::unordered_map<uint32_t, std::set<K>> e2k;
    for (const K &k : order1)
      if (has(cp1, k.first, k.second)) {
        order2.push_back(k);
        for (uint32_t u : cp1[k].edges) e2k[u].insert(k);
      }
    std::map<K, Bundle> cp3;
    for (const K &k : order2) {
      bool contained = false;
      for (uint32_t u : out[k.first])
        if (alive[u]) {
          auto it = e2k.find(u);
          if (it != e2k.end() && it->second.size() > 1) contained = true;
        }
      if (!contained) cp3[k] = cp1[k], order3.push_back(k);
    }
    std::vector<K> final_keys;
    for (const K &k : order3)
      if (has(cp3, k.first, k.second)) final_keys.push_back(k);
    for (const K &k : final_keys)
      for (uint32_t u : cp3[k].edges)
        if (alive[u]) remove_edge(u), type[u] = T_CONTAINED;   // (the script spares the type "spur", which no unitig has: spur:2 is overwritten)
    std::map<K, uint32_t> index;
    for (const K &k : final_keys) {
      const Bundle &b = cp3[k];
      index[k] = (uint32_t)S.size();
      S.push_back(b.s), T.push_back(b.t), via.push_back(NA), last_tail.push_back(NA), len.push_back(b.len), score.push_back(b.score), n_edges.push_back(0);
      type.push_back(T_COMPOUND), dual.push_back(NONE), alive.push_back(0);
      sub.push_back(b.edges);
    }
    for (const K &k : final_keys) {
      const uint32_t c = index[k];
      dual[c] = index[K{rev[k.second], rev[k.first]}];
      PGX_REQUIRE(S[c] != T[c], PGX_EINVAL, "pgx_ctg_paths: the bundle at node %llu ends where it starts", (unsigned long long)key[S[c]]);
      add_edge(c);
    }
  }

  void bridges() {
    std::set<uint32_t> marked;
    for (uint32_t u = 0; u < S.size(); ++u) {
      if (!alive[u]) continue;
      const uint32_t s = S[u], t = T[u];
      if (in_deg[s] == 1 && out_deg[s] == 2 && in_deg[t] == 2 && out_deg[t] == 1 && len[u] < 60000) marked.insert(u), marked.insert(dual_of(u, "a repeat bridge"));
    }
    for (uint32_t u : marked) {
      PGX_REQUIRE(alive[u], PGX_EINVAL, "pgx_ctg_paths: unitig %u, the dual of a repeat bridge, is not in the graph (the script's remove_edge raises)", u);
      remove_edge(u);
      type[u] = T_BRIDGE;
    }
  }

  uint32_t single_out(uint32_t x) {
    for (uint32_t u : out[x])
      if (alive[u]) return u;
    return NONE;
  }

  // one walk of construct_c_path_from_utgs on the host, from the edge u0: its path and path_length (what the device walks are held to;
  // used for what they leave: the walks no start node reaches, and a walk that found no round to itself)
  int64_t walk_one(uint32_t u0, std::vector<uint32_t> *path) {
    std::unordered_set<uint32_t> nodes{S[u0]};
    uint32_t u = u0, t = T[u];
    int64_t plen = 0;
    path->clear();
    while (out_deg[t] == 1) {
      if (nodes.count(t) || (rev[t] != NONE && nodes.count(rev[t]))) break;
      int64_t ln = len[u];
      if (in_deg[t] > 1) {
        const uint64_t b = best_tail[t];
        if (type[u] == T_SIMPLE && b != last_tail[u]) break;
        if (type[u] == T_COMPOUND) {
          bool found = false;
          for (uint32_t x : sub[u - n_u]) {
            if (via[x] != key[t]) continue;
            ln = len[x];   // (the script's loop overwrites length and score: those of the last such sub-unitig count)
            if (key[T[x]] == via[x] && last_tail[x] == b) found = true;
          }
          if (!found) break;
        }
      }
      path->push_back(u), nodes.insert(t);
      plen += ln;
      u = single_out(t);
      t = T[u];
    }
    path->push_back(u);
    return plen + len[u];
  }
};

typedef std::vector<std::pair<int64_t, std::vector<uint32_t>>> CPath;
// construct_c_path_from_utgs: (path_length, path) of every walk, in the order the script's loop makes them.  The loop pops the start
// nodes (not (in 1, out 1), with an out-edge) in ascending key and walks every out-edge of each -- those walks do not depend on each
// other and run on the device, a lane per start edge (k_cp_edge_pass, k_cp_walk, k_cp_walk_paths).  The loop ends when no edge is free,
// so the start nodes behind the one whose walks cover the last free edge are not walked: that is read off the paths.  What no start
// node reaches (closed cycles of (1, 1) nodes, what lies behind a stop at `rev t`) the script walks from the tail of the smallest free
// edge, one pop at a time: serial by its nature, rare, and done here on the host.
void contig_walks(Cascade &cs, CPath *c_path, uint64_t *device_walks) {
  hipStream_t st = ctx().stream;
  const uint32_t n_all = (uint32_t)cs.S.size(), n_nodes = (uint32_t)cs.key.size();
  std::vector<uint32_t> w_edge, w_rank, single(n_nodes, NONE);
  uint32_t rank = 0, n_alive = 0;
  for (uint32_t x = 0; x < n_nodes; ++x) {
    if (cs.out_deg[x] == 1) single[x] = cs.single_out(x);
    if (!cs.out_deg[x] || (cs.in_deg[x] == 1 && cs.out_deg[x] == 1)) continue;
    for (uint32_t u : cs.out[x])
      if (cs.alive[u]) w_edge.push_back(u), w_rank.push_back(rank);
    ++rank;
  }
  for (uint32_t u = 0; u < n_all; ++u) n_alive += cs.alive[u];
  const uint32_t K = (uint32_t)w_edge.size();
  std::vector<uint32_t> cnt(K, 0), paths;
  std::vector<int64_t> plen(K, 0);
  std::vector<uint64_t> off((size_t)K + 1, 0);
  std::vector<uint8_t> state(K, 0);
  if (K) {
    PrimWs tmp;
    std::vector<uint32_t> sub_off(1, 0), sub_list;
    for (const auto &b : cs.sub) sub_list.insert(sub_list.end(), b.begin(), b.end()), sub_off.push_back((uint32_t)sub_list.size());
    DevBuf<uint32_t> d_S(n_all), d_T(n_all), d_type(n_all), d_sub_off(sub_off.size()), d_sub(sub_list.size()), d_in(n_nodes), d_out(n_nodes), d_single(n_nodes), d_rev(n_nodes);
    DevBuf<int64_t> d_len(n_all), d_contrib(n_all), d_plen(K);
    DevBuf<uint64_t> d_via(n_all), d_last(n_all), d_key(n_nodes), d_best(n_nodes), d_off((size_t)K + 1);
    DevBuf<uint8_t> d_alive(n_all), d_pass(n_all), d_state(K);
    DevBuf<uint32_t> d_edge(K), d_cnt(K), d_owner(n_nodes), d_num(2);
    d_S.upload(cs.S.data(), n_all), d_T.upload(cs.T.data(), n_all), d_type.upload(cs.type.data(), n_all), d_len.upload(cs.len.data(), n_all);
    d_via.upload(cs.via.data(), n_all), d_last.upload(cs.last_tail.data(), n_all), d_alive.upload(cs.alive.data(), n_all);
    d_sub_off.upload(sub_off.data(), sub_off.size()), d_sub.upload(sub_list.data(), sub_list.size());
    d_key.upload(cs.key.data(), n_nodes), d_best.upload(cs.best_tail.data(), n_nodes), d_in.upload(cs.in_deg.data(), n_nodes), d_out.upload(cs.out_deg.data(), n_nodes);
    d_single.upload(single.data(), n_nodes), d_rev.upload(cs.rev.data(), n_nodes), d_edge.upload(w_edge.data(), K);
    const WalkG g{d_S.p, d_T.p, d_type.p, d_len.p, d_via.p, d_last.p, d_sub_off.p, d_sub.p, cs.n_u, d_key.p, d_best.p, d_in.p, d_out.p, d_single.p, d_rev.p};
    LAUNCH(k_cp_edge_pass, n_all, g, d_alive.p, n_all, d_pass.p, d_contrib.p);
    PGX_HIP(hipMemsetAsync(d_state.p, 0, K, st));
    PGX_HIP(hipMemsetAsync(d_cnt.p, 0, (size_t)K * sizeof(uint32_t), st));
    // a round: every walk not made yet runs, claiming the nodes it passes; one that meets another's claim waits for the next round (the
    // walks that share a stretch run the same way along it, so the one in front is never the one that waits)
    uint32_t h_num[2] = {K, 0};
    for (uint32_t round = 0; h_num[0] && round < 64; ++round) {
      PGX_HIP(hipMemsetAsync(d_owner.p, 0xFF, (size_t)n_nodes * sizeof(uint32_t), st));
      PGX_HIP(hipMemsetAsync(d_num.p, 0, 2 * sizeof(uint32_t), st));
      LAUNCH(k_cp_walk, K, g, d_pass.p, d_contrib.p, d_edge.p, K, n_alive, d_owner.p, d_state.p, d_cnt.p, d_plen.p, d_num.p);
      PGX_HIP(hipGetLastError());
      d_num.download(h_num, 2);
      pgx::sync();
      PGX_REQUIRE(h_num[1] == 0, PGX_EHIP, "pgx_ctg_paths: %u contig walks did not end (a bug)", h_num[1]);
    }
    const uint64_t total = scan_to_total(d_cnt.p, d_off.p, K, &tmp);
    DevBuf<uint32_t> d_paths(total);
    LAUNCH(k_cp_walk_paths, K, g, d_edge.p, d_cnt.p, d_off.p, K, d_paths.p);
    PGX_HIP(hipGetLastError());
    paths.resize(total);
    d_cnt.download(cnt.data(), K), d_plen.download(plen.data(), K), d_off.download(off.data(), (size_t)K + 1), d_state.download(state.data(), K), d_paths.download(paths.data(), total);
    pgx::sync();
  }
  // the walks in the script's order; those of the start nodes behind the last one that found a free edge are not made
  std::vector<uint32_t> first_cover(n_all, NONE);
  CPath made(K);
  for (uint32_t k = 0; k < K; ++k) {
    if (state[k]) made[k] = {plen[k], std::vector<uint32_t>(paths.begin() + off[k], paths.begin() + off[k + 1])}, ++*device_walks;
    else made[k].first = cs.walk_one(w_edge[k], &made[k].second);
    for (uint32_t e : made[k].second) first_cover[e] = std::min(first_cover[e], w_rank[k]);
  }
  uint32_t last_rank = 0;
  bool left = false;
  for (uint32_t u = 0; u < n_all; ++u)
    if (cs.alive[u]) {
      if (first_cover[u] == NONE) left = true;
      else last_rank = std::max(last_rank, first_cover[u]);
    }
  std::vector<uint8_t> is_free(cs.alive);
  for (uint32_t k = 0; k < K; ++k) {
    if (!left && w_rank[k] > last_rank) break;
    for (uint32_t e : made[k].second) is_free[e] = 0;
    c_path->push_back(std::move(made[k]));
  }
  for (uint32_t e = 0; e < n_all; ++e) {   // ascending: the smallest free edge, popped; every out-edge of its tail is walked
    if (!is_free[e]) continue;
    is_free[e] = 0;
    for (uint32_t u0 : std::vector<uint32_t>(cs.out[cs.S[e]])) {
      if (!cs.alive[u0]) continue;
      std::vector<uint32_t> path;
      const int64_t pl = cs.walk_one(u0, &path);
      for (uint32_t x : path) is_free[x] = 0;
      c_path->emplace_back(pl, std::move(path));
    }
  }
}

void build_ctg_paths(pgx_unitigs *u, pgx_ctg_paths *c) {
  hipStream_t st = ctx().stream;
  PrimWs tmp;
  const UnitigsView v = unitigs_device_view(u, "pgx_unitigs_contig_paths");
  const uint32_t n_u = (uint32_t)v.n_u, m = (uint32_t)v.m;
  c->u = u, c->u_serial = v.serial, c->m_slots = m;
  Cascade cs;
  cs.n_u = n_u;
  std::vector<pgx_unitig> tab(n_u);
  std::unique_ptr<KernelTimer> part(new KernelTimer("ctg_paths_graph", m));
  if (n_u) {
    // ---- the unitig graph on the device
    DevBuf<uint64_t> st_keys(2 * (size_t)n_u), sorted_keys(2 * (size_t)n_u), nodes(2 * (size_t)n_u), last_tail(n_u);
    DevBuf<uint32_t> run_len(2 * (size_t)n_u);
    LAUNCH(k_cp_keys, n_u, v.tab, v.slot_w, n_u, st_keys.p, last_tail.p);
    sort_keys(st_keys.p, sorted_keys.p, 2 * (size_t)n_u, 0, 33, &tmp);
    const uint32_t n_nodes = (uint32_t)run_lengths(sorted_keys.p, nodes.p, run_len.p, 2 * (size_t)n_u, &tmp);
    DevBuf<uint32_t> s_node(n_u), t_node(n_u), iota(n_u), sorted_s(n_u), sorted_t(n_u), out_list(n_u), in_list(n_u), out_off((size_t)n_nodes + 1), in_off((size_t)n_nodes + 1);
    DevBuf<uint32_t> dual(n_u), best(n_nodes), err(1);
    DevBuf<uint64_t> best_tail(n_nodes);
    LAUNCH(k_cp_node_ids, n_u, v.tab, nodes.p, n_nodes, n_u, s_node.p, t_node.p, iota.p);
    sort_pairs(s_node.p, sorted_s.p, iota.p, out_list.p, n_u, 0, 32, &tmp);
    sort_pairs(t_node.p, sorted_t.p, iota.p, in_list.p, n_u, 0, 32, &tmp);
    LAUNCH(k_cp_offsets, (size_t)n_nodes + 1, sorted_s.p, sorted_t.p, n_u, n_nodes, out_off.p, in_off.p);
    PGX_HIP(hipMemsetAsync(err.p, 0xFF, sizeof(uint32_t), st));
    LAUNCH(k_cp_duals, n_u, v.tab, last_tail.p, nodes.p, n_nodes, out_off.p, out_list.p, n_u, dual.p, err.p);
    PGX_HIP(hipMemsetAsync(best.p, 0, (size_t)n_nodes * sizeof(uint32_t), st));
    PGX_HIP(hipMemsetAsync(best_tail.p, 0xFF, (size_t)n_nodes * sizeof(uint64_t), st));
    LAUNCH(k_cp_best, m, v.slot_w, v.paths, m, nodes.p, n_nodes, best.p);
    LAUNCH(k_cp_best_tail, m, v.slot_w, v.slot_u, v.paths, v.tab, m, nodes.p, n_nodes, best.p, best_tail.p);
    PGX_HIP(hipGetLastError());
    // ---- down, behind one synchronisation
    std::vector<uint32_t> h_out_list(n_u), h_in_list(n_u), h_out_off((size_t)n_nodes + 1), h_in_off((size_t)n_nodes + 1);
    uint32_t h_err = NONE;
    cs.S.resize(n_u), cs.T.resize(n_u), cs.dual.resize(n_u), cs.last_tail.resize(n_u), cs.key.resize(n_nodes), cs.best_tail.resize(n_nodes);
    PGX_HIP(hipMemcpyAsync(tab.data(), v.tab, (size_t)n_u * sizeof(pgx_unitig), hipMemcpyDeviceToHost, st));
    s_node.download(cs.S.data(), n_u), t_node.download(cs.T.data(), n_u), dual.download(cs.dual.data(), n_u), last_tail.download(cs.last_tail.data(), n_u);
    nodes.download(cs.key.data(), n_nodes), best_tail.download(cs.best_tail.data(), n_nodes);
    out_list.download(h_out_list.data(), n_u), in_list.download(h_in_list.data(), n_u), out_off.download(h_out_off.data(), (size_t)n_nodes + 1);
    in_off.download(h_in_off.data(), (size_t)n_nodes + 1), err.download(&h_err, 1);
    pgx::sync();
    PGX_REQUIRE(h_err == NONE, PGX_EINVAL, "pgx_ctg_paths: unitig %u has no dual (no unitig starts with the reverse of its last edge)", h_err);
    part.reset(), part.reset(new KernelTimer("ctg_paths_clean", n_u));
    const double host0 = wall_ms();
    cs.via.resize(n_u), cs.len.resize(n_u), cs.score.resize(n_u), cs.n_edges.resize(n_u), cs.type.assign(n_u, T_SIMPLE), cs.alive.assign(n_u, 0);
    cs.out.resize(n_nodes), cs.in.resize(n_nodes), cs.in_deg.assign(n_nodes, 0), cs.out_deg.assign(n_nodes, 0), cs.stamp.assign(n_nodes, 0), cs.rev.resize(n_nodes);
    for (uint32_t x = 0; x < n_nodes; ++x) {
      const auto it = std::lower_bound(cs.key.begin(), cs.key.end(), cs.key[x] ^ 1u);
      cs.rev[x] = it != cs.key.end() && *it == (cs.key[x] ^ 1u) ? (uint32_t)(it - cs.key.begin()) : NONE;
    }
    for (uint32_t k = 0; k < n_u; ++k) {
      const pgx_unitig &t = tab[k];
      cs.via[k] = (uint64_t)t.via_rid << 1 | t.via_end, cs.len[k] = t.length, cs.score[k] = t.score, cs.n_edges[k] = t.n_edges;
    }
    // phase 1: a unitig with s != t is an edge; the lists come sorted (ascending unitig index within a node)
    for (uint32_t x = 0; x < n_nodes; ++x) {
      for (uint32_t k = h_out_off[x]; k < h_out_off[x + 1]; ++k)
        if (cs.S[h_out_list[k]] != cs.T[h_out_list[k]]) cs.out[x].push_back(h_out_list[k]), ++cs.out_deg[x], cs.alive[h_out_list[k]] = 1;
      for (uint32_t k = h_in_off[x]; k < h_in_off[x + 1]; ++k)
        if (cs.S[h_in_list[k]] != cs.T[h_in_list[k]]) cs.in[x].push_back(h_in_list[k]), ++cs.in_deg[x];
    }
    cs.spurs(50000);
    cs.dups();
    cs.compounds();
    cs.bridges();
    cs.spurs(80000);
    c->st.host_us = (uint64_t)((wall_ms() - host0) * 1000.0);
  }
  // ---- the contig walks and the claim
  part.reset(), part.reset(new KernelTimer("ctg_paths_walk", n_u));
  const double host1 = wall_ms();
  const uint32_t n_all = (uint32_t)cs.S.size(), n_c = n_all - n_u;
  std::vector<Head> ctg_head;
  std::vector<Piece> ctg_piece;
  c->row_off.assign(1, 0);
  {
    CPath c_path;
    contig_walks(cs, &c_path, &c->st.device_walks);
    std::stable_sort(c_path.begin(), c_path.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
    std::vector<uint8_t> is_free(cs.alive);
    uint32_t ctg_id = 0;
    auto add_line = [&](uint32_t kind, uint32_t id, const std::vector<uint32_t> &row, bool circ) {
      Head h{kind, id, row[0], circ, cs.key[cs.T[row.back()]], 0, 0};
      for (size_t k = 0; k < row.size(); ++k) {
        h.len += cs.len[row[k]], h.score += cs.score[row[k]];
        ctg_piece.push_back(Piece{row[k], k == 0 ? (uint32_t)ctg_head.size() : NONE, k + 1 == row.size()});
        c->row_u.push_back(row[k]);
      }
      ctg_head.push_back(h);
      c->row_off.push_back(c->row_u.size());
      c->st.longest_ctg = std::max<uint64_t>(c->st.longest_ctg, row.size());
    };
    std::vector<uint32_t> keep, rv;
    for (auto &cp : c_path) {
      keep.clear();
      for (uint32_t e : cp.second) {
        if (is_free[e] && cs.dual[e] != NONE && is_free[cs.dual[e]]) keep.push_back(e);
        else break;
      }
      if (keep.empty()) continue;
      rv.clear();
      for (size_t k = keep.size(); k-- > 0;) rv.push_back(cs.dual[keep[k]]);
      const bool circ = cs.T[keep.back()] == cs.S[keep[0]];
      add_line(1, ctg_id, keep, circ), add_line(2, ctg_id, rv, circ);
      ++ctg_id;
      ++(circ ? c->st.ctg_circular : c->st.ctg_linear);
      for (uint32_t e : keep) is_free[e] = 0;
      for (uint32_t e : rv) is_free[e] = 0;
    }
    for (uint32_t k = 0; k < n_u; ++k)
      if (cs.S[k] == cs.T[k]) add_line(3, ctg_id++, std::vector<uint32_t>(1, k), true), ++c->st.ctg_circular;
  }
  c->st.host_us += (uint64_t)((wall_ms() - host1) * 1000.0);
  // ---- the table, the statistics
  c->table.resize(n_all);
  uint64_t by_type[N_TYPES] = {};
  for (uint32_t k = 0; k < n_all; ++k) c->table[k] = pgx_ctg_unitig{cs.type[k], cs.dual[k]}, ++by_type[cs.type[k]];
  c->st.unitigs = n_all, c->st.simple = by_type[T_SIMPLE], c->st.spur2 = by_type[T_SPUR2], c->st.simple_dup = by_type[T_DUP], c->st.contained = by_type[T_CONTAINED];
  c->st.repeat_bridge = by_type[T_BRIDGE], c->st.compound = by_type[T_COMPOUND], c->st.ctg_lines = ctg_head.size(), c->st.row_entries = c->row_u.size();
  c->st.spur_rounds = cs.spur_rounds;
  // ---- the texts laid out on the device
  part.reset(), part.reset(new KernelTimer("ctg_paths_text", (uint64_t)m + ctg_piece.size()));
  std::vector<Ent> ent(n_all);
  for (uint32_t k = 0; k < n_all; ++k) ent[k] = Ent{cs.key[cs.S[k]], cs.via[k], cs.key[cs.T[k]], cs.len[k], cs.score[k], cs.type[k], 0};
  std::vector<Head> utg_head(n_c);
  std::vector<Piece> utg_piece;
  std::vector<uint32_t> sub_off(1, 0);
  for (uint32_t k = 0; k < n_c; ++k) {
    const std::vector<uint32_t> &b = cs.sub[k];
    utg_head[k] = Head{0, 0, n_u + k, 0, 0, 0, 0};
    for (size_t i = 0; i < b.size(); ++i) utg_piece.push_back(Piece{b[i], i == 0 ? k : NONE, i + 1 == b.size()});
    sub_off.push_back((uint32_t)utg_piece.size());
  }
  PGX_REQUIRE((uint64_t)m + utg_piece.size() < NONE && ctg_piece.size() < NONE, PGX_EINVAL, "pgx_ctg_paths: more than 2^32 - 1 pieces of text");
  c->ent.alloc(n_all), c->ent.upload(ent.data(), n_all);
  c->utg_piece.alloc(utg_piece.size()), c->utg_piece.upload(utg_piece.data(), utg_piece.size());
  c->utg_head.alloc(n_c), c->utg_head.upload(utg_head.data(), n_c);
  c->ctg_piece.alloc(ctg_piece.size()), c->ctg_piece.upload(ctg_piece.data(), ctg_piece.size());
  c->ctg_head.alloc(ctg_head.size()), c->ctg_head.upload(ctg_head.data(), ctg_head.size());
  c->n_utg_pieces = m + (uint32_t)utg_piece.size(), c->n_ctg_pieces = (uint32_t)ctg_piece.size();
  {
    DevBuf<uint32_t> d_sub_off(sub_off.size()), line_piece((size_t)n_all + 1);
    d_sub_off.upload(sub_off.data(), sub_off.size());
    LAUNCH(k_cp_utg_line_piece, (size_t)n_all + 1, v.tab, n_u, d_sub_off.p, n_c, m, line_piece.p);
    const TextSrc src{c->ent.p, v.tab, v.slot_u, v.slot_w, m, c->utg_piece.p, c->utg_head.p, c->n_utg_pieces};
    plan_text(src, line_piece.p, n_all, &c->utg, &tmp);
    std::vector<uint32_t> rows32(c->row_off.begin(), c->row_off.end());
    DevBuf<uint32_t> d_rows(rows32.size());
    d_rows.upload(rows32.data(), rows32.size());
    const TextSrc csrc{c->ent.p, nullptr, nullptr, nullptr, 0, c->ctg_piece.p, c->ctg_head.p, c->n_ctg_pieces};
    plan_text(csrc, d_rows.p, ctg_head.size(), &c->ctg, &tmp);
    pgx::sync();   // (the uploads read host vectors that end with this scope)
  }
  part.reset();
}

void require_cp(const pgx_ctg_paths *c, const char *who) {
  PGX_REQUIRE(c, PGX_EARG, "%s: null argument", who);
  PGX_REQUIRE(!c->shut && ctx().ready, PGX_ESTATE, "%s: pgx_shutdown ran while the contig paths were alive (free them)", who);
}

int build_entry(const char *who, pgx_unitigs *u, bool owns, pgx_ctg_paths **out) {
  return live_build(who, g_cp, out, [&] { PGX_REQUIRE(u, PGX_EARG, "%s: null argument", who); }, [&](pgx_ctg_paths *c, uint64_t *n) {
    MemTag tag("ctg_paths");
    *n = unitigs_device_view(u, who).n_u;
    KernelTimer tm("ctg_paths", *n);
    build_ctg_paths(u, c);
    c->owns_u = owns;
  }, "contig paths", "unitigs");
}

int text_entry(const char *who, pgx_ctg_paths *c, bool utg, uint64_t max_lines, char **text, size_t *text_len, int *done) {
  return text_call(text, text_len, done, [&] {
    require_cp(c, who);
    TextPlan &plan = utg ? c->utg : c->ctg;
    TextSrc src{c->ent.p, nullptr, nullptr, nullptr, 0, c->ctg_piece.p, c->ctg_head.p, c->n_ctg_pieces};
    // utg_data reads the unitigs' slot arrays -- where text_next will format something: it refuses its arguments, and hands out the empty
    // text behind the last line, before it looks at the source
    if (utg && text && text_len && done && max_lines && plan.cursor < plan.n_lines) {
      PGX_REQUIRE(unitigs_live(c->u, c->u_serial), PGX_ESTATE, "%s: the unitigs these contig paths were made of are gone (utg_data reads their paths)", who);
      const UnitigsView v = unitigs_device_view(c->u, who);
      src = TextSrc{c->ent.p, v.tab, v.slot_u, v.slot_w, c->m_slots, c->utg_piece.p, c->utg_head.p, c->n_utg_pieces};
    }
    text_next(who, plan, src, c->stage, TextNames{"ctg_paths", "ctg_paths_text", "ctg_paths", "cp.text"}, max_lines, text, text_len, done);
  });
}
}  // namespace
}  // namespace pgx

extern "C" int pgx_unitigs_contig_paths(pgx_unitigs *u, pgx_ctg_paths **out) { return build_entry("pgx_unitigs_contig_paths", u, false, out); }

extern "C" int pgx_ctg_paths_build(const pgx_sgraph_edge *edges, uint64_t n, pgx_ctg_paths **out) {
  if (!out) return guarded([&] { PGX_REQUIRE(out, PGX_EARG, "pgx_ctg_paths_build: null argument"); });
  *out = nullptr;
  pgx_unitigs *u = nullptr;
  int rc = pgx_unitigs_build(edges, n, &u);   // (checks what it checks, and says so under its own name)
  if (rc != PGX_OK) return rc;
  rc = build_entry("pgx_ctg_paths_build", u, true, out);
  if (rc != PGX_OK) pgx_unitigs_free(u);
  return rc;
}

extern "C" int pgx_ctg_paths_stats(const pgx_ctg_paths *c, pgx_ctg_paths_stats_t *out) {
  return guarded([&] {
    PGX_REQUIRE(out, PGX_EARG, "pgx_ctg_paths_stats: null argument");
    require_cp(c, "pgx_ctg_paths_stats");
    *out = c->st;
  });
}

extern "C" int pgx_ctg_paths_table(const pgx_ctg_paths *c, uint64_t first, uint64_t n, pgx_ctg_unitig *out) {
  return guarded([&] {
    require_cp(c, "pgx_ctg_paths_table");
    PGX_REQUIRE(first <= c->st.unitigs && n <= c->st.unitigs - first && (n == 0 || out), PGX_EARG, "pgx_ctg_paths_table: unitigs %llu .. + %llu of %llu",
                (unsigned long long)first, (unsigned long long)n, (unsigned long long)c->st.unitigs);
    std::copy(c->table.begin() + first, c->table.begin() + first + n, out);
  });
}

extern "C" int pgx_ctg_paths_rows(const pgx_ctg_paths *c, uint64_t *row_off, uint32_t *unitig) {
  return guarded([&] {
    require_cp(c, "pgx_ctg_paths_rows");
    if (row_off) std::copy(c->row_off.begin(), c->row_off.end(), row_off);
    if (unitig) std::copy(c->row_u.begin(), c->row_u.end(), unitig);
  });
}

extern "C" int pgx_ctg_paths_utg_text(pgx_ctg_paths *c, uint64_t max_lines, char **text, size_t *text_len, int *done) {
  return text_entry("pgx_ctg_paths_utg_text", c, true, max_lines, text, text_len, done);
}

extern "C" int pgx_ctg_paths_ctg_text(pgx_ctg_paths *c, uint64_t max_lines, char **text, size_t *text_len, int *done) {
  return text_entry("pgx_ctg_paths_ctg_text", c, false, max_lines, text, text_len, done);
}

extern "C" int pgx_ctg_paths_free(pgx_ctg_paths *c) {
  if (!c) return PGX_OK;
  pgx_unitigs *u = c->owns_u ? c->u : nullptr;
  g_cp.destroy(c);
  if (u) pgx_unitigs_free(u);
  return PGX_OK;
}
