// pgx_gfa.hip -- the assembly graph as GFA 1.0: the phase-1 unitigs (pgx_unitigs.hip) as segments with sequences, and the links between
// them.  The rule (include/pgx.h, "assembly graph as GFA"), over live unitigs and the edge records they were built from:
//   * dual(u) is the unitig that holds the reverse of u's first edge; u is canonical iff u < dual(u); a canonical unitig is a segment;
//   * a segment has one tiling row per edge of its path, and its bases are what the contig layout (pgx_contigs.hip) makes of the rows;
//   * (a, b) is a directed link iff t(a) == s(b); of a link and its dual (dual b, dual a) the smaller pair is written.
// Device layout.  unitig_of[e]: the unitig of the edge with creation index e (one scatter over the path array: each edge has one writer).
// G edges are numbered gi = 0 .. m-1 in creation order (gsel[gi]: the creation index); the out-list of a node is a range of
//   by_v   (vkey, gi) ascending                (a stable sort: within a node the edges ascend by creation index, and so do the unitigs they
//                                               start -- the links come out in ascending (a, b) without a sort of their own)
// and, for host records only, the reverse of an edge is looked up in
//   by_vw  (vkey, wkey, gi) ascending          (pgx_gedges.h: GEdges, find_vw)
// No launch and no host round trip per unitig or per link.  No result depends on the order in which atomics land: they count.
// The text: the bases come to the host once, from the layout; the heads and tails of the S lines and the L lines are formatted on the
// device with the piece scheme of pgx_text.h and the file is put together on the host, as contigs_from_rows writes its FASTA -- one copy
// of the bases.

#include <atomic>

#include "pgx_gedges.h"

typedef pgx_sgraph_edge Edge;

namespace pgx {
namespace {
// the counters of a build
enum : uint32_t { C_BEYOND = 0, C_FOREIGN = 1, C_DUAL = 2, C_LINK = 3, C_N = 4 };

// ---------------------------------------------------------------------------------------------------------
// the records against the unitigs, the edge -> unitig map
// ---------------------------------------------------------------------------------------------------------
// A thread per path slot k.  cnt[C_BEYOND] counts the path indices beyond the records, cnt[C_FOREIGN] the slots whose record is not the G
// edge the unitigs saw there (another node entered, another start node at a unitig's first slot).  unitig_of[] is written for the rest.
__global__ void k_gf_map(const uint32_t *__restrict__ paths, const uint32_t *__restrict__ slot_u, const uint64_t *__restrict__ slot_w, const pgx_unitig *__restrict__ tab,
                         const Edge *__restrict__ edges, uint32_t n, uint32_t m, uint32_t n_u, uint32_t *__restrict__ unitig_of, uint32_t *__restrict__ cnt) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const uint32_t e = paths[k], u = slot_u[k];
  if (e >= n) {
    atomicAdd(&cnt[C_BEYOND], 1u);
    return;
  }
  const Edge r = edges[e];
  bool ok = u < n_u && r.type == PGX_SGRAPH_G && wkey(r) == slot_w[k];
  if (ok && tab[u].first == k) ok = vkey(r) == ((uint64_t)tab[u].s_rid << 1 | tab[u].s_end);
  if (!ok) atomicAdd(&cnt[C_FOREIGN], 1u);
  else unitig_of[e] = u;
}

// ---------------------------------------------------------------------------------------------------------
// dual, segments, rows
// ---------------------------------------------------------------------------------------------------------
// A thread per unitig: the unitig of the reverse of its first edge.  sv == nullptr: the records are a built graph's, the reverse of e is
// e ^ 1; else (sv, sw, se) is by_vw and the reverse (rev w, rev v) is searched there.
__global__ void k_gf_dual(const pgx_unitig *__restrict__ tab, const uint32_t *__restrict__ paths, uint32_t n_u, uint32_t m, const Edge *__restrict__ edges, uint32_t n,
                          const uint32_t *__restrict__ unitig_of, const uint32_t *__restrict__ gsel, const uint64_t *__restrict__ sv, const uint64_t *__restrict__ sw,
                          const uint32_t *__restrict__ se, uint32_t *__restrict__ dual) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_u) return;
  uint32_t r = NONE;
  if (tab[u].first < m) {
    const uint32_t e = paths[tab[u].first];
    if (!sv) {
      r = e ^ 1u;
    } else {
      const uint64_t rv = wkey(edges[e]) ^ 1u, rw = vkey(edges[e]) ^ 1u;
      const uint32_t i = find_vw(sv, sw, m, rv, rw);
      if (i != NONE) r = gsel[se[i]];
    }
  }
  dual[u] = r < n ? unitig_of[r] : NONE;
}
// cnt[C_DUAL] counts the unitigs without a dual, their own dual, or whose dual's dual is another; flag[u] = u is canonical
__global__ void k_gf_canon(const uint32_t *__restrict__ dual, uint32_t n_u, uint8_t *__restrict__ flag, uint32_t *__restrict__ cnt) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_u) return;
  const uint32_t d = dual[u];
  const bool ok = d < n_u && d != u && dual[d] == u;
  if (!ok) atomicAdd(&cnt[C_DUAL], 1u);
  flag[u] = ok && u < d;
}
// (only behind a clean k_gf_canon: every dual is in range)
__global__ void k_gf_segs(const uint32_t *__restrict__ seg_unitig, uint32_t n_seg, const pgx_unitig *__restrict__ tab, const uint32_t *__restrict__ dual,
                          uint32_t *__restrict__ seg_of, pgx_gfa_segment *__restrict__ segs, uint32_t *__restrict__ n_rows) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_seg) return;
  const uint32_t u = seg_unitig[j], d = dual[u];
  pgx_gfa_segment s = {};
  s.unitig = u, s.dual = d, s.n_rows = tab[u].n_edges, s.circular = tab[u].circular;
  segs[j] = s, n_rows[j] = s.n_rows, seg_of[u] = j, seg_of[d] = j;
}
__global__ void k_gf_first_rows(const uint64_t *__restrict__ first_row, uint32_t n_seg, pgx_gfa_segment *__restrict__ segs) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n_seg) segs[j].first_row = first_row[j];
}
// Row slot r: its segment by binary search of the first-row offsets (as k_tl_rows finds its path), its edge through the path array, the
// 24-byte row.  Grid-stride (stride_grid).  first_row: n_seg + 1 entries; every path index is below n (k_gf_map counted none beyond).
__global__ void k_gf_rows(const uint64_t *__restrict__ first_row, const pgx_gfa_segment *__restrict__ segs, uint32_t n_seg, const pgx_unitig *__restrict__ tab,
                          const uint32_t *__restrict__ paths, uint32_t m, const Edge *__restrict__ edges, uint32_t n_rows, pgx_tile_row *__restrict__ rows) {
  for (uint64_t r64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r64 < n_rows; r64 += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = (uint32_t)r64;
    const uint32_t j = last_le(first_row, n_seg, r);
    const uint64_t k = tab[segs[j].unitig].first + (r - first_row[j]);
    pgx_tile_row row = {};
    if (k < m) {
      const Edge e = edges[paths[k]];
      row.ctg = j, row.rid0 = e.v_rid, row.rid1 = e.w_rid, row.s = e.sp, row.e = e.tp, row.strand0 = e.v_end & 1u ? 0 : 1, row.strand1 = e.w_end & 1u ? 0 : 1;
    }
    rows[r] = row;
  }
}

// ---------------------------------------------------------------------------------------------------------
// links
// ---------------------------------------------------------------------------------------------------------
// per directed unitig a: where the out-list of t(a) starts in by_v, and its width
__global__ void k_gf_link_width(const pgx_unitig *__restrict__ tab, uint32_t n_u, const uint64_t *__restrict__ ov, uint32_t m, uint32_t *__restrict__ lo_out,
                                uint32_t *__restrict__ width) {
  const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n_u) return;
  const uint64_t t = (uint64_t)tab[a].t_rid << 1 | tab[a].t_end;
  const uint32_t lo = lower_bound(ov, m, t);
  lo_out[a] = lo, width[a] = lower_bound(ov, m, t + 1) - lo;
}
// Link slot i: a by binary search of the scanned widths, b = the unitig whose first edge is the i - loff[a]-th out-edge of t(a); keep[i]:
// (a, b) is smaller than its dual (dual b, dual a).  cnt[C_LINK] counts the out-edges that start no unitig and the links that are their
// own dual.  Grid-stride (stride_grid).
__global__ void k_gf_link_fill(const uint64_t *__restrict__ loff, const uint32_t *__restrict__ lo_out, uint32_t n_u, uint32_t n_dir, const uint32_t *__restrict__ oe,
                               const uint32_t *__restrict__ gsel, uint32_t m, const uint32_t *__restrict__ unitig_of, const pgx_unitig *__restrict__ tab,
                               const uint32_t *__restrict__ paths, const uint32_t *__restrict__ dual, uint32_t *__restrict__ la, uint32_t *__restrict__ lb,
                               uint8_t *__restrict__ keep, uint32_t *__restrict__ cnt) {
  for (uint64_t i64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i64 < n_dir; i64 += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t i = (uint32_t)i64;
    const uint32_t a = last_le(loff, n_u, i);
    const uint64_t p = (uint64_t)lo_out[a] + (i - loff[a]);
    uint32_t b = NONE;
    if (p < m) {
      const uint32_t e = gsel[oe[p]];
      b = unitig_of[e];
      if (b >= n_u || tab[b].first >= m || paths[tab[b].first] != e) b = NONE;
    }
    bool k = false;
    if (b == NONE) {
      atomicAdd(&cnt[C_LINK], 1u);
      b = 0;
    } else {
      const uint32_t da = dual[a], db = dual[b];
      if (db == a && da == b) atomicAdd(&cnt[C_LINK], 1u);
      k = a < db || (a == db && b < da);
    }
    la[i] = a, lb[i] = b, keep[i] = k;
  }
}
__global__ void k_gf_links(const uint32_t *__restrict__ kept, uint32_t n_links, const uint32_t *__restrict__ la, const uint32_t *__restrict__ lb,
                           const uint32_t *__restrict__ dual, const uint32_t *__restrict__ seg_of, pgx_gfa_link *__restrict__ links) {
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= n_links) return;
  const uint32_t a = la[kept[l]], b = lb[kept[l]];
  pgx_gfa_link k = {};
  k.from_seg = seg_of[a], k.to_seg = seg_of[b], k.from_rev = a > dual[a], k.to_rev = b > dual[b];
  links[l] = k;
}

// ---------------------------------------------------------------------------------------------------------
// the text but the bases.  Pieces 2j and 2j + 1: the head of segment j's line ("S\t<name>\t") and its tail ("\tLN:i:<bases>\n", or
// "*\n" without sequences); piece 2 n_seg + l: link l's line.  The piece source of pgx_text.h's piece scheme.
// ---------------------------------------------------------------------------------------------------------
struct GfaPieces {
  const pgx_gfa_segment *__restrict__ segs;
  const pgx_gfa_link *__restrict__ links;
  uint32_t n_seg;
  uint32_t with_seq;
  uint32_t n;                            // 2 n_seg + links
  static constexpr uint32_t MAX = 48;    // a name is <= 13 bytes ("utg" and ten digits): a head 16, a tail <= 27, a link 36
  template <bool WRITE>
  __device__ static void name(LineOut<WRITE> &o, uint32_t unitig) {
    o.ch('u'), o.ch('t'), o.ch('g'), o.u32(unitig, 6);
  }
  template <bool WRITE>
  __device__ uint32_t piece(uint32_t j, char *dst) const {
    LineOut<WRITE> o{dst, 0};
    if (j < 2 * n_seg) {
      const pgx_gfa_segment s = segs[j >> 1];
      if (!(j & 1)) {
        o.ch('S'), o.ch('\t'), name(o, s.unitig), o.ch('\t');
      } else if (with_seq) {
        for (const char *c = "\tLN:i:"; *c; ++c) o.ch(*c);
        o.u64(s.seq_len), o.ch('\n');
      } else {
        o.ch('*'), o.ch('\n');
      }
    } else {
      const pgx_gfa_link l = links[j - 2 * n_seg];
      o.ch('L'), o.ch('\t'), name(o, segs[l.from_seg].unitig), o.ch('\t'), o.ch(l.from_rev ? '-' : '+'), o.ch('\t');
      name(o, segs[l.to_seg].unitig), o.ch('\t'), o.ch(l.to_rev ? '-' : '+'), o.ch('\t'), o.ch('*'), o.ch('\n');
    }
    return o.n;
  }
};
const char GFA_HEADER[] = "H\tVN:Z:1.0\n";
}  // namespace
}  // namespace pgx

using namespace pgx;

struct pgx_gfa {
  DevBuf<pgx_gfa_segment> segs;   // (MemTag "gfa", as all of these)
  DevBuf<pgx_gfa_link> links;
  DevBuf<pgx_tile_row> rows;
  // the file, on the host: the formatted pieces back to back (piece p at [poff[p], poff[p + 1])) and the segments' bases (segment j's at
  // seq_off[j] .. seq_off[j + 1]; none without a database)
  std::vector<char> pieces;
  std::vector<uint64_t> poff, seq_off;
  std::vector<const char *> seq_at;   // per segment: its bases, in `bases` or in a batch of `batches`
  char *bases = nullptr;          // a resident database: the layout's text (out_alloc)
  ContigPieces batches;           // the file level: the texts of the layout's batches
  pgx_gfa_stats_t st = {};
  bool with_seq = false;
  bool shut = false;
  void drop_device_state() { segs.release(), links.release(), rows.release(); }
  ~pgx_gfa() { out_free(bases); }
};

namespace pgx {
namespace {
LiveSet<pgx_gfa> g_gfa;
ShutdownHook g_gfa_hook([] { g_gfa.shutdown(); });

void require_gfa(const pgx_gfa *f, const char *who) {
  PGX_REQUIRE(f, PGX_EARG, "%s: null argument", who);
  PGX_REQUIRE(!f->shut && ctx().ready, PGX_ESTATE, "%s: pgx_shutdown ran while the GFA was alive (free it)", who);
}

// where the segments' bases come from: a resident database, or <prefix>.idx / .seqdb (the file level), or neither
struct SeqSource {
  pgx_seqdb *db = nullptr;
  const char *prefix = nullptr;
  explicit operator bool() const { return db || prefix; }
};

// the segments' bases through the contig layout -- one call on a resident database, the batches of contigs_from_rows at the file level;
// a refused row is named by segment, place in the path and edge
void layout_segments(const char *who, pgx_gfa *f, const UnitigsView &uv, const SeqSource &src, const std::vector<pgx_gfa_segment> &segs) {
  hipStream_t st = ctx().stream;
  const size_t n_seg = segs.size(), n_rows = f->st.rows;
  std::vector<pgx_tile_row> rows(n_rows);
  f->rows.download(rows.data(), n_rows);
  pgx::sync();
  uint64_t total = 0;
  f->seq_at.assign(n_seg, nullptr);
  try {
    if (src.db) {
      contigs_resident_rows(who, src.db, rows, n_seg, &f->bases, f->seq_off.data(), &total);
      for (size_t j = 0; j < n_seg; ++j) f->seq_at[j] = f->bases + f->seq_off[j];
    } else {
      contig_pieces_from_rows(who, src.prefix, [&](const TileRowFn &add) {
        for (size_t i = 0; i < n_rows; ++i) {
          const pgx_tile_row &r = rows[i];
          add(std::to_string(r.ctg), r.rid0, r.rid1, r.s, r.e, r.strand0, r.strand1, i);
        }
      }, f->batches);
      for (const ContigPieces::Piece &pc : f->batches.pieces)
        for (size_t c = 0; c + 1 < pc.off.size(); ++c) {
          const size_t j = pc.ctg0 + c;
          PGX_REQUIRE(j < n_seg, PGX_EHIP, "%s: the layout answers segment %zu of %zu (a bug)", who, j, n_seg);
          f->seq_at[j] = pc.text + pc.off[c], f->seq_off[j + 1] = pc.off[c + 1] - pc.off[c];
        }
      for (size_t j = 0; j < n_seg; ++j) f->seq_off[j + 1] += f->seq_off[j];
      total = f->seq_off[n_seg];
      PGX_REQUIRE(f->batches.names.size() == n_seg && total == f->batches.bases, PGX_EHIP, "%s: the layout answers %zu of %zu segments (a bug)", who,
                  f->batches.names.size(), n_seg);
    }
  } catch (const Fail &fail) {
    if (fail.code != PGX_EARG || fail.piece < 0 || (uint64_t)fail.piece >= n_rows) throw;
    size_t j = 0;   // the last segment that starts at or before the row
    for (size_t lo = 0, hi = n_seg; lo < hi;) {
      const size_t mid = lo + ((hi - lo) >> 1);
      if (segs[mid].first_row <= (uint64_t)fail.piece) j = mid, lo = mid + 1;
      else hi = mid;
    }
    const uint64_t at = (uint64_t)fail.piece - segs[j].first_row;
    pgx_unitig un = {};
    uint32_t edge = NONE;
    PGX_HIP(hipMemcpyAsync(&un, uv.tab + segs[j].unitig, sizeof(un), hipMemcpyDeviceToHost, st));
    pgx::sync();
    if (un.first + at < uv.m) {
      PGX_HIP(hipMemcpyAsync(&edge, uv.paths + un.first + at, sizeof(edge), hipMemcpyDeviceToHost, st));
      pgx::sync();
    }
    const std::string why = pgx_last_error();
    set_error("%s: segment %zu (utg%06u), position %llu of its path, edge %u: %s", who, j, segs[j].unitig, (unsigned long long)at, edge, why.c_str());
    throw Fail{PGX_EARG};
  }
  f->st.bases = total;
}

// fills f from the unitigs and the n device edge records; pairs: the records are a built graph's (edge e's reverse is e ^ 1)
void build_gfa(const char *who, const UnitigsView &uv, const Edge *d_edges, uint64_t n64, bool pairs, const SeqSource &seq, pgx_gfa *f) {
  hipStream_t st = ctx().stream;
  PrimWs tmp;
  PGX_REQUIRE(n64 <= (uint64_t)INT32_MAX, PGX_EARG, "pgx_gfa_build: %llu edge records, more than 2^31 - 1", (unsigned long long)n64);
  const uint32_t n = (uint32_t)n64, m = (uint32_t)uv.m, n_u = (uint32_t)uv.n_u;
  f->with_seq = (bool)seq;
  f->st.unitigs = n_u;
  f->poff.assign(1, 0), f->seq_off.assign(1, 0);
  // ---- the records against the unitigs, the edge -> unitig map, the sorted lists
  std::unique_ptr<KernelTimer> part(new KernelTimer("gfa_dual", n));
  GEdges g;
  g.select(d_edges, n, &tmp);
  PGX_REQUIRE(g.m == m, PGX_EARG, "pgx_gfa_build: the edge records hold %u G edges, the unitigs were built from %u", g.m, m);
  if (m == 0) return;
  DevBuf<uint32_t> cnt(C_N), unitig_of(n);
  PGX_HIP(hipMemsetAsync(cnt.p, 0, C_N * sizeof(uint32_t), st));
  PGX_HIP(hipMemsetAsync(unitig_of.p, 0xFF, (size_t)n * sizeof(uint32_t), st));
  LAUNCH(k_gf_map, m, uv.paths, uv.slot_u, uv.slot_w, uv.tab, d_edges, n, m, n_u, unitig_of.p, cnt.p);
  PGX_HIP(hipGetLastError());
  uint32_t h_cnt[C_N];
  cnt.download(h_cnt, C_N);
  pgx::sync();
  PGX_REQUIRE(h_cnt[C_BEYOND] == 0, PGX_EARG, "pgx_gfa_build: %u path indices lie beyond the %u edge records", h_cnt[C_BEYOND], n);
  PGX_REQUIRE(h_cnt[C_FOREIGN] == 0, PGX_EARG, "pgx_gfa_build: %u path edges are not the G edges the unitigs were built from (the records of another graph)",
              h_cnt[C_FOREIGN]);
  DevBuf<uint64_t> ov(m);
  DevBuf<uint32_t> oe(m);
  g.keys(NoRule{}, nullptr);
  sort_pairs(g.vk.p, ov.p, g.ids.p, oe.p, m, 0, 33, &tmp);
  DevBuf<uint32_t> dual(n_u);
  if (!pairs) g.by_w(&tmp), g.by_vw(nullptr, &tmp);   // host records: the reverse of an edge is looked up in by_vw
  LAUNCH(k_gf_dual, n_u, uv.tab, uv.paths, n_u, m, d_edges, n, unitig_of.p, g.gsel.p, g.sv.p, g.sw.p, g.out_e.p, dual.p);
  g.vk.release(), g.wk.release(), g.release_lists();
  // ---- segments
  uint32_t n_seg = 0;
  DevBuf<uint32_t> seg_unitig(n_u), seg_of(n_u);
  {
    DevBuf<uint8_t> flag(n_u);
    LAUNCH(k_gf_canon, n_u, dual.p, n_u, flag.p, cnt.p);
    PGX_HIP(hipGetLastError());
    cnt.download(h_cnt, C_N);
    n_seg = select_indices(flag.p, n_u, seg_unitig.p, &tmp);   // (synchronises: h_cnt is there)
  }
  PGX_REQUIRE(h_cnt[C_DUAL] == 0 && 2 * (uint64_t)n_seg == n_u, PGX_ESTATE, "pgx_gfa_build: %u of %u unitigs have no dual of their own (%u segments): nothing is written",
              h_cnt[C_DUAL], n_u, n_seg);
  part.reset(), part.reset(new KernelTimer("gfa_rows", m));
  f->segs.alloc(n_seg);
  DevBuf<uint64_t> first_row((size_t)n_seg + 1);
  {
    DevBuf<uint32_t> seg_rows(n_seg);
    LAUNCH(k_gf_segs, n_seg, seg_unitig.p, n_seg, uv.tab, dual.p, seg_of.p, f->segs.p, seg_rows.p);
    const uint64_t n_rows = scan_to_total(seg_rows.p, first_row.p, n_seg, &tmp);
    PGX_REQUIRE(2 * n_rows == m, PGX_ESTATE, "pgx_gfa_build: the segments hold %llu rows, not half of the %u G edges: nothing is written", (unsigned long long)n_rows, m);
    f->st.segments = n_seg, f->st.rows = n_rows;
  }
  const uint32_t n_rows = (uint32_t)f->st.rows;
  f->rows.alloc(n_rows);
  LAUNCH(k_gf_first_rows, n_seg, first_row.p, n_seg, f->segs.p);
  hipLaunchKernelGGL(k_gf_rows, dim3(stride_grid(cdiv(n_rows, 256), 8)), dim3(256), 0, st, first_row.p, f->segs.p, n_seg, uv.tab, uv.paths, m, d_edges, n_rows, f->rows.p);
  PGX_HIP(hipGetLastError());
  part.reset();
  // ---- sequences: the rows come to the host once and go through the contig layout
  std::vector<pgx_gfa_segment> h_segs(n_seg);
  f->seq_off.assign((size_t)n_seg + 1, 0);
  if (seq) {
    f->segs.download(h_segs.data(), n_seg);
    pgx::sync();
    layout_segments(who, f, uv, seq, h_segs);
    for (uint32_t j = 0; j < n_seg; ++j) h_segs[j].seq_off = f->seq_off[j], h_segs[j].seq_len = f->seq_off[j + 1] - f->seq_off[j];
    f->segs.upload(h_segs.data(), n_seg);
  }
  // ---- links
  part.reset(new KernelTimer("gfa_links", n_u));
  uint32_t n_links = 0;
  {
    DevBuf<uint32_t> lo_out(n_u), width(n_u);
    DevBuf<uint64_t> loff((size_t)n_u + 1);
    LAUNCH(k_gf_link_width, n_u, uv.tab, n_u, ov.p, m, lo_out.p, width.p);
    const uint64_t n_dir64 = scan_to_total(width.p, loff.p, n_u, &tmp);
    PGX_REQUIRE(n_dir64 <= (uint64_t)INT32_MAX, PGX_EARG, "pgx_gfa_build: %llu directed links, more than 2^31 - 1", (unsigned long long)n_dir64);
    const uint32_t n_dir = (uint32_t)n_dir64;
    f->st.links_directed = n_dir;
    if (n_dir) {
      DevBuf<uint32_t> la(n_dir), lb(n_dir), kept(n_dir);
      DevBuf<uint8_t> keep(n_dir);
      hipLaunchKernelGGL(k_gf_link_fill, dim3(stride_grid(cdiv(n_dir, 256), 8)), dim3(256), 0, st, loff.p, lo_out.p, n_u, n_dir, oe.p, g.gsel.p, m, unitig_of.p, uv.tab,
                         uv.paths, dual.p, la.p, lb.p, keep.p, cnt.p);
      PGX_HIP(hipGetLastError());
      cnt.download(h_cnt, C_N);
      n_links = select_indices(keep.p, n_dir, kept.p, &tmp);   // (synchronises)
      PGX_REQUIRE(h_cnt[C_LINK] == 0 && 2 * (uint64_t)n_links == n_dir, PGX_ESTATE,
                  "pgx_gfa_build: %u of %u directed links start no unitig or are their own dual (%u kept): nothing is written", h_cnt[C_LINK], n_dir, n_links);
      f->links.alloc(n_links);
      LAUNCH(k_gf_links, n_links, kept.p, n_links, la.p, lb.p, dual.p, seg_of.p, f->links.p);
      PGX_HIP(hipGetLastError());
    }
    f->st.links = n_links;
  }
  // ---- the text but the bases
  part.reset(), part.reset(new KernelTimer("gfa_text", (uint64_t)n_seg + n_links));
  const uint64_t n_piece = 2 * (uint64_t)n_seg + n_links;
  PGX_REQUIRE(n_piece < (1ULL << 31), PGX_EARG, "pgx_gfa_build: %llu text pieces, more than 2^31 - 1", (unsigned long long)n_piece);
  const GfaPieces src{f->segs.p, f->links.p, n_seg, f->with_seq ? 1u : 0u, (uint32_t)n_piece};
  TextPlan plan;
  plan_text(src, (const uint32_t *)nullptr, n_piece, &plan, &tmp);
  f->poff.assign(n_piece + 1, 0);
  plan.poff.download(f->poff.data(), n_piece + 1);
  pgx::sync();
  const uint64_t total = f->poff[n_piece];
  DevBuf<char> d_text(total + 16);
  hipLaunchKernelGGL(k_piece_format<GfaPieces>, dim3(cdiv(total, TEXT_TILE)), dim3(TEXT_THREADS), 0, st, src, plan.poff.p, (uint64_t)0, total, d_text.p);
  PGX_HIP(hipGetLastError());
  f->pieces.resize(total);
  PGX_HIP(hipMemcpyAsync(f->pieces.data(), d_text.p, total, hipMemcpyDeviceToHost, st));
  pgx::sync();
  part.reset();
}

// the file's parts in order: emit(ptr, len) takes each; its length
template <class Emit>
uint64_t gfa_parts(const pgx_gfa *f, Emit &&emit) {
  uint64_t total = 0;
  auto put = [&](const char *p, uint64_t len) {
    if (len) emit(p, len);
    total += len;
  };
  put(GFA_HEADER, sizeof(GFA_HEADER) - 1);
  const size_t n_seg = f->st.segments;
  const char *pc = f->pieces.data();
  for (size_t j = 0; j < n_seg; ++j) {
    put(pc + f->poff[2 * j], f->poff[2 * j + 1] - f->poff[2 * j]);
    if (f->with_seq) put(f->seq_at[j], f->seq_off[j + 1] - f->seq_off[j]);
    put(pc + f->poff[2 * j + 1], f->poff[2 * j + 2] - f->poff[2 * j + 1]);
  }
  put(pc + f->poff[2 * n_seg], f->poff.back() - f->poff[2 * n_seg]);   // the links
  return total;
}

template <class T>
void table_out(const char *who, const DevBuf<T> &tab, uint64_t have, uint64_t first, uint64_t n, T *out) {
  PGX_REQUIRE(first <= have && n <= have - first && (n == 0 || out), PGX_EARG, "%s: entries %llu .. + %llu of %llu", who, (unsigned long long)first,
              (unsigned long long)n, (unsigned long long)have);
  if (n == 0) return;
  PGX_HIP(hipMemcpyAsync(out, tab.p + first, n * sizeof(T), hipMemcpyDeviceToHost, ctx().stream));
  pgx::sync();
}
}  // namespace
}  // namespace pgx

namespace pgx {
namespace {
// the common part of the two builders
int build_entry(const char *who, pgx_unitigs *u, pgx_sgraph *g, const pgx_sgraph_edge *edges, uint64_t n_edges, const SeqSource &seq, pgx_gfa **out) {
  return live_build(who, g_gfa, out, [&] {
    PGX_REQUIRE(u, PGX_EARG, "%s: null argument", who);
    PGX_REQUIRE((g != nullptr) != (edges != nullptr), PGX_EARG, "%s: exactly one of a graph and host edge records is given (%s)", who,
                g ? "both are" : "neither is");
  }, [&](pgx_gfa *f, uint64_t *n) {
    MemTag tag("gfa");
    const UnitigsView uv = unitigs_device_view(u, who);
    DevBuf<Edge> own;
    const Edge *d_edges = nullptr;
    if (g) {
      d_edges = sgraph_device_edges(g, who, n);
    } else {
      PGX_REQUIRE(n_edges <= (uint64_t)INT32_MAX, PGX_EARG, "%s: %llu edge records, more than 2^31 - 1", who, (unsigned long long)n_edges);
      *n = n_edges;
      own.alloc(n_edges);
      own.upload(edges, n_edges);
      d_edges = own.p;
    }
    KernelTimer tm("gfa", *n);
    build_gfa(who, uv, d_edges, *n, g != nullptr, seq, f);
  }, "GFA", "edges");
}
}  // namespace
}  // namespace pgx

extern "C" int pgx_gfa_build(pgx_unitigs *u, pgx_sgraph *g, const pgx_sgraph_edge *edges, uint64_t n_edges, pgx_seqdb *db, pgx_gfa **out) {
  SeqSource seq;
  seq.db = db;
  return build_entry("pgx_gfa_build", u, g, edges, n_edges, seq, out);
}

extern "C" int pgx_gfa_build_files(pgx_unitigs *u, pgx_sgraph *g, const pgx_sgraph_edge *edges, uint64_t n_edges, const char *seqdb_prefix, pgx_gfa **out) {
  SeqSource seq;
  seq.prefix = seqdb_prefix;
  return build_entry("pgx_gfa_build_files", u, g, edges, n_edges, seq, out);
}

extern "C" int pgx_gfa_stats(const pgx_gfa *f, pgx_gfa_stats_t *out) {
  return guarded([&] {
    PGX_REQUIRE(out, PGX_EARG, "pgx_gfa_stats: null argument");
    require_gfa(f, "pgx_gfa_stats");
    *out = f->st;
  });
}

extern "C" int pgx_gfa_segments(const pgx_gfa *f, uint64_t first, uint64_t n, pgx_gfa_segment *out) {
  return guarded([&] {
    require_gfa(f, "pgx_gfa_segments");
    table_out("pgx_gfa_segments", f->segs, f->st.segments, first, n, out);
  });
}

extern "C" int pgx_gfa_links(const pgx_gfa *f, uint64_t first, uint64_t n, pgx_gfa_link *out) {
  return guarded([&] {
    require_gfa(f, "pgx_gfa_links");
    table_out("pgx_gfa_links", f->links, f->st.links, first, n, out);
  });
}

extern "C" int pgx_gfa_rows(const pgx_gfa *f, uint64_t first, uint64_t n, pgx_tile_row *out) {
  return guarded([&] {
    require_gfa(f, "pgx_gfa_rows");
    table_out("pgx_gfa_rows", f->rows, f->st.rows, first, n, out);
  });
}

extern "C" int pgx_gfa_text(pgx_gfa *f, char **text, size_t *len) {
  return text_call(text, len, nullptr, [&] {
    PGX_REQUIRE(text && len, PGX_EARG, "pgx_gfa_text: null argument");
    require_gfa(f, "pgx_gfa_text");
    const uint64_t total = gfa_parts(f, [](const char *, uint64_t) {});
    char *t = caller_text(nullptr, total);
    uint64_t at = 0;
    gfa_parts(f, [&](const char *p, uint64_t n) { memcpy(t + at, p, n), at += n; });
    *text = t, *len = total;
  });
}

extern "C" int pgx_gfa_write(pgx_gfa *f, const char *path) {
  return guarded([&] {
    require_gfa(f, "pgx_gfa_write");
    FILE *o = path ? fopen(path, "wb") : stdout;
    PGX_REQUIRE(o, PGX_EIO, "pgx_gfa_write: cannot write %s", path);
    bool ok = true;
    gfa_parts(f, [&](const char *p, uint64_t n) { ok = ok && fwrite(p, 1, n, o) == n; });
    ok = (path ? fclose(o) == 0 : fflush(o) == 0) && ok;
    PGX_REQUIRE(ok, PGX_EIO, "pgx_gfa_write: writing %s failed", path ? path : "stdout");
  });
}

extern "C" int pgx_gfa_free(pgx_gfa *f) {
  if (f) g_gfa.destroy(f);
  return PGX_OK;
}
