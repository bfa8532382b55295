// pgx_tiling.hip -- the tiling paths (py/scripts/graph_to_path.py:134-326): from sg_edges_list (a file, or a built string graph on the
// device), utg_data and ctg_paths to p_ctg_tiling_path and a_ctg_tiling_path, byte for byte, and to the same rows as pgx_tile_row.  The
// rule is stated in DESIGN.md, "tiling paths".  Who does what:
//   device  sg_edges_list text -> edge records (the hot path: the file goes up in pieces, a lane tokenises a line); the edge table
//           as a list sorted by (v, w) with its duplicate and E/B checks (by_vw of pgx_gedges.h, looked up by find_vw); the unitig
//           index (the three keys under three stable sorts, one binary search per name) and the dual-skip rule of ctg_paths (a sort by
//           canonical key, the group's first row wins); every
//           node and edge of every path: path slots by binary search of the segments' offsets, the edge of every consecutive pair by
//           binary search of the table, |s - t|, the running length of a contig, the rows, the lengths of the lines and the text
//           (tiles of 8 KiB formatted in LDS, 16-byte stores).
//   host    utg_data and ctg_paths (a few percent of the bytes) are tokenised in one pass with no allocation per token; the kept rows
//           are walked in file order to raise what the script would raise; the compound unitigs' shortest-path rounds run once for
//           all bundles, on edge scores that ONE device lookup fetched.  A path reaches the device as segments of a node pool.
// No result depends on the order in which atomics land: they take a minimum (the first offending line, edge or row) or count.

#include <algorithm>
#include <queue>
#include <string>
#include <tuple>
#include <unordered_map>

#include "pgx_gedges.h"

typedef pgx_sgraph_edge Edge;

namespace pgx {
namespace {
constexpr uint32_t SG_LINE_MAX = 256;    // bytes of a sg_edges_list line, its '\n' not counted
constexpr uint32_t CTG_NAME_MAX = 96;     // bytes of a contig name in a tiling path line (an alternate's suffix included)
constexpr uint64_t VIA_NA = ~0ULL;    // the `via` of a compound unitig ("NA")
enum : uint8_t { PE_OK = 0, PE_LONG, PE_FIELDS, PE_NODE, PE_RID, PE_INT, PE_IDT, PE_BYTE };
const char *const PE_TEXT[] = {"", "is longer than 256 bytes", "does not have 8 fields", "has a node name that is not '%09d:B' or '%09d:E' of a read id below 2^31",
                               "has a read id that is not '%09d' of a number below 2^31", "has a number that is not a decimal integer in range",
                               "has an identity that is not a decimal with at most two fraction digits", "has a byte that is not ASCII"};

// ---------------------------------------------------------------------------------------------------------
// fields (host and device; is_blank and parse_int: pgx_text.h): the names and numbers that print back as they were read
// ---------------------------------------------------------------------------------------------------------
// the digits "%09d" prints for a value in [0, 2^31): nine, or ten without a leading zero
__host__ __device__ inline bool parse_rid(const char *p, uint32_t n, uint32_t *rid) {
  if (n < 9 || n > 10 || (n > 9 && p[0] == '0')) return false;
  uint64_t v = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (p[i] < '0' || p[i] > '9') return false;
    v = v * 10 + (uint32_t)(p[i] - '0');
  }
  if (v > 0x7FFFFFFFu) return false;
  *rid = (uint32_t)v;
  return true;
}
__host__ __device__ inline bool parse_node(const char *p, uint32_t n, uint64_t *key) {
  if (n < 3 || p[n - 2] != ':' || (p[n - 1] != 'B' && p[n - 1] != 'E')) return false;
  uint32_t rid;
  if (!parse_rid(p, n - 2, &rid)) return false;
  *key = (uint64_t)rid << 1 | (p[n - 1] == 'E');
  return true;
}
// an identity in hundredths: [-] up to 9 digits [. up to 2 digits], a digit at least; no exponent, no nan, no "-0" (which prints "-0.00")
__host__ __device__ inline bool parse_idt(const char *p, uint32_t n, int64_t *h) {
  const bool neg = n && p[0] == '-';
  uint32_t i = neg, ni = 0, nf = 0;
  int64_t v = 0, f = 0;
  for (; i < n && p[i] >= '0' && p[i] <= '9'; ++i, ++ni) v = v * 10 + (p[i] - '0');
  if (ni > 9) return false;
  if (i < n && p[i] == '.')
    for (++i; i < n && p[i] >= '0' && p[i] <= '9'; ++i, ++nf) f = f * 10 + (p[i] - '0');
  if (i != n || nf > 2 || ni + nf == 0) return false;
  v = v * 100 + (nf == 1 ? f * 10 : f);
  if (neg && v == 0) return false;
  *h = neg ? -v : v;
  return true;
}

// ---------------------------------------------------------------------------------------------------------
// sg_edges_list text -> edge records
// ---------------------------------------------------------------------------------------------------------
// flag[i] = text[i] == '\n', four bytes to a thread (the buffers are padded with zeros to a multiple of 4); *count += the newlines
__global__ void k_tl_newlines(const uint32_t *__restrict__ text4, uint32_t n4, uint32_t *__restrict__ flag4, uint32_t *__restrict__ count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t c = 0;
  if (i < n4) {
    const uint32_t x = text4[i] ^ 0x0A0A0A0Au;
    uint32_t f = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (((x >> (8 * k)) & 0xFFu) == 0) f |= 1u << (8 * k), ++c;
    flag4[i] = f;
  }
  for (int off = 32; off; off >>= 1) c += __shfl_down(c, off);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

struct Cursor {
  const char *p;
  uint32_t i, n;
  bool ascii;
  __device__ bool next(uint32_t &a, uint32_t &l) {
    while (i < n && is_blank((unsigned char)p[i])) ++i;
    if (i >= n) return false;
    a = i;
    while (i < n && !is_blank((unsigned char)p[i])) ascii &= !(p[i] & 0x80), ++i;
    l = i - a;
    return true;
  }
};
// A lane per line: line k is text[nlpos[k - 1] + 1, nlpos[k]).  keep[k]: the line is not blank (its record is rec[k], hund[k]); code[k]: why
// it is refused, and err[0] = min(err[0], k) then.  all: the numbers of every line must parse (else: those of the G lines, which is all
// the script reads of the others).
__global__ void k_tl_tokenise(const char *__restrict__ text, const uint32_t *__restrict__ nlpos, uint32_t nl, uint32_t all, Edge *__restrict__ rec,
                              int64_t *__restrict__ hund, uint8_t *__restrict__ keep, uint8_t *__restrict__ code, uint32_t *__restrict__ err) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nl) return;
  const uint32_t start = k ? nlpos[k - 1] + 1 : 0, len = nlpos[k] - start;
  uint8_t why = PE_OK, kept = 0;
  Edge e = {};
  int64_t h = 0;
  if (len > SG_LINE_MAX) {
    why = PE_LONG;
  } else {
    Cursor c{text + start, 0, len, true};
    uint32_t a[8], l[8], nf = 0;
#pragma unroll
    for (int f = 0; f < 8; ++f)
      if (nf == (uint32_t)f && c.next(a[f], l[f])) ++nf;
    uint32_t xa, xl;
    const bool more = nf == 8 && c.next(xa, xl);
    if (nf == 0) {
      // a blank line: skipped
    } else if (nf != 8 || more) {
      why = PE_FIELDS;
    } else {
      kept = 1;
      const char *p = c.p;
      const char *ty = p + a[7];
      e.type = l[7] == 1 && ty[0] == 'G' ? PGX_SGRAPH_G : l[7] == 2 && ty[0] == 'T' && ty[1] == 'R' ? PGX_SGRAPH_TR : l[7] == 1 && ty[0] == 'S' ? PGX_SGRAPH_S
               : l[7] == 1 && ty[0] == 'R' ? PGX_SGRAPH_R : 4;
      uint64_t vk = 0, wk = 0;
      int64_t sp = 0, tp = 0, score = 0;
      uint32_t label = 0;
      if (!c.ascii) why = PE_BYTE;
      else if (!parse_node(p + a[0], l[0], &vk) || !parse_node(p + a[1], l[1], &wk)) why = PE_NODE;
      else if (!parse_rid(p + a[2], l[2], &label)) why = PE_RID;
      else if (!parse_int(p + a[3], l[3], &sp) || !parse_int(p + a[4], l[4], &tp) || !parse_int(p + a[5], l[5], &score) || sp < INT32_MIN || sp > INT32_MAX ||
               tp < INT32_MIN || tp > INT32_MAX)
        why = PE_INT;
      else if (!parse_idt(p + a[6], l[6], &h)) why = PE_IDT;
      if (why != PE_OK && !all && e.type != PGX_SGRAPH_G) why = PE_OK, vk = wk = 0, label = 0, sp = tp = score = h = 0;   // (a line the script only counts the fields of)
      e.v_rid = (uint32_t)(vk >> 1), e.v_end = (uint8_t)(vk & 1), e.w_rid = (uint32_t)(wk >> 1), e.w_end = (uint8_t)(wk & 1);
      e.label_rid = label, e.sp = (int32_t)sp, e.tp = (int32_t)tp, e.score = score;
      // tenths, for the records pgx_sgraph_parse hands out: the exact decimal rounded half to even
      const int64_t ah = h < 0 ? -h : h, q = ah / 10, r = ah - q * 10, t = q + (r > 5 || (r == 5 && (q & 1)));
      e.idt_tenths = h < 0 ? -t : t;
    }
  }
  rec[k] = e, hund[k] = h, keep[k] = kept && why == PE_OK, code[k] = why;
  if (why != PE_OK) atomicMin(err, k);
}
__global__ void k_tl_compact(const Edge *__restrict__ rec, const int64_t *__restrict__ hund, const uint32_t *__restrict__ list, uint32_t n, uint32_t line_base,
                             Edge *__restrict__ rec_out, int64_t *__restrict__ hund_out, uint32_t *__restrict__ line_out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) rec_out[j] = rec[list[j]], hund_out[j] = hund[list[j]], line_out[j] = line_base + list[j];
}
// a device graph's records: hundredths from tenths, the line of record i is i
__global__ void k_tl_from_graph(const Edge *__restrict__ rec, uint32_t n, int64_t *__restrict__ hund, uint32_t *__restrict__ line) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) hund[i] = rec[i].idt_tenths * 10, line[i] = i;
}

// ---------------------------------------------------------------------------------------------------------
// the edge table: the G edges sorted by (v, w)
// ---------------------------------------------------------------------------------------------------------
// the script's assertion on a G edge: w ends in E when s < t, else in B
struct EndRule {
  __device__ bool operator()(const Edge &e) const { return (e.sp < e.tp) != ((e.w_end & 1u) == 1u); }
};
// the scores of n edges named by their two keys (the bundles' edges, all at once); found[i] = 0: the table lacks it
__global__ void k_tl_scores(const uint64_t *__restrict__ v, const uint64_t *__restrict__ w, uint32_t n, const uint64_t *__restrict__ sv, const uint64_t *__restrict__ sw,
                            const uint32_t *__restrict__ se, const uint32_t *__restrict__ gsel, uint32_t m, const Edge *__restrict__ edges, int64_t *__restrict__ score,
                            uint8_t *__restrict__ found) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t at = find_vw(sv, sw, m, v[i], w[i]);
  found[i] = at != NONE, score[i] = at != NONE ? edges[gsel[se[at]]].score : 0;
}

// ---------------------------------------------------------------------------------------------------------
// the unitig index: the (s, via, t) keys sorted, looked up by binary search; the dual-skip rule of ctg_paths
// ---------------------------------------------------------------------------------------------------------
// err[0] = min(err[0], the unitig whose key an earlier one has) (stable sorts: i is the later of the two)
__global__ void k_tl_u_dups(const uint64_t *__restrict__ ss, const uint64_t *__restrict__ sv, const uint64_t *__restrict__ st, const uint32_t *__restrict__ su, uint32_t n,
                            uint32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i && i < n && ss[i] == ss[i - 1] && sv[i] == sv[i - 1] && st[i] == st[i - 1]) atomicMin(err, su[i]);
}
// out[i] = the unitig with key (rs[i], rv[i], rt[i]), NONE: the index lacks it
__global__ void k_tl_u_find(const uint64_t *__restrict__ rs, const uint64_t *__restrict__ rv, const uint64_t *__restrict__ rt, uint32_t n_ref, const uint64_t *__restrict__ ss,
                            const uint64_t *__restrict__ sv, const uint64_t *__restrict__ st, const uint32_t *__restrict__ su, uint32_t n, uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ref) return;
  const uint64_t a = rs[i], b = rv[i], c = rt[i];
  const uint32_t lo = bisect(0, n, [&](uint32_t k) { return ss[k] < a || (ss[k] == a && (sv[k] < b || (sv[k] == b && st[k] < c))); });
  out[i] = lo < n && ss[lo] == a && sv[lo] == b && st[lo] == c ? su[lo] : NONE;
}
// the canonical key of a row: the smaller of K = (s0, t0) and its dual (rev t0, rev s0)
__global__ void k_tl_dual_keys(const uint64_t *__restrict__ s0, const uint64_t *__restrict__ t0, uint32_t n, uint64_t *__restrict__ c0, uint64_t *__restrict__ c1) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t a = s0[i], b = t0[i], da = b ^ 1u, db = a ^ 1u;
  const bool dual_first = da < a || (da == a && db < b);
  c0[i] = dual_first ? da : a, c1[i] = dual_first ? db : b;
}
// The rows sorted by canonical key (stable: a group's first entry is its first row in the file).  The key of that row wins: every row of
// the group with the winning key is kept, every row with the other is skipped; of a key that is its own dual only the first row is kept.
__global__ void k_tl_dual_keep(const uint64_t *__restrict__ sc0, const uint64_t *__restrict__ sc1, const uint32_t *__restrict__ order, const uint64_t *__restrict__ s0,
                               const uint64_t *__restrict__ t0, uint32_t n, uint8_t *__restrict__ keep) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t a = sc0[i], b = sc1[i];
  const uint32_t lo = find_vw(sc0, sc1, i + 1, a, b);   // the group's first entry (at i at the latest)
  const uint32_t winner = order[lo], row = order[i];
  const bool same = s0[row] == s0[winner] && t0[row] == t0[winner], self_dual = s0[row] == (t0[row] ^ 1u);
  keep[row] = same && (!self_dual || row == winner);
}

// ---------------------------------------------------------------------------------------------------------
// paths -> rows
// ---------------------------------------------------------------------------------------------------------
struct Segment {   // n nodes of the pool from `off` on, part of path `path`
  uint32_t off, n, path, pad;
};
struct alignas(16) RowInfo {   // what a line prints beside its pgx_tile_row
  int64_t score, hund;
  uint32_t label, dl, path, pad;
};
// A thread per row r: its path p by binary search of the paths' first rows, its two nodes -- slots r + p and r + p + 1 of the concatenated
// paths, a path of k nodes has k - 1 rows -- by binary search of the segments' offsets, its edge by binary search of the table.
// err[0] = min(err[0], r) where the table lacks the edge; err[1] counts indices out of range (never: they go into loads).
__global__ void k_tl_rows(const uint64_t *__restrict__ path_row0, const uint32_t *__restrict__ path_ctg, uint32_t n_path, const Segment *__restrict__ seg,
                          const uint64_t *__restrict__ node_off, uint32_t n_seg, const uint64_t *__restrict__ pool, uint64_t pool_n, const uint64_t *__restrict__ sv,
                          const uint64_t *__restrict__ sw, const uint32_t *__restrict__ se, const uint32_t *__restrict__ gsel, uint32_t m, const Edge *__restrict__ edges,
                          const int64_t *__restrict__ hund, uint32_t n_rows, pgx_tile_row *__restrict__ rows, RowInfo *__restrict__ info, uint32_t *__restrict__ dl, uint32_t *__restrict__ err) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const uint32_t p = last_le(path_row0, n_path, r);
  uint64_t key[2];
  bool ok = true;
  for (int k = 0; k < 2; ++k) {
    const uint64_t slot = (uint64_t)r + p + k;
    const uint32_t s = last_le(node_off, n_seg, slot);
    const uint64_t at = (uint64_t)seg[s].off + (slot - node_off[s]);
    ok &= slot - node_off[s] < seg[s].n && at < pool_n && seg[s].path == p;
    key[k] = ok ? pool[at] : 0;
  }
  pgx_tile_row row = {};
  RowInfo ri = {};
  uint32_t d = 0;
  if (!ok) {
    atomicAdd(&err[1], 1u);
  } else {
    const uint32_t at = find_vw(sv, sw, m, key[0], key[1]);
    if (at == NONE) {
      atomicMin(&err[0], r);
    } else {
      const uint32_t ei = gsel[se[at]];
      const Edge e = edges[ei];
      const int64_t diff = (int64_t)e.sp - (int64_t)e.tp;
      d = (uint32_t)(diff < 0 ? -diff : diff);
      row.ctg = path_ctg[p], row.rid0 = e.v_rid, row.rid1 = e.w_rid, row.s = e.sp, row.e = e.tp, row.strand0 = e.v_end & 1u ? 0 : 1, row.strand1 = e.w_end & 1u ? 0 : 1;
      ri.score = e.score, ri.hund = hund[ei], ri.label = e.label_rid, ri.dl = d, ri.path = p;
    }
  }
  rows[r] = row, info[r] = ri, dl[r] = d;
}

// ---------------------------------------------------------------------------------------------------------
// the text: '%s %s %s %s %d %d %d %0.2f %d %d\n' % (ctg_id, v, w, rid, s, t, aln_score, idt, ctg_length, |s - t|), a line per row
// ---------------------------------------------------------------------------------------------------------
// A piece is a line: the piece source of pgx_text.h's piece scheme, which lays the text out and formats it.
struct RowLines {
  const pgx_tile_row *__restrict__ rows;
  const RowInfo *__restrict__ info;
  const uint64_t *__restrict__ cum, *__restrict__ row0;
  const uint32_t *__restrict__ name_off;
  const char *__restrict__ names;
  uint32_t n;                            // rows
  static constexpr uint32_t MAX = 256;   // CTG_NAME_MAX + 2 names of <= 13 + a rid of <= 11 + 2 numbers of <= 11 + a score of <= 20 + an identity of <= 24 + a length
                                         // of <= 20 + a difference of <= 10 + 9 blanks + '\n' = 239
  template <bool WRITE>
  __device__ uint32_t piece(uint32_t r, char *dst) const {
    LineOut<WRITE> o{dst, 0};
    const pgx_tile_row row = rows[r];
    const RowInfo ri = info[r];
    const uint32_t a = name_off[ri.path], b = name_off[ri.path + 1];
    if (WRITE)
      for (uint32_t k = a; k < b; ++k) dst[k - a] = names[k];
    o.n = b - a;
    o.ch(' '), o.node(row.rid0, row.strand0 == 0), o.ch(' '), o.node(row.rid1, row.strand1 == 0), o.ch(' '), o.rid((int32_t)ri.label), o.ch(' ');
    o.i32(row.s), o.ch(' '), o.i32(row.e), o.ch(' '), o.i64(ri.score), o.ch(' ');
    const uint64_t ah = ri.hund < 0 ? 0ULL - (uint64_t)ri.hund : (uint64_t)ri.hund, whole = ah / 100u;
    if (ri.hund < 0) o.ch('-');
    o.u64(whole), o.ch('.'), o.u32((uint32_t)(ah - whole * 100u), 2), o.ch(' ');
    o.u64(cum[r] - cum[row0[ri.path]]), o.ch(' '), o.u32(ri.dl), o.ch('\n');
    return o.n;
  }
};

// ---------------------------------------------------------------------------------------------------------
// host: the parsed sg_edges_list on the device
// ---------------------------------------------------------------------------------------------------------
struct DevEdges {
  DevBuf<Edge> own;              // the records of a parsed file (a device graph's stay where they are)
  const Edge *rec = nullptr;
  DevBuf<int64_t> hund;          // identity in hundredths, record by record
  DevBuf<uint32_t> line;         // the 0-based line of the file a record came from
  uint32_t n = 0;
};
uint64_t piece_bytes() {
  uint64_t v = 1ULL << 30;
  if (const char *s = getenv("PGX_TILING_PIECE")) v = strtoull(s, nullptr, 10);
  return std::min<uint64_t>(std::max<uint64_t>(v, 2 * SG_LINE_MAX), 1ULL << 30);
}
struct Pinned {
  char *p = nullptr;
  ~Pinned() {
    if (p) (void)hipHostFree(p);
  }
};
struct File {
  FILE *f = nullptr;
  ~File() {
    if (f) fclose(f);
  }
};
struct Part {   // the records of one piece of the file
  DevBuf<Edge> rec;
  DevBuf<int64_t> hund;
  DevBuf<uint32_t> line;
  uint32_t n = 0, lines = 0;   // records; lines of the piece, the blank ones counted
};
struct PieceWs {   // what every piece is parsed through
  DevBuf<char> text;
  DevBuf<uint8_t> flag;
  DevBuf<uint32_t> cnt;   // [0] newlines of the piece, [1] its first refused line
  PrimWs tmp;
  explicit PieceWs(uint64_t cap) : text(cap), flag(cap), cnt(2) {}
};
// One piece: the `used` bytes at p, whole lines, with four bytes of room behind them.  Its newlines, a lane per line, the first refused
// line, the records of the kept lines.  line0, rec0: the lines and records of the pieces before it; meanwhile() runs on the host while
// the lanes tokenise.  all: see k_tl_tokenise.
template <class F>
Part parse_piece(const char *path, bool all, char *p, uint64_t used, uint64_t line0, uint64_t rec0, PieceWs &ws, F &&meanwhile) {
  hipStream_t st = ctx().stream;
  const uint32_t n = (uint32_t)used, n4 = (n + 3) / 4;
  char save[4];   // the last word's pad goes up as zeros; what stands there (the start of the next piece) comes back once the copy has run
  memcpy(save, p + used, 4), memset(p + used, 0, 4);
  PGX_HIP(hipMemcpyAsync(ws.text.p, p, (size_t)n4 * 4, hipMemcpyHostToDevice, st));
  PGX_HIP(hipMemsetAsync(ws.cnt.p, 0, sizeof(uint32_t), st));
  PGX_HIP(hipMemsetAsync(ws.cnt.p + 1, 0xFF, sizeof(uint32_t), st));
  LAUNCH(k_tl_newlines, n4, (const uint32_t *)ws.text.p, n4, (uint32_t *)ws.flag.p, ws.cnt.p);
  PGX_HIP(hipGetLastError());
  uint32_t nl = 0;
  ws.cnt.download(&nl, 1);
  pgx::sync();
  memcpy(p + used, save, 4);
  PGX_REQUIRE(line0 + nl < NONE, PGX_EINVAL, "%s: more than 2^32 - 2 lines", path);
  DevBuf<uint32_t> nlpos(nl), list(nl);
  DevBuf<Edge> rec(nl);
  DevBuf<int64_t> hund(nl);
  DevBuf<uint8_t> keep(nl), code(nl);
  const uint32_t got = select_indices(ws.flag.p, n, nlpos.p, &ws.tmp);
  PGX_REQUIRE(got == nl, PGX_EHIP, "pgx_tiling: %u newlines counted, %u selected (a bug)", nl, got);
  LAUNCH(k_tl_tokenise, nl, ws.text.p, nlpos.p, nl, all ? 1u : 0u, rec.p, hund.p, keep.p, code.p, ws.cnt.p + 1);
  PGX_HIP(hipGetLastError());
  meanwhile();
  uint32_t bad = NONE;
  PGX_HIP(hipMemcpyAsync(&bad, ws.cnt.p + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  pgx::sync();
  if (bad != NONE) {
    uint8_t why = PE_OK;
    PGX_HIP(hipMemcpyAsync(&why, code.p + bad, 1, hipMemcpyDeviceToHost, st));
    pgx::sync();
    PGX_REQUIRE(false, PGX_EINVAL, "%s: line %llu %s", path, (unsigned long long)(line0 + bad), PE_TEXT[why < 8 ? why : 0]);
  }
  Part part;
  part.lines = nl;
  part.n = select_indices(keep.p, nl, list.p, &ws.tmp);
  PGX_REQUIRE(rec0 + part.n <= (uint64_t)INT32_MAX, PGX_EINVAL, "%s: more than 2^31 - 1 edge lines", path);
  part.rec.alloc(part.n), part.hund.alloc(part.n), part.line.alloc(part.n);
  if (part.n) LAUNCH(k_tl_compact, part.n, rec.p, hund.p, list.p, part.n, (uint32_t)line0, part.rec.p, part.hund.p, part.line.p);
  PGX_HIP(hipGetLastError());
  return part;
}
// the parts one behind the other (a single part as it is)
void concat_parts(std::vector<Part> &parts, uint64_t records, DevEdges &out) {
  hipStream_t st = ctx().stream;
  out.n = (uint32_t)records;
  if (parts.size() == 1) {
    out.own = std::move(parts[0].rec), out.hund = std::move(parts[0].hund), out.line = std::move(parts[0].line);
  } else {
    out.own.alloc(records), out.hund.alloc(records), out.line.alloc(records);
    uint64_t at = 0;
    for (Part &p : parts) {
      if (p.n) {
        PGX_HIP(hipMemcpyAsync(out.own.p + at, p.rec.p, (size_t)p.n * sizeof(Edge), hipMemcpyDeviceToDevice, st));
        PGX_HIP(hipMemcpyAsync(out.hund.p + at, p.hund.p, (size_t)p.n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        PGX_HIP(hipMemcpyAsync(out.line.p + at, p.line.p, (size_t)p.n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
      }
      at += p.n;
      p.rec.release(), p.hund.release(), p.line.release();   // (stream-ordered: the copies come first)
    }
  }
  out.rec = out.own.p;
}
// The file in pieces of piece_bytes(): each is cut at its last newline (what follows it opens the next piece), uploaded, and parsed; the
// next piece is read while the lanes tokenise this one.  all: see k_tl_tokenise.
void parse_sg_file(const char *path, bool all, DevEdges &out) {
  File in;
  in.f = fopen(path, "rb");
  PGX_REQUIRE(in.f, PGX_EINVAL, "%s: cannot be opened", path);
  long end_at = -1;
  if (fseek(in.f, 0, SEEK_END) == 0) end_at = ftell(in.f);
  PGX_REQUIRE(end_at >= 0 && fseek(in.f, 0, SEEK_SET) == 0, PGX_EINVAL, "%s: not a file whose size can be told (a pipe?)", path);
  const uint64_t size = (uint64_t)end_at;
  const uint64_t piece = std::max<uint64_t>(std::min<uint64_t>(piece_bytes(), size + 1), 2 * SG_LINE_MAX), cap = SG_LINE_MAX + 1 + piece + 8;   // (size + 1: a small file is one short read)
  Pinned pin[2];
  for (int k = 0; k < 2; ++k) PGX_HIP(hipHostMalloc((void **)&pin[k].p, cap, hipHostMallocDefault));
  PieceWs ws(cap);
  std::vector<Part> parts;
  uint64_t lines = 0, records = 0;
  // fill(b, carry): the next piece behind the `carry` bytes already at the start of pin[b]; returns the bytes up to and with the last
  // newline (0: the end of the file) and leaves in *rest what follows them
  bool eof = false;
  // line0: the line the piece starts with.  An unfinished line of more than SG_LINE_MAX bytes at the piece's end is not refused here but
  // left to the caller (*too_long), who first reports what the piece before it holds
  auto fill = [&](int b, uint64_t carry, uint64_t *rest, uint64_t *too_long) -> uint64_t {
    *too_long = NONE;
    *rest = 0;
    if (eof) return 0;
    uint64_t have = carry + fread(pin[b].p + carry, 1, piece, in.f);
    PGX_REQUIRE(!ferror(in.f), PGX_EINVAL, "%s: read error", path);
    if (have < carry + piece) {
      eof = true;
      if (have && pin[b].p[have - 1] != '\n') pin[b].p[have++] = '\n';   // (a last line without a newline)
      return have;
    }
    const char *nl = (const char *)memrchr(pin[b].p, '\n', have);
    const uint64_t used = nl ? (uint64_t)(nl - pin[b].p) + 1 : 0;
    *rest = have - used;
    if (*rest > SG_LINE_MAX) *too_long = (uint64_t)std::count(pin[b].p, pin[b].p + used, '\n');   // (used == 0 included: piece >= 2 * SG_LINE_MAX)
    return used;
  };
  int b = 0;
  uint64_t rest = 0, too_long = NONE, used = fill(b, 0, &rest, &too_long);
  auto refuse_long = [&](uint64_t at) { PGX_REQUIRE(false, PGX_EINVAL, "%s: line %llu %s", path, (unsigned long long)at, PE_TEXT[PE_LONG]); };
  if (too_long != NONE && used == 0) refuse_long(too_long);
  while (used) {
    const uint64_t this_long = too_long;   // (of THIS piece's tail: lines + this_long is its line)
    uint64_t next_used = 0, next_rest = 0, next_long = NONE;
    Part part = parse_piece(path, all, pin[b].p, used, lines, records, ws, [&] {   // the next piece, while the lanes work
      memmove(pin[b ^ 1].p, pin[b].p + used, rest);
      if (this_long == NONE) next_used = fill(b ^ 1, rest, &next_rest, &next_long);   // (else nothing more is read)
    });
    if (this_long != NONE) refuse_long(lines + this_long);
    lines += part.lines, records += part.n;
    parts.push_back(std::move(part));
    b ^= 1, used = next_used, rest = next_rest, too_long = next_long;
    if (too_long != NONE && used == 0) refuse_long(lines + too_long);
  }
  concat_parts(parts, records, out);
  pgx::sync();   // the pinned buffers go
}

// ---------------------------------------------------------------------------------------------------------
// host: the edge table
// ---------------------------------------------------------------------------------------------------------
typedef GEdges EdgeTable;   // of pgx_gedges.h, what is left of it: by_vw (sv, sw, out_e) and gsel
uint32_t line_of(const DevEdges &e, uint32_t rec) {
  uint32_t l = 0;
  PGX_HIP(hipMemcpyAsync(&l, e.line.p + rec, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx().stream));
  pgx::sync();
  return l;
}
// the G edges' by_vw of pgx_gedges.h with its duplicate check, under the script's assertion
void build_table(const DevEdges &e, const char *sg_name, EdgeTable &t) {
  hipStream_t st = ctx().stream;
  PrimWs tmp;
  if (e.n == 0) return;
  t.select(e.rec, e.n, &tmp);
  if (t.m == 0) return;
  DevBuf<uint32_t> err(2);
  PGX_HIP(hipMemsetAsync(err.p, 0xFF, 2 * sizeof(uint32_t), st));
  t.keys(EndRule{}, err.p);
  t.by_w(&tmp);
  t.by_vw(err.p + 1, &tmp);
  PGX_HIP(hipGetLastError());
  t.vk.release(), t.wk.release(), t.ids.release(), t.swk.release(), t.in_e.release();
  uint32_t h[2];
  err.download(h, 2);
  pgx::sync();
  PGX_REQUIRE(h[0] == NONE, PGX_EINVAL, "%s: line %u: a G edge whose w does not end in E for s < t, or in B otherwise (the script asserts it)", sg_name, line_of(e, h[0]));
  PGX_REQUIRE(h[1] == NONE, PGX_EINVAL, "%s: line %u repeats the (v, w) of an earlier G line (the script would keep the later one; its own files never do)", sg_name,
              line_of(e, h[1]));
}

// ---------------------------------------------------------------------------------------------------------
// host: utg_data, ctg_paths, the bundles
// ---------------------------------------------------------------------------------------------------------
struct Tok {
  const char *p;
  uint32_t n;
};
// the lines of a text, each as its first up to 8 fields
struct Lines {
  const char *p, *end;
  uint64_t line = (uint64_t)-1;
  Tok f[8];
  uint32_t nf = 0;
  Lines(const char *text, size_t n) : p(text), end(text + n) {}
  bool next() {
    if (p >= end) return false;
    ++line;
    const char *e = (const char *)memchr(p, '\n', (size_t)(end - p));
    const char *stop = e ? e : end;
    nf = 0;
    const char *q = p;
    while (true) {
      while (q < stop && is_blank((unsigned char)*q)) ++q;
      if (q >= stop) break;
      const char *a = q;
      while (q < stop && !is_blank((unsigned char)*q)) ++q;
      if (nf < 8) f[nf] = Tok{a, (uint32_t)(q - a)};
      ++nf;
    }
    p = e ? e + 1 : end;
    return true;
  }
};
bool tok_is(const Tok &t, const char *s) { return t.n == strlen(s) && memcmp(t.p, s, t.n) == 0; }
// the next piece of t up to `sep` (which is skipped); false: t is used up
bool split(Tok &t, char sep, Tok *piece, bool *started) {
  if (*started && t.p == nullptr) return false;
  *started = true;
  const char *e = (const char *)memchr(t.p, sep, t.n);
  if (e) {
    *piece = Tok{t.p, (uint32_t)(e - t.p)};
    t.n -= (uint32_t)(e - t.p) + 1, t.p = e + 1;
  } else {
    *piece = t, t.p = nullptr, t.n = 0;
  }
  return true;
}
struct Key3 {
  uint64_t s, v, t;
  bool operator==(const Key3 &o) const { return s == o.s && v == o.v && t == o.t; }
};
// "s~v~t" (v may be NA)
bool parse_key3(Tok t, Key3 *k) {
  Tok part[3];
  bool started = false;
  for (int i = 0; i < 3; ++i)
    if (!split(t, '~', &part[i], &started)) return false;
  Tok more;
  if (split(t, '~', &more, &started)) return false;
  if (!parse_node(part[0].p, part[0].n, &k->s) || !parse_node(part[2].p, part[2].n, &k->t)) return false;
  if (tok_is(part[1], "NA")) k->v = VIA_NA;
  else if (!parse_node(part[1].p, part[1].n, &k->v)) return false;
  return true;
}
enum : uint8_t { UT_SIMPLE = 0, UT_CONTAINED = 1, UT_COMPOUND = 2 };
struct Utg {
  Key3 key;
  uint8_t type;
  bool bad;       // its path does not parse: an error once something names it
  uint64_t line;
  uint64_t off;   // simple, contained: its nodes pool[off, off + n); compound: its sub-unitigs subs[off, off + n)
  uint32_t n;
};
struct Alt {
  int64_t weight;
  std::vector<uint64_t> path;
};
void node_name(uint64_t key, char *buf) { snprintf(buf, 16, "%09d:%c", (int32_t)(uint32_t)(key >> 1), key & 1 ? 'E' : 'B'); }
// do the names of a compare above those of b, as Python compares lists of strings
bool names_above(const std::vector<uint64_t> &a, const std::vector<uint64_t> &b) {
  for (size_t i = 0; i < a.size() && i < b.size(); ++i)
    if (a[i] != b[i]) {
      char x[16], y[16];
      node_name(a[i], x), node_name(b[i], y);
      return strcmp(x, y) > 0;
    }
  return a.size() > b.size();
}
// a bundle's digraph: nodes and neighbours in order of first insertion, an edge seen twice is one edge
struct Bundle {
  struct E {
    uint32_t to;
    int64_t w;
    bool gone;
  };
  std::unordered_map<uint64_t, uint32_t> id;
  std::vector<uint64_t> key;
  std::vector<std::vector<E>> adj;
  uint32_t node(uint64_t k) {
    auto it = id.find(k);
    if (it != id.end()) return it->second;
    id.emplace(k, (uint32_t)key.size()), key.push_back(k), adj.emplace_back();
    return (uint32_t)key.size() - 1;
  }
  void add_edge(uint64_t a, uint64_t b, int64_t w) {
    const uint32_t u = node(a), v = node(b);
    for (const E &e : adj[u])
      if (e.to == v) return;
    adj[u].push_back(E{v, w, false});
  }
  // forward Dijkstra from s: priority (distance, push sequence), a predecessor changes only on a strictly smaller distance, the search
  // stops when t is popped.  false: no path.  *tie: more than one path of the minimum weight exists (path counting over tight edges)
  bool search(uint32_t s, uint32_t t, Alt *out, bool *tie) const {
    const size_t n = key.size();
    const int64_t INF = INT64_MAX;
    std::vector<int64_t> dist(n, INF);
    std::vector<uint32_t> pred(n, NONE), order;
    std::vector<uint8_t> done(n, 0);
    typedef std::tuple<int64_t, uint64_t, uint32_t> Item;
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> pq;
    uint64_t seq = 0;
    dist[s] = 0, pq.emplace(0, seq++, s);
    while (!pq.empty()) {
      const Item it = pq.top();
      pq.pop();
      const uint32_t u = std::get<2>(it);
      if (done[u]) continue;
      done[u] = 1, order.push_back(u);
      if (u == t) break;
      for (const E &e : adj[u]) {
        if (e.gone) continue;
        const int64_t nd = dist[u] + e.w;
        if (nd < dist[e.to]) dist[e.to] = nd, pred[e.to] = u, pq.emplace(nd, seq++, e.to);
      }
    }
    if (!done[t]) return false;
    // paths of the minimum weight, counted up to 2: the nodes in the order they were popped are in ascending distance, and a tight edge
    // goes from a smaller distance to a larger one (weights > 0)
    std::vector<uint8_t> cnt(n, 0);
    cnt[s] = 1;
    for (uint32_t u : order) {
      if (u == t) break;
      for (const E &e : adj[u])
        if (!e.gone && done[e.to] && dist[u] + e.w == dist[e.to]) cnt[e.to] = (uint8_t)std::min(2, cnt[e.to] + cnt[u]);
    }
    *tie = cnt[t] > 1;
    out->weight = dist[t];
    out->path.clear();
    for (uint32_t u = t; u != NONE; u = pred[u]) out->path.push_back(key[u]);
    std::reverse(out->path.begin(), out->path.end());
    return true;
  }
  void remove_path(const std::vector<uint64_t> &path) {
    for (size_t i = 0; i + 1 < path.size(); ++i) {
      const uint32_t u = id[path[i]], v = id[path[i + 1]];
      for (E &e : adj[u])
        if (e.to == v) e.gone = true;
    }
  }
};

// one set of paths (the primary file's, or the alternate file's) as the device takes it
struct PathSet {
  std::vector<Segment> seg;
  std::vector<uint64_t> row0;       // paths + 1: the first row of every path
  std::vector<uint32_t> ctg;        // the contig number of every path: names in order of first appearance
  std::vector<uint64_t> src_line;   // the line of ctg_paths a path came from
  std::vector<uint32_t> name_off;   // paths + 1
  std::string names;                // the paths' names, one after the other
  std::vector<std::string> distinct;
  std::unordered_map<std::string, uint32_t> number;
  uint64_t nodes = 0;
  PathSet() : row0(1, 0), name_off(1, 0) {}
  void open(const std::string &name, uint64_t line) {
    auto it = number.find(name);
    if (it == number.end()) it = number.emplace(name, (uint32_t)distinct.size()).first, distinct.push_back(name);
    ctg.push_back(it->second), src_line.push_back(line), names += name, name_off.push_back((uint32_t)names.size());
  }
  void add(uint64_t off, uint64_t n) { seg.push_back(Segment{(uint32_t)off, (uint32_t)n, (uint32_t)ctg.size() - 1, 0}), nodes += n; }
  void close() { row0.push_back(nodes - ctg.size()); }   // (every path has two nodes at least)
  uint32_t paths() const { return (uint32_t)ctg.size(); }
};
}  // namespace
}  // namespace pgx

using namespace pgx;

struct pgx_tiling {
  struct Set {
    DevBuf<pgx_tile_row> rows;
    DevBuf<RowInfo> info;
    DevBuf<uint64_t> cum, row0;   // rows + 1: running |s - t|; paths + 1: the first row of each path
    DevBuf<uint32_t> name_off;
    DevBuf<char> names;
    std::string distinct;   // the contigs' names, a line each
    std::vector<std::string> ctg_names;
    TextPlan text;                // a line per row
    uint64_t n_rows = 0, n_ctg = 0;
    RowLines lines() const { return RowLines{rows.p, info.p, cum.p, row0.p, name_off.p, names.p, (uint32_t)n_rows}; }
  } set[2];
  pgx_tiling_stats_t st = {};
  TextStage stage;
  bool shut = false;
  void drop_device_state() {
    for (Set &s : set) s.rows.release(), s.info.release(), s.cum.release(), s.text.release(), s.row0.release(), s.name_off.release(), s.names.release();
    stage.drop();
  }
};

namespace pgx {
namespace {
LiveSet<pgx_tiling> g_tl;
ShutdownHook g_tl_hook([] { g_tl.shutdown(); });

// the rows and line offsets of one path set
void build_set(const PathSet &ps, const DevBuf<uint64_t> &d_pool, uint64_t pool_n, const DevEdges &e, const EdgeTable &t, const std::vector<uint64_t> &pool,
               const char *ctg_name, pgx_tiling::Set &out) {
  hipStream_t st = ctx().stream;
  PrimWs tmp;
  for (const std::string &nm : ps.distinct) out.distinct += nm, out.distinct += '\n';
  out.ctg_names = ps.distinct;
  out.n_ctg = ps.distinct.size();
  const uint32_t n_path = ps.paths(), n_seg = (uint32_t)ps.seg.size();
  const uint64_t n_rows = ps.nodes - n_path;
  PGX_REQUIRE(n_rows <= (uint64_t)INT32_MAX && ps.names.size() < NONE, PGX_EINVAL, "%s: more than 2^31 - 1 rows of tiling path", ctg_name);
  out.n_rows = n_rows;
  if (n_rows == 0) return;
  DevBuf<Segment> seg(n_seg);
  DevBuf<uint32_t> seg_n(n_seg), path_ctg(n_path), dl(n_rows), err(2);
  DevBuf<uint64_t> node_off((size_t)n_seg + 1);
  out.row0.alloc((size_t)n_path + 1), out.name_off.alloc((size_t)n_path + 1), out.names.alloc(ps.names.size() + 1);
  out.rows.alloc(n_rows), out.info.alloc(n_rows), out.cum.alloc(n_rows + 1);
  std::vector<uint32_t> h_seg_n(n_seg);
  for (uint32_t i = 0; i < n_seg; ++i) h_seg_n[i] = ps.seg[i].n;
  seg.upload(ps.seg.data(), n_seg), seg_n.upload(h_seg_n.data(), n_seg), path_ctg.upload(ps.ctg.data(), n_path);
  out.row0.upload(ps.row0.data(), (size_t)n_path + 1), out.name_off.upload(ps.name_off.data(), (size_t)n_path + 1), out.names.upload(ps.names.data(), ps.names.size());
  PGX_HIP(hipMemsetAsync(err.p, 0xFF, sizeof(uint32_t), st));
  PGX_HIP(hipMemsetAsync(err.p + 1, 0, sizeof(uint32_t), st));
  const uint64_t nodes = scan_to_total(seg_n.p, node_off.p, n_seg, &tmp);   // (synchronises: the host vectors above are read)
  PGX_REQUIRE(nodes == ps.nodes, PGX_EHIP, "pgx_tiling: the segments hold %llu of %llu nodes (a bug)", (unsigned long long)nodes, (unsigned long long)ps.nodes);
  LAUNCH(k_tl_rows, n_rows, out.row0.p, path_ctg.p, n_path, seg.p, node_off.p, n_seg, d_pool.p, pool_n, t.sv.p, t.sw.p, t.out_e.p, t.gsel.p, t.m, e.rec, e.hund.p, (uint32_t)n_rows,
         out.rows.p, out.info.p, dl.p, err.p);
  PGX_HIP(hipGetLastError());
  uint32_t h[2];
  err.download(h, 2);
  pgx::sync();
  PGX_REQUIRE(h[1] == 0, PGX_EHIP, "pgx_tiling: %u rows found no place in a path (a bug)", h[1]);
  if (h[0] != NONE) {   // the first row whose edge the table lacks: its path, and its nodes from the host's copy of the pool
    const uint32_t p = (uint32_t)(std::upper_bound(ps.row0.begin(), ps.row0.begin() + n_path, (uint64_t)h[0]) - ps.row0.begin()) - 1;
    auto node_at = [&](uint64_t slot) -> uint64_t {
      uint64_t acc = 0;
      for (const Segment &s : ps.seg) {
        if (slot < acc + s.n) return pool[s.off + (slot - acc)];
        acc += s.n;
      }
      return 0;
    };
    const uint64_t key[2] = {node_at((uint64_t)h[0] + p), node_at((uint64_t)h[0] + p + 1)};
    char a[16], b[16];
    node_name(key[0], a), node_name(key[1], b);
    PGX_REQUIRE(false, PGX_EINVAL, "%s: line %llu: the edge %s %s of its path is not a G edge of the edge table", ctg_name, (unsigned long long)ps.src_line[p], a, b);
  }
  (void)scan_to_total(dl.p, out.cum.p, n_rows, &tmp);
  plan_text(out.lines(), (const uint32_t *)nullptr, n_rows, &out.text, &tmp);   // (no first pieces: a piece per line)
}

struct Inputs {
  const char *sg_fn;
  pgx_sgraph *g;
  const char *utg, *ctg;
  size_t utg_len, ctg_len;
  const char *utg_name, *ctg_name;
};
struct UtgData {   // utg_data, tokenised
  std::vector<uint64_t> pool;   // the nodes of the simple and contained unitigs' paths; the alternates join it later
  std::vector<Key3> subs;       // the sub-unitigs the compound lines name
  std::vector<Utg> utgs;
};
struct CtgRow {
  uint64_t line;
  std::string name;
  uint32_t ref0, n_ref;        // its unitigs: refs[ref0, ref0 + n_ref)
  const char *defect;          // why the row is refused if it is kept
};
struct CtgRows {   // ctg_paths, tokenised
  std::vector<CtgRow> rows;
  std::vector<uint64_t> s0, t0;   // every row's key
  std::vector<Key3> refs;         // the unitigs the rows name
};
struct KeptRow {
  uint64_t line;
  std::string name;
  std::vector<uint32_t> utg;
};

// ---- the edge records: a file, or a live graph's
void edge_records(const Inputs &in, DevEdges &e) {
  hipStream_t st = ctx().stream;
  if (in.sg_fn) {
    parse_sg_file(in.sg_fn, false, e);
    return;
  }
  uint64_t n = 0;
  e.rec = sgraph_device_edges(in.g, "pgx_tiling_build", &n);
  PGX_REQUIRE(n <= (uint64_t)INT32_MAX, PGX_EINVAL, "pgx_tiling_build: %llu edge records, more than 2^31 - 1", (unsigned long long)n);
  e.n = (uint32_t)n, e.hund.alloc(n), e.line.alloc(n);
  if (n) LAUNCH(k_tl_from_graph, n, e.rec, e.n, e.hund.p, e.line.p);
  PGX_HIP(hipGetLastError());
}

// ---- utg_data: the pool, the subs and the unitigs
void read_utg_data(const Inputs &in, pgx_tiling_stats_t &S, UtgData &U) {
  for (Lines ln(in.utg, in.utg_len); ln.next();) {
    if (ln.nf == 0) continue;
    PGX_REQUIRE(ln.nf == 7, PGX_EINVAL, "%s: line %llu does not have 7 fields", in.utg_name, (unsigned long long)ln.line);
    Utg u{};
    if (tok_is(ln.f[3], "simple")) u.type = UT_SIMPLE, ++S.utg_simple;
    else if (tok_is(ln.f[3], "contained")) u.type = UT_CONTAINED, ++S.utg_contained;
    else if (tok_is(ln.f[3], "compound")) u.type = UT_COMPOUND, ++S.utg_compound;
    else continue;
    Key3 k;
    int64_t number;
    const bool key_ok = parse_node(ln.f[0].p, ln.f[0].n, &k.s) && parse_node(ln.f[2].p, ln.f[2].n, &k.t) &&
                        (tok_is(ln.f[1], "NA") ? (k.v = VIA_NA, true) : parse_node(ln.f[1].p, ln.f[1].n, &k.v));
    PGX_REQUIRE(key_ok, PGX_EINVAL, "%s: line %llu: s, via or t is not a node name ('%%09d:B' or '%%09d:E' of a read id below 2^31; via may be NA)", in.utg_name,
                (unsigned long long)ln.line);
    PGX_REQUIRE(parse_int(ln.f[4].p, ln.f[4].n, &number) && parse_int(ln.f[5].p, ln.f[5].n, &number), PGX_EINVAL, "%s: line %llu: length or score is not a decimal integer",
                in.utg_name, (unsigned long long)ln.line);
    u.line = ln.line, u.key = k;
    Tok path = ln.f[6], piece;
    bool started = false;
    if (u.type == UT_COMPOUND) {
      u.off = U.subs.size();
      while (split(path, '|', &piece, &started)) {
        Key3 sk;
        if (!parse_key3(piece, &sk)) u.bad = true;
        else U.subs.push_back(sk);
      }
      u.n = (uint32_t)(U.subs.size() - u.off);
    } else {
      u.off = U.pool.size();
      while (split(path, '~', &piece, &started)) {
        uint64_t key;
        if (!parse_node(piece.p, piece.n, &key)) u.bad = true;
        else U.pool.push_back(key);
      }
      u.n = (uint32_t)(U.pool.size() - u.off);
    }
    U.utgs.push_back(u);
  }
  PGX_REQUIRE(U.utgs.size() <= (size_t)INT32_MAX && U.subs.size() <= (size_t)INT32_MAX, PGX_EINVAL, "%s: more than 2^31 - 1 unitigs", in.utg_name);
}

// ---- ctg_paths, tokenised: every row's key and the unitigs it names; what the script reads of a kept row only is noted, not refused yet
void read_ctg_paths(const Inputs &in, size_t n_subs, CtgRows &C) {
  for (Lines ln(in.ctg, in.ctg_len); ln.next();) {
    if (ln.nf == 0) continue;
    PGX_REQUIRE(ln.nf == 7, PGX_EINVAL, "%s: line %llu does not have 7 fields", in.ctg_name, (unsigned long long)ln.line);
    Tok iu = ln.f[2], first;
    bool started = false;
    (void)split(iu, '~', &first, &started);
    uint64_t s0, t0;
    PGX_REQUIRE(parse_node(first.p, first.n, &s0) && parse_node(ln.f[3].p, ln.f[3].n, &t0), PGX_EINVAL,
                "%s: line %llu: the first node of i_utig or t0 is not a node name ('%%09d:B' or '%%09d:E' of a read id below 2^31)", in.ctg_name, (unsigned long long)ln.line);
    CtgRow row{ln.line, std::string(ln.f[0].p, ln.f[0].n), (uint32_t)C.refs.size(), 0, nullptr};
    int64_t number;
    if (!parse_int(ln.f[4].p, ln.f[4].n, &number)) row.defect = "length is not a decimal integer";
    else if (ln.f[0].n > CTG_NAME_MAX - 7) row.defect = "a contig name of more than 89 bytes";
    Tok list = ln.f[6], piece;
    started = false;
    while (!row.defect && split(list, '|', &piece, &started)) {
      Key3 k;
      if (!parse_key3(piece, &k)) row.defect = "a unitig that is not s~via~t of node names";
      else C.refs.push_back(k);
    }
    row.n_ref = (uint32_t)C.refs.size() - row.ref0;
    C.rows.push_back(std::move(row)), C.s0.push_back(s0), C.t0.push_back(t0);
  }
  PGX_REQUIRE(C.rows.size() <= (size_t)INT32_MAX && C.refs.size() + n_subs <= (size_t)INT32_MAX, PGX_EINVAL, "%s: more than 2^31 - 1 rows or unitig names", in.ctg_name);
}

// ---- the dual rule on the device: the rows sorted by canonical key, the group's first row wins.  keep[r]: row r is kept
std::vector<uint8_t> dual_rule(const CtgRows &C) {
  hipStream_t st = ctx().stream;
  const uint32_t n_row = (uint32_t)C.rows.size();
  std::vector<uint8_t> keep(n_row, 0);
  if (n_row == 0) return keep;
  PrimWs tmp;
  DevBuf<uint64_t> s0(n_row), t0(n_row), c0(n_row), c1(n_row), sc0(n_row), sc1(n_row);
  DevBuf<uint32_t> order(n_row);
  DevBuf<uint8_t> d_keep(n_row);
  s0.upload(C.s0.data(), n_row), t0.upload(C.t0.data(), n_row);
  LAUNCH(k_tl_dual_keys, n_row, s0.p, t0.p, n_row, c0.p, c1.p);
  sort_order({{c0.p, 33}, {c1.p, 33}}, n_row, nullptr, order.p, sc0.p, &tmp);
  gather(c1.p, order.p, n_row, sc1.p, &tmp);
  LAUNCH(k_tl_dual_keep, n_row, sc0.p, sc1.p, order.p, s0.p, t0.p, n_row, d_keep.p);
  PGX_HIP(hipGetLastError());
  d_keep.download(keep.data(), n_row);
  pgx::sync();
  return keep;
}

// ---- the unitig index on the device (the three keys in one stable order, duplicates refused) and one binary search per name: the rows'
// unitigs, then the compound lines' sub-unitigs, in one launch.  found[i]: the unitig of name i, NONE: the index lacks it
std::vector<uint32_t> find_unitigs(const Inputs &in, const UtgData &U, const CtgRows &C) {
  hipStream_t st = ctx().stream;
  const uint32_t n_u = (uint32_t)U.utgs.size(), n_find = (uint32_t)(C.refs.size() + U.subs.size());
  std::vector<uint32_t> found(n_find, NONE);
  if (n_u == 0) return found;
  PrimWs tmp;
  std::vector<uint64_t> h[3];
  for (const Utg &u : U.utgs) h[0].push_back(u.key.s), h[1].push_back(u.key.v), h[2].push_back(u.key.t);
  DevBuf<uint64_t> ks(n_u), kv(n_u), kt(n_u), ss(n_u), sv(n_u), st_(n_u);
  DevBuf<uint32_t> su(n_u), err(1);
  ks.upload(h[0].data(), n_u), kv.upload(h[1].data(), n_u), kt.upload(h[2].data(), n_u);
  PGX_HIP(hipMemsetAsync(err.p, 0xFF, sizeof(uint32_t), st));
  sort_order({{ks.p, 33}, {kv.p, 64}, {kt.p, 33}}, n_u, nullptr, su.p, ss.p, &tmp);   // (64: via may be VIA_NA)
  gather(kv.p, su.p, n_u, sv.p, &tmp);
  gather(kt.p, su.p, n_u, st_.p, &tmp);
  LAUNCH(k_tl_u_dups, n_u, ss.p, sv.p, st_.p, su.p, n_u, err.p);
  PGX_HIP(hipGetLastError());
  uint32_t dup = NONE;
  err.download(&dup, 1);
  pgx::sync();   // (also: the host vectors above are read)
  PGX_REQUIRE(dup == NONE, PGX_EINVAL, "%s: line %llu repeats the (s, via, t) of an earlier line (the script would keep the later one; its own files never do)", in.utg_name,
              (unsigned long long)U.utgs[dup < n_u ? dup : 0].line);
  if (n_find == 0) return found;
  for (int k = 0; k < 3; ++k) h[k].clear();
  for (const std::vector<Key3> *list : {&C.refs, &U.subs})
    for (const Key3 &k : *list) h[0].push_back(k.s), h[1].push_back(k.v), h[2].push_back(k.t);
  DevBuf<uint64_t> rs(n_find), rv(n_find), rt(n_find);
  DevBuf<uint32_t> out_u(n_find);
  rs.upload(h[0].data(), n_find), rv.upload(h[1].data(), n_find), rt.upload(h[2].data(), n_find);
  LAUNCH(k_tl_u_find, n_find, rs.p, rv.p, rt.p, n_find, ss.p, sv.p, st_.p, su.p, n_u, out_u.p);
  PGX_HIP(hipGetLastError());
  out_u.download(found.data(), n_find);
  pgx::sync();
  return found;
}

// ---- the kept rows in file order: what the script would raise on, and the compound unitigs in use (bundles; bundle_of: per unitig, its
// number among them)
std::vector<KeptRow> kept_rows(const Inputs &in, pgx_tiling_stats_t &S, const UtgData &U, CtgRows &C, const std::vector<uint8_t> &keep, const uint32_t *ref_utg,
                               std::vector<uint32_t> &bundle_of, std::vector<uint32_t> &bundles) {
  const uint32_t n_u = (uint32_t)U.utgs.size();
  std::vector<KeptRow> kept;
  bundle_of.assign(n_u, NONE);
  for (size_t r = 0; r < C.rows.size(); ++r) {
    CtgRow &row = C.rows[r];
    if (!keep[r]) {
      ++S.ctg_skipped;
      continue;
    }
    PGX_REQUIRE(!row.defect, PGX_EINVAL, "%s: line %llu: %s", in.ctg_name, (unsigned long long)row.line, row.defect);
    KeptRow k{row.line, std::move(row.name), {}};
    for (uint32_t j = row.ref0; j < row.ref0 + row.n_ref; ++j) {
      const uint32_t ui = ref_utg[j];
      PGX_REQUIRE(ui < n_u, PGX_EINVAL, "%s: line %llu names a unitig that %s lacks (as simple, contained or compound)", in.ctg_name, (unsigned long long)row.line, in.utg_name);
      const Utg &u = U.utgs[ui];
      PGX_REQUIRE(!u.bad, PGX_EINVAL, "%s: line %llu names the unitig of %s line %llu, whose path does not parse", in.ctg_name, (unsigned long long)row.line, in.utg_name,
                  (unsigned long long)u.line);
      if (u.type == UT_COMPOUND && bundle_of[ui] == NONE) bundle_of[ui] = (uint32_t)bundles.size(), bundles.push_back(ui);
      k.utg.push_back(ui);
    }
    kept.push_back(std::move(k));
  }
  return kept;
}

// ---- the bundles: every edge of every sub-unitig of the compound unitigs in use, their scores in one lookup; then the rounds: a bundle's
// shortest paths one after the other, each removed before the next, sorted as the script sorts them
std::vector<std::vector<Alt>> bundle_alts(const Inputs &in, pgx_tiling_stats_t &S, const UtgData &U, const uint32_t *sub_utg, const std::vector<uint32_t> &bundles,
                                          const DevEdges &e, const EdgeTable &t) {
  hipStream_t st = ctx().stream;
  std::vector<uint64_t> ev, ew;
  const uint32_t n_u = (uint32_t)U.utgs.size();
  for (uint32_t ui : bundles) {
    const Utg &u = U.utgs[ui];
    for (uint32_t j = 0; j < u.n; ++j) {
      PGX_REQUIRE(sub_utg[u.off + j] < n_u, PGX_EINVAL, "%s: line %llu names a sub-unitig that the file lacks (as simple, contained or compound)", in.utg_name,
                  (unsigned long long)u.line);
      const Utg &sub = U.utgs[sub_utg[u.off + j]];
      PGX_REQUIRE(sub.type != UT_COMPOUND, PGX_EINVAL, "%s: line %llu: a sub-unitig (line %llu) is itself compound", in.utg_name, (unsigned long long)u.line,
                  (unsigned long long)sub.line);
      PGX_REQUIRE(!sub.bad, PGX_EINVAL, "%s: line %llu names the sub-unitig of line %llu, whose path does not parse", in.utg_name, (unsigned long long)u.line,
                  (unsigned long long)sub.line);
      for (uint32_t k = 0; k + 1 < sub.n; ++k) ev.push_back(U.pool[sub.off + k]), ew.push_back(U.pool[sub.off + k + 1]);
    }
  }
  const size_t ne = ev.size();
  PGX_REQUIRE(ne <= (size_t)INT32_MAX, PGX_EINVAL, "%s: more than 2^31 - 1 edges in compound unitigs", in.utg_name);
  std::vector<int64_t> score(ne);
  std::vector<uint8_t> found(ne);
  if (ne) {
    DevBuf<uint64_t> dv(ne), dw(ne);
    DevBuf<int64_t> ds(ne);
    DevBuf<uint8_t> df(ne);
    dv.upload(ev.data(), ne), dw.upload(ew.data(), ne);
    LAUNCH(k_tl_scores, ne, dv.p, dw.p, (uint32_t)ne, t.sv.p, t.sw.p, t.out_e.p, t.gsel.p, t.m, e.rec, ds.p, df.p);
    PGX_HIP(hipGetLastError());
    ds.download(score.data(), ne), df.download(found.data(), ne);
    pgx::sync();
  }
  std::vector<std::vector<Alt>> alts(bundles.size());
  size_t at = 0;
  for (size_t b = 0; b < bundles.size(); ++b) {
    const Utg &u = U.utgs[bundles[b]];
    const unsigned long long line = (unsigned long long)u.line;
    Bundle g;
    for (uint32_t j = 0; j < u.n; ++j) {
      const Utg &sub = U.utgs[sub_utg[u.off + j]];
      for (uint32_t k = 0; k + 1 < sub.n; ++k, ++at) {
        PGX_REQUIRE(found[at], PGX_EINVAL, "%s: line %llu: an edge of the sub-unitig of line %llu is not a G edge of the edge table", in.utg_name, line,
                    (unsigned long long)sub.line);
        PGX_REQUIRE(score[at] > 0, PGX_EINVAL, "%s: line %llu: an edge of the sub-unitig of line %llu has aln_score <= 0 (the shortest-path rounds need weights > 0)",
                    in.utg_name, line, (unsigned long long)sub.line);
        PGX_REQUIRE(score[at] < (1LL << 40), PGX_EINVAL, "%s: line %llu: an edge of the sub-unitig of line %llu has aln_score >= 2^40 (the sums of a round stay exact)",
                    in.utg_name, line, (unsigned long long)sub.line);
        g.add_edge(ev[at], ew[at], score[at]);
      }
    }
    const Key3 self = u.key;
    auto si = g.id.find(self.s), ti = g.id.find(self.t);
    PGX_REQUIRE(si != g.id.end() && ti != g.id.end(), PGX_EINVAL, "%s: line %llu: s or t is not a node of the compound unitig's graph", in.utg_name, line);
    PGX_REQUIRE(self.s != self.t, PGX_EINVAL, "%s: line %llu: a compound unitig with s == t (the script's rounds would not end)", in.utg_name, line);
    Alt a;
    bool tie = false;
    PGX_REQUIRE(g.search(si->second, ti->second, &a, &tie), PGX_EINVAL, "%s: line %llu: no path from s to t in the compound unitig's graph", in.utg_name, line);
    do {
      S.compound_tie_rounds += tie;
      g.remove_path(a.path);
      alts[b].push_back(a);
    } while (g.search(si->second, ti->second, &a, &tie));
    std::sort(alts[b].begin(), alts[b].end(), [](const Alt &x, const Alt &y) { return x.weight != y.weight ? x.weight > y.weight : names_above(x.path, y.path); });
  }
  return alts;
}

// ---- the chosen paths join the pool behind the file's nodes; ctg_paths, second pass: the kept rows as segments of the pool, the primary
// paths in ps[0], the alternates in ps[1]
void path_sets(const Inputs &in, pgx_tiling_stats_t &S, UtgData &U, const std::vector<KeptRow> &kept, const std::vector<uint32_t> &bundle_of,
               const std::vector<std::vector<Alt>> &alts, PathSet ps[2]) {
  std::vector<uint64_t> &pool = U.pool;
  std::vector<std::vector<uint64_t>> alt_off(alts.size());
  for (size_t b = 0; b < alts.size(); ++b)
    for (const Alt &a : alts[b]) alt_off[b].push_back(pool.size()), pool.insert(pool.end(), a.path.begin(), a.path.end());
  PGX_REQUIRE(pool.size() < NONE, PGX_EINVAL, "%s: more than 2^32 - 2 nodes in unitig paths", in.utg_name);
  for (const KeptRow &row : kept) {
    uint64_t len = 0;
    std::vector<std::pair<uint64_t, uint64_t>> segs;
    std::vector<std::pair<std::pair<uint64_t, uint64_t>, uint32_t>> group;   // (s, t) of the row's compound unitigs in order of first appearance, the bundle of the last
    auto extend = [&](uint64_t off, uint64_t n) {
      const uint64_t skip = len ? 1 : 0;
      segs.emplace_back(off + skip, n - skip), len += n - skip;
    };
    for (uint32_t ui : row.utg) {
      const Utg &u = U.utgs[ui];
      if (u.type == UT_SIMPLE) {
        extend(u.off, u.n);
      } else if (u.type == UT_COMPOUND) {
        const uint32_t b = bundle_of[ui];
        extend(alt_off[b][0], alts[b][0].path.size());
        const std::pair<uint64_t, uint64_t> st_key(alts[b][0].path.front(), alts[b][0].path.back());
        size_t gi = 0;
        while (gi < group.size() && group[gi].first != st_key) ++gi;
        if (gi == group.size()) group.emplace_back(st_key, b);
        else group[gi].second = b;
      }
    }
    if (len == 0) {
      ++S.ctg_empty;
      continue;
    }
    PGX_REQUIRE(len >= 2, PGX_EINVAL, "%s: line %llu: a path of one node (the script would write an empty line)", in.ctg_name, (unsigned long long)row.line);
    ++S.ctg_kept;
    ps[0].open(row.name, row.line);
    for (const auto &sg : segs) ps[0].add(sg.first, sg.second);
    ps[0].close();
    for (size_t a_id = 0; a_id < group.size(); ++a_id) {
      const uint32_t b = group[a_id].second;
      for (size_t sub_id = 1; sub_id < alts[b].size(); ++sub_id) {
        char suffix[64];
        snprintf(suffix, sizeof(suffix), "-%03d-%02d", (int)(a_id + 1), (int)sub_id);
        PGX_REQUIRE(row.name.size() + strlen(suffix) <= CTG_NAME_MAX, PGX_EINVAL, "%s: line %llu: an alternate's name of more than %u bytes", in.ctg_name,
                    (unsigned long long)row.line, CTG_NAME_MAX);
        ps[1].open(row.name + suffix, row.line);
        ps[1].add(alt_off[b][sub_id], alts[b][sub_id].path.size());
        ps[1].close();
        ++S.alternates;
      }
    }
  }
}

// the stage as its phases.  tiling_paths opens before utg_data is read and closes with the function; host_us: from there to the path
// sets, the device sorts of the dual rule and the unitig index included
void build_tiling(const Inputs &in, pgx_tiling *out) {
  pgx_tiling_stats_t &S = out->st;
  std::unique_ptr<KernelTimer> part(new KernelTimer("tiling_parse", 0));
  DevEdges e;
  edge_records(in, e);
  S.sg_lines = e.n;
  part.reset(), part.reset(new KernelTimer("tiling_index", e.n));
  EdgeTable t;
  build_table(e, in.sg_fn ? in.sg_fn : "the string graph", t);
  S.g_edges = t.m;
  part.reset(), part.reset(new KernelTimer("tiling_paths", t.m));
  const double host0 = wall_ms();
  UtgData U;
  read_utg_data(in, S, U);
  CtgRows C;
  read_ctg_paths(in, U.subs.size(), C);
  const std::vector<uint8_t> keep = dual_rule(C);
  const std::vector<uint32_t> found = find_unitigs(in, U, C);
  const uint32_t *ref_utg = found.data(), *sub_utg = found.data() + C.refs.size();
  std::vector<uint32_t> bundle_of, bundles;
  const std::vector<KeptRow> kept = kept_rows(in, S, U, C, keep, ref_utg, bundle_of, bundles);
  const std::vector<std::vector<Alt>> alts = bundle_alts(in, S, U, sub_utg, bundles, e, t);
  PathSet ps[2];
  path_sets(in, S, U, kept, bundle_of, alts, ps);
  S.host_us = (uint64_t)((wall_ms() - host0) * 1000.0);
  // every node and edge of every path
  DevBuf<uint64_t> d_pool(U.pool.size() + 1);
  d_pool.upload(U.pool.data(), U.pool.size());
  for (int w = 0; w < 2; ++w) build_set(ps[w], d_pool, U.pool.size(), e, t, U.pool, in.ctg_name, out->set[w]);
  S.p_rows = out->set[0].n_rows, S.a_rows = out->set[1].n_rows;
  pgx::sync();
}

void require_tiling(const pgx_tiling *t, int which, const char *who) {
  PGX_REQUIRE(t, PGX_EARG, "%s: null argument", who);
  PGX_REQUIRE(!t->shut && ctx().ready, PGX_ESTATE, "%s: pgx_shutdown ran while the tiling paths were alive (free them)", who);
  PGX_REQUIRE(which == 0 || which == 1, PGX_EARG, "%s: which is 0 (primary) or 1 (alternate)", who);
}

int tiling_entry(const char *who, const Inputs &in, pgx_tiling **out) {
  auto pre = [&] {
    PGX_REQUIRE((in.sg_fn != nullptr) != (in.g != nullptr), PGX_EARG, "%s: one of a sg_edges_list file and a string graph", who);
    PGX_REQUIRE((in.utg || !in.utg_len) && (in.ctg || !in.ctg_len), PGX_EARG, "%s: null argument", who);
  };
  return live_build(who, g_tl, out, pre, [&](pgx_tiling *t, uint64_t *n) {
    *n = in.utg_len + in.ctg_len;
    MemTag tag("tiling");
    KernelTimer tm("tiling", 0);
    build_tiling(in, t);
  }, "tiling paths", "bytes of unitigs and contig paths");
}
}  // namespace
}  // namespace pgx

extern "C" int pgx_sgraph_parse(const char *sg_edges_list_fn, pgx_sgraph_edge **edges, int64_t **idt_hundredths, uint64_t *n) {
  if (edges) *edges = nullptr;
  if (idt_hundredths) *idt_hundredths = nullptr;
  if (n) *n = 0;
  const int rc = guarded([&] {
    PGX_REQUIRE(sg_edges_list_fn && edges && n, PGX_EARG, "pgx_sgraph_parse: null argument");
    PGX_REQUIRE(ctx().ready, PGX_ESTATE, "pgx_sgraph_parse: no device context (pgx_init has not been called, or found no HIP device)");
    int code = PGX_OK;
    try {
      MemTag tag("tiling");
      KernelTimer tm("tiling", 0), tm_parse("tiling_parse", 0);
      DevEdges e;
      parse_sg_file(sg_edges_list_fn, true, e);
      *edges = (pgx_sgraph_edge *)out_alloc(e.n ? (size_t)e.n * sizeof(Edge) : 1);
      if (idt_hundredths) *idt_hundredths = (int64_t *)out_alloc(e.n ? (size_t)e.n * sizeof(int64_t) : 1);
      if (e.n) {
        PGX_HIP(hipMemcpyAsync(*edges, e.rec, (size_t)e.n * sizeof(Edge), hipMemcpyDeviceToHost, ctx().stream));
        if (idt_hundredths) e.hund.download(*idt_hundredths, e.n);
      }
      pgx::sync();
      *n = e.n;
    } catch (const Fail &f) {
      code = build_fail_code(f, "pgx_sgraph_parse", "edge records", 0, "lines");
    }
    timing_flush();
    return code;
  });
  if (rc != PGX_OK) {
    if (edges && *edges) out_free(*edges), *edges = nullptr;
    if (idt_hundredths && *idt_hundredths) out_free(*idt_hundredths), *idt_hundredths = nullptr;
  }
  return rc;
}

extern "C" int pgx_tiling_build(const char *sg_edges_list_fn, pgx_sgraph *g, const char *utg_text, size_t utg_len, const char *ctg_text, size_t ctg_len, pgx_tiling **out) {
  return tiling_entry("pgx_tiling_build", Inputs{sg_edges_list_fn, g, utg_text, ctg_text, utg_len, ctg_len, "utg_data", "ctg_paths"}, out);
}

extern "C" int pgx_tiling_stats(const pgx_tiling *t, pgx_tiling_stats_t *out) {
  return guarded([&] {
    PGX_REQUIRE(out, PGX_EARG, "pgx_tiling_stats: null argument");
    require_tiling(t, 0, "pgx_tiling_stats");
    *out = t->st;
  });
}

extern "C" int pgx_tiling_rows(const pgx_tiling *t, int which, uint64_t first, uint64_t n, pgx_tile_row *out) {
  return guarded([&] {
    require_tiling(t, which, "pgx_tiling_rows");
    const pgx_tiling::Set &s = t->set[which];
    PGX_REQUIRE(first <= s.n_rows && n <= s.n_rows - first && (n == 0 || out), PGX_EARG, "pgx_tiling_rows: rows %llu .. + %llu of %llu", (unsigned long long)first,
                (unsigned long long)n, (unsigned long long)s.n_rows);
    if (n == 0) return;
    PGX_HIP(hipMemcpyAsync(out, s.rows.p + first, n * sizeof(pgx_tile_row), hipMemcpyDeviceToHost, ctx().stream));
    pgx::sync();
  });
}

extern "C" int pgx_tiling_names(const pgx_tiling *t, int which, char **text, size_t *text_len, uint64_t *n_ctg) {
  return text_call(text, text_len, nullptr, [&] {
    require_tiling(t, which, "pgx_tiling_names");
    PGX_REQUIRE(text && text_len, PGX_EARG, "pgx_tiling_names: null argument");
    const pgx_tiling::Set &s = t->set[which];
    *text = caller_text(s.distinct.data(), s.distinct.size());
    *text_len = s.distinct.size();
    if (n_ctg) *n_ctg = s.n_ctg;
  });
}

extern "C" int pgx_tiling_text(pgx_tiling *t, int which, uint64_t max_lines, char **text, size_t *text_len, int *done) {
  return text_call(text, text_len, done, [&] {
    require_tiling(t, which, "pgx_tiling_text");
    pgx_tiling::Set &s = t->set[which];
    text_next("pgx_tiling_text", s.text, s.lines(), t->stage, TextNames{"tiling", "tiling_text", "tiling", "tl.text"}, max_lines, text, text_len, done);
  });
}

// contig FASTA from the rows of file `which`: the rows come to the host once (24 bytes each) and go through the layout pgx_contigs_chunk
// runs on a parsed file -- no text is written and parsed again
extern "C" int pgx_tiling_contigs(const pgx_tiling *t, int which, const char *seqdb_prefix, const char *out_path, uint64_t *n_ctg, uint64_t *n_bases) {
  std::vector<pgx_tile_row> rows;
  const int rc = guarded([&] {
    require_tiling(t, which, "pgx_tiling_contigs");
    const pgx_tiling::Set &s = t->set[which];
    rows.resize(s.n_rows);
    if (s.n_rows) {
      PGX_HIP(hipMemcpyAsync(rows.data(), s.rows.p, s.n_rows * sizeof(pgx_tile_row), hipMemcpyDeviceToHost, ctx().stream));
      pgx::sync();
    }
  });
  if (rc != PGX_OK) return rc;
  const std::vector<std::string> &names = t->set[which].ctg_names;
  return contigs_from_rows("pgx_tiling_contigs", seqdb_prefix, [&](const TileRowFn &add) {
    for (size_t i = 0; i < rows.size(); ++i) {
      const pgx_tile_row &r = rows[i];
      add(names[r.ctg], r.rid0, r.rid1, r.s, r.e, r.strand0, r.strand1, i);
    }
  }, out_path, n_ctg, n_bases);
}

extern "C" int pgx_tiling_free(pgx_tiling *t) {
  if (t) g_tl.destroy(t);
  return PGX_OK;
}

// the file level: nothing is written unless everything was built -- both texts are whole in host memory before the first file is opened
extern "C" int pgx_tiling_chunk(const char *sg_edges_list_fn, const char *utg_data_fn, const char *ctg_paths_fn, const char *p_out, const char *a_out,
                                pgx_tiling_stats_t *stats) {
  pgx_tiling *t = nullptr;
  const int rc = guarded([&] {
    PGX_REQUIRE(sg_edges_list_fn && utg_data_fn && ctg_paths_fn && p_out && a_out, PGX_EARG, "pgx_tiling_chunk: null argument");
    std::vector<uint8_t> utg, ctg;
    PGX_REQUIRE(read_file(utg_data_fn, utg), PGX_EINVAL, "%s: cannot be read", utg_data_fn);
    PGX_REQUIRE(read_file(ctg_paths_fn, ctg), PGX_EINVAL, "%s: cannot be read", ctg_paths_fn);
    const int code = tiling_entry("pgx_tiling_chunk", Inputs{sg_edges_list_fn, nullptr, (const char *)utg.data(), (const char *)ctg.data(), utg.size(), ctg.size(), utg_data_fn,
                                                             ctg_paths_fn}, &t);
    if (code != PGX_OK) return code;
    std::string text[2];
    for (int w = 0; w < 2; ++w)
      for (int done = 0; !done;) {
        char *piece = nullptr;
        size_t len = 0;
        const int c = pgx_tiling_text(t, w, 1ULL << 22, &piece, &len, &done);
        if (c != PGX_OK) return c;
        text[w].append(piece, len);
        free(piece);
      }
    const char *path[2] = {p_out, a_out};
    for (int w = 0; w < 2; ++w) {
      File f;
      f.f = fopen(path[w], "wb");
      PGX_REQUIRE(f.f, PGX_EINVAL, "%s: cannot be written", path[w]);
      PGX_REQUIRE(fwrite(text[w].data(), 1, text[w].size(), f.f) == text[w].size(), PGX_EINVAL, "%s: write error", path[w]);
    }
    if (stats) *stats = t->st;
    return (int)PGX_OK;
  });
  pgx_tiling_free(t);
  return rc;
}
