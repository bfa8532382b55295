// pgx_cns_job.hip -- pg_asm_cns.py as a whole (py/scripts/pg_asm_cns.py), from the map's text to the FASTA.  The rule: DESIGN.md section 4.7b.
// First its layout (:53-139): the map rows of a chunk to the table of pieces (a contig's groups, each a template of the contig) and the
// table of read entries (which read, on which strand, at which shift, for which piece), in the order the script answers and aligns them:
//
//   k_lay_check     every row against the contig lengths and the encodings below; the first row of every contig (atomicMin)
//   rank            contigs numbered in order of first appearance: a scan over the rows that are a contig's first
//   sort            stable, by (contig rank, p1): a contig's rows in the order the script's sort leaves them
//   k_lay_walk      a thread per contig: the chain of groups, every jump a binary search in the sorted p1; once to count, once to fill
//   k_lay_assign    a thread per row: the group it joins, by binary search among its contig's groups (a closing row joins none)
//   entries         the joined rows sorted by (group, read, strand, offset); per (group, read, strand) the first appearance among the
//                   group's rows (atomicMin) and the chain of offsets more than 50 apart (a thread per run); the entries then sorted by
//                   (group, shift, first appearance), which is the script's stable sort by shift of its print order
// Then the job over it (cns_job_dev):
//   k_par_*         the map file's text to rows in bounded pieces of the file: lines by select, a thread per line, the chunk filter
//   k_job_items     a batch of pieces as a pool layout: templates and reads as items, and the batch as pgx_cns_pieces takes it
//   k_job_decode    biseq bytes of the two resident databases to the ASCII pool, 16 bytes per thread
//   cns_pieces_dev  the inner loop (pgx_cns_align.hip), the text left on the device
//   k_st_*          the stitch's requests (faln_dev runs them without strings) and what every piece keeps
//   k_job_fasta     headers, kept bytes and newlines to the FASTA, 16 bytes per thread
#include <algorithm>
#include <string>

#include "pgx_text.h"

namespace pgx {
namespace {

constexpr int64_t FIRST_ANCHOR = 1000, FLANK = 1000, JOIN = 50000, KEEP = 100000, CHAIN = 50;
constexpr int64_t FIT = 1ll << 29;   // |p1|, |rb| below this: offsets and shifts stay inside int32
constexpr uint32_t NONE = UINT32_MAX;
enum { E_CTG, E_LEN0, E_FIT, E_TMPL, E_SLOTS };

struct Grp {
  uint32_t rank, seg;
  int32_t la, right;              // left_anchor and right as the script prints them
  uint32_t r0, r1, skip, end;     // its rows: sorted positions [r0, r1) without `skip`; end: one past the last position it spans
};

__device__ __forceinline__ uint32_t bias(int32_t v) { return (uint32_t)v ^ 0x80000000u; }
__device__ __forceinline__ int32_t unbias(uint32_t v) { return (int32_t)(v ^ 0x80000000u); }

__global__ void k_lay_check(const int64_t *rows, uint32_t n, const int64_t *ctg_len, uint64_t n_ctg, uint32_t *first, uint32_t *err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t *r = rows + (size_t)i * 9;
  const int64_t ctg = r[0], p1 = r[1], read = r[3], rb = r[4], strand = r[6];
  if (ctg < 0 || (uint64_t)ctg >= n_ctg || ctg_len[ctg] < 0) {
    atomicMin(&err[E_CTG], i);
    return;
  }
  if (ctg_len[ctg] == 0) atomicMin(&err[E_LEN0], i);
  if (p1 <= -FIT || p1 >= FIT || rb <= -FIT || rb >= FIT || read < 0 || read > (int64_t)UINT32_MAX || strand < 0 || strand > 1 || ctg_len[ctg] >= FIT)
    atomicMin(&err[E_FIT], i);
  atomicMin(&first[ctg], i);
}
__global__ void k_lay_is_first(const int64_t *rows, uint32_t n, const uint32_t *first, uint32_t *flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flag[i] = first[rows[(size_t)i * 9]] == i;
}
__global__ void k_lay_rank(const int64_t *rows, uint32_t n, const uint32_t *flag, const uint32_t *before, uint32_t *rank, uint32_t *ctg_of) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const uint32_t ctg = (uint32_t)rows[(size_t)i * 9];
  rank[ctg] = before[i], ctg_of[before[i]] = ctg;
}
__global__ void k_lay_key(const int64_t *rows, uint32_t n, const uint32_t *rank, uint64_t *key, uint32_t *val) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t *r = rows + (size_t)i * 9;
  key[i] = (uint64_t)rank[r[0]] << 32 | bias((int32_t)r[1]);
  val[i] = i;
}
// cstart[r]: where contig rank r begins among the sorted rows; cstart[n_used] = n
__global__ void k_lay_starts(const uint64_t *skey, uint32_t n, uint32_t n_used, uint32_t *cstart, int32_t *sp1) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t r = (uint32_t)(skey[j] >> 32);
  sp1[j] = unbias((uint32_t)skey[j]);
  if (j == 0 || (uint32_t)(skey[j - 1] >> 32) != r) cstart[r] = j;
  if (j == 0) cstart[n_used] = n;
}

// pg_asm_cns.py:72-98 for contig rank c.  FILL == false: count[c] = its groups.  FILL == true: the groups at out[goff[c] ..].
template <bool FILL>
__global__ void k_lay_walk(uint32_t n_used, const uint32_t *cstart, const int32_t *sp1, const uint32_t *ctg_of, const int64_t *ctg_len, uint32_t *count,
                           const uint32_t *goff, Grp *out) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_used) return;
  const uint32_t lo = cstart[c], hi = cstart[c + 1];
  const int64_t L = ctg_len[ctg_of[c]];
  const uint32_t base = FILL ? goff[c] : 0, room = FILL ? goff[c + 1] - base : 0;
  int64_t la = FIRST_ANCHOR;
  uint32_t pos = lo, ng = 0;
  Grp cur = {};
  bool have = false;
  auto emit = [&](int64_t left, int64_t right, uint32_t r0, uint32_t r1, uint32_t end) {
    if (have) {
      if (FILL && ng - 1 < room) out[base + ng - 1] = cur;
    }
    cur.rank = c, cur.seg = ng, cur.la = (int32_t)left, cur.right = (int32_t)right, cur.r0 = r0, cur.r1 = r1, cur.skip = NONE, cur.end = end;
    have = true, ++ng;
  };
  while (pos < hi) {
    uint32_t a = pos, b = hi;   // the first row from pos on with p1 - left_anchor >= 50000
    while (a < b) {
      const uint32_t m = a + (b - a) / 2;
      if ((int64_t)sp1[m] - la < JOIN) a = m + 1;
      else b = m;
    }
    if (a == hi) break;
    const int64_t p = sp1[a];
    if (p - la < KEEP) emit(la, p, pos, a, a + 1);
    else emit(la, p, a, a, a + 1);
    la = p, pos = a + 1;
  }
  const int64_t d = L - la;
  if (d >= KEEP) {
    emit(la, L, hi, hi, hi);
  } else if (d > FLANK) {
    emit(la, L, pos, hi, hi);
  } else if (have) {   // the previous group ends at the contig's end and takes the open rows behind its own
    cur.right = (int32_t)L;
    if (cur.r0 == cur.r1) cur.r0 = pos, cur.r1 = hi;
    else cur.skip = cur.end - 1, cur.r1 = hi;
    cur.end = hi;
  } else {
    emit(la, L, hi, hi, hi);
  }
  if (FILL) {
    if (ng - 1 < room) out[base + ng - 1] = cur;
  } else {
    count[c] = ng;
  }
}
__global__ void k_lay_gcheck(const Grp *g, uint32_t ng, const uint32_t *ctg_of, const int64_t *ctg_len, uint32_t *err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ng) return;
  const int64_t t_len = (int64_t)g[i].right - ((int64_t)g[i].la - FLANK);
  if (t_len <= 0 || g[i].right > ctg_len[ctg_of[g[i].rank]]) atomicMin(&err[E_TMPL], i);
}
// the group sorted row j joins (NONE: none)
__global__ void k_lay_assign(const uint64_t *skey, uint32_t n, const uint32_t *goff, const Grp *g, uint32_t *grp, uint8_t *joined) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t c = (uint32_t)(skey[j] >> 32);
  uint32_t a = goff[c], b = goff[c + 1];   // the first of the contig's groups that ends behind j
  while (a < b) {
    const uint32_t m = a + (b - a) / 2;
    if (g[m].end <= j) a = m + 1;
    else b = m;
  }
  const bool in = a < goff[c + 1] && j >= g[a].r0 && j < g[a].r1 && j != g[a].skip;
  grp[j] = in ? a : NONE, joined[j] = in;
}
// entry candidate e = joined row list[e]: its offset p1 - rb, and the first sort's key
__global__ void k_ent_offset(const int64_t *rows, const uint32_t *sidx, const uint32_t *list, uint32_t m, int32_t *off, uint32_t *key, uint32_t *val) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  const int64_t *r = rows + (size_t)sidx[list[e]] * 9;
  off[e] = (int32_t)(r[1] - r[4]);
  key[e] = bias(off[e]), val[e] = e;
}
__global__ void k_ent_key(const int64_t *rows, const uint32_t *sidx, const uint32_t *list, const uint32_t *grp, const uint32_t *order, uint32_t m, uint64_t *key) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= m) return;
  const uint32_t j = list[order[x]];
  const int64_t *r = rows + (size_t)sidx[j] * 9;
  key[x] = (uint64_t)grp[j] << 33 | (uint64_t)(uint32_t)r[3] << 1 | (uint64_t)r[6];
}
__global__ void k_ent_heads(const uint64_t *key, uint32_t m, uint32_t *head) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x < m) head[x] = x == 0 || key[x] != key[x - 1];
}
// run[x]: the (group, read, strand) of sorted candidate x; the run's start, its first appearance among the group's rows, the offsets in order
__global__ void k_ent_runs(const uint32_t *head, const uint32_t *before, const uint32_t *order, const uint32_t *list, const int32_t *off, uint32_t m, uint32_t n_runs,
                           uint32_t *run, uint32_t *run_start, uint32_t *first_app, int32_t *soff) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= m) return;
  const uint32_t r = before[x] + head[x] - 1;
  run[x] = r, soff[x] = off[order[x]];
  if (head[x]) run_start[r] = x;
  if (x == 0) run_start[n_runs] = m;
  atomicMin(&first_app[r], list[order[x]]);
}
// pg_asm_cns.py:128-136: an entry at the smallest offset, another at every offset more than 50 above the last entry's
__global__ void k_ent_chain(const uint32_t *run_start, uint32_t n_runs, const int32_t *soff, uint8_t *emit) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_runs) return;
  const uint32_t s = run_start[r], e = run_start[r + 1];
  int64_t cur = soff[s];
  emit[s] = 1;
  for (uint32_t x = s + 1; x < e; ++x) {
    const bool take = soff[x] > cur + CHAIN;
    if (take) cur = soff[x];
    emit[x] = take;
  }
}
__global__ void k_ent_first_key(const uint32_t *list2, const uint32_t *run, const uint32_t *first_app, uint32_t n_ent, uint32_t *key, uint32_t *val) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_ent) key[t] = first_app[run[list2[t]]], val[t] = t;
}
__global__ void k_ent_shift_key(const uint32_t *list2, const uint32_t *order, const uint64_t *ckey, const int32_t *soff, const Grp *g, uint32_t n_ent, uint64_t *key) {
  const uint32_t y = blockIdx.x * blockDim.x + threadIdx.x;
  if (y >= n_ent) return;
  const uint32_t x = list2[order[y]];
  const uint32_t gi = (uint32_t)(ckey[x] >> 33);
  key[y] = (uint64_t)gi << 32 | bias(soff[x] - (g[gi].la - (int32_t)FLANK));
}
__global__ void k_ent_write(const uint64_t *skey, const uint32_t *order, const uint32_t *list2, const uint64_t *ckey, uint32_t n_ent, pgx_cns_job_read *out) {
  const uint32_t y = blockIdx.x * blockDim.x + threadIdx.x;
  if (y >= n_ent) return;
  const uint64_t ck = ckey[list2[order[y]]];
  pgx_cns_job_read e;
  e.piece = (uint32_t)(skey[y] >> 32), e.read = (uint32_t)(ck >> 1), e.read_shift = unbias((uint32_t)skey[y]), e.strand = (uint32_t)(ck & 1);
  out[y] = e;
}
__global__ void k_lay_pieces(const Grp *g, uint32_t ng, const uint32_t *ctg_of, const uint64_t *skey, uint32_t n_ent, pgx_cns_job_piece *out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ng) return;
  auto lower = [&](uint64_t k) {
    uint32_t a = 0, b = n_ent;
    while (a < b) {
      const uint32_t m = a + (b - a) / 2;
      if (skey[m] < k) a = m + 1;
      else b = m;
    }
    return a;
  };
  const uint32_t f = lower((uint64_t)i << 32), l = lower(((uint64_t)i + 1) << 32);
  pgx_cns_job_piece p = {};
  p.ctg = ctg_of[g[i].rank], p.seg = g[i].seg, p.left = g[i].la - (int32_t)FLANK, p.t_len = (uint32_t)(g[i].right - p.left);
  p.n_mapped = g[i].r1 - g[i].r0 - (g[i].skip != NONE), p.read_first = f, p.n_read = l - f;
  out[i] = p;
}

}  // namespace

// The layout of n > 0 rows on the device (n x 9 int64) against ctg_len (by contig id; negative: the idx lacks it): the tables, on the device.
// d_row_name: what the refusals call row i (its number among the caller's rows, or its line in the file; nullptr: i), row_word: "row" / "line"
void cns_layout_dev(const char *who, const int64_t *d_rows, size_t n_rows, const int64_t *d_len, size_t n_ctg, DevBuf<pgx_cns_job_piece> &pieces, size_t *n_piece,
                    DevBuf<pgx_cns_job_read> &reads, size_t *n_read, const uint32_t *d_row_name = nullptr, const char *row_word = "row") {
  hipStream_t st = ctx().stream;
  const uint32_t n = (uint32_t)n_rows;
  PrimWs ws;
  DevBuf<uint32_t> err(E_SLOTS), first(n_ctg ? n_ctg : 1), flag(n), before(n);
  PGX_HIP(hipMemsetAsync(err.p, 0xFF, E_SLOTS * sizeof(uint32_t), st));
  PGX_HIP(hipMemsetAsync(first.p, 0xFF, first.n * sizeof(uint32_t), st));
  LAUNCH(k_lay_check, n, d_rows, n, d_len, (uint64_t)n_ctg, first.p, err.p);
  uint32_t h[E_SLOTS];
  err.download(h, E_SLOTS);
  sync();
  auto field = [&](uint32_t row, int f) {
    int64_t v = 0;
    PGX_HIP(hipMemcpyAsync(&v, d_rows + (size_t)row * 9 + f, sizeof(v), hipMemcpyDeviceToHost, st));
    sync();
    return (long long)v;
  };
  auto name = [&](uint32_t row) {
    uint32_t v = row;
    if (d_row_name) {
      PGX_HIP(hipMemcpyAsync(&v, d_row_name + row, sizeof(v), hipMemcpyDeviceToHost, st));
      sync();
    }
    return v;
  };
  PGX_REQUIRE(h[E_CTG] == UINT32_MAX, PGX_EINVAL, "%s: %s %u: contig %lld is not in the idx", who, row_word, name(h[E_CTG]), field(h[E_CTG], 0));
  PGX_REQUIRE(h[E_LEN0] == UINT32_MAX, PGX_EINVAL, "%s: %s %u: contig %lld has length 0", who, row_word, name(h[E_LEN0]), field(h[E_LEN0], 0));
  PGX_REQUIRE(h[E_FIT] == UINT32_MAX, PGX_EINVAL, "%s: %s %u (contig %lld): a position of 2^29 and more, a read id beyond 32 bits or a strand that is not 0 or 1", who,
              row_word, name(h[E_FIT]), field(h[E_FIT], 0));
  // contigs in order of first appearance
  LAUNCH(k_lay_is_first, n, d_rows, n, first.p, flag.p);
  exclusive_sum(flag.p, before.p, n, &ws);
  uint32_t last[2];
  PGX_HIP(hipMemcpyAsync(&last[0], flag.p + n - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  PGX_HIP(hipMemcpyAsync(&last[1], before.p + n - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  sync();
  const uint32_t n_used = last[0] + last[1];
  DevBuf<uint32_t> rank(first.n), ctg_of(n_used), val(n), sidx(n), cstart(n_used + 1), gcount(n_used), goff(n_used + 1);
  DevBuf<uint64_t> key(n), skey(n);
  DevBuf<int32_t> sp1(n);
  LAUNCH(k_lay_rank, n, d_rows, n, flag.p, before.p, rank.p, ctg_of.p);
  LAUNCH(k_lay_key, n, d_rows, n, rank.p, key.p, val.p);
  sort_pairs(key.p, skey.p, val.p, sidx.p, n, 0, 64, &ws);
  LAUNCH(k_lay_starts, n, skey.p, n, n_used, cstart.p, sp1.p);
  // the groups
  LAUNCH(k_lay_walk<false>, n_used, n_used, cstart.p, sp1.p, ctg_of.p, d_len, gcount.p, nullptr, nullptr);
  const uint32_t ng = scan_to_total(gcount.p, goff.p, n_used, &ws);
  PGX_REQUIRE(ng < (1u << 31), PGX_EARG, "%s: 2^31 pieces and more", who);
  DevBuf<Grp> grps(ng);
  LAUNCH(k_lay_walk<true>, n_used, n_used, cstart.p, sp1.p, ctg_of.p, d_len, nullptr, goff.p, grps.p);
  LAUNCH(k_lay_gcheck, ng, grps.p, ng, ctg_of.p, d_len, err.p);
  err.download(h, E_SLOTS);
  sync();
  if (h[E_TMPL] != UINT32_MAX) {
    Grp g;
    uint32_t ctg = 0;
    PGX_HIP(hipMemcpyAsync(&g, grps.p + h[E_TMPL], sizeof(g), hipMemcpyDeviceToHost, st));
    sync();
    PGX_HIP(hipMemcpyAsync(&ctg, ctg_of.p + g.rank, sizeof(ctg), hipMemcpyDeviceToHost, st));
    sync();
    PGX_REQUIRE(false, PGX_EINVAL, "%s: contig %u segment %u: the template [%d, %d) lies outside the contig", who, ctg, g.seg, g.la - (int)FLANK, g.right);
  }
  // the rows that join a group
  DevBuf<uint32_t> grp(n), list(n);
  DevBuf<uint8_t> joined(n);
  LAUNCH(k_lay_assign, n, skey.p, n, goff.p, grps.p, grp.p, joined.p);
  const uint32_t m = select_indices(joined.p, n, list.p, &ws);
  uint32_t n_ent = 0;
  DevBuf<uint64_t> fkey(1);
  if (m) {
    DevBuf<int32_t> off(m), soff(m);
    DevBuf<uint32_t> k1(m), k1s(m), v0(m), v1(m), order(m), head(m), hbefore(m), run(m);
    DevBuf<uint64_t> ck(m), cks(m);
    DevBuf<uint8_t> emit(m);
    LAUNCH(k_ent_offset, m, d_rows, sidx.p, list.p, m, off.p, k1.p, v0.p);
    sort_pairs(k1.p, k1s.p, v0.p, v1.p, m, 0, 32, &ws);
    LAUNCH(k_ent_key, m, d_rows, sidx.p, list.p, grp.p, v1.p, m, ck.p);
    sort_pairs(ck.p, cks.p, v1.p, order.p, m, 0, 64, &ws);
    LAUNCH(k_ent_heads, m, cks.p, m, head.p);
    exclusive_sum(head.p, hbefore.p, m, &ws);
    PGX_HIP(hipMemcpyAsync(&last[0], head.p + m - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PGX_HIP(hipMemcpyAsync(&last[1], hbefore.p + m - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    sync();
    const uint32_t n_runs = last[0] + last[1];
    DevBuf<uint32_t> run_start(n_runs + 1), first_app(n_runs), list2(m);
    PGX_HIP(hipMemsetAsync(first_app.p, 0xFF, n_runs * sizeof(uint32_t), st));
    LAUNCH(k_ent_runs, m, head.p, hbefore.p, order.p, list.p, off.p, m, n_runs, run.p, run_start.p, first_app.p, soff.p);
    LAUNCH(k_ent_chain, n_runs, run_start.p, n_runs, soff.p, emit.p);
    n_ent = select_indices(emit.p, m, list2.p, &ws);   // (> 0: every run has an entry)
    DevBuf<uint32_t> a1(n_ent), a1s(n_ent), t0(n_ent), t1(n_ent), forder(n_ent);
    DevBuf<uint64_t> sk(n_ent);
    fkey.alloc(n_ent);
    LAUNCH(k_ent_first_key, n_ent, list2.p, run.p, first_app.p, n_ent, a1.p, t0.p);
    sort_pairs(a1.p, a1s.p, t0.p, t1.p, n_ent, 0, 32, &ws);
    LAUNCH(k_ent_shift_key, n_ent, list2.p, t1.p, cks.p, soff.p, grps.p, n_ent, sk.p);
    sort_pairs(sk.p, fkey.p, t1.p, forder.p, n_ent, 0, 64, &ws);
    reads.alloc(n_ent);
    LAUNCH(k_ent_write, n_ent, fkey.p, forder.p, list2.p, cks.p, n_ent, reads.p);
  }
  pieces.alloc(ng);
  LAUNCH(k_lay_pieces, ng, grps.p, ng, ctg_of.p, fkey.p, n_ent, pieces.p);
  sync();   // (the temporaries above go back to the block cache: stream-ordered, but the caller may read from another stream)
  *n_piece = ng, *n_read = n_ent;
}

// ---------------------------------------------------------------------------------------------------------
// the job: rows -> layout -> per batch of pieces: decode to an ASCII pool, the inner loop -> stitch -> FASTA
// ---------------------------------------------------------------------------------------------------------
namespace {

constexpr uint32_t STITCH_Q = 1000, STITCH_T = 1050, STITCH_BAND = 400;
constexpr uint64_t COST_CAP = 1ull << 30;        // per batch: 2 * pool bytes + 300 per read entry, a bound on the tags of its consensus call (< 2^31)
constexpr uint32_t MAX_BATCH_PIECES = 1u << 20;  // pgx_cns_pieces' own bound
enum { J_READ, J_STITCH, J_SLOTS };
enum { P_OK = 0, P_FIELDS, P_INT, P_FIT, P_BYTE };
const char *const P_TEXT[] = {"", "does not have nine fields", "has a field that is not a decimal integer of at most 18 digits",
                              "has a number that does not fit (a negative contig or read id or one beyond 32 bits, a position of 2^29 and more, a strand that is not 0 or 1)",
                              "has a byte that is not ASCII"};

__host__ __device__ inline uint64_t pad16(uint64_t n) { return (n + 15) & ~15ull; }

struct Item {   // one sequence of a batch's pool
  uint64_t dst, src;
  uint32_t len, kind;   // kind 0: the contig database, low nibble; 1 / 2: the read database, low / high nibble
};

__global__ void k_job_present(const uint32_t *rid, uint32_t n, uint8_t *present) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) present[rid[i]] = 1;
}
__global__ void k_job_ctg_len(const uint32_t *rlen, const uint8_t *present, uint32_t n, int64_t *len) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n) len[c] = present[c] ? (int64_t)rlen[c] : -1;
}
// the chunk filter of pg_asm_cns.py:59 (a negative contig id is kept: the layout refuses it)
__global__ void k_job_filter(const int64_t *rows, uint32_t n, uint32_t total, uint32_t my, uint8_t *keep) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t ctg = rows[(size_t)i * 9];
  keep[i] = ctg < 0 || (uint64_t)ctg % total == my % total;
}
__global__ void k_job_take_rows(const int64_t *rows, const uint32_t *list, uint32_t m, uint32_t name_base, int64_t *out, uint32_t *row_name) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (m < 2^31: m * 9 needs 64 bits)
  if (t >= (uint64_t)m * 9) return;
  const uint32_t j = (uint32_t)(t / 9), f = (uint32_t)(t - (uint64_t)j * 9);
  out[t] = rows[(size_t)list[j] * 9 + f];
  if (f == 0) row_name[j] = name_base + list[j];
}
// the pool bytes of every read entry (its read's length, padded to 16); an entry whose read the idx lacks is reported
__global__ void k_job_entry_bytes(const pgx_cns_job_read *reads, uint32_t nr, const uint32_t *rlen, const uint8_t *present, uint32_t n_rid, uint32_t *bytes,
                                  uint32_t *err) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nr) return;
  const uint32_t rd = reads[e].read;
  if (rd >= n_rid || !present[rd]) {
    atomicMin(&err[J_READ], e);
    bytes[e] = 0;
  } else {
    bytes[e] = (uint32_t)pad16(rlen[rd]);
  }
}
__global__ void k_job_piece_cost(const pgx_cns_job_piece *pieces, uint32_t np, const uint64_t *ent_cum, uint64_t *pool, uint64_t *cost) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= np) return;
  const pgx_cns_job_piece pc = pieces[p];
  const uint64_t b = pad16(pc.t_len) + ent_cum[pc.read_first + pc.n_read] - ent_cum[pc.read_first];
  pool[p] = b, cost[p] = 2 * b + 300ull * pc.n_read;
}
// the pool of the batch of pieces [p0, p1) with entries [e0, e1): a piece's template, then its reads in order, each padded to 16 bytes;
// the sequences as items in pool order, and the batch as pgx_cns_pieces takes it
__global__ void k_job_items(const pgx_cns_job_piece *pieces, const pgx_cns_job_read *reads, uint32_t p0, uint32_t p1, uint32_t e0, uint32_t e1,
                            const uint64_t *pool_cum, const uint64_t *ent_cum, const uint64_t *ref_roff, const uint64_t *read_roff, const uint32_t *read_rlen,
                            Item *items, pgx_cns_piece *bp, pgx_cns_read *br) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t npb = p1 - p0, neb = e1 - e0;
  if (i >= npb + neb) return;
  Item it;
  if (i < npb) {
    const pgx_cns_job_piece pc = pieces[p0 + i];
    it.dst = pool_cum[p0 + i] - pool_cum[p0], it.src = ref_roff[pc.ctg] + (uint64_t)pc.left, it.len = pc.t_len, it.kind = 0;
    items[i + (pc.read_first - e0)] = it;
    pgx_cns_piece o = {};
    o.seq_off = it.dst, o.t_len = pc.t_len;
    bp[i] = o;
  } else {
    const uint32_t e = e0 + (i - npb);
    const pgx_cns_job_read rd = reads[e];
    const pgx_cns_job_piece pc = pieces[rd.piece];
    it.dst = pool_cum[rd.piece] - pool_cum[p0] + pad16(pc.t_len) + (ent_cum[e] - ent_cum[pc.read_first]);
    it.src = read_roff[rd.read], it.len = read_rlen[rd.read], it.kind = 1 + (rd.strand & 1);
    items[(rd.piece - p0 + 1) + (e - e0)] = it;
    pgx_cns_read o = {};
    o.seq_off = it.dst, o.seq_len = it.len, o.piece = rd.piece - p0, o.read_shift = rd.read_shift;
    br[e - e0] = o;
  }
}
// decode_biseq (src/shmr_utils.c:53-62) into the pool: a thread per 16 bytes of it, one 16-byte load of biseq bytes (the databases keep
// 1 KiB of padding behind their last byte), one 16-byte store.  Strand 0 is the low nibble, strand 1 the high one at the same place.
__global__ void k_job_decode(const Item *__restrict__ items, uint32_t n_items, const uint8_t *__restrict__ ref_seq, const uint8_t *__restrict__ read_seq,
                             uint64_t pool_bytes, uint8_t *__restrict__ pool) {
  const uint64_t at = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
  if (at >= pool_bytes) return;
  uint32_t a = 0, b = n_items;   // the first item that ends behind `at`
  while (a < b) {
    const uint32_t mid = a + ((b - a) >> 1);
    if (items[mid].dst + pad16(items[mid].len) <= at) a = mid + 1;
    else b = mid;
  }
  uint4 out = make_uint4(0, 0, 0, 0);
  if (a < n_items && items[a].dst <= at) {
    const Item it = items[a];
    const uint64_t x = at - it.dst;
    const uint32_t n = (uint32_t)min((uint64_t)16, (uint64_t)it.len - x);
    const uint8_t *src = (it.kind == 0 ? ref_seq : read_seq) + it.src + x;
    uint64_t w[2], o[2] = {0, 0};
    __builtin_memcpy(w, src, 16);
    const int sh = it.kind == 2 ? 4 : 0;
    // bits_to_base: "NACNGNNN" "TNNNNNNN"
    const uint64_t LO = (uint64_t)'N' | (uint64_t)'A' << 8 | (uint64_t)'C' << 16 | (uint64_t)'N' << 24 | (uint64_t)'G' << 32 | (uint64_t)'N' << 40 |
                        (uint64_t)'N' << 48 | (uint64_t)'N' << 56;
    const uint64_t HI = (uint64_t)'T' | 0x4E4E4E4E4E4E4E00ull;   // "TNNNNNNN"
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
      const uint32_t code = (uint32_t)(w[k >> 3] >> (8 * (k & 7) + sh)) & 15u;
      const uint64_t ch = ((code & 8 ? HI : LO) >> (8 * (code & 7))) & 0xFFu;
      if (k < n) o[k >> 3] |= ch << (8 * (k & 7));
    }
    out = make_uint4((uint32_t)o[0], (uint32_t)(o[0] >> 32), (uint32_t)o[1], (uint32_t)(o[1] >> 32));
  }
  *reinterpret_cast<uint4 *>(pool + at) = out;
}
__global__ void k_job_add_base(const uint64_t *off, uint32_t n, uint64_t base, uint64_t *out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = base + off[i];
}
// pg_asm_cns.py:255: the last 1,000 bytes of the segment before against the first 1,050 of this one (a contig's first segment: nothing).
// The length check is a defence: a template of a contig with two segments has 2,002 bases at least, so only a consensus call that answers
// less than half its template could get below 1,050 ("Refusals")
__global__ void k_st_reqs(const pgx_cns_job_piece *pieces, uint32_t np, const uint64_t *seg_off, pgx_faln_req *reqs, uint32_t *err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  pgx_faln_req rq = {};
  rq.band = STITCH_BAND;
  if (pieces[i].seg > 0) {
    if (seg_off[i] - seg_off[i - 1] < STITCH_Q || seg_off[i + 1] - seg_off[i] < STITCH_T) atomicMin(&err[J_STITCH], i);
    else rq.q_off = seg_off[i] - STITCH_Q, rq.q_len = STITCH_Q, rq.t_off = seg_off[i], rq.t_len = STITCH_T;
  }
  reqs[i] = rq;
}
// what piece i gives to the FASTA: its contig's header in front of a first segment, the bytes kept of it, a newline behind a last one
__global__ void k_st_keep(const pgx_cns_job_piece *pieces, uint32_t np, const uint64_t *seg_off, const pgx_faln_res *res, const uint64_t *name_off, uint32_t *from,
                          uint32_t *kept, uint32_t *out_len, uint8_t *is_first) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  const pgx_cns_job_piece pc = pieces[i];
  const uint64_t len = seg_off[i + 1] - seg_off[i];
  const uint64_t fr = pc.seg > 0 ? (uint64_t)res[i].aln_t_e : 0;
  const bool last = i + 1 == np || pieces[i + 1].seg == 0;
  const uint64_t cut = (!last && res[i + 1].aln_q_e < (int32_t)STITCH_Q) ? STITCH_Q - (uint32_t)res[i + 1].aln_q_e : 0;
  uint64_t k = len > fr ? len - fr : 0;
  k = k > cut ? k - cut : 0;
  const uint64_t hdr = pc.seg == 0 ? name_off[pc.ctg + 1] - name_off[pc.ctg] + 2 : 0;
  from[i] = (uint32_t)fr, kept[i] = (uint32_t)k, out_len[i] = (uint32_t)(hdr + k + last), is_first[i] = pc.seg == 0;
}
// a thread per 16 bytes of the FASTA (16 bytes of room behind `total`): the piece by binary search of the offsets
__global__ void k_job_fasta(const pgx_cns_job_piece *__restrict__ pieces, uint32_t np, const uint64_t *__restrict__ poff, const uint64_t *__restrict__ seg_off,
                            const char *__restrict__ seg_text, const uint32_t *__restrict__ from, const uint32_t *__restrict__ kept, const char *__restrict__ names,
                            const uint64_t *__restrict__ name_off, uint64_t total, char *__restrict__ out) {
  const uint64_t at = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
  if (at >= total) return;
  uint32_t a = 0, b = np;
  while (a < b) {
    const uint32_t mid = a + ((b - a) >> 1);
    if (poff[mid + 1] <= at) a = mid + 1;
    else b = mid;
  }
  uint32_t p = a;
  union {
    uint4 v;
    char c[16];
  } u;
  u.v = make_uint4(0, 0, 0, 0);
  const uint32_t n = (uint32_t)min((uint64_t)16, total - at);
  for (uint32_t k = 0; k < n; ++k) {
    const uint64_t pos = at + k;
    while (poff[p + 1] <= pos) ++p;
    uint64_t x = pos - poff[p];
    const uint32_t ctg = pieces[p].ctg;
    const uint64_t nl = pieces[p].seg == 0 ? name_off[ctg + 1] - name_off[ctg] : 0, hdr = pieces[p].seg == 0 ? nl + 2 : 0;
    char ch;
    if (x < hdr) ch = x == 0 ? '>' : x == nl + 1 ? '\n' : names[name_off[ctg] + x - 1];
    else if (x - hdr < kept[p]) ch = seg_text[seg_off[p] + from[p] + (x - hdr)];
    else ch = '\n';
    u.c[k] = ch;
  }
  *reinterpret_cast<uint4 *>(out + at) = u.v;
}
__global__ void k_job_ctg_off(const uint32_t *first_piece, uint32_t n_used, const uint64_t *poff, uint32_t np, uint64_t *ctg_off) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k <= n_used) ctg_off[k] = k < n_used ? poff[first_piece[k]] : poff[np];
}

// ---- map text -> rows ----------------------------------------------------------------------------------------------------------------
}  // namespace
__global__ void k_par_newlines(const char *text, uint32_t n, uint8_t *flag) {   // (pgx_internal.h: the map merge finds its lines with it too)
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flag[i] = text[i] == '\n';
}
namespace {
// A thread per line: line k is text[nlpos[k - 1] + 1, nlpos[k]).  rows[k]: its nine numbers; keep[k]: it belongs to the chunk; a line the
// script dies on: code[k], and err[0] = min(err[0], k)
__global__ void k_par_lines(const char *__restrict__ text, const uint32_t *__restrict__ nlpos, uint32_t nl, uint32_t total, uint32_t my, int64_t *__restrict__ rows,
                            uint8_t *__restrict__ keep, uint8_t *__restrict__ code, uint32_t *__restrict__ err) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nl) return;
  const uint32_t start = k ? nlpos[k - 1] + 1 : 0, len = nlpos[k] - start;
  const char *p = text + start;
  uint32_t i = 0, nf = 0;
  uint8_t why = P_OK;
  int64_t v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  while (true) {
    while (i < len && is_blank((unsigned char)p[i])) ++i;
    if (i >= len) break;
    const uint32_t a = i;
    bool ascii = true;
    while (i < len && !is_blank((unsigned char)p[i])) ascii &= !(p[i] & 0x80), ++i;
    if (!ascii) why = why ? why : P_BYTE;
    else if (nf < 9 && !parse_int(p + a, i - a, &v[nf])) why = why ? why : P_INT;
    ++nf;
  }
  if (!why && nf != 9) why = P_FIELDS;
  if (!why && (v[0] < 0 || v[0] > (int64_t)UINT32_MAX || v[3] < 0 || v[3] > (int64_t)UINT32_MAX || v[1] <= -FIT || v[1] >= FIT || v[4] <= -FIT || v[4] >= FIT ||
               v[6] < 0 || v[6] > 1))
    why = P_FIT;
#pragma unroll
  for (int f = 0; f < 9; ++f) rows[(size_t)k * 9 + f] = v[f];
  keep[k] = !why && (uint64_t)v[0] % total == my % total;
  code[k] = why;
  if (why) atomicMin(err, k);
}

struct JobNames {   // the contigs' names by contig id, on the device
  DevBuf<char> text;
  DevBuf<uint64_t> off;
  size_t n = 0;
};

uint32_t batch_hook() {
  const char *e = getenv("PGX_CNS_JOB_BATCH");
  const long v = e ? atol(e) : 0;
  return v > 0 ? (uint32_t)std::min<long>(v, MAX_BATCH_PIECES) : 0;
}

// a refusal of the inner loop names a piece of the job: say which contig and segment that is
[[noreturn]] void rethrow_named(const Fail &f, const std::vector<pgx_cns_job_piece> &pieces) {
  if (f.piece >= 0 && (uint64_t)f.piece < pieces.size()) {   // (the number the refusal itself carries: PGX_REQUIRE_PIECE)
    const std::string msg = pgx_last_error();
    set_error("%s (piece %lld is contig %u segment %u)", msg.c_str(), (long long)f.piece, pieces[f.piece].ctg, pieces[f.piece].seg);
  }
  throw f;
}

}  // namespace

// The job on rows that passed the chunk filter (device, n x 9 int64; d_row_name as cns_layout_dev's).  The FASTA text stays on the device:
// d_text[0 .. *total), contig k of *n_out at d_ctg_off[k] .. d_ctg_off[k + 1].
static void cns_job_dev(const char *who, pgx_seqdb *rdb, pgx_seqdb *cdb, const int64_t *d_rows, size_t n_rows, const uint32_t *d_row_name, const char *row_word,
                        const JobNames &names, DevBuf<char> &d_text, uint64_t *total, DevBuf<uint64_t> &d_ctg_off, uint64_t *n_out, pgx_cns_job_stats *stats) {
  hipStream_t st = ctx().stream;
  pgx_cns_job_stats js = {};
  js.n_rows = n_rows;
  *total = 0, *n_out = 0;
  d_ctg_off.alloc(1);
  PGX_HIP(hipMemsetAsync(d_ctg_off.p, 0, sizeof(uint64_t), st));
  if (n_rows == 0) {
    if (stats) *stats = js;
    return;
  }
  PGX_REQUIRE(rdb->d_seq.p && cdb->d_seq.p, PGX_ESTATE, "%s: a database whose bytes were released or compacted", who);
  PGX_REQUIRE(names.n >= cdb->rlen_by_rid.size(), PGX_EARG, "%s: %zu contig names for contig ids up to %zu", who, names.n, cdb->rlen_by_rid.size());
  const double t0 = wall_ms();
  PrimWs ws;
  // the layout
  const uint32_t n_ctg = (uint32_t)cdb->rlen_by_rid.size(), n_rid = (uint32_t)rdb->rlen_by_rid.size();
  DevBuf<uint8_t> c_present(n_ctg ? n_ctg : 1), r_present(n_rid ? n_rid : 1);
  DevBuf<int64_t> d_len(n_ctg ? n_ctg : 1);
  {
    DevBuf<uint32_t> ids(std::max(cdb->rid.size(), rdb->rid.size()) + 1);
    PGX_HIP(hipMemsetAsync(c_present.p, 0, c_present.n, st));
    PGX_HIP(hipMemsetAsync(r_present.p, 0, r_present.n, st));
    ids.upload(cdb->rid.data(), cdb->rid.size());
    if (!cdb->rid.empty()) LAUNCH(k_job_present, cdb->rid.size(), ids.p, (uint32_t)cdb->rid.size(), c_present.p);
    sync();
    ids.upload(rdb->rid.data(), rdb->rid.size());
    if (!rdb->rid.empty()) LAUNCH(k_job_present, rdb->rid.size(), ids.p, (uint32_t)rdb->rid.size(), r_present.p);
    if (n_ctg) LAUNCH(k_job_ctg_len, n_ctg, cdb->d_rlen.p, c_present.p, n_ctg, d_len.p);
    sync();
  }
  DevBuf<pgx_cns_job_piece> pieces;
  DevBuf<pgx_cns_job_read> reads;
  size_t np64 = 0, nr64 = 0;
  cns_layout_dev(who, d_rows, n_rows, d_len.p, n_ctg, pieces, &np64, reads, &nr64, d_row_name, row_word);
  const uint32_t np = (uint32_t)np64, nr = (uint32_t)nr64;
  js.n_pieces = np, js.n_reads = nr;
  // what every piece costs; the reads the idx lacks
  DevBuf<uint32_t> err(J_SLOTS), ent_bytes(nr ? nr : 1);
  DevBuf<uint64_t> ent_cum(nr + 1), pool_b(np), cost(np), pool_cum(np + 1), cost_cum(np + 1);
  PGX_HIP(hipMemsetAsync(err.p, 0xFF, J_SLOTS * sizeof(uint32_t), st));
  if (nr) LAUNCH(k_job_entry_bytes, nr, reads.p, nr, rdb->d_rlen.p, r_present.p, n_rid, ent_bytes.p, err.p);
  (void)scan_to_total(ent_bytes.p, ent_cum.p, nr, &ws);
  LAUNCH(k_job_piece_cost, np, pieces.p, np, ent_cum.p, pool_b.p, cost.p);
  (void)scan_to_total(pool_b.p, pool_cum.p, np, &ws);
  (void)scan_to_total(cost.p, cost_cum.p, np, &ws);
  std::vector<pgx_cns_job_piece> h_pieces(np);
  std::vector<uint64_t> h_pool(np + 1), h_cost(np + 1);
  uint32_t h[J_SLOTS];
  pieces.download(h_pieces.data(), np);
  pool_cum.download(h_pool.data(), np + 1);
  cost_cum.download(h_cost.data(), np + 1);
  err.download(h, J_SLOTS);
  sync();
  if (h[J_READ] != UINT32_MAX) {
    pgx_cns_job_read e;
    PGX_HIP(hipMemcpyAsync(&e, reads.p + h[J_READ], sizeof(e), hipMemcpyDeviceToHost, st));
    sync();
    PGX_REQUIRE(false, PGX_EINVAL, "%s: contig %u segment %u: read %u is not in the idx", who, h_pieces[e.piece].ctg, h_pieces[e.piece].seg, e.read);
  }
  const double t1 = wall_ms();
  js.layout_ms = t1 - t0;
  // the inner loop, batch by batch; the segments wait on the device
  std::vector<CnsPiecesDev> outs;
  std::vector<uint32_t> starts;
  const uint32_t hook = batch_hook();
  uint64_t seg_total = 0;
  for (uint32_t p0 = 0; p0 < np;) {
    uint32_t p1;
    if (hook) {
      p1 = std::min(np, p0 + hook);
    } else {   // the pieces whose cost, counted from p0, stays within the cap; one at least
      p1 = (uint32_t)(std::upper_bound(h_cost.begin() + p0 + 1, h_cost.end(), h_cost[p0] + COST_CAP) - h_cost.begin()) - 1;
      p1 = std::min(std::max(p1, p0 + 1), p0 + MAX_BATCH_PIECES);
    }
    const uint32_t e0 = h_pieces[p0].read_first, e1 = p1 < np ? h_pieces[p1].read_first : nr;
    const uint32_t npb = p1 - p0, neb = e1 - e0, n_items = npb + neb;
    const uint64_t bytes = h_pool[p1] - h_pool[p0];
    const double b0 = wall_ms();
    DevBuf<Item> items(n_items);
    DevBuf<pgx_cns_piece> bp(npb);
    DevBuf<pgx_cns_read> br(neb ? neb : 1);
    DevBuf<uint8_t> pool(bytes + 16);
    PGX_HIP(hipMemsetAsync(pool.p + bytes, 0, 16, st));
    LAUNCH(k_job_items, n_items, pieces.p, reads.p, p0, p1, e0, e1, pool_cum.p, ent_cum.p, cdb->d_roff.p, rdb->d_roff.p, rdb->d_rlen.p, items.p, bp.p, br.p);
    LAUNCH(k_job_decode, cdiv(bytes, 16), items.p, n_items, cdb->d_seq.p, rdb->d_seq.p, bytes, pool.p);
    sync();
    const double b1 = wall_ms();
    js.decode_ms += b1 - b0, js.pool_bytes += bytes;
    outs.emplace_back();
    starts.push_back(p0);
    pgx_cns_pieces_stats ps = {};
    try {
      cns_pieces_dev(who, bp.p, npb, br.p, neb, pool.p, bytes, 1, outs.back(), &ps, p0);
    } catch (const Fail &f) {
      rethrow_named(f, h_pieces);
    }
    js.pieces_ms += wall_ms() - b1;
    js.n_accepted += ps.n_accepted, js.n_by_rule += ps.n_by_rule, js.n_called += ps.n_called, ++js.n_batches;
    js.align.n_req += ps.align.n_req, js.align.n_aligned += ps.align.n_aligned, js.align.n_cells += ps.align.n_cells, js.align.str_bytes += ps.align.str_bytes;
    js.align.gpu_ms += ps.align.gpu_ms, js.align.count_ms += ps.align.count_ms, js.align.fill_ms += ps.align.fill_ms, js.align.back_ms += ps.align.back_ms;
    js.call.n_aln += ps.call.n_aln, js.call.n_tags += ps.call.n_tags, js.call.n_edges += ps.call.n_edges, js.call.n_nodes += ps.call.n_nodes;
    js.call.text_bytes += ps.call.text_bytes, js.call.gpu_ms += ps.call.gpu_ms, js.call.tags_ms += ps.call.tags_ms, js.call.sort_ms += ps.call.sort_ms;
    js.call.score_ms += ps.call.score_ms, js.call.back_ms += ps.call.back_ms;
    seg_total += outs.back().total;
    p0 = p1;
  }
  const double t2 = wall_ms();
  // the segments in one text, the stitch
  DevBuf<char> seg_text(seg_total + 16);
  DevBuf<uint64_t> seg_off(np + 1);
  PGX_HIP(hipMemsetAsync(seg_text.p + seg_total, 0, 16, st));
  uint64_t base = 0;
  for (size_t b = 0; b < outs.size(); ++b) {
    const uint32_t p0 = starts[b], npb = (b + 1 < outs.size() ? starts[b + 1] : np) - p0;
    if (outs[b].total) PGX_HIP(hipMemcpyAsync(seg_text.p + base, outs[b].text.p, outs[b].total, hipMemcpyDeviceToDevice, st));
    LAUNCH(k_job_add_base, npb + 1, outs[b].off.p, npb + 1, base, seg_off.p + p0);
    base += outs[b].total;
  }
  DevBuf<pgx_faln_req> reqs(np);
  LAUNCH(k_st_reqs, np, pieces.p, np, seg_off.p, reqs.p, err.p);
  err.download(h, J_SLOTS);
  sync();
  outs.clear();
  if (h[J_STITCH] != UINT32_MAX) {
    uint64_t o[3];
    PGX_HIP(hipMemcpyAsync(o, seg_off.p + h[J_STITCH] - 1, sizeof(o), hipMemcpyDeviceToHost, st));
    sync();
    PGX_REQUIRE(false, PGX_EINVAL, "%s: contig %u segment %u: a stitch of %llu bytes against %llu (the script reads 1000 and 1050)", who, h_pieces[h[J_STITCH]].ctg,
                h_pieces[h[J_STITCH]].seg, (unsigned long long)(o[1] - o[0]), (unsigned long long)(o[2] - o[1]));
  }
  FalnOut fo;
  pgx_faln_stats fs = {};
  faln_dev(who, reqs.p, np, (const uint8_t *)seg_text.p, STITCH_BAND, fo, &fs);
  js.align.n_req += fs.n_req, js.align.n_aligned += fs.n_aligned, js.align.gpu_ms += fs.gpu_ms, js.align.count_ms += fs.count_ms;
  DevBuf<uint32_t> from(np), kept(np), out_len(np), first_piece(np);
  DevBuf<uint8_t> is_first(np);
  DevBuf<uint64_t> poff(np + 1);
  LAUNCH(k_st_keep, np, pieces.p, np, seg_off.p, fo.res.p, names.off.p, from.p, kept.p, out_len.p, is_first.p);
  const uint64_t n_bytes = scan_to_total(out_len.p, poff.p, np, &ws);
  const uint32_t n_used = select_indices(is_first.p, np, first_piece.p, &ws);
  d_text.alloc(n_bytes + 16);
  LAUNCH(k_job_fasta, cdiv(n_bytes, 16), pieces.p, np, poff.p, seg_off.p, seg_text.p, from.p, kept.p, names.text.p, names.off.p, n_bytes, d_text.p);
  d_ctg_off.alloc(n_used + 1);
  LAUNCH(k_job_ctg_off, n_used + 1, first_piece.p, n_used, poff.p, np, d_ctg_off.p);
  sync();
  js.stitch_ms = wall_ms() - t2;
  js.n_contigs = n_used, js.text_bytes = n_bytes, js.total_ms = wall_ms() - t0;
  *total = n_bytes, *n_out = n_used;
  if (stats) *stats = js;
}

static void upload_names(const char *who, const char *ctg_names, const uint64_t *name_off, size_t n_names, JobNames &out) {
  PGX_REQUIRE(n_names == 0 || (name_off && (ctg_names || name_off[n_names] == 0)), PGX_EARG, "%s: null argument", who);
  const uint64_t bytes = n_names ? name_off[n_names] : 0;
  out.n = n_names;
  out.text.alloc(bytes ? bytes : 1);
  out.off.alloc(n_names + 1);
  if (bytes) PGX_HIP(hipMemcpyAsync(out.text.p, ctg_names, bytes, hipMemcpyHostToDevice, ctx().stream));
  if (n_names) out.off.upload(name_off, n_names + 1);
  else PGX_HIP(hipMemsetAsync(out.off.p, 0, sizeof(uint64_t), ctx().stream));
}

// the text and the offsets to the caller's memory
static void job_hand_out(const DevBuf<char> &d_text, uint64_t total, const DevBuf<uint64_t> &d_ctg_off, uint64_t n_out, char **text, uint64_t **ctg_off) {
  char *t = caller_text(nullptr, total);
  uint64_t *o = (uint64_t *)malloc((n_out + 1) * sizeof(uint64_t));
  try {
    if (!o) throw std::bad_alloc();
    if (total) PGX_HIP(hipMemcpyAsync(t, d_text.p, total, hipMemcpyDeviceToHost, ctx().stream));
    d_ctg_off.download(o, n_out + 1);
    sync();
  } catch (...) {
    free(t), free(o);
    throw;
  }
  *text = t, *ctg_off = o;
}

}  // namespace pgx

using namespace pgx;

extern "C" {

int pgx_cns_layout(const int64_t *rows, size_t n_rows, const int64_t *ctg_len, size_t n_ctg, pgx_cns_job_piece **pieces, uint64_t *n_piece, pgx_cns_job_read **reads,
                   uint64_t *n_read) {
  return guarded([&] {
    require_ready();
    const char *who = "pgx_cns_layout";
    PGX_REQUIRE(pieces && n_piece && reads && n_read && (n_rows == 0 || rows) && (n_ctg == 0 || ctg_len), PGX_EARG, "%s: null argument", who);
    PGX_REQUIRE(n_rows < (1ull << 31) && n_ctg < (1ull << 32), PGX_EARG, "%s: too many rows or contigs for one call", who);
    *pieces = nullptr, *reads = nullptr, *n_piece = *n_read = 0;
    size_t np = 0, nr = 0;
    DevBuf<pgx_cns_job_piece> d_pieces;
    DevBuf<pgx_cns_job_read> d_reads;
    if (n_rows) {
      MemTag mem_tag("cns.job");
      DevBuf<int64_t> d_rows(n_rows * 9), d_len(n_ctg);
      d_rows.upload(rows, n_rows * 9);
      d_len.upload(ctg_len, n_ctg);
      cns_layout_dev(who, d_rows.p, n_rows, d_len.p, n_ctg, d_pieces, &np, d_reads, &nr);
    }
    pgx_cns_job_piece *op = (pgx_cns_job_piece *)out_alloc(np ? np * sizeof(pgx_cns_job_piece) : 1);
    pgx_cns_job_read *orr = nullptr;
    try {
      orr = (pgx_cns_job_read *)out_alloc(nr ? nr * sizeof(pgx_cns_job_read) : 1);
      d_pieces.download(op, np);
      d_reads.download(orr, nr);
      sync();
    } catch (...) {
      out_free(op), out_free(orr);
      throw;
    }
    *pieces = op, *reads = orr, *n_piece = np, *n_read = nr;
  });
}

int pgx_cns_job_resident(pgx_seqdb *reads, pgx_seqdb *ref, const int64_t *rows, size_t n_rows, uint32_t total_chunks, uint32_t my_chunk, const char *ctg_names,
                         const uint64_t *ctg_name_off, size_t n_names, char **text, uint64_t **ctg_off, uint64_t *n_ctg, uint64_t *text_len, pgx_cns_job_stats *stats) {
  return guarded([&] {
    require_ready();
    const char *who = "pgx_cns_job_resident";
    PGX_REQUIRE(reads && ref && text && ctg_off && n_ctg && text_len && (n_rows == 0 || rows), PGX_EARG, "%s: null argument", who);
    PGX_REQUIRE(n_rows < (1ull << 31), PGX_EARG, "%s: too many rows for one call", who);
    *text = nullptr, *ctg_off = nullptr, *n_ctg = *text_len = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    PGX_REQUIRE(total_chunks != 0, PGX_EINVAL, "%s: total_chunks == 0", who);
    MemTag mem_tag("cns.job");
    hipStream_t st = ctx().stream;
    JobNames names;
    upload_names(who, ctg_names, ctg_name_off, n_names, names);
    const uint32_t n = (uint32_t)n_rows;
    DevBuf<int64_t> d_rows(n_rows * 9), kept_rows;
    DevBuf<uint32_t> list(n ? n : 1), row_name;
    uint32_t m = 0;
    if (n) {
      DevBuf<uint8_t> keep(n);
      d_rows.upload(rows, n_rows * 9);
      LAUNCH(k_job_filter, n, d_rows.p, n, total_chunks, my_chunk, keep.p);
      m = select_indices(keep.p, n, list.p);
      kept_rows.alloc((size_t)m * 9 + 1), row_name.alloc(m + 1);
      if (m) LAUNCH(k_job_take_rows, (size_t)m * 9, d_rows.p, list.p, m, 0u, kept_rows.p, row_name.p);
    }
    DevBuf<char> d_text;
    DevBuf<uint64_t> d_off;
    uint64_t total = 0, n_out = 0;
    cns_job_dev(who, reads, ref, kept_rows.p, m, row_name.p, "row", names, d_text, &total, d_off, &n_out, stats);
    job_hand_out(d_text, total, d_off, n_out, text, ctg_off);
    *n_ctg = n_out, *text_len = total;
  });
}

namespace {
struct DbHandle {
  pgx_seqdb *db = nullptr;
  ~DbHandle() {
    if (db) pgx_seqdb_free(db);
  }
};
struct FileHandle {
  FILE *f = nullptr;
  bool own = true;
  ~FileHandle() {
    if (f && own) fclose(f);
  }
};
// the names of an idx file by id: `id name length offset` a line
void idx_names(const char *who, const std::string &path, std::string &text, std::vector<uint64_t> &off) {
  std::vector<uint8_t> raw;
  PGX_REQUIRE(read_file(path, raw), PGX_EIO, "%s: cannot read %s", who, path.c_str());
  std::vector<std::pair<uint64_t, std::pair<size_t, size_t>>> found;   // id, (start, length) of the name
  size_t i = 0;
  uint64_t top = 0;
  while (i < raw.size()) {
    size_t e = i;
    while (e < raw.size() && raw[e] != '\n') ++e;
    size_t a = i;
    while (a < e && is_blank(raw[a])) ++a;
    size_t b = a;
    uint64_t id = 0;
    while (b < e && raw[b] >= '0' && raw[b] <= '9') id = id * 10 + (raw[b] - '0'), ++b;
    size_t c = b;
    while (c < e && is_blank(raw[c])) ++c;
    size_t d = c;
    while (d < e && !is_blank(raw[d])) ++d;
    if (b > a && d > c) found.push_back({id, {c, d - c}}), top = std::max(top, id + 1);
    i = e + 1;
  }
  PGX_REQUIRE(top < (1ull << 32), PGX_EINVAL, "%s: %s holds an id beyond 32 bits", who, path.c_str());
  std::vector<std::pair<size_t, size_t>> by_id(top, {0, 0});
  for (const auto &f : found) by_id[f.first] = f.second;
  off.assign(top + 1, 0);
  for (uint64_t k = 0; k < top; ++k) {
    text.append((const char *)raw.data() + by_id[k].first, by_id[k].second);
    off[k + 1] = text.size();
  }
}
}  // namespace

int pgx_cns_job(const char *read_db_prefix, const char *ref_db_prefix, const char *map_path, uint32_t total_chunks, uint32_t my_chunk, const char *out_path,
                pgx_cns_job_stats *stats) {
  return guarded([&] {
    require_ready();
    const char *who = "pgx_cns_job";
    PGX_REQUIRE(read_db_prefix && ref_db_prefix && map_path, PGX_EARG, "%s: null argument", who);
    if (stats) memset(stats, 0, sizeof(*stats));
    PGX_REQUIRE(total_chunks != 0, PGX_EINVAL, "%s: total_chunks == 0", who);
    hipStream_t st = ctx().stream;
    DbHandle rdb, cdb;
    int rc = pgx_seqdb_load(read_db_prefix, &rdb.db);
    if (rc == PGX_OK) rc = pgx_seqdb_load(ref_db_prefix, &cdb.db);
    if (rc != PGX_OK) throw Fail{rc};
    std::string name_text;
    std::vector<uint64_t> name_off;
    idx_names(who, std::string(ref_db_prefix) + ".idx", name_text, name_off);
    MemTag mem_tag("cns.job");
    JobNames names;
    upload_names(who, name_text.data(), name_off.data(), name_off.size() - 1, names);
    // the map text to rows, in bounded pieces of the file that end at a line's end
    FileHandle in;
    in.f = fopen(map_path, "rb");
    PGX_REQUIRE(in.f, PGX_EIO, "%s: cannot open %s", who, map_path);
    const char *pe = getenv("PGX_CNS_JOB_MAP_PIECE");
    const size_t piece = pe && atol(pe) > 0 ? (size_t)atol(pe) : (size_t)64 << 20;
    std::vector<char> buf;
    std::vector<DevBuf<int64_t>> row_parts;
    std::vector<DevBuf<uint32_t>> name_parts;
    std::vector<uint32_t> part_n;
    uint64_t lines_before = 0, kept = 0;
    bool eof = false;
    PrimWs ws;
    while (!eof) {
      const size_t had = buf.size();
      buf.resize(had + piece);
      const size_t got = fread(buf.data() + had, 1, piece, in.f);
      PGX_REQUIRE(got == piece || !ferror(in.f), PGX_EIO, "%s: cannot read %s", who, map_path);
      buf.resize(had + got);
      eof = got < piece;
      if (eof && !buf.empty() && buf.back() != '\n') buf.push_back('\n');
      const char *last = buf.empty() ? nullptr : (const char *)memrchr(buf.data(), '\n', buf.size());
      if (!last) continue;   // (a line longer than a piece: read on)
      const size_t nb = (size_t)(last - buf.data()) + 1;
      PGX_REQUIRE(nb < (1ull << 31), PGX_EARG, "%s: a piece of %s of 2^31 bytes and more", who, map_path);
      const uint32_t n = (uint32_t)nb;
      DevBuf<char> d_text(n);
      DevBuf<uint8_t> flag(n);
      DevBuf<uint32_t> nlpos(n), err(1);
      PGX_HIP(hipMemcpyAsync(d_text.p, buf.data(), n, hipMemcpyHostToDevice, st));
      PGX_HIP(hipMemsetAsync(err.p, 0xFF, sizeof(uint32_t), st));
      LAUNCH(k_par_newlines, n, d_text.p, n, flag.p);
      const uint32_t nl = select_indices(flag.p, n, nlpos.p, &ws);
      PGX_REQUIRE(lines_before + nl < (1ull << 32), PGX_EARG, "%s: %s has 2^32 lines and more", who, map_path);
      DevBuf<int64_t> rows((size_t)nl * 9);
      DevBuf<uint8_t> keep(nl), code(nl);
      DevBuf<uint32_t> list(nl);
      LAUNCH(k_par_lines, nl, d_text.p, nlpos.p, nl, total_chunks, my_chunk, rows.p, keep.p, code.p, err.p);
      uint32_t bad = 0;
      err.download(&bad, 1);
      sync();
      if (bad != UINT32_MAX) {
        uint8_t why = 0;
        PGX_HIP(hipMemcpyAsync(&why, code.p + bad, 1, hipMemcpyDeviceToHost, st));
        sync();
        PGX_REQUIRE(false, PGX_EINVAL, "%s: line %llu of %s %s", who, (unsigned long long)(lines_before + bad + 1), map_path, P_TEXT[why < 5 ? why : 0]);
      }
      const uint32_t m = select_indices(keep.p, nl, list.p, &ws);
      if (m) {
        row_parts.emplace_back((size_t)m * 9);
        name_parts.emplace_back(m);
        part_n.push_back(m);
        LAUNCH(k_job_take_rows, (size_t)m * 9, rows.p, list.p, m, (uint32_t)(lines_before + 1), row_parts.back().p, name_parts.back().p);
        sync();   // (rows and list go back to the block cache with this scope)
      }
      kept += m, lines_before += nl;
      buf.erase(buf.begin(), buf.begin() + nb);
    }
    PGX_REQUIRE(buf.empty(), PGX_EIO, "%s: %s: a last line without an end", who, map_path);
    PGX_REQUIRE(kept < (1ull << 31), PGX_EARG, "%s: %llu rows in the chunk are too many for one call", who, (unsigned long long)kept);
    DevBuf<int64_t> d_rows(kept * 9 + 1);
    DevBuf<uint32_t> d_names(kept + 1);
    uint64_t at = 0;
    for (size_t k = 0; k < row_parts.size(); ++k) {
      PGX_HIP(hipMemcpyAsync(d_rows.p + at * 9, row_parts[k].p, (size_t)part_n[k] * 9 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
      PGX_HIP(hipMemcpyAsync(d_names.p + at, name_parts[k].p, (size_t)part_n[k] * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
      at += part_n[k];
    }
    sync();
    row_parts.clear(), name_parts.clear();
    DevBuf<char> d_text;
    DevBuf<uint64_t> d_off;
    uint64_t total = 0, n_out = 0;
    cns_job_dev(who, rdb.db, cdb.db, d_rows.p, kept, d_names.p, "line", names, d_text, &total, d_off, &n_out, stats);
    char *text = nullptr;
    uint64_t *off = nullptr;
    job_hand_out(d_text, total, d_off, n_out, &text, &off);
    FileHandle out;
    out.f = out_path ? fopen(out_path, "wb") : stdout, out.own = out_path != nullptr;
    const bool ok = out.f && fwrite(text, 1, total, out.f) == total && fflush(out.f) == 0;
    free(text), free(off);
    PGX_REQUIRE(ok, PGX_EIO, "%s: cannot write %s", who, out_path ? out_path : "stdout");
  });
}

}  // extern "C"
