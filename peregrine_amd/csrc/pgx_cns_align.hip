// pgx_cns_align.hip -- falcon.align (the reference's falcon/DW_banded.c:104-315), the banded O(ND) aligner WITH trace-back that
// pg_asm_cns.py runs for every read of every piece, for a batch of requests over one pool of bytes; and pgx_cns_pieces, the script's
// inner loop (py/scripts/pg_asm_cns.py:143-244) for a batch of pieces: aligner, acceptance rule and consensus call (pgx_cns.hip) without
// the alignment strings leaving the device.  The rule and the trace layout: DESIGN.md section 4.7a.
//
//   k_faln_front<false>  a wavefront per request runs the front (lanes over the band's diagonals, V as an LDS ring, long snakes extended
//                        by the whole wavefront 8 bytes per lane and iteration) and stores nothing but the answer and three counts:
//                        the rows (d-steps), the cells (visited (d, k)) and the columns its strings will have
//   scans                the three counts to offsets: every array below is sized by what the device counted
//   k_faln_front<true>   the same front once more, for the requests that aligned and want strings, storing per cell the snake's end and
//                        whether the step came from diagonal k + 1 (x2 << 1 | from_above), per row {min_k, first cell}
//   k_faln_back          a wavefront per request: 64 steps of the path at a time from the end cell back to d = 0 (one dependent load per
//                        step: the cell a step came from is also where its snake began), the steps' column counts scanned across the
//                        lanes, then the columns: an indel column and a snake per step, snakes longer than SNAKE_OWN by the whole wavefront
//   k_cp_*               pgx_cns_pieces: requests from pieces and reads, the acceptance rule, the rows of the consensus call
#include "pgx_internal.h"

namespace pgx {
namespace {

constexpr uint32_t MAX_BAND = 4096;   // V ring of 2 * band + 4 slots rounded up to a power of two: 16,384 slots, 64 KiB of LDS
constexpr int SNAKE_OWN = 8;          // a snake of at most this many columns is written by the lane that holds its step
constexpr uint32_t CP_BACKBONE_BAND = 50, CP_READ_BAND = 150;
constexpr int32_t CP_ACCEPT = 48;
enum { F_RANGE, F_LEN, F_BAND, F_PIECE_RANGE, F_TLEN, F_READ_PIECE, F_STORE, F_SLOTS };
enum { C_ALIGNED, C_MAX_BAND, C_ACCEPTED, C_SLOTS };

__device__ __forceinline__ uint64_t load8(const uint8_t *p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}
// how many of the 8 bytes at a and at b are equal from the first on
__device__ __forceinline__ int match8b(const uint8_t *a, const uint8_t *b) {
  const uint64_t diff = load8(a) ^ load8(b);
  return diff ? (__builtin_ctzll(diff) >> 3) : 8;
}
__device__ __forceinline__ uint64_t ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ int wave_max(int v) {
  for (int s = 32; s; s >>= 1) v = max(v, __shfl_xor(v, s));
  return v;
}

// the requests as given: the smallest offender per condition, the widest band
__global__ void k_faln_check(const pgx_faln_req *reqs, uint32_t n, uint64_t seq_bytes, uint32_t *err, uint32_t *ctr) {
  const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n) return;
  const pgx_faln_req r = reqs[a];
  if (r.q_off > seq_bytes || r.q_len > seq_bytes - r.q_off || r.t_off > seq_bytes || r.t_len > seq_bytes - r.t_off) atomicMin(&err[F_RANGE], a);
  else if ((uint64_t)r.q_len + r.t_len >= (1ull << 31)) atomicMin(&err[F_LEN], a);
  else if (r.band > MAX_BAND) atomicMin(&err[F_BAND], a);
  else atomicMax(&ctr[C_MAX_BAND], r.band);
}

// One wavefront per request.  FILL == false: res[a] (str_off left 0) and the counts nrow / ncell / ncol (all 0 unless it aligned and wants
// strings).  FILL == true, for the requests that have cells: the same front, storing cells[] and rows[] inside the counted ranges, and
// res[a].str_off.  Both are the same deterministic code on the same bytes, so the counts of the first bound the stores of the second;
// a store outside them is skipped and reported (err[F_STORE]).
template <bool FILL>
__global__ __launch_bounds__(64) void k_faln_front(const pgx_faln_req *__restrict__ reqs, uint32_t n, const uint8_t *__restrict__ seq, int ring,
                                                  pgx_faln_res *res, uint64_t *nrow, uint64_t *ncell, uint64_t *ncol, const uint64_t *row_off,
                                                  const uint64_t *cell_off, const uint64_t *col_off, uint32_t *cells, int2 *rows, uint32_t *err, uint32_t *ctr) {
  extern __shared__ int32_t V[];
  const uint32_t a = blockIdx.x;
  const int lane = threadIdx.x;
  const pgx_faln_req rq = reqs[a];
  uint64_t cell_base = 0, cell_n = 0, row_base = 0, row_n = 0;
  if (FILL) {
    cell_base = cell_off[a], cell_n = cell_off[a + 1] - cell_base;
    row_base = row_off[a], row_n = row_off[a + 1] - row_base;
    if (lane == 0) res[a].str_off = col_off[a + 1] > col_off[a] ? col_off[a] : 0;
    if (cell_n == 0) return;
  }
  const uint8_t *q = seq + rq.q_off, *t = seq + rq.t_off;
  const int q_len = (int)rq.q_len, t_len = (int)rq.t_len, band = (int)rq.band;
  const int max_d = (q_len == 0 || t_len == 0) ? 0 : (int)(0.3 * (double)(q_len + t_len));   // DW_banded.c:138, one IEEE double multiply
  const int band_size = band * 2;
  const int mask = ring - 1;
  for (int i = lane; i < ring; i += 64) V[i] = 0;
  __syncthreads();

  int best_m = -1, min_k = 0, max_k = 0;
  bool matched = false;
  int q_end = 0, t_end = 0, dist = 0;
  uint64_t n_cells = 0;
  for (int d = 0; d < max_d; ++d) {
    if (max_k - min_k > band_size) break;
    const int nk = ((max_k - min_k) >> 1) + 1;
    if (FILL && lane == 0) {
      if ((uint64_t)d < row_n) rows[row_base + d] = make_int2(min_k, (int)(uint32_t)n_cells);
      else atomicMin(&err[F_STORE], a);
    }
    int x = 0, y = 0;
    for (int base = 0; base < nk && !matched; base += 64) {
      const int j = base + lane;
      const bool active = j < nk;
      const int k = min_k + 2 * j;
      bool more = false, from_above = false;
      x = 0, y = 0;
      if (active) {
        const int va = V[(k - 1) & mask], vb = V[(k + 1) & mask];
        from_above = k == min_k || (k != max_k && va < vb);
        x = from_above ? vb : va + 1;
        y = x - k;
        const int rem = min(q_len - x, t_len - y);
        if (rem > 0) {   // the probe: off the main diagonals a snake almost always ends inside it
          const int m = min(match8b(q + x, t + y), rem);
          x += m, y += m;
          more = m == 8 && rem > 8;
        }
      }
      uint64_t mm = ballot64(more);
      while (mm) {   // a long snake: 512 bytes per iteration by the whole wavefront
        const int L = __builtin_ctzll(mm);
        const int xs = __builtin_amdgcn_readlane(x, L), ys = __builtin_amdgcn_readlane(y, L);
        const int rem = min(q_len - xs, t_len - ys);   // > 0 by construction
        const int off = lane * 8;
        int m = 0;
        if (off < rem) m = min(match8b(q + xs + off, t + ys + off), rem - off);
        const uint64_t stop = ballot64(m < 8);
        int ext;
        if (stop) {
          const int f = __builtin_ctzll(stop);
          ext = 8 * f + __builtin_amdgcn_readlane(m, f);
        } else {
          ext = 512;
        }
        if (lane == L) x += ext, y += ext;
        if (stop || ext >= rem) mm &= mm - 1;
      }
      const bool hit = active && (x >= q_len || y >= t_len);
      const uint64_t hitmask = ballot64(hit);
      const int hl = hitmask ? __builtin_ctzll(hitmask) : 64;
      const bool valid = active && lane <= hl;   // the first diagonal, ascending, that reaches an end closes the row
      if (valid) V[k & mask] = x;
      if (FILL && valid) {
        const uint64_t c = n_cells + (uint32_t)lane;
        if (c < cell_n) cells[cell_base + c] = (uint32_t)x << 1 | (uint32_t)from_above;
        else atomicMin(&err[F_STORE], a);
      }
      n_cells += hitmask ? (uint32_t)hl + 1 : (uint32_t)min(64, nk - base);
      best_m = max(best_m, wave_max(valid ? x + y : -1));
      if (hitmask) {
        matched = true;
        q_end = __builtin_amdgcn_readlane(x, hl), t_end = __builtin_amdgcn_readlane(y, hl);
      }
    }
    __syncthreads();
    if (matched) {
      dist = d;
      break;
    }
    // the band for the next step (DW_banded.c:213-228)
    int new_min = max_k, new_max = min_k;
    const int thr = best_m - band;
    for (int base = 0; base < nk; base += 64) {
      const int j = base + lane;
      const int k2 = min_k + 2 * j;
      int u;
      if (nk <= 64) u = x + y;   // still in registers
      else u = j < nk ? 2 * V[k2 & mask] - k2 : 0;
      const uint64_t m = ballot64(j < nk && u >= thr);
      if (m) {
        new_min = min(new_min, min_k + 2 * (base + __builtin_ctzll(m)));
        new_max = max(new_max, min_k + 2 * (base + 63 - __builtin_clzll(m)));
      }
    }
    max_k = new_max + 1;
    min_k = new_min - 1;
  }
  if (FILL || lane != 0) return;
  pgx_faln_res r = {};
  const bool strings = matched && rq.want_str != 0;
  if (matched) {
    r.aln_str_size = (q_end + t_end + dist) / 2, r.dist = dist, r.aln_q_e = q_end, r.aln_t_e = t_end;
    atomicAdd(&ctr[C_ALIGNED], 1u);
  }
  res[a] = r;
  nrow[a] = strings ? (uint64_t)dist + 1 : 0;
  ncell[a] = strings ? n_cells : 0;
  ncol[a] = strings ? (uint64_t)r.aln_str_size : 0;   // an indel column per step and the snakes: (x + y + d) / 2
}

__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v, int lane) {
  for (int s = 1; s < 64; s <<= 1) {
    const uint32_t o = __shfl_up(v, s);
    if (lane >= s) v += o;
  }
  return v;
}

// One wavefront per request with cells: the path from the end cell (the last cell stored) back to d = 0, and the two strings.
// Step (d, k) came from diagonal k + 1 of row d - 1 (a template base against a gap) or from k - 1 (a read base against a gap); its snake
// begins at that cell's x2, plus one in the second case.  Lane i of a chunk holds the i-th step from the chunk's top.
__global__ __launch_bounds__(64) void k_faln_back(const pgx_faln_req *__restrict__ reqs, uint32_t n, const uint8_t *__restrict__ seq,
                                                 const pgx_faln_res *__restrict__ res, const uint64_t *__restrict__ row_off,
                                                 const uint64_t *__restrict__ cell_off, const uint64_t *__restrict__ col_off,
                                                 const uint32_t *__restrict__ cells, const int2 *__restrict__ rows, uint8_t *q_str, uint8_t *t_str, uint32_t *err) {
  const uint32_t a = blockIdx.x;
  const int lane = threadIdx.x;
  const uint64_t cell_base = cell_off[a], cell_n = cell_off[a + 1] - cell_base;
  if (cell_n == 0) return;
  const pgx_faln_req rq = reqs[a];
  const pgx_faln_res rs = res[a];
  const uint64_t row_base = row_off[a];
  const uint32_t total = (uint32_t)(col_off[a + 1] - col_off[a]);
  const uint8_t *q = seq + rq.q_off, *t = seq + rq.t_off;
  uint8_t *qs = q_str + col_off[a], *ts = t_str + col_off[a];
  int d = __builtin_amdgcn_readfirstlane(rs.dist), k = __builtin_amdgcn_readfirstlane(rs.aln_q_e - rs.aln_t_e);
  uint32_t c = __builtin_amdgcn_readfirstlane(cells[cell_base + cell_n - 1]);
  uint32_t pos_end = total;
  bool bad = false;
  while (d >= 0) {
    const int m = min(64, d + 1);
    int rmin = 0;
    uint32_t rfirst = 0;
    if (lane < m && d - 1 - lane >= 0) {   // the rows the chunk's steps came from
      const int2 r = rows[row_base + (uint64_t)(d - 1 - lane)];
      rmin = r.x, rfirst = (uint32_t)r.y;
    }
    int my_x1 = 0, my_k = 0, my_len = 0;
    bool my_indel = false, my_above = false;
    for (int i = 0; i < m; ++i) {
      const int x2 = (int)(c >> 1);
      const bool above = c & 1;
      const int pk = above ? k + 1 : k - 1;
      int x1 = 0;
      uint32_t cp = 0;
      if (d > 0) {
        const uint64_t idx = (uint64_t)__builtin_amdgcn_readlane(rfirst, i) + (uint32_t)((pk - __builtin_amdgcn_readlane(rmin, i)) >> 1);
        if (idx >= cell_n) {
          bad = true;
          break;
        }
        cp = __builtin_amdgcn_readfirstlane(lane == 0 ? cells[cell_base + idx] : 0u);
        x1 = (int)(cp >> 1) + (above ? 0 : 1);
      }
      if (lane == i) my_x1 = x1, my_k = k, my_len = x2 - x1, my_indel = d > 0, my_above = above;
      c = cp, k = pk, --d;
    }
    if (bad) break;
    const uint32_t cols = lane < m ? (uint32_t)my_len + (my_indel ? 1u : 0u) : 0u;
    const uint32_t incl = wave_inclusive_sum(cols, lane);
    const uint32_t chunk = __shfl(incl, 63);
    if (ballot64(my_len < 0) || chunk > pos_end) {
      bad = true;
      break;
    }
    uint32_t pos = pos_end - incl;   // this lane's first column
    pos_end -= chunk;
    const int y1 = my_x1 - my_k;
    if (lane < m && my_indel) {
      qs[pos] = my_above ? (uint8_t)'-' : q[my_x1 - 1];
      ts[pos] = my_above ? t[y1 - 1] : (uint8_t)'-';
      ++pos;
    }
    if (lane < m && my_len <= SNAKE_OWN)
      for (int i = 0; i < my_len; ++i) {
        const uint8_t b = q[my_x1 + i];
        qs[pos + i] = b, ts[pos + i] = b;   // (a snake's bytes are equal in both)
      }
    uint64_t longs = ballot64(lane < m && my_len > SNAKE_OWN);
    while (longs) {
      const int L = __builtin_ctzll(longs);
      longs &= longs - 1;
      const int xs = __builtin_amdgcn_readlane(my_x1, L), len = __builtin_amdgcn_readlane(my_len, L);
      const uint32_t ps = __builtin_amdgcn_readlane(pos, L);
      for (int off = lane; off < len; off += 64) {
        const uint8_t b = q[xs + off];
        qs[ps + off] = b, ts[ps + off] = b;
      }
    }
  }
  if ((bad || pos_end != 0) && lane == 0) atomicMin(&err[F_STORE], a);
}

struct Events {
  hipEvent_t e[5] = {};
  Events() {
    for (auto &x : e) PGX_HIP(hipEventCreate(&x));
  }
  ~Events() {
    for (auto &x : e)
      if (x) (void)hipEventDestroy(x);
  }
  void mark(int i) { PGX_HIP(hipEventRecord(e[i], ctx().stream)); }
  double ms(int a, int b) {
    float f = 0;
    PGX_HIP(hipEventElapsedTime(&f, e[a], e[b]));
    return f;
  }
};

// falcon.align for n > 0 requests in device memory over the device's copy of the pool (which has 16 bytes of padding behind it: a probe
// reads 8 bytes at a time).  max_band: the widest band among them.  err: F_SLOTS slots, set to 0xFF..; ctr: C_SLOTS counters, [C_ALIGNED] 0.
void faln_run(const char *who, const pgx_faln_req *d_reqs, size_t n, const uint8_t *d_seq, uint32_t max_band, uint32_t *d_err, uint32_t *d_ctr, FalnOut &out,
              pgx_faln_stats *stats) {
  hipStream_t st = ctx().stream;
  int ring = 64;
  while ((uint32_t)ring < 2 * max_band + 4) ring <<= 1;
  const size_t lds = (size_t)ring * sizeof(int32_t);
  const uint32_t nb = (uint32_t)n;
  Events ev;
  PrimWs ws;
  out.res.alloc(n);
  DevBuf<uint64_t> nrow(n), ncell(n), ncol(n), row_off(n + 1), cell_off(n + 1), col_off(n + 1);
  ev.mark(0);
  hipLaunchKernelGGL(k_faln_front<false>, dim3(nb), dim3(64), lds, st, d_reqs, nb, d_seq, ring, out.res.p, nrow.p, ncell.p, ncol.p, nullptr, nullptr, nullptr,
                     nullptr, nullptr, d_err, d_ctr);
  ev.mark(1);
  const uint64_t n_rows = scan_to_total(nrow.p, row_off.p, n, &ws);
  const uint64_t n_cells = scan_to_total(ncell.p, cell_off.p, n, &ws);
  const uint64_t n_cols = scan_to_total(ncol.p, col_off.p, n, &ws);
  DevBuf<uint32_t> cells(n_cells ? n_cells : 1);
  DevBuf<int2> rows(n_rows ? n_rows : 1);
  out.q_str.alloc(n_cols ? n_cols : 1);
  out.t_str.alloc(n_cols ? n_cols : 1);
  out.str_bytes = n_cols;
  ev.mark(2);
  hipLaunchKernelGGL(k_faln_front<true>, dim3(nb), dim3(64), lds, st, d_reqs, nb, d_seq, ring, out.res.p, nullptr, nullptr, nullptr, row_off.p, cell_off.p,
                     col_off.p, cells.p, rows.p, d_err, d_ctr);
  ev.mark(3);
  hipLaunchKernelGGL(k_faln_back, dim3(nb), dim3(64), 0, st, d_reqs, nb, d_seq, out.res.p, row_off.p, cell_off.p, col_off.p, cells.p, rows.p, out.q_str.p,
                     out.t_str.p, d_err);
  ev.mark(4);
  uint32_t h_err = 0, h_aligned = 0;
  PGX_HIP(hipMemcpyAsync(&h_err, d_err + F_STORE, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  PGX_HIP(hipMemcpyAsync(&h_aligned, d_ctr + C_ALIGNED, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  sync();
  PGX_REQUIRE(h_err == UINT32_MAX, PGX_EHIP, "%s: request %u: the filling pass left the trace the counting pass measured", who, h_err);
  if (stats) {
    stats->n_req = n, stats->n_aligned = h_aligned, stats->n_cells = n_cells, stats->str_bytes = n_cols;
    stats->count_ms = ev.ms(0, 1), stats->fill_ms = ev.ms(2, 3), stats->back_ms = ev.ms(3, 4), stats->gpu_ms = ev.ms(0, 4);
  }
}

void upload_pool(DevBuf<uint8_t> &d_seq, const char *seq, size_t seq_bytes) {
  d_seq.alloc(seq_bytes + 16);
  d_seq.upload((const uint8_t *)seq, seq_bytes);
  PGX_HIP(hipMemsetAsync(d_seq.p + seq_bytes, 0, 16, ctx().stream));
}

// ---- pgx_cns_pieces --------------------------------------------------------------------------------------------------------------------------
struct CpRow {   // per request: the piece, where its target begins in the piece, and what it is
  uint32_t piece;
  int32_t t_offset;
  uint32_t kind, q_len;   // q_len: the query as the acceptance rule sees it
};
enum { KIND_BACKBONE, KIND_NEG, KIND_POS, KIND_SKIP };

// request p < n_piece: the back-bone of piece p; request n_piece + r: read r ("the pieces")
__global__ void k_cp_reqs(const pgx_cns_piece *pieces, uint32_t n_piece, const pgx_cns_read *reads, uint32_t n_read, uint64_t seq_bytes, pgx_faln_req *reqs,
                          CpRow *meta, uint32_t *err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_piece + n_read) return;
  pgx_faln_req rq = {};
  CpRow m = {};
  m.kind = KIND_SKIP;
  if (i < n_piece) {
    const pgx_cns_piece pc = pieces[i];
    m.piece = i;
    if (pc.seq_off > seq_bytes || pc.t_len > seq_bytes - pc.seq_off || pc.t_len > (uint32_t)INT32_MAX / 2) atomicMin(&err[F_PIECE_RANGE], i);
    else if (pc.t_len == 0) atomicMin(&err[F_TLEN], i);
    else rq.q_off = rq.t_off = pc.seq_off, rq.q_len = rq.t_len = pc.t_len, rq.band = CP_BACKBONE_BAND, rq.want_str = 1, m.kind = KIND_BACKBONE, m.q_len = pc.t_len;
  } else {
    const uint32_t r = i - n_piece;
    const pgx_cns_read rd = reads[r];
    m.piece = rd.piece;
    if (rd.piece >= n_piece) {
      atomicMin(&err[F_READ_PIECE], r);
    } else if (rd.seq_off > seq_bytes || rd.seq_len > seq_bytes - rd.seq_off) {
      atomicMin(&err[F_RANGE], r);
    } else {
      const pgx_cns_piece pc = pieces[rd.piece];
      const int64_t shift = rd.read_shift;
      const int64_t q_len = shift < 0 ? (int64_t)rd.seq_len + shift : (int64_t)rd.seq_len;
      const int64_t t_len = shift < 0 ? (int64_t)pc.t_len : (int64_t)pc.t_len - shift;
      if (q_len > 0 && t_len > 0 && pc.seq_off <= seq_bytes && pc.t_len <= seq_bytes - pc.seq_off) {
        if (q_len + t_len >= (1ll << 31)) {
          atomicMin(&err[F_LEN], r);
        } else {
          rq.q_off = rd.seq_off + (uint64_t)(shift < 0 ? -shift : 0), rq.q_len = (uint32_t)q_len;
          rq.t_off = pc.seq_off + (uint64_t)(shift < 0 ? 0 : shift), rq.t_len = (uint32_t)t_len;
          rq.band = CP_READ_BAND, rq.want_str = 1;
          m.kind = shift < 0 ? KIND_NEG : KIND_POS, m.t_offset = shift < 0 ? 0 : (int32_t)shift, m.q_len = (uint32_t)q_len;
        }
      }
    }
  }
  reqs[i] = rq, meta[i] = m;
}

// the acceptance rule of pg_asm_cns.py:189-216 and the row of the consensus call of every request: keep[i] = the row is the back-bone's
// or an accepted read's
__global__ void k_cp_accept(const pgx_faln_res *res, const CpRow *meta, uint32_t n_piece, uint32_t n_read, pgx_cns_aln *alns, uint8_t *keep, uint8_t *used,
                            unsigned long long *aln_base, uint32_t *ctr) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_piece + n_read) return;
  const pgx_faln_res r = res[i];
  const CpRow m = meta[i];
  bool ok = m.kind == KIND_BACKBONE;
  if (m.kind == KIND_NEG || m.kind == KIND_POS) {
    const int64_t q_e = r.aln_q_e, d1 = q_e - (int64_t)m.q_len, d2 = (int64_t)meta[m.piece].q_len - m.t_offset - q_e;
    ok = (d1 < 0 ? -d1 : d1) < CP_ACCEPT;
    // ... or the QUERY span against what is left of the target (meta[piece]: the back-bone's row), as the script compares them
    if (m.kind == KIND_POS && !ok) ok = (d2 < 0 ? -d2 : d2) < CP_ACCEPT;
    used[i - n_piece] = ok;
    if (ok) atomicAdd(&aln_base[m.piece], (unsigned long long)r.aln_t_e), atomicAdd(&ctr[C_ACCEPTED], 1u);
  } else if (m.kind == KIND_SKIP && i >= n_piece) {
    used[i - n_piece] = 0;
  }
  pgx_cns_aln al = {};
  al.piece = m.piece, al.t_offset = m.t_offset, al.str_off = r.str_off, al.str_len = ok ? (uint32_t)r.aln_str_size : 0u;
  alns[i] = al;
  keep[i] = ok;
}
// the rows of the pieces that enter the call, renumbered: call_no[p] = piece p's number in the call, UINT32_MAX for none
__global__ void k_cp_renumber(pgx_cns_aln *alns, uint8_t *keep, uint32_t n, const uint32_t *call_no) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = call_no[alns[i].piece];
  if (c == UINT32_MAX) keep[i] = 0;
  else alns[i].piece = c;
}
__global__ void k_cp_gather(const pgx_cns_aln *in, const uint32_t *list, uint32_t n, pgx_cns_aln *out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[list[i]];
}

// which pieces enter the consensus call: those whose accepted reads cover 3 * t_len template bases and more (pg_asm_cns.py:235)
__global__ void k_cp_called(const pgx_cns_piece *pieces, const unsigned long long *aln_base, uint32_t np, uint8_t *called) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < np) called[p] = aln_base[p] >= 3ull * pieces[p].t_len;
}
__global__ void k_cp_call_tables(const uint32_t *call_piece, uint32_t n_call, const pgx_cns_piece *pieces, uint32_t name_base, uint32_t *call_no, uint32_t *call_tlen,
                                 uint32_t *call_name) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_call) return;
  const uint32_t p = call_piece[i];
  call_no[p] = i, call_tlen[i] = pieces[p].t_len, call_name[i] = name_base + p;
}
// the text: a piece of the call as the call answered it, the others their template through ASCII lower-casing
__global__ void k_cp_out_len(const pgx_cns_piece *pieces, const uint32_t *call_no, const uint64_t *c_off, uint32_t np, uint32_t *len) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= np) return;
  const uint32_t c = call_no[p];
  len[p] = c == UINT32_MAX ? pieces[p].t_len : (uint32_t)(c_off[c + 1] - c_off[c]);
}
// a thread per 16 bytes of the text (out has 16 bytes of room behind `total`): the piece by binary search of the offsets
__global__ void k_cp_out_text(const pgx_cns_piece *__restrict__ pieces, const uint32_t *__restrict__ call_no, const uint64_t *__restrict__ c_off,
                              const char *__restrict__ c_text, const uint8_t *__restrict__ seq, const uint64_t *__restrict__ off, uint32_t np, uint64_t total,
                              char *__restrict__ out) {
  const uint64_t at = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
  if (at >= total) return;
  uint32_t a = 0, b = np;   // the last piece that starts at or before `at` and is not empty there
  while (a < b) {
    const uint32_t mid = a + ((b - a) >> 1);
    if (off[mid + 1] <= at) a = mid + 1;
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
    while (off[p + 1] <= pos) ++p;   // (pos < total = off[np])
    const uint64_t x = pos - off[p];
    const uint32_t cn = call_no[p];
    char ch;
    if (cn == UINT32_MAX) {
      ch = (char)seq[pieces[p].seq_off + x];
      if (ch >= 'A' && ch <= 'Z') ch = (char)(ch + 32);
    } else {
      ch = c_text[c_off[cn] + x];
    }
    u.c[k] = ch;
  }
  *reinterpret_cast<uint4 *>(out + at) = u.v;
}

}  // namespace
void faln_dev(const char *who, const pgx_faln_req *d_reqs, size_t n, const uint8_t *d_seq, uint32_t max_band, FalnOut &out, pgx_faln_stats *stats) {
  hipStream_t st = ctx().stream;
  DevBuf<uint32_t> err(F_SLOTS), ctr(C_SLOTS);
  PGX_HIP(hipMemsetAsync(err.p, 0xFF, F_SLOTS * sizeof(uint32_t), st));
  PGX_HIP(hipMemsetAsync(ctr.p, 0, C_SLOTS * sizeof(uint32_t), st));
  faln_run(who, d_reqs, n, d_seq, max_band, err.p, ctr.p, out, stats);
}

// name_base: the caller's number of piece 0 (the refusals name name_base + p)
void cns_pieces_dev(const char *who, const pgx_cns_piece *d_pieces, uint32_t np, const pgx_cns_read *d_reads, uint32_t nr, const uint8_t *d_seq, uint64_t seq_bytes,
                    uint32_t min_cov, CnsPiecesDev &res, pgx_cns_pieces_stats *stats, uint32_t name_base) {
  hipStream_t st = ctx().stream;
  const uint32_t n = np + nr;
  DevBuf<uint8_t> keep(n), called(np);
  res.used.alloc(nr ? nr : 1);
  DevBuf<uint32_t> err(F_SLOTS), ctr(C_SLOTS);
  DevBuf<pgx_faln_req> d_reqs(n);
  DevBuf<CpRow> meta(n);
  DevBuf<pgx_cns_aln> alns(n);
  DevBuf<unsigned long long> aln_base(np);
  PGX_HIP(hipMemsetAsync(err.p, 0xFF, F_SLOTS * sizeof(uint32_t), st));
  PGX_HIP(hipMemsetAsync(ctr.p, 0, C_SLOTS * sizeof(uint32_t), st));
  PGX_HIP(hipMemsetAsync(aln_base.p, 0, np * sizeof(unsigned long long), st));
  LAUNCH(k_cp_reqs, n, d_pieces, np, d_reads, nr, seq_bytes, d_reqs.p, meta.p, err.p);
  uint32_t h[F_SLOTS];
  err.download(h, F_SLOTS);
  sync();
  PGX_REQUIRE_PIECE(h[F_PIECE_RANGE] == UINT32_MAX, PGX_EARG, name_base + h[F_PIECE_RANGE], "%s: piece %u lies outside the %zu bytes given (or is longer than 2^30)", who, name_base + h[F_PIECE_RANGE],
              (size_t)seq_bytes);
  PGX_REQUIRE(h[F_READ_PIECE] == UINT32_MAX, PGX_EARG, "%s: read %u names a piece beyond the %u given", who, h[F_READ_PIECE], np);
  PGX_REQUIRE(h[F_RANGE] == UINT32_MAX, PGX_EARG, "%s: read %u lies outside the %zu bytes given", who, h[F_RANGE], (size_t)seq_bytes);
  PGX_REQUIRE(h[F_LEN] == UINT32_MAX, PGX_EARG, "%s: read %u: query and target of 2^31 bytes and more together", who, h[F_LEN]);
  PGX_REQUIRE_PIECE(h[F_TLEN] == UINT32_MAX, PGX_EINVAL, name_base + h[F_TLEN], "%s: piece %u: a template of no bases", who, name_base + h[F_TLEN]);
  FalnOut out;
  pgx_faln_stats ast = {};
  faln_run(who, d_reqs.p, n, d_seq, CP_READ_BAND, err.p, ctr.p, out, &ast);
  LAUNCH(k_cp_accept, n, out.res.p, meta.p, np, nr, alns.p, keep.p, res.used.p, aln_base.p, ctr.p);
  // which pieces enter the call, their numbers in it, their template lengths (the call takes those from the host)
  PrimWs ws;
  DevBuf<uint32_t> call_piece(np), call_no(np), call_tlen(np), call_name(np);
  LAUNCH(k_cp_called, np, d_pieces, aln_base.p, np, called.p);
  PGX_HIP(hipMemsetAsync(call_no.p, 0xFF, np * sizeof(uint32_t), st));
  const uint32_t n_call = select_indices(called.p, np, call_piece.p, &ws);
  DevBuf<char> c_text;
  DevBuf<uint64_t> c_off(1);
  pgx_cns_stats cst = {};
  if (n_call) {
    LAUNCH(k_cp_call_tables, n_call, call_piece.p, n_call, d_pieces, name_base, call_no.p, call_tlen.p, call_name.p);
    std::vector<uint32_t> h_tlen(n_call), h_name(n_call);
    call_tlen.download(h_tlen.data(), n_call);
    call_name.download(h_name.data(), n_call);
    DevBuf<uint32_t> list(n);
    LAUNCH(k_cp_renumber, n, alns.p, keep.p, n, call_no.p);
    const uint32_t n_keep = select_indices(keep.p, n, list.p, &ws);   // (synchronises: the two downloads are there)
    DevBuf<pgx_cns_aln> rows(n_keep);
    if (n_keep) LAUNCH(k_cp_gather, n_keep, alns.p, list.p, n_keep, rows.p);
    cns_call_dev(who, rows.p, n_keep, out.q_str.p, out.t_str.p, out.str_bytes, h_tlen.data(), n_call, min_cov, nullptr, nullptr, &cst, h_name.data(), &c_text, &c_off);
  }
  DevBuf<uint32_t> len(np);
  res.off.alloc(np + 1);
  LAUNCH(k_cp_out_len, np, d_pieces, call_no.p, c_off.p, np, len.p);
  res.total = scan_to_total(len.p, res.off.p, np, &ws);
  res.text.alloc(res.total + 16);
  if (res.total) LAUNCH(k_cp_out_text, cdiv(res.total, 16), d_pieces, call_no.p, c_off.p, c_text.p, d_seq, res.off.p, np, res.total, res.text.p);
  uint32_t hc[C_SLOTS];
  ctr.download(hc, C_SLOTS);
  sync();
  if (stats) {
    stats->align = ast, stats->call = cst;
    stats->n_pieces = np, stats->n_reads = nr, stats->n_accepted = hc[C_ACCEPTED], stats->n_rejected = nr - hc[C_ACCEPTED];
    stats->n_by_rule = np - n_call, stats->n_called = n_call;
  }
}

}  // namespace pgx

using namespace pgx;

extern "C" {

int pgx_falcon_align(const pgx_faln_req *reqs, size_t n, const char *seq, size_t seq_bytes, pgx_faln_res *res, char **q_str, char **t_str,
                     uint64_t *str_bytes, pgx_faln_stats *stats) {
  return guarded([&] {
    require_ready();
    const char *who = "pgx_falcon_align";
    PGX_REQUIRE(q_str && t_str && str_bytes && (n == 0 || (reqs && res)) && (seq_bytes == 0 || seq), PGX_EARG, "%s: null argument", who);
    PGX_REQUIRE(n < (1ull << 31), PGX_EARG, "%s: too many requests for one call", who);
    *q_str = *t_str = nullptr, *str_bytes = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) {
      *q_str = caller_text(nullptr, 0), *t_str = caller_text(nullptr, 0);
      return;
    }
    MemTag mem_tag("cns.align");
    hipStream_t st = ctx().stream;
    DevBuf<pgx_faln_req> d_reqs(n);
    DevBuf<uint8_t> d_seq;
    DevBuf<uint32_t> err(F_SLOTS), ctr(C_SLOTS);
    d_reqs.upload(reqs, n);
    upload_pool(d_seq, seq, seq_bytes);
    PGX_HIP(hipMemsetAsync(err.p, 0xFF, F_SLOTS * sizeof(uint32_t), st));
    PGX_HIP(hipMemsetAsync(ctr.p, 0, C_SLOTS * sizeof(uint32_t), st));
    LAUNCH(k_faln_check, n, d_reqs.p, (uint32_t)n, (uint64_t)seq_bytes, err.p, ctr.p);
    uint32_t h[F_SLOTS], hc[C_SLOTS];
    err.download(h, F_SLOTS);
    ctr.download(hc, C_SLOTS);
    sync();
    PGX_REQUIRE(h[F_RANGE] == UINT32_MAX, PGX_EARG, "%s: request %u lies outside the %zu bytes given", who, h[F_RANGE], seq_bytes);
    PGX_REQUIRE(h[F_LEN] == UINT32_MAX, PGX_EARG, "%s: request %u: query and target of 2^31 bytes and more together", who, h[F_LEN]);
    PGX_REQUIRE(h[F_BAND] == UINT32_MAX, PGX_EARG, "%s: request %u: a band above %u", who, h[F_BAND], MAX_BAND);
    FalnOut out;
    faln_run(who, d_reqs.p, n, d_seq.p, hc[C_MAX_BAND], err.p, ctr.p, out, stats);
    char *qo = caller_text(nullptr, out.str_bytes), *to = nullptr;
    try {
      to = caller_text(nullptr, out.str_bytes);
      out.res.download(res, n);
      out.q_str.download((uint8_t *)qo, out.str_bytes);
      out.t_str.download((uint8_t *)to, out.str_bytes);
      sync();
    } catch (...) {
      free(qo), free(to);
      throw;
    }
    *q_str = qo, *t_str = to, *str_bytes = out.str_bytes;
  });
}

int pgx_cns_pieces(const pgx_cns_piece *pieces, size_t n_piece, const pgx_cns_read *reads, size_t n_read, const char *seq, size_t seq_bytes, uint32_t min_cov,
                   char **text, uint64_t *piece_off, uint8_t *read_used, pgx_cns_pieces_stats *stats) {
  return guarded([&] {
    require_ready();
    const char *who = "pgx_cns_pieces";
    PGX_REQUIRE(text && piece_off && (n_piece == 0 || pieces) && (n_read == 0 || reads) && (seq_bytes == 0 || seq), PGX_EARG, "%s: null argument", who);
    PGX_REQUIRE(n_piece <= (1u << 20), PGX_EARG, "%s: more than %u pieces in one call", who, 1u << 20);
    PGX_REQUIRE(n_read < (1ull << 31) - (1u << 20), PGX_EARG, "%s: too many reads for one call", who);
    *text = nullptr;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_piece == 0) {
      PGX_REQUIRE(n_read == 0, PGX_EARG, "%s: read 0 names a piece beyond the 0 given", who);
      *text = caller_text(nullptr, 0);
      piece_off[0] = 0;
      return;
    }
    MemTag mem_tag("cns.align");
    const uint32_t np = (uint32_t)n_piece, nr = (uint32_t)n_read;
    DevBuf<pgx_cns_piece> d_pieces(np);
    DevBuf<pgx_cns_read> d_reads(nr);
    DevBuf<uint8_t> d_seq;
    d_pieces.upload(pieces, np);
    d_reads.upload(reads, nr);
    upload_pool(d_seq, seq, seq_bytes);
    CnsPiecesDev out;
    cns_pieces_dev(who, d_pieces.p, np, d_reads.p, nr, d_seq.p, seq_bytes, min_cov, out, stats, 0);
    char *o = caller_text(nullptr, out.total);
    try {
      if (out.total) PGX_HIP(hipMemcpyAsync(o, out.text.p, out.total, hipMemcpyDeviceToHost, ctx().stream));
      out.off.download(piece_off, np + 1);
      if (read_used) out.used.download(read_used, nr);
      sync();
    } catch (...) {
      free(o);
      throw;
    }
    *text = o;
  });
}

}  // extern "C"
