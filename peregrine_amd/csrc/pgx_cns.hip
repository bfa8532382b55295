// pgx_cns.hip -- the consensus call of the reference's falcon/falcon.c (get_align_tags :67-122, get_cns_from_align_tags :277-397) for a
// batch of pieces: alignment strings in, one consensus per piece out, bit for bit.  The rule, restated in integers: DESIGN.md section 4.7.
//
//   k_cns_scan     a wavefront per alignment walks its columns 64 at a time (ballots + popcounts give every column its template position
//                  and its delta): first pass the number of tags (the cut at delta 255) and the refusals, second pass the tag rows
//                  (pgx_cns_tags) or the two sort keys of every tag and the coverage counts (pgx_cns_call)
//   sort           edges = runs of equal (piece, tag key, predecessor key): two stable radix sorts (pgx_prims.hip), head flags, selects
//   k_cns_edges    per edge: its count, its doubled score 2 * count - (coverage - 1), its predecessor's node (binary search among the
//                  piece's nodes before its own)
//   k_cns_score    a wavefront per piece walks its edges in sorted order, 64 loaded at a time, the state in scalar registers -- the rule is
//                  a chain through the template, and a batch has thousands of pieces to fill the device with -- keeping the scores of
//                  the last RING nodes in LDS (older ones: read back from memory)
//   k_cns_back     a wavefront per piece: the best edges back from the end node, a window of BACK_WIN nodes in LDS at a time; lane 0
//                  follows the links, all lanes turn the nodes it passed into bases
//   k_cns_text     every piece's bases, reversed, into one text
#include "pgx_internal.h"

namespace pgx {
namespace {

constexpr int PIECE_SHIFT = 43;                  // node key: piece << 43 | t_pos << 12 | delta << 4 | letter
constexpr uint32_t MAX_PIECES = 1u << 20;
constexpr uint32_t MAX_ALNS_PER_PIECE = 65535;   // the reference counts in uint16_t
constexpr int RING = 1024;                       // node scores k_cns_score keeps in LDS
constexpr int BACK_WIN = 2048;                   // nodes of a piece k_cns_back holds in LDS at a time
enum { E_BYTE, E_TPOS, E_OFFSET, E_PIECE, E_RANGE, E_MANY, E_NOEND, E_SLOTS };
enum { SCAN_COUNT, SCAN_TAGS, SCAN_KEYS };

// the letters of an alignment string in ASCII order: - . A C G N T a c g n t ('.' only ever as the predecessor of a first column)
__device__ __forceinline__ int letter_code(uint8_t b) {
  switch (b) {
    case '-': return 0;
    case '.': return 1;
    case 'A': return 2;
    case 'C': return 3;
    case 'G': return 4;
    case 'N': return 5;
    case 'T': return 6;
    case 'a': return 7;
    case 'c': return 8;
    case 'g': return 9;
    case 'n': return 10;
    case 't': return 11;
  }
  return -1;
}
__device__ __forceinline__ bool bad_letter(uint8_t b) { return letter_code(b) < 2 && b != '-'; }   // not one of ACGTNacgtn-
__device__ __forceinline__ uint8_t code_letter(uint32_t c) { return (uint8_t)("-.ACGNTacgnt"[c]); }

// One wavefront per alignment.  SCAN_COUNT: ntag[a] = the tags it yields (columns before the first with delta >= 255 or a negative template
// position), naln[piece] += 1, and the refusals into err[] (the smallest piece -- for rows that name no piece or no string, the smallest
// row -- per condition).  The other modes run on input that passed, take ntag[] as the length, and write what they are for.
template <int MODE>
__global__ __launch_bounds__(256) void k_cns_scan(const pgx_cns_aln *alns, uint32_t n_aln, const uint8_t *q_str, const uint8_t *t_str, uint64_t str_bytes,
                                                  const uint32_t *piece_tlen, uint32_t n_piece, uint32_t *ntag, uint32_t *naln, uint32_t *err,
                                                  const uint64_t *tag_off, pgx_cns_tag *tags, uint64_t *key_hi, uint64_t *key_lo,
                                                  const uint64_t *cov_off, uint32_t *cov) {
  const uint32_t a = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (a >= n_aln) return;
  const pgx_cns_aln al = alns[a];
  uint32_t n = al.str_len;
  int64_t t_len = INT32_MAX;
  if (MODE == SCAN_COUNT) {
    uint32_t bad = E_SLOTS;
    if (piece_tlen && al.piece >= n_piece) bad = E_PIECE;
    else if (al.str_off > str_bytes || al.str_len > str_bytes - al.str_off) bad = E_RANGE;
    else if (al.t_offset < 0) bad = E_OFFSET;
    if (bad != E_SLOTS) {
      if (lane == 0) atomicMin(&err[bad], bad == E_OFFSET ? al.piece : a), ntag[a] = 0;
      return;
    }
    if (lane == 0 && naln) atomicAdd(&naln[al.piece], 1u);
  } else {
    n = ntag[a];
  }
  if (piece_tlen) t_len = piece_tlen[al.piece];
  const uint8_t *q = q_str + al.str_off, *t = t_str + al.str_off;
  const uint64_t out0 = MODE == SCAN_COUNT ? 0 : tag_off[a];
  const uint64_t below = (2ull << lane) - 1;   // this lane's column and the ones before it
  uint32_t cut = n, seen_t = 0, carry_jj = 0;
  int32_t last_tpos = al.t_offset - 1;         // the previous chunk's last column, as a predecessor
  uint32_t last_jj = 0, last_q = '.';
  for (uint32_t base = 0; base < n; base += 64) {
    const uint32_t k = base + lane;
    const bool in = k < n;
    const uint8_t qb = in ? q[k] : (uint8_t)'-', tb = in ? t[k] : (uint8_t)'-';
    const uint64_t qm = __ballot(qb != '-'), tm = __ballot(tb != '-');
    const uint64_t lt = tm & below;
    uint32_t jj;
    if (lt == 0) {
      jj = carry_jj + (uint32_t)__popcll(qm & below);
    } else {
      const int h = 63 - __clzll((long long)lt);          // the last template base at or before this column
      jj = (uint32_t)__popcll(qm & below & ~((2ull << h) - 1));
    }
    const int64_t tpos = (int64_t)al.s2 - 1 + seen_t + __popcll(lt) + al.t_offset;
    if (MODE == SCAN_COUNT) {
      const uint64_t stop = __ballot(in && (jj >= 255 || tpos < 0));
      if (cut == n && stop) cut = base + (uint32_t)__ffsll((long long)stop) - 1;
      const uint64_t bad_byte = __ballot(in && (bad_letter(qb) || bad_letter(tb)));
      const uint64_t past = __ballot(in && k < cut && tpos >= t_len);
      if (lane == 0 && bad_byte) atomicMin(&err[E_BYTE], al.piece);
      if (lane == 0 && past) atomicMin(&err[E_TPOS], al.piece);
    } else {
      // the predecessor: the previous column (lane - 1, or what the previous chunk left), for column 0 (t_offset - 1, 0, '.')
      int32_t p_tpos = __shfl_up((int32_t)tpos, 1);
      uint32_t p_jj = __shfl_up(jj, 1), p_q = __shfl_up((uint32_t)qb, 1);
      if (lane == 0) p_tpos = last_tpos, p_jj = last_jj, p_q = last_q;
      last_tpos = __shfl((int32_t)tpos, 63), last_jj = __shfl(jj, 63), last_q = __shfl((uint32_t)qb, 63);
      if (in) {
        if (MODE == SCAN_TAGS) {
          tags[out0 + k] = pgx_cns_tag{(int32_t)tpos, p_tpos, (uint8_t)jj, qb, (uint8_t)p_jj, (uint8_t)p_q};
        } else {
          key_hi[out0 + k] = (uint64_t)al.piece << PIECE_SHIFT | (uint64_t)(uint32_t)tpos << 12 | (uint64_t)jj << 4 | (uint64_t)letter_code(qb);
          key_lo[out0 + k] = (uint64_t)(uint32_t)p_tpos << 12 | (uint64_t)p_jj << 4 | (uint64_t)letter_code((uint8_t)p_q);
          if (jj == 0) atomicAdd(&cov[cov_off[al.piece] + (uint64_t)tpos], 1u);
        }
      }
    }
    seen_t += (uint32_t)__popcll(tm);
    if (tm == 0) carry_jj += (uint32_t)__popcll(qm);
    else carry_jj = (uint32_t)__popcll(qm & ~((2ull << (63 - __clzll((long long)tm))) - 1));
  }
  if (MODE == SCAN_COUNT && lane == 0) ntag[a] = cut;
}

__global__ void k_cns_piece_check(const uint32_t *naln, uint32_t n_piece, uint32_t *err) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n_piece && naln[p] > MAX_ALNS_PER_PIECE) atomicMin(&err[E_MANY], p);
}
// hi, lo: the keys of the sorted tags.  An edge starts where either changes.
__global__ void k_cns_edge_heads(const uint64_t *hi, const uint64_t *lo, uint32_t n, uint8_t *flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flag[i] = i == 0 || hi[i] != hi[i - 1] || lo[i] != lo[i - 1];
}
// a node starts at the edge whose tag key differs from the edge before
__global__ void k_cns_node_heads(const uint64_t *hi, const uint32_t *estart, uint32_t n_edge, uint8_t *flag) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n_edge) flag[e] = e == 0 || hi[estart[e]] != hi[estart[e - 1]];
}
// per node: its key, and its index into every one of its edges
__global__ void k_cns_nodes(const uint64_t *hi, const uint32_t *estart, const uint32_t *nfirst, uint32_t n_node, uint32_t n_edge, uint64_t *node_key,
                            uint32_t *e_nid) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_node) return;
  const uint32_t e0 = nfirst[v], e1 = v + 1 < n_node ? nfirst[v + 1] : n_edge;
  node_key[v] = hi[estart[e0]];
  for (uint32_t e = e0; e < e1; ++e) e_nid[e] = v;
}
__device__ __forceinline__ uint32_t lower_bound_key(const uint64_t *keys, uint32_t lo, uint32_t hi, uint64_t key) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// pnode[p] = the first node of piece p (n_piece + 1 entries), pedge[p] = its first edge
__global__ void k_cns_piece_bounds(const uint64_t *node_key, const uint32_t *nfirst, uint32_t n_node, uint32_t n_edge, uint32_t n_piece, uint32_t *pnode,
                                   uint32_t *pedge) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > n_piece) return;
  const uint32_t v = lower_bound_key(node_key, 0, n_node, (uint64_t)p << PIECE_SHIFT);
  pnode[p] = v;
  pedge[p] = v < n_node ? nfirst[v] : n_edge;
}
// per edge: the doubled score of the rule's step 1 and the node of its predecessor (-1: the predecessor is the '.' of a first column)
__global__ void k_cns_edges(const uint64_t *hi, const uint64_t *lo, const uint32_t *estart, uint32_t n_edge, uint32_t n_tag, const uint32_t *e_nid,
                            const uint64_t *node_key, const uint32_t *pnode, const uint64_t *cov_off, const uint32_t *cov, int32_t *e_score,
                            int32_t *e_pred) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edge) return;
  const uint32_t i = estart[e], count = (e + 1 < n_edge ? estart[e + 1] : n_tag) - i;
  const uint64_t h = hi[i], l = lo[i];
  const uint32_t piece = (uint32_t)(h >> PIECE_SHIFT), tpos = (uint32_t)(h >> 12) & 0x7FFFFFFFu;
  e_score[e] = (int32_t)(2 * (int64_t)count - ((int64_t)cov[cov_off[piece] + tpos] - 1));
  int32_t pred = -1;
  if ((l & 15) != 1 && (l >> 43) == 0) {   // (a position of 2^31 and more is no node's)
    const uint64_t want = (uint64_t)piece << PIECE_SHIFT | l;
    const uint32_t v = lower_bound_key(node_key, pnode[piece], e_nid[e], want);
    if (v < e_nid[e] && node_key[v] == want) pred = (int32_t)v;
  }
  e_pred[e] = pred;
}

__device__ __forceinline__ int64_t first_lane64(int64_t x) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x), hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)x >> 32));
  return (int64_t)((uint64_t)hi << 32 | lo);
}
// One wavefront per piece: the scores of its nodes in edge order and the end node.  Every lane loads one of the next 64 edges; then the
// whole wavefront walks them in order with the state in scalar registers (an edge's fields come out of its lane by v_readlane), so that
// the chain costs scalar compares and, where the predecessor is not the node just closed, one read of the LDS ring.  Lane 0 stores.
__global__ __launch_bounds__(64) void k_cns_score(const uint32_t *pedge, const int32_t *e_score, const int32_t *e_pred, const uint32_t *e_nid, int64_t *node_best,
                                                 int32_t *node_via, int32_t *end_node, uint32_t *err) {
  __shared__ int64_t ring[RING];
  const uint32_t p = blockIdx.x, lane = threadIdx.x;
  const uint32_t e0 = pedge[p], e1 = pedge[p + 1];
  int64_t cur_best = 0, prev_best = 0, top = 0;   // prev_best: of node cur - 1, the node closed last
  int32_t cur = -1, cur_via = -1, end = -1;
  int32_t nx_score = 0, nx_pred = -1, nx_nid = 0;
  if (e0 + lane < e1) nx_score = e_score[e0 + lane], nx_pred = e_pred[e0 + lane], nx_nid = (int32_t)e_nid[e0 + lane];
  for (uint32_t base = e0; base < e1; base += 64) {
    const int32_t my_score = nx_score, my_pred = nx_pred, my_nid = nx_nid;
    if (base + 64 + lane < e1) nx_score = e_score[base + 64 + lane], nx_pred = e_pred[base + 64 + lane], nx_nid = (int32_t)e_nid[base + 64 + lane];
    const uint32_t m = min(64u, e1 - base);
    for (uint32_t i = 0; i < m; ++i) {
      const int32_t v = __builtin_amdgcn_readlane(my_nid, i), pred = __builtin_amdgcn_readlane(my_pred, i);
      const int64_t s = __builtin_amdgcn_readlane(my_score, i);
      if (v != cur) {   // the node's first edge: the node is made with this edge's own score, whatever precedes it
        if (cur >= 0) {
          if (lane == 0) node_best[cur] = cur_best, node_via[cur] = cur_via;
          ring[cur & (RING - 1)] = cur_best;   // (every lane the same value)
          prev_best = cur_best;
        }
        cur = v, cur_best = s, cur_via = pred;
      }
      if (pred < 0) continue;
      int64_t before;
      if (pred == cur - 1) before = prev_best;
      else if (cur - pred <= RING) before = first_lane64(ring[pred & (RING - 1)]);
      else before = first_lane64(lane == 0 ? node_best[pred] : 0);   // (the lane that stored it)
      const int64_t sum = s + before;
      if (sum > cur_best) {
        cur_best = sum, cur_via = pred;
        if (sum > top) top = sum, end = cur;
      }
    }
  }
  if (lane != 0) return;
  if (cur >= 0) node_best[cur] = cur_best, node_via[cur] = cur_via;
  if (end < 0) atomicMin(&err[E_NOEND], p);
  end_node[p] = end;
}

// One wavefront per piece: from the end node along the best edges, BACK_WIN nodes of node_via[] in LDS at a time (a predecessor has a smaller
// index): lane 0 follows the links inside the window and lists the nodes it passes, then all lanes turn the list into bases (rev[]: last
// base first, at most one per node of the piece).
__global__ __launch_bounds__(64) void k_cns_back(const uint32_t *pnode, const int32_t *end_node, const int32_t *node_via, const uint64_t *node_key,
                                                const uint64_t *cov_off, const uint32_t *cov, uint32_t min_cov, uint8_t *rev, uint32_t *len) {
  __shared__ int32_t win[BACK_WIN];
  __shared__ int32_t list[BACK_WIN];
  __shared__ int32_t s_next, s_m;
  const uint32_t p = blockIdx.x, lane = threadIdx.x;
  const int32_t first = (int32_t)pnode[p];
  uint8_t *out = rev + first;
  uint32_t n = 0;
  int32_t v = end_node[p];
  while (v >= first) {   // (no end node: -1)
    const int32_t lo = max(first, v - (BACK_WIN - 1));
    for (int32_t i = (int32_t)lane; i <= v - lo; i += 64) win[i] = node_via[lo + i];
    __syncthreads();
    if (lane == 0) {
      int32_t m = 0;
      while (v >= lo) list[m++] = v, v = win[v - lo];   // strictly falling: at most BACK_WIN entries
      s_next = v, s_m = m;
    }
    __syncthreads();
    v = s_next;
    const int32_t m = s_m;
    for (int32_t base = 0; base < m; base += 64) {
      const bool in = base + (int32_t)lane < m;
      const uint64_t key = in ? node_key[list[base + lane]] : 0;
      const uint32_t c = (uint32_t)key & 15;
      const bool keep = in && c != 0;   // a '-' node yields no base
      const uint64_t mask = __ballot(keep);
      if (keep) {
        const uint32_t depth = cov[cov_off[p] + ((uint32_t)(key >> 12) & 0x7FFFFFFFu)];
        out[n + (uint32_t)__popcll(mask & ((1ull << lane) - 1))] = code_letter(depth > min_cov || c >= 7 ? c : c + 5);
      }
      n += (uint32_t)__popcll(mask);
    }
    __syncthreads();
  }
  if (lane == 0) len[p] = n;
}

__global__ __launch_bounds__(256) void k_cns_text(const uint8_t *rev, const uint32_t *pnode, const uint32_t *len, const uint64_t *piece_off, char *text) {
  const uint32_t p = blockIdx.x, n = len[p];
  const uint8_t *in = rev + pnode[p];
  char *out = text + piece_off[p];
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) out[i] = (char)in[n - 1 - i];
}

struct Events {
  hipEvent_t e[6] = {};
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

// the first pass over the alignments and its verdict: ntag, and -- piece_tlen != nullptr -- naln
// names: the caller's number of every piece, where the pieces here are a selection of the caller's (nullptr: their own)
void scan_and_check(const char *who, const pgx_cns_aln *d_alns, size_t n_aln, const uint8_t *d_q, const uint8_t *d_t, size_t str_bytes, const uint32_t *d_tlen,
                    uint32_t n_piece, DevBuf<uint32_t> &ntag, DevBuf<uint32_t> &err, const uint32_t *names = nullptr) {
  hipStream_t st = ctx().stream;
  DevBuf<uint32_t> naln(d_tlen ? n_piece : 0);
  err.alloc(E_SLOTS);
  ntag.alloc(n_aln);
  PGX_HIP(hipMemsetAsync(err.p, 0xFF, E_SLOTS * sizeof(uint32_t), st));
  if (naln.n) PGX_HIP(hipMemsetAsync(naln.p, 0, naln.n * sizeof(uint32_t), st));
  if (n_aln)
    hipLaunchKernelGGL(k_cns_scan<SCAN_COUNT>, dim3(cdiv(n_aln, 4)), dim3(256), 0, st, d_alns, (uint32_t)n_aln, d_q, d_t, (uint64_t)str_bytes, d_tlen, n_piece,
                       ntag.p, naln.p, err.p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (naln.n) LAUNCH(k_cns_piece_check, n_piece, naln.p, n_piece, err.p);
  uint32_t h[E_SLOTS];
  err.download(h, E_SLOTS);
  sync();
  for (int e : {E_OFFSET, E_MANY, E_BYTE, E_TPOS})
    if (names && h[e] != UINT32_MAX) h[e] = names[h[e]];
  PGX_REQUIRE(h[E_PIECE] == UINT32_MAX, PGX_EARG, "%s: alignment %u names a piece beyond the %u given", who, h[E_PIECE], n_piece);
  PGX_REQUIRE(h[E_RANGE] == UINT32_MAX, PGX_EARG, "%s: the strings of alignment %u lie outside the %zu bytes given", who, h[E_RANGE], str_bytes);
  PGX_REQUIRE_PIECE(h[E_OFFSET] == UINT32_MAX, PGX_EINVAL, h[E_OFFSET], "%s: piece %u: an alignment with a negative t_offset", who, h[E_OFFSET]);
  PGX_REQUIRE_PIECE(h[E_MANY] == UINT32_MAX, PGX_EINVAL, h[E_MANY], "%s: piece %u: more than %u alignments (the reference counts them in 16 bits)", who, h[E_MANY], MAX_ALNS_PER_PIECE);
  PGX_REQUIRE_PIECE(h[E_BYTE] == UINT32_MAX, PGX_EINVAL, h[E_BYTE], "%s: piece %u: an alignment string holds a byte outside ACGTNacgtn-", who, h[E_BYTE]);
  PGX_REQUIRE_PIECE(h[E_TPOS] == UINT32_MAX, PGX_EINVAL, h[E_TPOS], "%s: piece %u: an alignment runs past the end of the template", who, h[E_TPOS]);
}

void check_args(const char *who, const void *alns, size_t n_aln, const void *q, const void *t, size_t str_bytes) {
  PGX_REQUIRE(n_aln == 0 || alns, PGX_EARG, "%s: null argument", who);
  PGX_REQUIRE(str_bytes == 0 || (q && t), PGX_EARG, "%s: null argument", who);
  PGX_REQUIRE(n_aln < (1ull << 31), PGX_EARG, "%s: too many alignments for one call", who);
}

}  // namespace

void cns_call_dev(const char *who, const pgx_cns_aln *d_alns, size_t n_aln, const uint8_t *d_q, const uint8_t *d_t, size_t str_bytes, const uint32_t *piece_tlen,
                  size_t n_piece, uint32_t min_cov, char **text, uint64_t *piece_off, pgx_cns_stats *stats, const uint32_t *names, DevBuf<char> *d_text_out,
                  DevBuf<uint64_t> *d_off_out) {
  const bool stay = d_text_out && d_off_out;   // the text and its offsets stay on the device
  PGX_REQUIRE((stay || (text && piece_off)) && (n_piece == 0 || piece_tlen), PGX_EARG, "%s: null argument", who);
  check_args(who, d_alns, n_aln, d_q, d_t, str_bytes);
  PGX_REQUIRE(n_piece <= MAX_PIECES, PGX_EARG, "%s: more than %u pieces in one call", who, MAX_PIECES);
  std::vector<uint64_t> cov_off(n_piece + 1, 0);
  for (size_t p = 0; p < n_piece; ++p) {
    PGX_REQUIRE_PIECE(piece_tlen[p] <= (uint32_t)INT32_MAX, PGX_EARG, names ? (size_t)names[p] : p, "%s: piece %zu: a template of %u bases", who, names ? (size_t)names[p] : p, piece_tlen[p]);
    cov_off[p + 1] = cov_off[p] + piece_tlen[p];
  }
  if (text) *text = nullptr;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (n_piece == 0) {
    PGX_REQUIRE(n_aln == 0, PGX_EARG, "%s: alignments without pieces", who);
    if (stay) {
      d_text_out->alloc(1), d_off_out->alloc(1);
      PGX_HIP(hipMemsetAsync(d_off_out->p, 0, sizeof(uint64_t), ctx().stream));
      return;
    }
    *text = caller_text(nullptr, 0);
    piece_off[0] = 0;
    return;
  }
  MemTag mem_tag("cns");
  hipStream_t st = ctx().stream;
  const uint32_t np = (uint32_t)n_piece;
  Events ev;
  ev.mark(0);
  DevBuf<uint32_t> d_tlen(np), ntag, err;
  DevBuf<uint64_t> d_cov_off(np + 1);
  d_tlen.upload(piece_tlen, np);
  d_cov_off.upload(cov_off.data(), np + 1);
  scan_and_check(who, d_alns, n_aln, d_q, d_t, str_bytes, d_tlen.p, np, ntag, err, names);
  PrimWs ws;
  DevBuf<uint64_t> tag_off(n_aln + 1);
  const uint64_t n_tag64 = scan_to_total(ntag.p, tag_off.p, n_aln, &ws);
  PGX_REQUIRE(n_tag64 < (1ull << 31), PGX_EARG, "%s: %llu tags are too many for one call", who, (unsigned long long)n_tag64);
  const uint32_t n_tag = (uint32_t)n_tag64;
  DevBuf<uint32_t> cov(cov_off[np] ? cov_off[np] : 1);
  PGX_HIP(hipMemsetAsync(cov.p, 0, cov.n * sizeof(uint32_t), st));
  DevBuf<uint64_t> hi(n_tag), lo(n_tag);
  if (n_aln)
    hipLaunchKernelGGL(k_cns_scan<SCAN_KEYS>, dim3(cdiv(n_aln, 4)), dim3(256), 0, st, d_alns, (uint32_t)n_aln, d_q, d_t, (uint64_t)str_bytes, d_tlen.p, np, ntag.p,
                       nullptr, err.p, tag_off.p, nullptr, hi.p, lo.p, d_cov_off.p, cov.p);
  ev.mark(1);
  // edges in the rule's order: by predecessor key first, then -- stable -- by (piece, tag key)
  uint32_t n_edge = 0, n_node = 0;
  DevBuf<uint32_t> estart, nfirst, e_nid;
  DevBuf<uint64_t> node_key;
  {
    DevBuf<uint32_t> order(n_tag);
    DevBuf<uint8_t> flag(n_tag);
    int piece_bits = 1;
    while ((1u << piece_bits) < np) ++piece_bits;
    sort_order({{hi.p, PIECE_SHIFT + piece_bits}, {lo.p, 44}}, n_tag, nullptr, order.p, hi.p, &ws);
    DevBuf<uint64_t> tmp(n_tag);
    gather(lo.p, order.p, n_tag, tmp.p, &ws);
    lo = std::move(tmp);   // hi, lo: the sorted tags' keys
    if (n_tag) LAUNCH(k_cns_edge_heads, n_tag, hi.p, lo.p, n_tag, flag.p);
    estart.alloc(n_tag);
    n_edge = select_indices(flag.p, n_tag, estart.p, &ws);
    if (n_edge) LAUNCH(k_cns_node_heads, n_edge, hi.p, estart.p, n_edge, flag.p);
    nfirst.alloc(n_edge);
    n_node = select_indices(flag.p, n_edge, nfirst.p, &ws);
  }
  node_key.alloc(n_node);
  e_nid.alloc(n_edge);
  DevBuf<uint32_t> pnode(np + 1), pedge(np + 1), len(np);
  DevBuf<int32_t> e_score(n_edge), e_pred(n_edge), node_via(n_node);
  DevBuf<int64_t> node_best(n_node);
  DevBuf<uint8_t> rev(n_node ? n_node : 1);
  if (n_node) LAUNCH(k_cns_nodes, n_node, hi.p, estart.p, nfirst.p, n_node, n_edge, node_key.p, e_nid.p);
  LAUNCH(k_cns_piece_bounds, np + 1, node_key.p, nfirst.p, n_node, n_edge, np, pnode.p, pedge.p);
  if (n_edge) LAUNCH(k_cns_edges, n_edge, hi.p, lo.p, estart.p, n_edge, n_tag, e_nid.p, node_key.p, pnode.p, d_cov_off.p, cov.p, e_score.p, e_pred.p);
  ev.mark(2);
  DevBuf<int32_t> end_node(np);
  hipLaunchKernelGGL(k_cns_score, dim3(np), dim3(64), 0, st, pedge.p, e_score.p, e_pred.p, e_nid.p, node_best.p, node_via.p, end_node.p, err.p);
  ev.mark(3);
  hipLaunchKernelGGL(k_cns_back, dim3(np), dim3(64), 0, st, pnode.p, end_node.p, node_via.p, node_key.p, d_cov_off.p, cov.p, min_cov, rev.p, len.p);
  ev.mark(4);
  uint32_t no_end = 0;
  PGX_HIP(hipMemcpyAsync(&no_end, err.p + E_NOEND, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  DevBuf<uint64_t> d_off(np + 1);
  const uint64_t total = scan_to_total(len.p, d_off.p, np, &ws);   // (synchronises)
  PGX_REQUIRE_PIECE(no_end == UINT32_MAX, PGX_EINVAL, names ? names[no_end] : no_end, "%s: piece %u: no alignment path scores above zero, the reference has no consensus for it", who,
              names ? names[no_end] : no_end);
  DevBuf<char> d_text(total ? total : 1);
  hipLaunchKernelGGL(k_cns_text, dim3(np), dim3(256), 0, st, rev.p, pnode.p, len.p, d_off.p, d_text.p);
  ev.mark(5);
  if (stay) {
    sync();
    *d_text_out = std::move(d_text), *d_off_out = std::move(d_off);
  } else {
    char *out = caller_text(nullptr, total);
    try {
      if (total) PGX_HIP(hipMemcpyAsync(out, d_text.p, total, hipMemcpyDeviceToHost, st));
      d_off.download(piece_off, np + 1);
      sync();
    } catch (...) {
      free(out);
      throw;
    }
    *text = out;
  }
  if (stats) {
    stats->n_aln = n_aln, stats->n_tags = n_tag, stats->n_edges = n_edge, stats->n_nodes = n_node, stats->text_bytes = total;
    stats->tags_ms = ev.ms(0, 1), stats->sort_ms = ev.ms(1, 2), stats->score_ms = ev.ms(2, 3), stats->back_ms = ev.ms(3, 4), stats->gpu_ms = ev.ms(0, 5);
  }
}

}  // namespace pgx

using namespace pgx;

extern "C" {

int pgx_cns_call_dev(const pgx_cns_aln *d_alns, size_t n_aln, const char *d_q_str, const char *d_t_str, size_t str_bytes, const uint32_t *piece_tlen,
                     size_t n_piece, uint32_t min_cov, char **text, uint64_t *piece_off, pgx_cns_stats *stats) {
  return guarded([&] {
    require_ready();
    cns_call_dev("pgx_cns_call_dev", d_alns, n_aln, (const uint8_t *)d_q_str, (const uint8_t *)d_t_str, str_bytes, piece_tlen, n_piece, min_cov, text, piece_off,
                 stats, nullptr);
  });
}

int pgx_cns_call(const pgx_cns_aln *alns, size_t n_aln, const char *q_str, const char *t_str, size_t str_bytes, const uint32_t *piece_tlen, size_t n_piece,
                 uint32_t min_cov, char **text, uint64_t *piece_off, pgx_cns_stats *stats) {
  return guarded([&] {
    require_ready();
    check_args("pgx_cns_call", alns, n_aln, q_str, t_str, str_bytes);
    MemTag mem_tag("cns");
    DevBuf<pgx_cns_aln> d_alns(n_aln);
    DevBuf<uint8_t> d_q(str_bytes), d_t(str_bytes);
    d_alns.upload(alns, n_aln);
    d_q.upload((const uint8_t *)q_str, str_bytes);
    d_t.upload((const uint8_t *)t_str, str_bytes);
    cns_call_dev("pgx_cns_call", d_alns.p, n_aln, d_q.p, d_t.p, str_bytes, piece_tlen, n_piece, min_cov, text, piece_off, stats, nullptr);
  });
}

int pgx_cns_tags(const pgx_cns_aln *alns, size_t n_aln, const char *q_str, const char *t_str, size_t str_bytes, pgx_cns_tag **tags, uint64_t *tag_off) {
  return guarded([&] {
    require_ready();
    const char *who = "pgx_cns_tags";
    PGX_REQUIRE(tags && tag_off, PGX_EARG, "%s: null argument", who);
    check_args(who, alns, n_aln, q_str, t_str, str_bytes);
    *tags = nullptr;
    MemTag mem_tag("cns");
    hipStream_t st = ctx().stream;
    DevBuf<pgx_cns_aln> d_alns(n_aln);
    DevBuf<uint8_t> d_q(str_bytes), d_t(str_bytes);
    d_alns.upload(alns, n_aln);
    d_q.upload((const uint8_t *)q_str, str_bytes);
    d_t.upload((const uint8_t *)t_str, str_bytes);
    DevBuf<uint32_t> ntag, err;
    scan_and_check(who, d_alns.p, n_aln, d_q.p, d_t.p, str_bytes, nullptr, 0, ntag, err);
    DevBuf<uint64_t> d_off(n_aln + 1);
    const uint64_t n_tag = scan_to_total(ntag.p, d_off.p, n_aln);
    DevBuf<pgx_cns_tag> d_tags(n_tag);
    if (n_aln)
      hipLaunchKernelGGL(k_cns_scan<SCAN_TAGS>, dim3(cdiv(n_aln, 4)), dim3(256), 0, st, d_alns.p, (uint32_t)n_aln, d_q.p, d_t.p, (uint64_t)str_bytes, nullptr, 0u,
                         ntag.p, nullptr, err.p, d_off.p, d_tags.p, nullptr, nullptr, nullptr, nullptr);
    pgx_cns_tag *out = (pgx_cns_tag *)out_alloc(n_tag ? n_tag * sizeof(pgx_cns_tag) : 1);
    try {
      d_tags.download(out, n_tag);
      d_off.download(tag_off, n_aln + 1);
      sync();
    } catch (...) {
      out_free(out);
      throw;
    }
    *tags = out;
  });
}

}  // extern "C"
