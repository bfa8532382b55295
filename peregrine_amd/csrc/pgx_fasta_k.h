// pgx_fasta_k.h -- the kernels that pgx_fasta.hip (a FASTA text) and pgx_reads.hip (FASTA/FASTQ texts in pieces, 4.8a) share:
// the first header marker, the line starts, the sequence-line and record tables, the names, the gather of the kept bytes into the pool and
// the two-strand encoding.  Each file that includes this gets its own copies (internal linkage).
#pragma once
#include "pgx_internal.h"

namespace pgx {
namespace {

constexpr uint64_t NONE = ~0ull;
// The reference's reader learns of the end of its input when a refill of its 16 KiB buffer comes back short: at the last byte of a text
// whose length is no multiple of 16 KiB it knows (eof_seen), and then (a) a header marker that is the very last byte starts no record and
// (b) a last line that is one byte without '\n' is not given the '\r' rule.  Behind a text of k * 16 KiB it does not know yet: the marker
// starts a record with an empty name, and the rule applies.
constexpr uint64_t KS_BUF = 16384;
constexpr uint32_t TILE = 4096, TPB = 256;   // a block's tile of text / pool bytes: 16 rounds of 256 consecutive bytes

__device__ __forceinline__ uint32_t fa_fwd(uint32_t c) {   // (as pgx_mkseqdb.hip: A/a C/c G/g T/t, everything else 0)
  c |= 0x20;
  return c == 'a' ? 1u : c == 'c' ? 2u : c == 'g' ? 4u : c == 't' ? 8u : 0u;
}
__device__ __forceinline__ uint32_t fa_rev(uint32_t c) {
  c |= 0x20;
  return c == 'a' ? 8u : c == 'c' ? 4u : c == 'g' ? 2u : c == 't' ? 1u : 0u;
}
__device__ __forceinline__ bool fa_marker(uint32_t c) { return c == '>' || c == '@'; }
__device__ __forceinline__ bool fa_space(uint32_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

// the first index in [lo, hi) with a[index] > v (hi: none); a ascending
template <typename T>
__device__ __forceinline__ uint64_t upper_bound(const T *__restrict__ a, uint64_t lo, uint64_t hi, T v) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] > v) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// m0: the smallest i with b[i] in {'>', '@'}.  *m0 starts as NONE.
__global__ __launch_bounds__(TPB) void k_fa_first(const uint8_t *__restrict__ b, uint64_t n, unsigned long long *m0) {
  const uint64_t base = (uint64_t)blockIdx.x * TILE;
  for (uint32_t it = 0; it < TILE / TPB; ++it) {
    const uint64_t i = base + it * TPB + threadIdx.x;
    const bool mk = i < n && fa_marker(b[i]);
    const uint64_t m = __ballot(mk);
    if (m) {   // (wave-uniform: the lowest set lane holds the smallest i of this wavefront, and later rounds only hold larger ones)
      if ((threadIdx.x & 63) == 0) atomicMin(m0, (unsigned long long)(i + (uint64_t)__builtin_ctzll(m)));
      break;
    }
  }
}

// line starts behind m0: ls[i] = (i == m0) or (i > m0 and b[i - 1] == '\n'); acc[0] += their number; acc[1] = the smallest line start
// > m0 that holds '+' (starts as NONE)
__global__ __launch_bounds__(TPB) void k_fa_marks(const uint8_t *__restrict__ b, uint64_t n, uint64_t m0, uint8_t *__restrict__ ls,
                                                  unsigned long long *acc) {
  const uint64_t base = (uint64_t)blockIdx.x * TILE;
  const uint32_t lane = threadIdx.x & 63;
  uint32_t cnt = 0;
  uint64_t plus_at = NONE;
  for (uint32_t it = 0; it < TILE / TPB; ++it) {
    const uint64_t i = base + it * TPB + threadIdx.x;
    bool start = false, plus = false;
    if (i < n) {
      start = i == m0 || (i > m0 && b[i - 1] == '\n');
      plus = start && i > m0 && b[i] == '+';
      ls[i] = start ? 1 : 0;
    }
    const uint64_t ms = __ballot(start), mp = __ballot(plus);
    cnt += (uint32_t)__popcll(ms);
    if (mp && plus_at == NONE) plus_at = i - lane + (uint64_t)__builtin_ctzll(mp);   // (the wavefront's first lane holds i - lane)
  }
  if (lane == 0) {
    if (cnt) atomicAdd(acc, (unsigned long long)cnt);
    if (plus_at != NONE) atomicMin(acc + 1, (unsigned long long)plus_at);
  }
}

// select_indices answers positions relative to the piece it ran on
__global__ void k_fa_add_base(uint64_t *list, uint64_t cnt, uint64_t base) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < cnt) list[t] += base;
}

// the sequence-line table: line t of it is line sl[t]; its record is the number of record headers up to it, less one (rec_incl[j + 1]: the
// inclusive count); kept: its length, less one trailing '\r' unless it is exactly "\r" and its record's first sequence line, or -- with
// eof_seen -- the text's last line without a '\n'
__global__ void k_fa_seq_lines(const uint8_t *__restrict__ b, uint64_t n, const uint64_t *__restrict__ start, uint64_t n_lines,
                               const uint32_t *__restrict__ sl, uint32_t n_sl, const uint32_t *__restrict__ rec_incl, uint32_t eof_seen,
                               uint64_t *__restrict__ l_start, uint64_t *__restrict__ l_kept, uint32_t *__restrict__ l_rec) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_sl) return;
  const uint64_t j = sl[t];
  const uint64_t s = start[j];
  const uint64_t e = j + 1 < n_lines ? start[j + 1] - 1 : (b[n - 1] == '\n' ? n - 1 : n);
  const uint64_t len = e - s;   // (>= 1: is_seq)
  const uint32_t rec = rec_incl[j + 1] - 1;
  const bool first = t == 0 || rec_incl[(uint64_t)sl[t - 1] + 1] - 1 != rec;
  const bool drop = b[e - 1] == '\r' && !(len == 1 && (first || (e == n && eof_seen)));
  l_start[t] = s, l_kept[t] = len - (drop ? 1 : 0), l_rec[t] = rec;
}

// the record table: record r's header is line hl[r]; its name runs from the byte behind the marker to the first whitespace or the end of
// the text; roff[r] = the pool offset of its first sequence line (pool_off has n_sl + 1 entries: the last is the pool's size)
__global__ void k_fa_records(const uint8_t *__restrict__ b, uint64_t n, const uint64_t *__restrict__ start, const uint32_t *__restrict__ hl,
                             uint32_t n_rec, const uint32_t *__restrict__ l_rec, uint32_t n_sl, const uint64_t *__restrict__ pool_off,
                             uint64_t *__restrict__ hdr_off, uint64_t *__restrict__ name_len1, uint64_t *__restrict__ roff) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > n_rec) return;
  if (r == n_rec) {
    roff[r] = pool_off[n_sl];
    return;
  }
  const uint64_t h = start[hl[r]];
  uint64_t i = h + 1;
  while (i < n && !fa_space(b[i])) ++i;
  hdr_off[r] = h, name_len1[r] = i - h;   // (the name's length and one more, for the '\n' that ends it in the compact buffer)
  roff[r] = pool_off[r ? upper_bound<uint32_t>(l_rec, 0, n_sl, r - 1) : 0];   // the first sequence line of a record >= r
}

// the names, a line each
__global__ void k_fa_names(const uint8_t *__restrict__ b, const uint64_t *__restrict__ hdr_off, const uint64_t *__restrict__ name_off,
                           uint32_t n_rec, char *__restrict__ out) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rec) return;
  const uint64_t o = name_off[r], len = name_off[r + 1] - o - 1;
  const uint8_t *s = b + hdr_off[r] + 1;
  for (uint64_t k = 0; k < len; ++k) out[o + k] = (char)s[k];
  out[o + len] = '\n';
}

// the kept bytes into the pool: a block takes TILE text bytes; the sequence lines that can hold one of them are [lo, hi) of the table,
// found once per block, and a byte's line by search among those
__global__ __launch_bounds__(TPB) void k_fa_gather(const uint8_t *__restrict__ b, uint64_t n, const uint64_t *__restrict__ l_start,
                                                   const uint64_t *__restrict__ l_kept, const uint64_t *__restrict__ pool_off, uint32_t n_sl,
                                                   uint8_t *__restrict__ pool, uint64_t pool_size) {
  __shared__ uint64_t s_rng[2];
  const uint64_t base = (uint64_t)blockIdx.x * TILE;
  const uint64_t last = (base + TILE < n ? base + TILE : n) - 1;
  if (threadIdx.x < 2) s_rng[threadIdx.x] = upper_bound<uint64_t>(l_start, 0, n_sl, threadIdx.x ? last : base);
  __syncthreads();
  const uint64_t hi = s_rng[1];
  if (hi == 0) return;   // (no sequence line starts at or before this tile's last byte)
  const uint64_t lo = s_rng[0] ? s_rng[0] - 1 : 0;
  for (uint32_t it = 0; it < TILE / TPB; ++it) {
    const uint64_t i = base + it * TPB + threadIdx.x;
    if (i >= n) break;
    const uint64_t u = upper_bound<uint64_t>(l_start, lo, hi, i);
    if (u == 0) continue;
    const uint64_t d = i - l_start[u - 1];
    if (d >= l_kept[u - 1]) continue;
    const uint64_t q = pool_off[u - 1] + d;
    if (q < pool_size) pool[q] = b[i];
  }
}

// out[roff + p] = rev(s[len - 1 - p]) << 4 | fwd(s[p]) (k_encode_biseq's byte): a block takes TILE pool bytes, a byte's record by search in
// roff (n_rec + 1 entries) among the records [lo, hi) that can hold one of the tile's bytes
__global__ __launch_bounds__(TPB) void k_fa_encode(const uint8_t *__restrict__ pool, uint64_t pool_size, const uint64_t *__restrict__ roff,
                                                   uint32_t n_rec, uint8_t *__restrict__ out) {
  __shared__ uint64_t s_rng[2];
  const uint64_t base = (uint64_t)blockIdx.x * TILE;
  const uint64_t last = (base + TILE < pool_size ? base + TILE : pool_size) - 1;
  if (threadIdx.x < 2) s_rng[threadIdx.x] = upper_bound<uint64_t>(roff, 0, n_rec, threadIdx.x ? last : base);
  __syncthreads();
  const uint64_t hi = s_rng[1];
  const uint64_t lo = s_rng[0] ? s_rng[0] - 1 : 0;
  for (uint32_t it = 0; it < TILE / TPB; ++it) {
    const uint64_t q = base + it * TPB + threadIdx.x;
    if (q >= pool_size) break;
    const uint64_t u = upper_bound<uint64_t>(roff, lo, hi, q);   // (>= 1: roff[0] == 0)
    if (u == 0) continue;
    const uint64_t o = roff[u - 1], e = roff[u];
    const uint64_t m = e - 1 - (q - o);   // the mirrored byte, inside [o, e)
    if (q >= e || m >= pool_size) continue;
    out[q] = (uint8_t)(fa_rev(pool[m]) << 4 | fa_fwd(pool[q]));
  }
}

}  // namespace
}  // namespace pgx
