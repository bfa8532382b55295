// pgx_sketch_win.h -- what the wavefront-per-read sketch kernels share (k_sketch_general in pgx_kernels.hip, k_sketch_hpc in
// pgx_sketch_hpc.hip): the minimizer hash, the base code of a seqdb byte, and the window passes of the closed form over one read's
// (or one segment's) entries in global scratch.
#pragma once
#include "pgx_internal.h"

namespace pgx {

// minimizer hash (src/mm_sketch.c:23-32), 64-bit form for any k <= 28
__device__ __forceinline__ uint64_t mix64(uint64_t key, uint64_t mask) {
  key = (~key + (key << 21)) & mask;
  key = key ^ key >> 24;
  key = ((key + (key << 3)) + (key << 8)) & mask;
  key = key ^ key >> 14;
  key = ((key + (key << 2)) + (key << 4)) & mask;
  key = key ^ key >> 28;
  key = (key + (key << 31)) & mask;
  return key;
}

__device__ __forceinline__ int code_of_nibble(uint32_t b) {
  // seqdb low nibble is one-hot A=1 C=2 G=4 T=8 (src/shmr_utils.c:18-30); anything else decodes to 'N'
  b &= 0xF;
  return (b == 1) ? 0 : (b == 2) ? 1 : (b == 4) ? 2 : (b == 8) ? 3 : 4;
}

// Running extremum within blocks of w consecutive elements (block b = [b w, (b+1) w)), the whole wavefront walking the array 64
// elements at a time with coalesced accesses: a segmented Hillis-Steele scan (segment heads at multiples of w) plus a carry
// between the 64-element slices.  FWD: dst[i] = op(src[block start .. i]);  !FWD: dst[i] = op(src[i .. block end]).
template <bool MIN, bool FWD>
__device__ __forceinline__ void block_running_extremum(const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, int count, int w,
                                                       int lane) {
  const uint64_t neutral = MIN ? ~0ULL : 0ULL;
  auto op = [](uint64_t a, uint64_t b) { return MIN ? (a < b ? a : b) : (a > b ? a : b); };
  const int nslice = (count + 63) / 64;
  uint64_t carry = neutral;
  for (int sl = 0; sl < nslice; ++sl) {
    const int c0 = (FWD ? sl : nslice - 1 - sl) * 64;
    const int i = c0 + (FWD ? lane : 63 - lane);  // scan order: ascending i when FWD, descending otherwise
    uint64_t v = i < count ? src[i] : neutral;
    // a segment starts at this lane (in scan order) when i is the first (FWD) / last (!FWD) element of its block
    int f = i < count && (FWD ? (i % w == 0) : (i % w == w - 1 || i == count - 1)) ? 1 : 0;
    const int head = f;
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t vu = (uint64_t)__shfl_up((int)(v >> 32), d, 64) << 32 | (uint32_t)__shfl_up((int)v, d, 64);
      const int fu = __shfl_up(f, d, 64);
      if (lane >= d) {
        if (!f) v = op(v, vu);
        f |= fu;
      }
    }
    if (!f) v = op(v, carry);  // no segment head at or before this lane inside the slice: the open segment continues
    if (i < count) dst[i] = v;
    (void)head;
    carry = (uint64_t)__shfl((int)(v >> 32), 63, 64) << 32 | (uint32_t)__shfl((int)v, 63, 64);
  }
}

// Passes 2 and 3 of the closed form (the header of k_sketch_general states it) over the n entries H[0 .. n) of one wavefront's read, or
// of one segment of it; WM, T1, T2: scratch of n elements each.  An entry equal to 2^64 - 1 is INFINITE: it takes part in every window
// and is never emitted (a hash is below 2^56, so only a kernel that writes whole keys has such entries).  Emitted element of entry p:
//   x = KEYS ? H[p] : H[p] << 8 | k,  y = yhi | (PY[p] & 0x7fffffff)     (bit 31 of PY is the caller's)
// written to dst[nout ...] while below cap.  Returns the number of emitted elements (counted past cap too: `over` says that some did not fit).
// One wavefront per block: the __syncthreads() order this wave's global writes before its reads.
template <bool KEYS>
__device__ __forceinline__ uint32_t sketch_windows(const uint64_t *__restrict__ H, const uint32_t *__restrict__ PY, uint64_t *__restrict__ WM,
                                                   uint64_t *__restrict__ T1, uint64_t *__restrict__ T2, int n, int w, int k, int lane,
                                                   uint64_t yhi, pgx_mm128 *__restrict__ dst, uint64_t cap, uint32_t nout, bool &over) {
  // ---- pass 2: window minima in O(1) per entry (van Herk / Gil-Werman over blocks of w entries) ---------------------
  // T1 = running minimum from the start of the entry's block, T2 = running minimum from the end of its block;
  // the window [s, s+w) is the tail of block(s) plus the head of the next block: WM[s] = min(T2[s], T1[s+w-1]).
  const int nwin = n - w + 1;  // number of full windows (<= 0: short read)
  if (nwin > 0) {
    block_running_extremum<true, true>(H, T1, n, w, lane);
    block_running_extremum<true, false>(H, T2, n, w, lane);
    __syncthreads();
    for (int v0 = 0; v0 < nwin; v0 += 64) {
      const int v = v0 + lane;
      if (v < nwin) WM[v] = (v % w == 0) ? T1[v + w - 1] : min(T2[v], T1[v + w - 1]);
    }
    __syncthreads();
    // the same over WM with maxima: GX(p) = max of WM over the (up to w) windows that contain entry p
    block_running_extremum<false, true>(WM, T1, nwin, w, lane);
    block_running_extremum<false, false>(WM, T2, nwin, w, lane);
  }
  // rightmost smallest of the first min(n, w - 1) entries (all n entries for a short read)
  const int lim = nwin > 0 ? w - 1 : n;
  uint64_t bh = ~0ULL;
  int bi = -1;
  for (int v = lane; v < lim; v += 64) {
    const uint64_t x = H[v];
    if (x <= bh) bh = x, bi = v;  // ascending v per lane: <= keeps the rightmost
  }
  for (int d = 32; d; d >>= 1) {
    const uint64_t oh = (uint64_t)__shfl_xor((int)(bh >> 32), d, 64) << 32 | (uint32_t)__shfl_xor((int)bh, d, 64);
    const int oi = __shfl_xor(bi, d, 64);
    if (oi >= 0 && (bi < 0 || oh < bh || (oh == bh && oi > bi))) bh = oh, bi = oi;
  }
  const int m_idx = bi;
  const uint64_t m_h = bh;
  const uint64_t h_last = nwin > 0 ? H[w - 1] : 0;
  __syncthreads();
  // ---- pass 3 ----------------------------------------------------------------------------------------------
  for (int p0 = 0; p0 < n; p0 += 64) {
    const int p = p0 + lane;
    bool emit = false;
    uint64_t hp = 0;
    if (p < n) {
      hp = H[p];
      if (nwin > 0) {
        const int s0 = p - w + 1 > 0 ? p - w + 1 : 0, s1 = p < nwin - 1 ? p : nwin - 1;
        uint64_t gx = 0;
        if (s1 - s0 + 1 == w) {  // all w windows exist: tail of block(s0) + head of the next block
          gx = (s0 % w == 0) ? T1[s1] : max(T2[s0], T1[s1]);
        } else {  // the first / last w-1 entries of the read: fewer windows, scanned directly
          for (int sidx = s0; sidx <= s1; ++sidx) gx = max(gx, WM[sidx]);
        }
        emit = gx == hp;  // (a window that contains p has minimum <= hash(p))
        if (p <= w - 2 && hp == m_h) emit = p != m_idx ? true : h_last > m_h;
      } else {
        emit = p == m_idx;
      }
      if (KEYS && hp == ~0ULL) emit = false;
    }
    const uint64_t em = __ballot(emit);
    if (emit) {
      const uint32_t r = nout + (uint32_t)__builtin_popcountll(em & ((1ULL << lane) - 1));
      if (r < cap) dst[r] = pgx_mm128{KEYS ? hp : hp << 8 | (uint64_t)k, yhi | (uint64_t)(PY[p] & 0x7fffffffu)};
      else over = true;
    }
    nout += (uint32_t)__builtin_popcountll(em);
  }
  return nout;
}

}  // namespace pgx
