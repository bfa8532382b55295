// pgx_sketch_hpc.hip -- mm_sketch with is_hpc = 1 (src/mm_sketch.c:84-150): minimizers of the HOMOPOLYMER-COMPRESSED read, positions and
// spans in raw read coordinates.  One wavefront per read, everything in run space (tools/hpc_sketch_model.py is the checked statement).
//
// The machine makes one iteration per maximal run of equal unambiguous bases (decided on codes) and one per ambiguous base:
//   * a run shifts its code into both k-mers (an ambiguous base shifts nothing and flushes nothing) and pushes its length; the span of
//     the k-mer that ends at run r is the sum of the last min(k, runs since the last ambiguous base) lengths;
//   * a strand-ambiguous k-mer (fwd == rev) makes no entry and does not advance `l`, but its run stays in later spans;
//   * otherwise ++l, and the entry is FINITE iff l >= k and span < 256, with the key x = hash << 8 | span and y = rid << 32 | i << 1 | strand,
//     i the raw index of the run's last base; every comparison is on the whole x;
//   * an ambiguous base sets l = 0 and makes one infinite entry.
// With the runs contiguous (every base belongs to one run, an ambiguous base is a run of its own), S[r] = first base of run r and
// S[runs] = len give  i = S[r+1] - 1  and, once l >= k (k runs since the last ambiguous base),  span = S[r+1] - S[r+1-k].
// The STREAM of a read is its kept runs (not strand-ambiguous) and its ambiguous bases, in order; a SEGMENT is a maximal stretch of stream
// entries with l >= k.  Then, exactly:
//   sketch = for every segment in order: the closed form (pgx_sketch_win.h) over its entries, infinite ones included, WITHOUT its last
//            element iff one of the segment's last w entries is finite (that element is the segment's pending minimum);
//            then ONE element: the rightmost smallest of the last w stream entries, if finite.
// A read without ambiguous bases is one segment: the same rule.
//
// Passes: runs (1 KiB tiles, aligned 16-byte loads, run starts balloted and prefix-summed into S[] / C[]), entries (a lane per run: the
// k-mers from the k preceding run codes, `l` as a prefix count of kept runs since the last ambiguous base, X[] / PY[] compacted), the
// window passes per segment, the end element.
#include <algorithm>

#include "pgx_internal.h"
#include "pgx_sketch_win.h"

namespace pgx {

namespace {

constexpr uint64_t INF = ~0ULL;

__global__ __launch_bounds__(64) void k_sketch_hpc(const uint8_t *__restrict__ seq, const ReadDesc *__restrict__ reads,
                                                   const uint32_t *__restrict__ list, uint32_t slot0, uint32_t n_list, int w, int k,
                                                   const uint64_t *__restrict__ scr_off, uint64_t *__restrict__ Xs, uint32_t *__restrict__ PYs,
                                                   uint64_t *__restrict__ WMs, uint64_t *__restrict__ T1s, uint64_t *__restrict__ T2s,
                                                   pgx_mm128 *__restrict__ slab, const uint64_t *__restrict__ slab_off, int off_by_list,
                                                   uint32_t *__restrict__ counts, uint32_t *__restrict__ flags, uint32_t *__restrict__ need) {
  const int lane = threadIdx.x;
  const uint64_t mask = (1ULL << (2 * k)) - 1;
  const int top = 2 * (k - 1);
  const uint64_t below_incl = lane == 63 ? ~0ULL : (2ULL << lane) - 1, below = (1ULL << lane) - 1;
  for (uint32_t it = blockIdx.x; it < n_list; it += gridDim.x) {
    const uint32_t slot = list ? list[it] : slot0 + it;
    const ReadDesc rd = reads[slot];
    const int len = (int)rd.len;
    if (len <= 0) {
      if (lane == 0) counts[slot] = 0, need[slot] = 0;
      continue;
    }
    uint64_t *X = Xs + scr_off[it], *WM = WMs + scr_off[it], *T1 = T1s + scr_off[it], *T2 = T2s + scr_off[it];
    uint32_t *PY = PYs + scr_off[it];
    // the run table lives in the window passes' scratch, which is idle until the entries exist: len + 1 starts in T1 (len 64-bit words),
    // len codes in T2
    uint32_t *S = reinterpret_cast<uint32_t *>(T1);
    uint8_t *C = reinterpret_cast<uint8_t *>(T2);
    // ---- runs ------------------------------------------------------------------------------------------------------------------
    // lane l owns bytes [16 l, 16 l + 16) of a 1 KiB tile that starts at the 16-byte boundary below the read (the seqdb buffer is aligned
    // and padded); codes: 0..3, 4 ambiguous, 5 outside the read.  A base starts a run iff it is ambiguous or its code differs from the
    // previous base's (the neighbour lane's last byte, the previous tile's last byte).
    const int lead = (int)(rd.off & 15);
    const uint8_t *base = seq + (rd.off - (uint64_t)lead);
    const int span_bytes = lead + len;
    int nr = 0;
    int carry_code = 5;
    for (int b0 = 0; b0 < span_bytes; b0 += 1024) {
      const int mine = b0 + lane * 16;
      uint64_t cw = 0;   // 16 codes of 4 bits
      int c15 = 5;
      if (mine < span_bytes) {
        const uint4 v = *reinterpret_cast<const uint4 *>(base + mine);
        const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int at = mine + u;
          const int c = (at >= lead && at < span_bytes) ? code_of_nibble(wd[u >> 2] >> (8 * (u & 3))) : 5;
          cw |= (uint64_t)c << (4 * u);
          c15 = c;
        }
      } else {
        cw = 0x5555555555555555ULL;
      }
      int prev = __shfl_up(c15, 1, 64);
      if (lane == 0) prev = carry_code;
      uint32_t st = 0;
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int c = (int)(cw >> (4 * u)) & 15;
        if (c < 5 && (c == 4 || c != prev)) st |= 1u << u;
        prev = c;
      }
      const int cs = __builtin_popcount(st);
      int is = cs;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(is, o, 64);
        if (lane >= o) is += t;
      }
      int wr = nr + is - cs;
      for (uint32_t x = st; x; x &= x - 1) {
        const int u = __builtin_ctz(x);
        S[wr] = (uint32_t)(mine + u - lead);
        C[wr] = (uint8_t)((cw >> (4 * u)) & 15);
        ++wr;
      }
      nr += __shfl(is, 63, 64);
      carry_code = __shfl(c15, 63, 64);
    }
    if (lane == 0) S[nr] = (uint32_t)len;
    __syncthreads();  // (one wavefront per block: orders this wave's global writes before its reads below)
    // ---- entries: a lane per run ------------------------------------------------------------------------------------------------
    int ns = 0;       // stream entries so far
    int l_carry = 0;  // kept runs since the last ambiguous base, before this slice
    for (int r0 = 0; r0 < nr; r0 += 64) {
      const int r = r0 + lane;
      const int c = r < nr ? (int)C[r] : 5;
      uint64_t fwd = 0, rev = 0;
      if (c < 4) {  // the k newest unambiguous run codes up to r: the j-th newest sits at bits 2j of fwd and top - 2j of rev
        int j = 0;
        for (int q = r; q >= 0 && j < k; --q) {
          const uint64_t cq = C[q];
          if (cq < 4) {
            fwd |= cq << (2 * j);
            rev |= (3ULL ^ cq) << (top - 2 * j);
            ++j;
          }
        }
      }
      const bool kept = c < 4 && fwd != rev, amb = c == 4;
      const uint64_t km = __ballot(kept), nm = __ballot(amb);
      const uint64_t nb = nm & below_incl;
      int l;
      if (nb) {
        const int hi = 63 - __builtin_clzll(nb);
        l = __builtin_popcountll(km & below_incl & ~((2ULL << hi) - 1));
      } else {
        l = l_carry + __builtin_popcountll(km & below_incl);
      }
      l_carry = __shfl(l, 63, 64);
      const bool closed = kept && l >= k;
      uint64_t x = INF;
      uint32_t py = 0;
      if (kept) {
        const uint32_t e = S[r + 1];
        const uint32_t strand = fwd < rev ? 0u : 1u;
        py = (e - 1) << 1 | strand | (closed ? 0x80000000u : 0u);
        if (closed) {
          const uint32_t sp = e - S[r + 1 - k >= 0 ? r + 1 - k : 0];
          if (sp < 256) x = mix64(strand ? rev : fwd, mask) << 8 | (uint64_t)sp;
        }
      }
      const bool member = kept || amb;
      const uint64_t mm = __ballot(member);
      if (member) {
        const int idx = ns + __builtin_popcountll(mm & below);
        X[idx] = x, PY[idx] = py;
      }
      ns += __builtin_popcountll(mm);
    }
    __syncthreads();
    // ---- segments: the window passes over every maximal stretch of entries with l >= k (bit 31 of PY) -----------------------------
    const uint64_t yhi = (uint64_t)rd.rid << 32;
    const uint64_t so = off_by_list ? slab_off[it] : slab_off[slot], cap = (off_by_list ? slab_off[it + 1] : slab_off[slot + 1]) - so;
    pgx_mm128 *dst = slab + so;
    // Writes are guarded by the slab's capacity, and whether the read fits is decided at the end from what SURVIVES: a segment writes its
    // pending element before the count steps back over it, so the highest place written can be one past the final count -- in a slab of
    // exactly that count (the second pass) the pending element is the one write that is dropped, and nothing is lost.
    uint32_t nout = 0;
    auto segment = [&](int a, int b) {
      const uint32_t before = nout;
      bool dropped = false;   // (a write past the capacity: the final count says whether it mattered)
      nout = sketch_windows<true>(X + a, PY + a, WM + a, T1 + a, T2 + a, b - a, w, k, lane, yhi, dst, cap, nout, dropped);
      bool fin = false;   // a finite entry among the segment's last w: its rightmost smallest was emitted last, and is pending
      for (int v = (b - w > a ? b - w : a) + lane; v < b; v += 64) fin |= X[v] != INF;
      if (__ballot(fin) && nout > before) --nout;
      __syncthreads();
    };
    int open = -1;
    uint64_t carry = 0;
    for (int v0 = 0; v0 < ns; v0 += 64) {
      const int v = v0 + lane;
      const uint64_t m = __ballot(v < ns && (PY[v] >> 31));
      const uint64_t pm = m << 1 | carry;
      uint64_t starts = m & ~pm, ends = ~m & pm;   // (an end bit sits on the first entry after a segment)
      while (starts | ends) {
        const int bs = starts ? __builtin_ctzll(starts) : 64, be = ends ? __builtin_ctzll(ends) : 64;
        if (be < bs) {
          segment(open, v0 + be);
          ends &= ends - 1;
        } else {
          open = v0 + bs;
          starts &= starts - 1;
        }
      }
      carry = m >> 63;
    }
    if (carry) segment(open, ns);
    // ---- the end of the sequence (:150): the rightmost smallest of the last w stream entries, if finite ---------------------------
    uint64_t bx = INF;
    int bi = -1;
    for (int v = (ns > w ? ns - w : 0) + lane; v < ns; v += 64) {
      const uint64_t x = X[v];
      if (x <= bx) bx = x, bi = v;
    }
    for (int d = 32; d; d >>= 1) {
      const uint64_t ox = (uint64_t)__shfl_xor((int)(bx >> 32), d, 64) << 32 | (uint32_t)__shfl_xor((int)bx, d, 64);
      const int oi = __shfl_xor(bi, d, 64);
      if (oi >= 0 && (bi < 0 || ox < bx || (ox == bx && oi > bi))) bx = ox, bi = oi;
    }
    if (bx != INF) {
      if (nout < cap && lane == 0) dst[nout] = pgx_mm128{bx, yhi | (uint64_t)(PY[bi] & 0x7fffffffu)};
      ++nout;
    }
    const bool anyover = nout > cap;   // an element at or past the capacity survives iff the final count is above it
    if (lane == 0) {
      counts[slot] = anyover ? 0u : nout;
      need[slot] = nout;
      if (anyover) flags[slot] = 1;
    }
    __syncthreads();
  }
}

}  // namespace

// k_sketch_hpc over n reads: slots slot0 .. slot0 + n - 1 of d_reads (d_list == nullptr), or the listed slots; lens[i] = length of the
// i-th of them.  off_by_list: d_slab_off counts per list position, not per slot.  A read that outgrows its slab is flagged, and
// d_need[slot] says how many elements it has.  Entry scratch as k_sketch_general's (36 B per base), in batches of at most ~256 Mbases.
void launch_sketch_hpc(const pgx_seqdb *db, const ReadDesc *d_reads, const std::vector<uint32_t> &lens, const uint32_t *d_list, int w, int k,
                       pgx_mm128 *d_slab, const uint64_t *d_slab_off, int off_by_list, uint32_t *d_counts, uint32_t *d_flags,
                       uint32_t *d_need) {
  hipStream_t st = ctx().stream;
  PGX_REQUIRE(db->d_seq.p, PGX_ESTATE,
              "the seqdb's bytes were released or compacted (pgx_seqdb_release_bytes / pgx_seqdb_compact_bytes): the homopolymer-compressed sketch reads them");
  if (lens.empty()) return;
  // every batch's scratch offsets (they restart at 0 with a batch) in one upload, the scratch sized for the largest batch: the launches
  // follow each other on the stream, which orders their use of the scratch, and the host waits once, at the end
  const uint64_t batch_bases = sketch_batch_bases();
  std::vector<uint64_t> so(lens.size());
  std::vector<size_t> first{0};
  uint64_t acc = 0, most = 0;
  for (size_t i = 0; i < lens.size(); ++i) {
    if (i > first.back() && acc + lens[i] > batch_bases) first.push_back(i), acc = 0;
    so[i] = acc;
    acc += (uint64_t)lens[i] + 1;
    most = std::max(most, acc);
  }
  first.push_back(lens.size());
  uint64_t *d_so = ws<uint64_t>("sk.hpc_off", so.size());
  uint64_t *X = ws<uint64_t>("sk.gen_h", most), *WMv = ws<uint64_t>("sk.gen_wm", most);
  uint64_t *T1 = ws<uint64_t>("sk.gen_t1", most), *T2 = ws<uint64_t>("sk.gen_t2", most);
  uint32_t *PY = ws<uint32_t>("sk.gen_py", most);
  PGX_HIP(hipMemcpyAsync(d_so, so.data(), so.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  for (size_t b = 0; b + 1 < first.size(); ++b) {
    const size_t b0 = first[b], b1 = first[b + 1];
    const unsigned grid = stride_grid(b1 - b0, 16);
    hipLaunchKernelGGL(k_sketch_hpc, dim3(grid), dim3(64), 0, st, db->d_seq.p, d_reads, d_list ? d_list + b0 : nullptr, (uint32_t)b0,
                       (uint32_t)(b1 - b0), w, k, d_so + b0, X, PY, WMv, T1, T2, d_slab, off_by_list ? d_slab_off + b0 : d_slab_off, off_by_list,
                       d_counts, d_flags, d_need);
    PGX_HIP(hipGetLastError());
  }
  sync();  // (so[] is a local)
}

}  // namespace pgx
