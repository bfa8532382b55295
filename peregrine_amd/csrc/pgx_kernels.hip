// pgx_kernels.hip -- gfx950 device code of libpgx.so (index stage + banded O(ND) confirmation).
//
// Kernels (each cites the reference routine whose results it must reproduce bit-for-bit):
//   (reads with ambiguous bases -- and whatever else a closed-form kernel flags -- are cut into runs of unambiguous bases that
//    the same closed-form kernels sketch; pgx_sketch_n.hip)
//   k_sketch_general : mm_sketch      closed form for any (w, k), one wavefront per read, entries in global scratch
//   k_sketch_wave    : mm_sketch      closed form, one wavefront per read            (pgx_sketch_fast.hip)
//   k_reduce_*       : mm_reduce      src/shmr_reduce.c:53-90
//   count            : mm_count       src/shmr_utils.c:131-160  radix sort + run-length
//   k_align_ph       : ovlp_match     src/DWmatch.c:66-204      eight candidates per wavefront         (pgx_align.hip)
#include <algorithm>

#include "pgx_internal.h"
#include "pgx_sketch_win.h"

namespace pgx {

// =========================================================================================================
// mm_reduce (src/shmr_reduce.c:53-90), data-parallel restatement:
//   element t of a read segment [s, e) closes the window [t-rs+1, t] once t-s >= rs-1; the winner is the
//   smallest x>>8 with ties to the lowest ring slot ((t'-s) % rs); it is emitted iff its y differs from the
//   winner of the previous window (== the last emitted element; the first window of a read always emits).
// =========================================================================================================
__global__ void k_mark_starts(const pgx_mm128 *__restrict__ in, size_t n, uint8_t *__restrict__ flag) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  flag[t] = (t == 0) || ((in[t].y >> 32) != (in[t - 1].y >> 32));
}

__device__ __forceinline__ size_t seg_start_of(const uint64_t *starts, uint32_t nseg, size_t t) {
  uint32_t lo = 0, hi = nseg;  // last start <= t
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (starts[mid] <= t) lo = mid;
    else hi = mid;
  }
  return starts[lo];
}

__device__ __forceinline__ pgx_mm128 reduce_winner(const pgx_mm128 *in, size_t s, size_t t, int rs) {
  // window elements t-rs+1 .. t ; slot of element u is (u - s) % rs
  pgx_mm128 best = in[t - rs + 1];
  uint64_t bh = best.x >> 8;
  int bslot = (int)((t - rs + 1 - s) % (size_t)rs);
  for (int j = 1; j < rs; ++j) {
    const size_t u = t - rs + 1 + j;
    const pgx_mm128 e = in[u];
    const uint64_t h = e.x >> 8;
    const int slot = (int)((u - s) % (size_t)rs);
    if (h < bh || (h == bh && slot < bslot)) best = e, bh = h, bslot = slot;
  }
  return best;
}

__global__ void k_reduce_flag(const pgx_mm128 *__restrict__ in, size_t n, const uint64_t *__restrict__ starts,
                              uint32_t nseg, int rs, pgx_mm128 *__restrict__ win, uint8_t *__restrict__ flag) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const size_t s = seg_start_of(starts, nseg, t);
  const size_t off = t - s;
  uint8_t f = 0;
  pgx_mm128 w{0, 0};
  if (off >= (size_t)rs - 1) {
    w = reduce_winner(in, s, t, rs);
    if (off == (size_t)rs - 1) f = 1;
    else f = reduce_winner(in, s, t - 1, rs).y != w.y;
  }
  win[t] = w;
  flag[t] = f;
}

void dev_reduce(const pgx_mm128 *d_in, size_t n, int rs, DevBuf<pgx_mm128> &out, size_t &n_out) {
  n_out = 0;
  if (n == 0) { out.alloc(0); return; }
  hipStream_t st = ctx().stream;
  KernelTimer tm("reduce", n);
  DevBuf<uint8_t> flag(n);
  DevBuf<uint64_t> starts(n);  // worst case every element its own read
  PrimWs tmp;
  hipLaunchKernelGGL(k_mark_starts, dim3(cdiv(n, 256)), dim3(256), 0, st, d_in, n, flag.p);
  const uint64_t nseg = select_indices(flag.p, n, starts.p, &tmp);
  DevBuf<pgx_mm128> win(n);
  hipLaunchKernelGGL(k_reduce_flag, dim3(cdiv(n, 256)), dim3(256), 0, st, d_in, n, starts.p, (uint32_t)nseg, rs, win.p,
                     flag.p);
  out.alloc(n);
  n_out = (size_t)select_values(win.p, flag.p, n, out.p, &tmp);
}

// =========================================================================================================
// mm_count: multiplicity of x>>8.  Radix sort + run-length encode; output sorted by mer.
// =========================================================================================================
__global__ void k_extract_hash(const pgx_mm128 *__restrict__ in, size_t n, uint64_t *__restrict__ keys) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) keys[t] = in[t].x >> 8;
}
__global__ void k_pack_counts(const uint64_t *__restrict__ mer, const uint32_t *__restrict__ cnt, size_t n,
                              pgx_mm_count *__restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) out[t] = pgx_mm_count{mer[t], cnt[t], 0u};
}

void dev_count(const pgx_mm128 *d_in, size_t n, int kmer_bits, DevBuf<pgx_mm_count> &out, size_t &n_out) {
  n_out = 0;
  if (n == 0) { out.alloc(0); return; }
  hipStream_t st = ctx().stream;
  KernelTimer tm("count", n);
  DevBuf<uint64_t> keys(n), sorted(n), uniq(n);
  DevBuf<uint32_t> cnt(n);
  PrimWs tmp;
  hipLaunchKernelGGL(k_extract_hash, dim3(cdiv(n, 256)), dim3(256), 0, st, d_in, n, keys.p);
  sort_keys(keys.p, sorted.p, n, 0, kmer_bits, &tmp);
  n_out = (size_t)run_lengths(sorted.p, uniq.p, cnt.p, n, &tmp);
  out.alloc(n_out);
  if (n_out) hipLaunchKernelGGL(k_pack_counts, dim3(cdiv(n_out, 256)), dim3(256), 0, st, uniq.p, cnt.p, n_out, out.p);
}

// =========================================================================================================
// sketch driver
// =========================================================================================================
// slab of read i: len / slab_div + slab_min elements from off[i] on (off: n + 1 entries); returns the bases of the reads
static uint64_t slab_offsets(const std::vector<ReadDesc> &reads, uint64_t slab_div, uint64_t slab_min, std::vector<uint64_t> &off) {
  off.assign(reads.size() + 1, 0);
  uint64_t bases = 0;
  for (size_t i = 0; i < reads.size(); ++i) {
    off[i + 1] = off[i] + (uint64_t)reads[i].len / slab_div + slab_min;
    bases += reads[i].len;
  }
  return bases;
}

// Where a read's final list lives: in its own slab (slab + slab_off[slot]) unless the pass that finished it wrote elsewhere -- exact
// slabs, the run-by-run path's lists -- and said so in src_of[slot] (nullptr: own slab; a later pass overwrites an earlier one's entry).
__global__ void k_set_sources(const pgx_mm128 **__restrict__ src_of, const uint32_t *__restrict__ list, uint32_t n_list,
                              const pgx_mm128 *__restrict__ base, const uint64_t *__restrict__ off) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_list) src_of[list[i]] = base + off[i];
}
static void set_sources(const pgx_mm128 **d_src_of, const uint32_t *d_list, uint32_t n_list, const pgx_mm128 *base, const uint64_t *d_off) {
  if (n_list) hipLaunchKernelGGL(k_set_sources, dim3(cdiv(n_list, 256)), dim3(256), 0, ctx().stream, d_src_of, d_list, n_list, base, d_off);
}
__global__ void k_gather_slabs(const pgx_mm128 *__restrict__ slab, const uint64_t *__restrict__ slab_off,
                               const pgx_mm128 *const *__restrict__ src_of, uint32_t n, const uint32_t *__restrict__ counts,
                               const uint64_t *__restrict__ out_off, pgx_mm128 *__restrict__ out) {
  const uint32_t slot = blockIdx.x;
  if (slot >= n) return;
  const pgx_mm128 *src = src_of[slot] ? src_of[slot] : slab + slab_off[slot];
  pgx_mm128 *dst = out + out_off[slot];
  const uint32_t c = counts[slot];
  for (uint32_t i = threadIdx.x; i < c; i += blockDim.x) dst[i] = src[i];
}
__global__ void k_need_of_list(const uint32_t *__restrict__ need, const uint32_t *__restrict__ list, uint32_t n, uint64_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = need[list[i]];
}

// =========================================================================================================
// k_sketch_general: the closed form of pgx_sketch_fast.hip (see its header) for ANY window and k-mer size
// (0 < w < 256, 0 < k <= 28; pg_run.py exposes both as --shimmer-w / --shimmer-k), one wavefront per read, three
// passes over the read's ENTRIES (non strand-ambiguous k-mers, numbered in position order) kept in global scratch:
//   1. entries: every lane builds the k-mer ending at its base, canonical strand, 64-bit hash (mm_sketch.c:23-32);
//      ballot-compacted to H[] (hash) and PY[] (position << 1 | strand);
//   2. WM[s] = minimum hash of the full window of w entries starting at s, and GX[p] = maximum of WM over the windows that
//      contain p, both in O(1) per entry from running extrema over blocks of w (van Herk / Gil-Werman);
//   3. entry p is emitted iff GX[p] == H[p] (some full window containing it has its hash as minimum), corrected for the first window
//      (m = rightmost smallest of entries 0..w-2: its ties are always emitted, m itself iff H[w-1] > H[m]); a read with
//      fewer than w entries emits only its rightmost smallest entry.
// O(k) work per base for the k-mers, O(1) per entry for the windows.
// Reads with an ambiguous base (the state machine restarts there) or more minimizers than their slab holds are
// flagged; the caller cuts them into runs of unambiguous bases / gives them larger slabs (pgx_sketch_n.hip).
// =========================================================================================================
__global__ __launch_bounds__(64) void k_sketch_general(const uint8_t *__restrict__ seq, const ReadDesc *__restrict__ reads,
                                                       const uint32_t *__restrict__ list, uint32_t n_list, int w, int k,
                                                       const uint64_t *__restrict__ scr_off, uint64_t *__restrict__ Hs,
                                                       uint32_t *__restrict__ PYs, uint64_t *__restrict__ WMs,
                                                       uint64_t *__restrict__ T1s, uint64_t *__restrict__ T2s,
                                                       pgx_mm128 *__restrict__ slab, const uint64_t *__restrict__ slab_off,
                                                       uint32_t *__restrict__ counts, uint32_t *__restrict__ flags) {
  const int lane = threadIdx.x;
  const uint64_t mask = (1ULL << (2 * k)) - 1, top = 2ULL * (uint64_t)(k - 1);
  for (uint32_t it = blockIdx.x; it < n_list; it += gridDim.x) {
    const uint32_t slot = list ? list[it] : it;
    const ReadDesc rd = reads[slot];
    const uint8_t *s = seq + rd.off;
    const int len = (int)rd.len;
    uint64_t *H = Hs + scr_off[it], *WM = WMs + scr_off[it], *T1 = T1s + scr_off[it], *T2 = T2s + scr_off[it];
    uint32_t *PY = PYs + scr_off[it];
    // ---- pass 1: every lane rolls the two k-mers over 16 consecutive bases (k-1 bases of run-in per lane) -----------
    int n = 0;
    bool bad = false;
    for (int t0 = 0; t0 < len; t0 += 64 * 16) {
      const int start = t0 + lane * 16;
      uint64_t hh[16];
      uint32_t vmask = 0, smask = 0;
      if (start < len) {
        uint64_t fwd = 0, rev = 0;
        for (int j = start - (k - 1) > 0 ? start - (k - 1) : 0; j < start; ++j) {
          const uint64_t c = (uint64_t)(code_of_nibble(s[j]) & 3);
          fwd = (fwd << 2 | c) & mask;
          rev = (rev >> 2) | (3ULL ^ c) << top;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int i = start + u;
          hh[u] = 0;
          if (i < len) {
            const int cc = code_of_nibble(s[i]);
            if (cc > 3) bad = true;
            const uint64_t c = (uint64_t)(cc & 3);
            fwd = (fwd << 2 | c) & mask;
            rev = (rev >> 2) | (3ULL ^ c) << top;
            if (i >= k - 1 && fwd != rev) {
              const uint32_t strand = fwd < rev ? 0u : 1u;
              hh[u] = mix64(strand ? rev : fwd, mask);
              vmask |= 1u << u, smask |= strand << u;
            }
          }
        }
      }
      const int cnt = __builtin_popcount(vmask);
      int incl = cnt;  // wave inclusive scan of the per-lane entry counts
      for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
      }
      int r = n + incl - cnt;
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (vmask >> u & 1u) {
          H[r] = hh[u];
          PY[r] = (uint32_t)(start + u) << 1 | (smask >> u & 1u);
          ++r;
        }
      n += __shfl(incl, 63, 64);
    }
    if (__ballot(bad)) {
      if (lane == 0) counts[slot] = 0, flags[slot] = 1;
      continue;
    }
    __syncthreads();  // (one wavefront per block: orders this wave's global writes before its reads below)
    // ---- passes 2 and 3: the window passes (pgx_sketch_win.h) -------------------------------------------------------
    const uint64_t cap = slab_off[slot + 1] - slab_off[slot];
    bool over = false;
    const uint32_t nout = sketch_windows<false>(H, PY, WM, T1, T2, n, w, k, lane, (uint64_t)rd.rid << 32, slab + slab_off[slot], cap, 0u, over);
    const bool anyover = __ballot(over) != 0;
    if (lane == 0) {
      counts[slot] = anyover ? 0u : nout;
      if (anyover) flags[slot] = 1;
    }
    __syncthreads();
  }
}

// k_sketch_general over the listed reads (d_list == nullptr: slots 0 .. lens.size()-1); lens[i] = length of the i-th listed read.
// Entry scratch (hash, position|strand, window minimum, two running-extremum arrays: 36 B per base) in batches of at most
// ~256 Mbases.
void launch_sketch_general(const pgx_seqdb *db, const ReadDesc *d_reads, const std::vector<uint32_t> &lens, const uint32_t *d_list,
                           int w, int k, pgx_mm128 *d_slab, const uint64_t *d_slab_off, uint32_t *d_counts, uint32_t *d_flags,
                           const uint8_t *bytes) {
  hipStream_t st = ctx().stream;
  if (!bytes) bytes = db->d_seq.p;
  const uint64_t batch_bases = sketch_batch_bases();
  DevBuf<uint32_t> iota;
  if (!d_list) {   // the kernel walks a list: the identity
    std::vector<uint32_t> id(lens.size());
    for (size_t i = 0; i < id.size(); ++i) id[i] = (uint32_t)i;
    iota.alloc(id.size());
    iota.upload(id.data(), id.size());
    sync();
    d_list = iota.p;
  }
  for (size_t b0 = 0; b0 < lens.size();) {
    std::vector<uint64_t> so;
    uint64_t acc = 0;
    size_t b1 = b0;
    while (b1 < lens.size() && (b1 == b0 || acc + lens[b1] <= batch_bases)) so.push_back(acc), acc += lens[b1], ++b1;
    uint64_t *d_so = ws<uint64_t>("sk.gen_off", so.size());
    uint64_t *H = ws<uint64_t>("sk.gen_h", acc), *WMv = ws<uint64_t>("sk.gen_wm", acc);
    uint64_t *T1 = ws<uint64_t>("sk.gen_t1", acc), *T2 = ws<uint64_t>("sk.gen_t2", acc);
    uint32_t *PY = ws<uint32_t>("sk.gen_py", acc);
    PGX_HIP(hipMemcpyAsync(d_so, so.data(), so.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    const unsigned grid = stride_grid(b1 - b0, 16);
    PGX_REQUIRE(bytes, PGX_ESTATE, "the seqdb's bytes were released (pgx_seqdb_release_bytes): the general sketch kernel (other w / k, L0 output) needs them");
    hipLaunchKernelGGL(k_sketch_general, dim3(grid), dim3(64), 0, st, bytes, d_reads, d_list + b0, (uint32_t)(b1 - b0), w, k,
                       d_so, H, PY, WMv, T1, T2, d_slab, d_slab_off, d_counts, d_flags);
    PGX_HIP(hipGetLastError());
    sync();  // (so[] is reused by the next batch)
    b0 = b1;
  }
}

// dev_sketch's hpc form: every read through k_sketch_hpc (pgx_sketch_hpc.hip), which takes ambiguous bases itself; the reads that outgrow
// their slabs once more into slabs of exactly the size the first pass reported (exact / exact_off, named in src_of).  Returns how many.
static uint32_t sketch_hpc_reads(const pgx_seqdb *db, const std::vector<uint32_t> &lens, int w, int k, uint64_t bases, const ReadDesc *d_reads,
                                 pgx_mm128 *slab, const uint64_t *d_slab_off, uint32_t *counts, uint32_t *d_flags, uint32_t *d_list,
                                 const pgx_mm128 **d_src_of, DevBuf<pgx_mm128> &exact, DevBuf<uint64_t> &exact_off) {
  hipStream_t st = ctx().stream;
  const uint32_t n = (uint32_t)lens.size();
  DevBuf<uint32_t> need(n);
  {
    KernelTimer tm("sketch_hpc", bases);
    launch_sketch_hpc(db, d_reads, lens, nullptr, w, k, slab, d_slab_off, 0, counts, d_flags, need.p);
  }
  const uint32_t n_redo = select_flagged(d_flags, n, d_list);
  if (!n_redo) return 0;
  KernelTimer tm("sketch_hpc_redo", 0);
  std::vector<uint32_t> redo(n_redo), redo_lens(n_redo);
  PGX_HIP(hipMemcpyAsync(redo.data(), d_list, (size_t)n_redo * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  sync();
  for (uint32_t i = 0; i < n_redo; ++i) redo_lens[i] = lens[redo[i]];
  exact_off.alloc((size_t)n_redo + 1);
  hipLaunchKernelGGL(k_need_of_list, dim3(cdiv(n_redo, 256)), dim3(256), 0, st, need.p, d_list, n_redo, exact_off.p + 1);
  const uint64_t total = scan_to_total(exact_off.p + 1, exact_off.p, n_redo);
  exact.alloc(total ? total : 1);
  PGX_HIP(hipMemsetAsync(d_flags, 0, (size_t)n * sizeof(uint32_t), st));
  launch_sketch_hpc(db, d_reads, redo_lens, d_list, w, k, exact.p, exact_off.p, 1, counts, d_flags, need.p);
  uint32_t *d_anybad = ws<uint32_t>("sk.hpc_bad", 1);
  PGX_HIP(hipMemsetAsync(d_anybad, 0, sizeof(uint32_t), st));
  reduce_max(d_flags, d_anybad, n);
  uint32_t anybad = 0;
  PGX_HIP(hipMemcpyAsync(&anybad, d_anybad, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  sync();
  PGX_REQUIRE(!anybad, PGX_EARG, "a read outgrew a slab of exactly the size its first pass reported");
  set_sources(d_src_of, d_list, n_redo, exact.p, exact_off.p);
  return n_redo;
}

// Level-0 minimizers of `reads`, one contiguous list in `reads` order.  Every read goes through the closed-form kernel of the
// (w, k) -- k_sketch_wave for k = 16 and w in {64, 80, 96, 128}, k_sketch_general otherwise -- single pass into per-read slabs, then
// an ordered gather; the reads it flags (an ambiguous base, a slab outgrown by low-complexity sequence) are cut into runs of
// unambiguous bases that the same kernels sketch (pgx_sketch_n.hip: dev_sketch_nreads).  n_literal (name kept from the C-ABI's
// reads_literal): how many reads took that second path.
// hpc: mm_sketch's is_hpc = 1 (sketch_hpc_reads above; n_literal counts the reads sketched a second time).
void dev_sketch(const pgx_seqdb *db, const std::vector<ReadDesc> &reads, int w, int k, DevBuf<pgx_mm128> &out,
                size_t &n_out, uint32_t *n_literal, bool hpc) {
  n_out = 0;
  if (n_literal) *n_literal = 0;
  const uint32_t n = (uint32_t)reads.size();
  if (n == 0) { out.alloc(0); return; }
  hipStream_t st = ctx().stream;
  std::vector<uint32_t> lens(n);
  for (uint32_t i = 0; i < n; ++i) {
    PGX_REQUIRE(reads[i].len < (1u << 30), PGX_EARG, "read %u is longer than 2^30 bases", reads[i].rid);
    lens[i] = reads[i].len;
  }
  // slab capacity: 5x the expected density 2/(w+1); a read that outgrows it (low complexity) takes the second path
  std::vector<uint64_t> slab_off;
  const uint64_t bases = slab_offsets(reads, 8, 64, slab_off);
  DevBuf<ReadDesc> d_reads(n);
  DevBuf<uint64_t> d_slab_off(n + 1), offs(n + 1);
  DevBuf<uint32_t> counts(n), d_flags(n), d_list(n);
  DevBuf<const pgx_mm128 *> d_src_of(n);
  DevBuf<pgx_mm128> slab(slab_off[n]);
  d_reads.upload(reads.data(), n);
  d_slab_off.upload(slab_off.data(), n + 1);
  PGX_HIP(hipMemsetAsync(counts.p, 0, n * sizeof(uint32_t), st));
  PGX_HIP(hipMemsetAsync(d_flags.p, 0, n * sizeof(uint32_t), st));
  PGX_HIP(hipMemsetAsync(d_src_of.p, 0, n * sizeof(pgx_mm128 *), st));
  DevBuf<pgx_mm128> nl0;
  DevBuf<uint64_t> nl0_off;
  if (hpc) {
    const uint32_t n_redo = sketch_hpc_reads(db, lens, w, k, bases, d_reads.p, slab.p, d_slab_off.p, counts.p, d_flags.p, d_list.p, d_src_of.p, nl0, nl0_off);
    if (n_literal) *n_literal = n_redo;
  } else {
    // (w, k) outside the specialised kernel's set: the general closed-form kernel takes the wave kernel's place
    if (k == 16 && (w == 64 || w == 80 || w == 96 || w == 128)) {
      KernelTimer tm("sketch", bases);
      launch_sketch_wave(db, d_reads.p, nullptr, n, w, k, slab.p, d_slab_off.p, counts.p, d_flags.p);
    } else {
      KernelTimer tm("sketch_general", bases);
      launch_sketch_general(db, d_reads.p, lens, nullptr, w, k, slab.p, d_slab_off.p, counts.p, d_flags.p);
    }
    // the flagged reads: segments of unambiguous bases through the same kernels, exact slabs on demand
    const uint32_t n_second = select_flagged(d_flags.p, n, d_list.p);
    if (n_second) {
      KernelTimer tm("sketch_nreads", 0);
      uint64_t tot2 = 0;
      dev_sketch_nreads(db, d_reads.p, d_list.p, n_second, w, k, nl0, nl0_off, &tot2);
      dev_scatter_counts(counts.p, d_list.p, n_second, nl0_off.p, nullptr);
      set_sources(d_src_of.p, d_list.p, n_second, nl0.p, nl0_off.p);
    }
    if (n_literal) *n_literal = n_second;
  }
  n_out = (size_t)scan_to_total(counts.p, offs.p, n);
  out.alloc(n_out);
  if (n_out == 0) return;
  {
    KernelTimer tm("sketch_gather", bases);
    hipLaunchKernelGGL(k_gather_slabs, dim3(n), dim3(64), 0, st, slab.p, d_slab_off.p, d_src_of.p, n, counts.p, offs.p, out.p);
  }
  sync();
}

// =========================================================================================================
// k_reduce_read: mm_reduce (src/shmr_reduce.c:53-90) applied `levels` times to ONE read's minimizers, in LDS, in place
// in the read's slab.  Same restatement as k_reduce_flag (winner = smallest x>>8, ties to the lowest ring slot
// offset % rs; emitted iff its y differs from the previous window's winner; the first window always emits).
// A read the sketch kernel flagged is left alone; one whose list is longer than RMAX gets flag bit 256: the run-by-run path, which
// reduces lists of any length (k_reduce_long), takes both.
// =========================================================================================================
constexpr int RMAX = 1024;  // minimizers per read handled in LDS (a 15 kb read has ~375 at w = 80)

__global__ __launch_bounds__(64) void k_reduce_read(pgx_mm128 *__restrict__ slab, const uint64_t *__restrict__ slab_off,
                                                    const ReadDesc *__restrict__ reads,
                                                    const uint32_t *__restrict__ counts0, uint32_t *__restrict__ flags,
                                                    uint32_t n, int rs, int levels, uint32_t *__restrict__ counts_top) {
  __shared__ uint64_t sx[RMAX];
  __shared__ uint32_t sy[RMAX];
  const int lane = threadIdx.x;
  const uint32_t slot = blockIdx.x;
  if (slot >= n) return;
  const uint32_t c0 = counts0[slot];
  const uint32_t flagged = flags[slot];
  if (flagged || c0 > (uint32_t)RMAX) {
    if (lane == 0) {
      counts_top[slot] = 0;
      if (!flagged) flags[slot] = 256u;
    }
    return;
  }
  pgx_mm128 *p = slab + slab_off[slot];
  for (uint32_t i = lane; i < c0; i += 64) {
    const pgx_mm128 e = p[i];
    sx[i] = e.x, sy[i] = (uint32_t)e.y;
  }
  int ncur = (int)c0;
  for (int lv = 0; lv < levels; ++lv) {
    __syncthreads();
    uint64_t wx[RMAX / 64];
    uint32_t wy[RMAX / 64];
    uint32_t emit = 0;
    uint32_t carry = 0;
#pragma unroll
    for (int r = 0; r < RMAX / 64; ++r) {
      const int t = lane + 64 * r;
      const bool valid = t < ncur && t >= rs - 1;
      uint64_t bx = 0;
      uint32_t by = 0;
      if (valid) {
        int u = t - rs + 1, sl = (t + 1) % rs;  // slot of element u is u % rs (offset within the read)
        bx = sx[u], by = sy[u];
        uint64_t bh = bx >> 8;
        int bsl = sl;
        for (int j = 1; j < rs; ++j) {
          ++u;
          if (++sl == rs) sl = 0;
          const uint64_t x = sx[u], hsh = x >> 8;
          if (hsh < bh || (hsh == bh && sl < bsl)) bx = x, by = sy[u], bh = hsh, bsl = sl;
        }
      }
      uint32_t prevy = (uint32_t)__shfl_up((int)by, 1, 64);
      if (lane == 0) prevy = carry;
      carry = (uint32_t)__builtin_amdgcn_readlane((int)by, 63);
      if (valid && (t == rs - 1 || by != prevy)) emit |= 1u << r;
      wx[r] = bx, wy[r] = by;
    }
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int r = 0; r < RMAX / 64; ++r) {
      const bool em = (emit >> r) & 1u;
      const uint64_t m = __ballot(em);
      if (em) {
        const int idx = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        sx[idx] = wx[r], sy[idx] = wy[r];
      }
      base += __builtin_popcountll(m);
    }
    ncur = base;
  }
  __syncthreads();
  const uint64_t yhi = (uint64_t)reads[slot].rid << 32;
  for (int i = lane; i < ncur; i += 64) p[i] = pgx_mm128{sx[i], yhi | sy[i]};
  if (lane == 0) counts_top[slot] = (uint32_t)ncur;
}

// =========================================================================================================
// the fused index path's driver: one decision, then a function per pass over an IndexRun
// =========================================================================================================
// Which first pass a (w, k, rs, levels) gets, and the slab divisor that goes with it (slab of a read: len / slab_div + slab_min elements).
//   blk:  k_sketch_blk -- block-per-lane closed form fused with the streaming reduce, L0 never leaves the CU, HBM traffic == the
//         algorithmic 1.04 B/base.  Only the TOP-level list reaches the slab (1 element per 408 bases at l = 2, per 142 at l = 1), so
//         the slabs are len / 48 resp. len / 24: six and three times the expected list.  (Rounds 1-4 reserved len / 8 for every path: 27 GB
//         of workspace for one index chunk of full-size configs[3], resident through the overlap stages too.)
//   else: k_sketch_wave + k_reduce_read (w = 64 / 96 / 128, or a reduction factor above RCARRY + 1): L0 goes through the slab, len / 8.
// (PGX_SLAB_DIV / PGX_SLAB_MIN: test knobs that make reads outgrow their slabs)
struct FirstPass {
  bool blk;
  uint64_t slab_div, slab_min;
};
static FirstPass choose_first_pass(int w, int k, int rs, int levels) {
  FirstPass fp;
  fp.blk = sketch_blk_supported(w, k, rs, levels);
  fp.slab_div = getenv("PGX_SLAB_DIV") ? std::max(1ll, atoll(getenv("PGX_SLAB_DIV"))) : !fp.blk ? 8 : levels >= 2 ? 48 : 24;
  fp.slab_min = getenv("PGX_SLAB_MIN") ? std::max(1ll, atoll(getenv("PGX_SLAB_MIN"))) : 64;
  return fp;
}

// What the passes of one call share.  A read is UNFINISHED iff its flag word is non-zero (the bits say why: flag_histogram); a pass takes
// the list of the reads flagged for it, clears their flags, and the kernels it runs flag again what they could not finish.
struct IndexRun {
  const pgx_seqdb *db;
  int w, k, rs, levels;
  uint32_t n;
  uint64_t bases;
  const ReadDesc *d_reads;
  const uint64_t *d_slab_off;
  pgx_mm128 *slab;
  const pgx_mm128 **d_src_of;               // per read: k_gather_slabs' rule
  uint32_t *d_cnt0, *d_flags, *d_ctop;      // per read: level-0 elements (k_sketch_wave -> k_reduce_read only), flag word, final elements
  uint64_t *d_offs;                         // n + 1: the reads' offsets in the final list
  uint32_t *d_list, *d_need;                // the current pass's reads; elements a read needs when it outgrew its slab
  DevBuf<pgx_mm128> run_lists;              // the run-by-run path's final lists (read by the gather)
  bool trace;
};

static void flag_histogram(const IndexRun &r, uint32_t n_listed, const char *what) {
  std::vector<uint32_t> hf(r.n);
  PGX_HIP(hipMemcpy(hf.data(), r.d_flags, (size_t)r.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  unsigned why[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t f : hf)
    for (int b = 0; b < 9; ++b) why[b] += (f >> b) & 1u;
  fprintf(stderr, "[pgx] index: %u of %u reads %s (short %u, ambiguous base %u, two drops in a tile %u, drop in the first window %u, close drops %u, "
          "tie burst %u / %u, slab %u, list longer than the in-LDS reduce holds %u)\n", n_listed, r.n, what, why[0], why[1], why[2], why[3], why[4],
          why[5], why[6], why[7], why[8]);
}

// The plan: read descriptors and slab offsets, computed and uploaded once per (plan, w, k, slab_div) -- the device half of the database's
// read selection.  false: some read is not for the closed-form kernels (the caller runs the general path).
static bool index_plan(pgx_seqdb::IndexPlan &pl, const std::vector<ReadDesc> &reads, int w, int k, const FirstPass &fp) {
  if (pl.plan_div == fp.slab_div && pl.plan_w == w && pl.plan_k == k) return pl.plan_ok;
  const size_t n = reads.size();
  {
    MemTag plan_tag("index.plans");
    pl.d_reads.alloc(n), pl.d_slab_off.alloc(n + 1);
  }
  pl.plan_div = 0;
  std::vector<uint64_t> slab_off;
  pl.plan_bases = slab_offsets(reads, fp.slab_div, fp.slab_min, slab_off);
  pl.plan_ok = std::all_of(reads.begin(), reads.end(), [&](const ReadDesc &rd) { return sketch_wave_eligible(rd, w, k); });
  if (pl.plan_ok) {
    pl.d_reads.upload(reads.data(), n);
    pl.d_slab_off.upload(slab_off.data(), n + 1);
    sync();  // (slab_off is a local)
  }
  pl.slab_total = slab_off[n], pl.plan_w = w, pl.plan_k = k, pl.plan_div = fp.slab_div;
  return pl.plan_ok;
}

static void index_workspaces(IndexRun &r, const pgx_seqdb::IndexPlan &pl) {
  const size_t n = r.n;
  r.bases = pl.plan_bases, r.d_reads = pl.d_reads.p, r.d_slab_off = pl.d_slab_off.p;
  const size_t per_read = sizeof(pgx_mm128 *) + 3 * sizeof(uint32_t);   // [src_of | counts0 | flags | counts_top], cleared together
  r.d_src_of = (const pgx_mm128 **)ws_raw("ix.cnt", n * per_read);
  r.d_cnt0 = (uint32_t *)(r.d_src_of + n), r.d_flags = r.d_cnt0 + n, r.d_ctop = r.d_flags + n;
  r.d_offs = ws<uint64_t>("ix.offs", n + 1);
  r.d_list = ws<uint32_t>("ix.redo", n);
  r.d_need = ws<uint32_t>("ix.need", n);
  r.slab = ws<pgx_mm128>("ix.slab", pl.slab_total);
  PGX_HIP(hipMemsetAsync(r.d_src_of, 0, n * per_read, ctx().stream));
}

static void first_pass(const IndexRun &r, const FirstPass &fp) {
  if (fp.blk) {
    KernelTimer tm("sketch", r.bases);
    launch_sketch_blk(r.db, r.d_reads, r.n, r.rs, r.levels, r.slab, r.d_slab_off, r.d_ctop, r.d_flags);
    return;
  }
  {
    KernelTimer tm("sketch", r.bases);
    launch_sketch_wave(r.db, r.d_reads, nullptr, r.n, r.w, r.k, r.slab, r.d_slab_off, r.d_cnt0, r.d_flags);
  }
  KernelTimer tm("reduce", r.bases);
  hipLaunchKernelGGL(k_reduce_read, dim3(r.n), dim3(64), 0, ctx().stream, r.slab, r.d_slab_off, r.d_reads, r.d_cnt0, r.d_flags, r.n, r.rs,
                     r.levels, r.d_ctop);
}

// What k_sketch_blk flagged (two drops close together, bursts of ties, very short reads ...), once more on k_sketch_wave in its fused
// form, into the same slabs.  It flags the reads that outgrow their slab and reports how many elements each has (d_need).
static void redo_on_wave(const IndexRun &r, uint32_t n_list) {
  dev_mark_slots(r.d_flags, r.d_list, n_list, 0u);
  launch_sketch_fused_list(r.db, r.d_reads, r.d_list, n_list, r.rs, r.levels, r.slab, r.d_slab_off, r.d_ctop, r.d_flags, r.d_need, 0);
}

// Low-complexity reads (a homopolymer or a short-period tandem array makes every position a tied minimum, on every level) can
// outgrow their slab: exactly those reads are redone into slabs of exactly the size the wave kernel reported.  (Round 1 redid the
// WHOLE chunk on the slow general path when a single read was left over: 0.4 s instead of 15 ms at 9 Gbases with 1 % low-complexity
// sequence.)  Reads with an ambiguous base are not listed: the kernel would walk them whole only to flag them again.
static void redo_into_exact_slabs(const IndexRun &r) {
  const uint32_t n_list = select_flagged(r.d_flags, r.n, r.d_list, 2u);
  if (!n_list) return;
  uint64_t *d_off = ws<uint64_t>("ix.off2", (size_t)n_list + 1);
  hipLaunchKernelGGL(k_need_of_list, dim3(cdiv(n_list, 256)), dim3(256), 0, ctx().stream, r.d_need, r.d_list, n_list, d_off + 1);
  const uint64_t total = scan_to_total(d_off + 1, d_off, n_list);
  pgx_mm128 *exact = ws<pgx_mm128>("ix.slab2", total);
  dev_mark_slots(r.d_flags, r.d_list, n_list, 0u);
  launch_sketch_fused_list(r.db, r.d_reads, r.d_list, n_list, r.rs, r.levels, exact, d_off, r.d_ctop, r.d_flags, nullptr, 1);
  set_sources(r.d_src_of, r.d_list, n_list, exact, d_off);
  if (r.trace) fprintf(stderr, "[pgx] index: %u reads outgrew their slabs and were redone into exact ones (%llu elements)\n", n_list, (unsigned long long)total);
}

// Every read still flagged -- an ambiguous base (mm_sketch.c:112-113), a list k_reduce_read cannot hold, whatever else the passes above
// left -- is cut into runs of unambiguous bases, every run sketched by the unfused closed-form kernel, the read's list assembled and
// reduced per read (pgx_sketch_n.hip).  That path takes any read: nothing is flagged after it.
static void run_by_run(IndexRun &r, uint32_t n_list) {
  DevBuf<pgx_mm128> l0;
  DevBuf<uint64_t> off;
  DevBuf<uint32_t> cnt;
  uint64_t total = 0;
  dev_sketch_nreads(r.db, r.d_reads, r.d_list, n_list, r.w, r.k, l0, off, &total);
  dev_reduce_nreads(l0, off, n_list, total, r.rs, r.levels, r.run_lists, cnt);
  dev_scatter_counts(r.d_ctop, r.d_list, n_list, nullptr, cnt.p);
  set_sources(r.d_src_of, r.d_list, n_list, r.run_lists.p, off.p);
  dev_mark_slots(r.d_flags, r.d_list, n_list, 0u);
  if (r.trace) fprintf(stderr, "[pgx] index: %u reads sketched run by run (%llu level-0 minimizers)\n", n_list, (unsigned long long)total);
}

static void gather(const IndexRun &r, const pgx_mm128 **d_top, size_t *n_top) {
  const uint64_t total = scan_to_total(r.d_ctop, r.d_offs, r.n);
  pgx_mm128 *top = ws<pgx_mm128>("ix.top", total);
  if (total) {
    KernelTimer tm("sketch_gather", r.bases);
    hipLaunchKernelGGL(k_gather_slabs, dim3(r.n), dim3(64), 0, ctx().stream, r.slab, r.d_slab_off, r.d_src_of, r.n, r.d_ctop, r.d_offs, top);
    if (r.run_lists.p) sync();   // (run_lists goes back to the block cache with the IndexRun)
  }
  *d_top = top, *n_top = (size_t)total;
}

bool dev_index_fused(const pgx_seqdb *db, const std::vector<ReadDesc> &reads, int w, int k, int rs, int levels,
                     const pgx_mm128 **d_top, size_t *n_top, pgx_seqdb::IndexPlan *plan, uint32_t *n_second) {
  if (n_second) *n_second = 0;
  if (reads.empty() || levels < 1 || levels > 2 || rs < 1) return false;
  IndexRun r{};
  r.db = db, r.w = w, r.k = k, r.rs = rs, r.levels = levels, r.n = (uint32_t)reads.size(), r.trace = getenv("PGX_TRACE") != nullptr;
  const double t0 = wall_ms();
  const FirstPass fp = choose_first_pass(w, k, rs, levels);
  pgx_seqdb::IndexPlan own;   // (no plan: for this call only)
  pgx_seqdb::IndexPlan &pl = plan ? *plan : own;
  if (!index_plan(pl, reads, w, k, fp)) return false;
  index_workspaces(r, pl);
  if (r.trace) {
    sync();
    fprintf(stderr, "[pgx] index: plan (slab offsets, descriptors, workspaces, uploads) %.2f ms\n", wall_ms() - t0);
  }
  first_pass(r, fp);
  if (fp.blk) {   // (k_sketch_wave + k_reduce_read have no second closed form: what they flag goes straight to the run-by-run path)
    const uint32_t n_redo = select_flagged(r.d_flags, r.n, r.d_list, 2u);
    if (r.trace) flag_histogram(r, n_redo, "redone by the fused wave kernel");
    if (n_redo) {
      KernelTimer tm("sketch_redo", 0);
      redo_on_wave(r, n_redo);
      redo_into_exact_slabs(r);
    }
  }
  const uint32_t n_runs = select_flagged(r.d_flags, r.n, r.d_list);
  if (r.trace && n_runs) flag_histogram(r, n_runs, "left for the run-by-run path");
  if (n_runs) {
    KernelTimer tm("sketch_nreads", 0);
    run_by_run(r, n_runs);
  }
  if (n_second) *n_second = n_runs;
  gather(r, d_top, n_top);
  if (r.trace) fprintf(stderr, "[pgx] index: sketch + reduce done at +%.2f ms\n", wall_ms() - t0);
  return true;
}

}  // namespace pgx
