// pgx_side.hip -- what a COMPACTED read database keeps of its bytes (pgx_seqdb_compact_bytes), and the byte view the byte-wise kernels read on it.
//
// A database with ambiguous bases cannot live on its 2-bit packs alone: a flagged read (d_nflag, pgx_pack.hip) is sketched run by run
// (pgx_sketch_n.hip, mm_sketch.c:112-113) and aligned nibble by nibble (DWmatch.c:136-137) from its bytes.  But only the flagged reads' bytes
// are information the packs lack.  Compaction keeps exactly those:
//   SIDE STORE   [16 zero bytes | slot of flagged read 0 | slot of flagged read 1 | ... | 1 KiB of zeros], flagged reads in ascending rid order;
//                a slot starts at a 16-byte boundary and holds lead = roff % 16 bytes, the read, and padding up to a multiple of 16 plus 16:
//                the read sits at an offset congruent mod 16 to its seqdb offset, so the kernels that load aligned 16-byte tiles from the
//                boundary below a read (k_nseg_scan, k_sketch_wave) split it into the same tiles as on the seqdb.  At most len + 46 bytes
//                per read, + 12 for its entry in the two tables (d_side_rid, d_side_off).
//   BYTE VIEW    what a byte-wise launch reads: a by-rid table of offsets from the side store's base that is valid for the reads the launch
//                touches -- a flagged read points into the side store, an unflagged one into a scratch region that k_unpack_reads fills from
//                the packs just before: byte[p] = (1 << F[p]) | (1 << R[p]) << 4, F / R the codes of the two strands at position p (the
//                inverse of pgx_pack.hip's pack4; shmr_utils.c:44-51).  The scratch uses the side store's slot rule.
// Bytes outside a read (a slot's lead and padding) are never looked at by a result: every kernel clips to the read's length, as it must on
// the seqdb, where the neighbours are other reads.

#include <algorithm>

#include "pgx_internal.h"

namespace pgx {
namespace {

__host__ __device__ inline uint64_t slot_bytes(uint64_t roff, uint32_t len) { return (((roff & 15u) + len + 15u) & ~15ULL) + 16u; }

// ---- building the side store -------------------------------------------------------------------------------------------------------
__global__ void k_side_need(const uint32_t *__restrict__ rids, uint32_t n, const uint64_t *__restrict__ roff, const uint32_t *__restrict__ rlen,
                            uint64_t *__restrict__ need) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) need[i] = slot_bytes(roff[rids[i]], rlen[rids[i]]);
}
// a wavefront per flagged read: the aligned 16-byte tiles that cover it, copied as they are (the lead bytes and the padding of the last
// tile are the file's neighbours; nothing reads them)
__global__ __launch_bounds__(64) void k_side_copy(const uint8_t *__restrict__ seq, const uint32_t *__restrict__ rids, uint32_t n,
                                                  const uint64_t *__restrict__ roff, const uint32_t *__restrict__ rlen,
                                                  const uint64_t *__restrict__ slot, uint8_t *__restrict__ side, uint64_t *__restrict__ side_off) {
  const uint32_t i = blockIdx.x;
  if (i >= n) return;
  const uint32_t rid = rids[i];
  const uint64_t ro = roff[rid], lead = ro & 15u, s0 = 16u + slot[i];
  const uint4 *src = reinterpret_cast<const uint4 *>(seq + (ro - lead));
  uint4 *dst = reinterpret_cast<uint4 *>(side + s0);
  const uint32_t tiles = (uint32_t)((lead + rlen[rid] + 15u) >> 4);
  for (uint32_t t = threadIdx.x; t < tiles; t += 64) dst[t] = src[t];
  if (threadIdx.x == 0) side_off[i] = s0 + lead;
}

// ---- the byte view -----------------------------------------------------------------------------------------------------------------
__global__ void k_view_flagged(const uint32_t *__restrict__ rids, const uint64_t *__restrict__ side_off, uint32_t n, uint64_t *__restrict__ boff) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) boff[rids[i]] = side_off[i];
}
// An unflagged read the view needs, claimed once: its place in the scratch region and in the list of reads to unpack from ONE atomic add on
// {reads claimed : 24 | scratch bytes : 40} (the order of the claims decides the layout of the scratch, nothing else).
constexpr int CLAIM_SHIFT = 40;
__device__ __forceinline__ void claim(uint32_t rid, const uint32_t *__restrict__ nflag, const uint64_t *__restrict__ roff,
                                      const uint32_t *__restrict__ rlen, uint32_t *__restrict__ mark, unsigned long long *__restrict__ state,
                                      uint32_t *__restrict__ plist, uint64_t *__restrict__ prel) {
  if (nflag[rid] & 1u) return;
  if (atomicExch(&mark[rid], 1u)) return;
  const unsigned long long o = atomicAdd(state, (1ULL << CLAIM_SHIFT) | slot_bytes(roff[rid], rlen[rid]));
  const uint32_t i = (uint32_t)(o >> CLAIM_SHIFT);
  plist[i] = rid, prel[i] = o & ((1ULL << CLAIM_SHIFT) - 1u);
}
__global__ void k_claim_keys(const pgx_align_key *__restrict__ keys, const uint32_t *__restrict__ list, uint32_t n, const uint32_t *__restrict__ nflag,
                             const uint64_t *__restrict__ roff, const uint32_t *__restrict__ rlen, uint32_t *__restrict__ mark,
                             unsigned long long *__restrict__ state, uint32_t *__restrict__ plist, uint64_t *__restrict__ prel) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const pgx_align_key key = keys[list[i]];
  claim(key.rid0, nflag, roff, rlen, mark, state, plist, prel);
  claim(key.rid1, nflag, roff, rlen, mark, state, plist, prel);
}
__global__ void k_claim_rids(const uint32_t *__restrict__ rids, uint32_t n, const uint32_t *__restrict__ nflag, const uint64_t *__restrict__ roff,
                             const uint32_t *__restrict__ rlen, uint32_t *__restrict__ mark, unsigned long long *__restrict__ state,
                             uint32_t *__restrict__ plist, uint64_t *__restrict__ prel) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) claim(rids[i], nflag, roff, rlen, mark, state, plist, prel);
}
__global__ void k_claim_reads(const ReadDesc *__restrict__ reads, const uint32_t *__restrict__ list, uint32_t n, const uint32_t *__restrict__ nflag,
                              const uint64_t *__restrict__ roff, const uint32_t *__restrict__ rlen, uint32_t *__restrict__ mark,
                              unsigned long long *__restrict__ state, uint32_t *__restrict__ plist, uint64_t *__restrict__ prel) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) claim(reads[list ? list[i] : i].rid, nflag, roff, rlen, mark, state, plist, prel);
}

// four 2-bit codes (the low 8 bits of b) -> four one-hot nibbles, one per byte: 0, 1, 2, 3 -> 1, 2, 4, 8
__device__ __forceinline__ uint32_t onehot4(uint32_t b) {
  b &= 0xFFu;
  uint32_t x = (b | (b << 12)) & 0x000F000Fu;
  x = (x | (x << 6)) & 0x03030303u;                            // a code per byte
  const uint32_t a = 0x01010101u + (x & 0x01010101u);          // 1 << (code & 1)
  const uint32_t hm = ((x >> 1) & 0x01010101u) * 0xFFu;        // bytes whose code has bit 1 set (no carry between bytes: 1 * 255)
  return a + ((a * 3u) & hm);                                  // ... times 4 there (a <= 2: 3 a <= 6 stays inside its byte)
}
__device__ __forceinline__ uint32_t biseq4(uint32_t f, uint32_t r) { return onehot4(f) | (onehot4(r) << 4); }
// k_unpack_reads: a wavefront per listed read, 1,024 bases per step -- lane l turns dword w = step * 64 + l of the forward strand and of the
// reverse complement (one coalesced dword load each) into the 16 biseq bytes [16 w, 16 w + 16) of the read and writes them with one 16-byte
// store (the wavefront's stores cover 1 KiB of consecutive addresses).  Bytes beyond the read's last base are written as zeros.  Lane 0
// enters the read into the view's table.  dst + rel[i] is the read's slot (16-byte aligned), delta = dst - the view's base.
__global__ __launch_bounds__(64) void k_unpack_reads(const uint32_t *__restrict__ pack, const uint64_t *__restrict__ poff, const uint64_t *__restrict__ roff,
                                                     const uint32_t *__restrict__ rlen, const uint32_t *__restrict__ list, const uint64_t *__restrict__ rel,
                                                     uint32_t n, uint8_t *__restrict__ dst, uint64_t delta, uint64_t *__restrict__ boff) {
  const uint32_t i = blockIdx.x;
  if (i >= n) return;
  const uint32_t rid = list[i], len = rlen[rid], nw = (len + 15u) >> 4;
  const uint64_t lead = roff[rid] & 15u, at = rel[i] + lead;
  const uint32_t *p0 = pack + poff[rid], *p1 = p0 + nw;
  uint8_t *out = dst + at;
  for (uint32_t w = threadIdx.x; w < nw; w += 64) {
    const uint32_t f = p0[w], r = p1[w];
    uint4 v;
    v.x = biseq4(f, r), v.y = biseq4(f >> 8, r >> 8), v.z = biseq4(f >> 16, r >> 16), v.w = biseq4(f >> 24, r >> 24);
    const uint32_t left = len - w * 16u;   // (>= 1)
    if (left < 16u) {
      uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t vb = left > 4u * j ? min(left - 4u * j, 4u) : 0u;
        d[j] &= vb >= 4u ? 0xFFFFFFFFu : ((1u << (8u * vb)) - 1u);
      }
      v.x = d[0], v.y = d[1], v.z = d[2], v.w = d[3];
    }
    __builtin_memcpy(out + (size_t)w * 16, &v, 16);
  }
  if (threadIdx.x == 0) boff[rid] = delta + at;
}
__global__ void k_translate_reads(const ReadDesc *__restrict__ reads, const uint32_t *__restrict__ list, uint32_t n, const uint64_t *__restrict__ boff,
                                  ReadDesc *__restrict__ tr, uint32_t *__restrict__ iota) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ReadDesc rd = reads[list ? list[i] : i];
  rd.off = boff[rd.rid];
  tr[i] = rd, iota[i] = i;
}

// the view for the reads a claim kernel names (at most max_claims distinct ones).  released: also on a database whose bytes were RELEASED (no
// flagged read, no side store): every read comes from the packs and the offsets count from the scratch region itself
template <typename Claim>
void view_build(const pgx_seqdb *db, size_t max_claims, ByteView &v, Claim &&launch_claim, bool released = false) {
  PGX_REQUIRE((seq_compacted(db) || (released && !db->d_seq.p)) && seq_packs_valid(db), PGX_ESTATE,
              "a byte view needs a compacted database (pgx_seqdb_compact_bytes)");
  hipStream_t st = ctx().stream;
  const size_t nr = db->rlen_by_rid.size();
  max_claims = std::min(max_claims, nr);
  PGX_REQUIRE(nr < (1ULL << (64 - CLAIM_SHIFT)), PGX_EARG, "too many reads for a byte view (%zu)", nr);
  uint64_t *boff = ws<uint64_t>("side.boff", nr);
  uint32_t *mark = ws<uint32_t>("side.mark", nr);
  unsigned long long *state = ws<unsigned long long>("side.state", 1);
  uint32_t *plist = ws<uint32_t>("side.plist", max_claims);
  uint64_t *prel = ws<uint64_t>("side.prel", max_claims);
  PGX_HIP(hipMemsetAsync(mark, 0, nr * sizeof(uint32_t), st));
  PGX_HIP(hipMemsetAsync(state, 0, sizeof(unsigned long long), st));
  const uint32_t nf = (uint32_t)db->d_side_rid.n;
  if (nf) hipLaunchKernelGGL(k_view_flagged, dim3(cdiv(nf, 256)), dim3(256), 0, st, db->d_side_rid.p, db->d_side_off.p, nf, boff);
  launch_claim(mark, state, plist, prel);
  unsigned long long h = 0;
  PGX_HIP(hipMemcpyAsync(&h, state, sizeof(h), hipMemcpyDeviceToHost, st));
  sync();
  const uint32_t np = (uint32_t)(h >> CLAIM_SHIFT);
  const uint64_t bytes = h & ((1ULL << CLAIM_SHIFT) - 1u);
  v.seq = db->d_side.p, v.off = boff;
  if (np) {
    KernelTimer tm("unpack", bytes);
    v.scratch.alloc(16 + bytes + 1024);   // (the side store's frame: 16 readable bytes in front, the zero tail the wide loads may run into behind)
    uint8_t *dst = v.scratch.p + 16;
    PGX_HIP(hipMemsetAsync(v.scratch.p, 0, 16, st));
    PGX_HIP(hipMemsetAsync(dst + bytes, 0, 1024, st));
    if (!v.seq) v.seq = v.scratch.p;   // (a released database: no side store to count from)
    hipLaunchKernelGGL(k_unpack_reads, dim3(np), dim3(64), 0, st, db->d_pack.p, db->d_poff.p, db->d_roff.p, db->d_rlen.p, plist, prel, np, dst,
                       (uint64_t)dst - (uint64_t)v.seq, boff);
  }
  PGX_HIP(hipGetLastError());
}

}  // namespace

uint64_t side_store_bytes(const pgx_seqdb *db) {
  return db->d_side.p ? db->d_side.n + db->d_side_rid.n * sizeof(uint32_t) + db->d_side_off.n * sizeof(uint64_t) : 0;
}

void side_build(pgx_seqdb *db) {
  PGX_REQUIRE(db->d_seq.p && seq_packs_valid(db) && db->n_flagged_reads, PGX_ESTATE, "the side store is built from the bytes of a database with flagged reads");
  hipStream_t st = ctx().stream;
  const uint32_t nr = (uint32_t)db->rlen_by_rid.size(), nf = db->n_flagged_reads;
  MemTag mem_tag("seqdb.side");
  DevBuf<uint32_t> rids(nf);
  DevBuf<uint64_t> offs(nf), slot((size_t)nf + 1);
  const uint32_t got = select_indices(db->d_nflag.p, nr, rids.p);   // the flagged rids, ascending
  PGX_REQUIRE(got == nf, PGX_EHIP, "the flag table names %u reads, the packs counted %u", got, nf);
  hipLaunchKernelGGL(k_side_need, dim3(cdiv(nf, 256)), dim3(256), 0, st, rids.p, nf, db->d_roff.p, db->d_rlen.p, slot.p);
  uint64_t total = 0;
  {
    PGX_HIP(hipMemsetAsync(slot.p + nf, 0, sizeof(uint64_t), st));
    exclusive_sum(slot.p, slot.p, (size_t)nf + 1);
    PGX_HIP(hipMemcpyAsync(&total, slot.p + nf, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    sync();
  }
  DevBuf<uint8_t> side(16 + total + 1024);
  PGX_HIP(hipMemsetAsync(side.p, 0, 16, st));
  PGX_HIP(hipMemsetAsync(side.p + 16 + total, 0, 1024, st));
  hipLaunchKernelGGL(k_side_copy, dim3(nf), dim3(64), 0, st, db->d_seq.p, rids.p, nf, db->d_roff.p, db->d_rlen.p, slot.p, side.p, offs.p);
  PGX_HIP(hipGetLastError());
  sync();
  db->d_side = std::move(side), db->d_side_rid = std::move(rids), db->d_side_off = std::move(offs);
  if (getenv("PGX_TRACE")) fprintf(stderr, "[pgx] side store: %u flagged reads, %.3f MB\n", nf, side_store_bytes(db) / 1e6);
}

void side_view_of_keys(const pgx_seqdb *db, const pgx_align_key *d_keys, const uint32_t *d_list, uint32_t n, ByteView &v) {
  view_build(db, 2 * (size_t)n, v, [&](uint32_t *mark, unsigned long long *state, uint32_t *plist, uint64_t *prel) {
    if (n)
      hipLaunchKernelGGL(k_claim_keys, dim3(cdiv(n, 256)), dim3(256), 0, ctx().stream, d_keys, d_list, n, db->d_nflag.p, db->d_roff.p, db->d_rlen.p, mark,
                         state, plist, prel);
  });
}
void side_view_of_reads(const pgx_seqdb *db, const ReadDesc *d_reads, const uint32_t *d_list, uint32_t n, ByteView &v) {
  view_build(db, n, v, [&](uint32_t *mark, unsigned long long *state, uint32_t *plist, uint64_t *prel) {
    if (n)
      hipLaunchKernelGGL(k_claim_reads, dim3(cdiv(n, 256)), dim3(256), 0, ctx().stream, d_reads, d_list, n, db->d_nflag.p, db->d_roff.p, db->d_rlen.p, mark,
                         state, plist, prel);
  });
}
void side_view_of_rids(const pgx_seqdb *db, const uint32_t *d_rids, uint32_t n, ByteView &v) {
  view_build(db, n, v, [&](uint32_t *mark, unsigned long long *state, uint32_t *plist, uint64_t *prel) {
    if (n)
      hipLaunchKernelGGL(k_claim_rids, dim3(cdiv(n, 256)), dim3(256), 0, ctx().stream, d_rids, n, db->d_nflag.p, db->d_roff.p, db->d_rlen.p, mark, state,
                         plist, prel);
  }, true);
}
void side_translate_reads(const ByteView &v, const ReadDesc *d_reads, const uint32_t *d_list, uint32_t n, ReadDesc *tr, uint32_t *iota) {
  if (n) hipLaunchKernelGGL(k_translate_reads, dim3(cdiv(n, 256)), dim3(256), 0, ctx().stream, d_reads, d_list, n, v.off, tr, iota);
}

}  // namespace pgx
