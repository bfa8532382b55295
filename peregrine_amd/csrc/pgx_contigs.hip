// pgx_contigs.hip -- contig layout: tiling paths -> contig bytes (py/scripts/path_to_contig.py), and pgx_align_batch2.
//
// The script walks a contig's rows one by one: ovlp_match of the last 500 bases of read v against the last |e - s| + 500 of read w, a
// segment of w cut at the match (seg = e - s + 500 - t_m_end bytes that end at e), placed at ctg_len - 500 + q_m_end, ctg_len moved to the
// segment's end; at the end every segment is copied into the contig in row order, later ones over earlier ones, over a background of 'N'.
// Here:
//   k_align1t    one alignment per row, a wavefront each (pgx_align.hip: k_align1's body with a target offset), on the reads' BYTES -- the
//                seqdb's, or a byte view of the reads the rows name, rebuilt from the packs (pgx_side.hip) when the bytes are gone
//   k_tile_geom  per row: seg, and the step ctg_len takes (q_m_end - 500 + seg); per contig: the first read's length.  The SEGMENTS of a
//                call are numbered k = row + contig + 1, with segment first_row[c] + c = read v of contig c's first row, whole
//   one exclusive sum over the steps of all segments: since a contig's length IS the sum of its steps, the sum in front of segment k is
//                the contig's offset in the output plus ctg_len before the row -- every segment's place in the concatenated output, every
//                contig's offset and the total from one scan, nothing segmented
//   k_tile_place per row: the segment's descriptor {output offset, source byte, length, strand}, and the checks that need the alignment
//                (a segment that starts before its contig or ends beyond it)
//   the error row: k_tile_geom (e - seg < 0) and k_tile_place both run on every call, whatever the other finds, and atomicMin
//                row << 2 | kind into ONE word: the host names the smallest offending row in contig order whatever its kind, and of two
//                kinds on one row the smaller (BAD_SOURCE < BAD_START < BAD_END).  A row with e - seg < 0 keeps its seg and its step, so
//                the places of all other rows are defined; its descriptor is stored and never read (no k_stitch after an offence)
//   two running maxima: PM[k] = the furthest end of the segments 0 .. k, and the smallest start of the segments k .. (as a maximum of
//                complements over the reversed order) -- both monotone in k whatever the rows do
//   k_stitch     a workgroup per 4 KiB tile of the output: the segments that can touch the tile [a, b) are k in [first PM > a, first
//                suffix-min start >= b) -- two binary searches; they are decoded into the tile's LDS image in ascending k, a barrier between
//                them, so the last-numbered covering segment wins byte by byte also where the starts are not monotone (a segment shorter
//                than 500 - q_m_end); the image, 'N' where nothing wrote, leaves with 16-byte stores.
// HBM of a call, booked under "contigs": 132 bytes per row, the output bytes, and -- without the seqdb's bytes -- one byte per base of the
// reads the rows name.

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <string>
#include <unordered_map>

#include "pgx_internal.h"

namespace pgx {
namespace {

constexpr int OVERHANG = 500;   // stitching_overhang_size (path_to_contig.py:9)
constexpr int BAND = 100;       // (path_to_contig.py:84)
constexpr uint32_t TILE = 4096, STITCH_THREADS = 256;

struct Seg {
  uint64_t dst;   // offset in the concatenated output
  uint64_t src;   // offset of its first byte from the byte source's base (modulo 2^64, as a byte view counts)
  uint32_t len;
  uint32_t strand;
};
// why a row cannot be laid out, known after its alignment; the host reads the smallest row << 2 | kind
enum : unsigned { BAD_SOURCE = 0, BAD_START = 1, BAD_END = 2 };
constexpr unsigned long long NO_BAD = ~0ULL;

// rows[i].s / .e arrive TRANSFORMED (s, e = len - s, len - e on strand 1) and checked (e > s, |e - s| + 500 <= len)
__global__ void k_tile_geom(const pgx_tile_row *__restrict__ rows, const pgx_match *__restrict__ match, uint32_t n, const uint32_t *__restrict__ rlen,
                            uint64_t *__restrict__ step, uint32_t *__restrict__ seg, unsigned long long *__restrict__ bad) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const pgx_tile_row r = rows[i];
  const pgx_match m = match[i];
  const int sg = r.e - r.s + OVERHANG - m.t_m_end;   // (>= 0: t_m_end <= the target's length = e - s + 500)
  const uint32_t k = i + r.ctg + 1;
  seg[i] = (uint32_t)sg;
  step[k] = (uint64_t)(int64_t)(m.q_m_end - OVERHANG + sg);
  if (i == 0 || rows[i - 1].ctg != r.ctg) step[k - 1] = rlen[r.rid0];   // the contig's first read
  if (r.e - sg < 0) atomicMin(bad, (unsigned long long)i << 2 | BAD_SOURCE);
}
// before[k]: the exclusive sum of the steps (n_seg + 1 entries).  rev_start[n_seg - 1 - k] = ~start of segment k, end[k] = its end;
// an empty segment covers nothing and gets the neutral element of both maxima.
__global__ void k_tile_place(const pgx_tile_row *__restrict__ rows, const pgx_match *__restrict__ match, const uint32_t *__restrict__ seg, uint32_t n,
                             uint32_t n_seg, const uint32_t *__restrict__ first_row, const uint64_t *__restrict__ before,
                             const uint64_t *__restrict__ off, const uint32_t *__restrict__ rlen, Seg *__restrict__ segs, uint64_t *__restrict__ end,
                             uint64_t *__restrict__ rev_start, uint64_t *__restrict__ ctg_off, unsigned long long *__restrict__ bad) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const pgx_tile_row r = rows[i];
  const uint32_t k = i + r.ctg + 1;
  const uint64_t c0 = before[first_row[r.ctg] + r.ctg], c1 = before[first_row[r.ctg + 1] + r.ctg + 1];   // the contig in the output
  auto put = [&](uint32_t kk, uint64_t dst, uint64_t src, uint32_t len, uint32_t strand) {
    segs[kk] = Seg{dst, src, len, strand};
    end[kk] = len ? dst + len : 0u;
    rev_start[n_seg - 1 - kk] = len ? ~dst : 0u;
  };
  if (i == first_row[r.ctg]) {
    const uint32_t l0 = rlen[r.rid0];
    put(k - 1, c0, off[r.rid0], l0, r.strand0);
    ctg_off[r.ctg] = c0;
    if (i == 0) ctg_off[rows[n - 1].ctg + 1] = before[n_seg];
    if ((int64_t)(c1 - c0) < (int64_t)l0) atomicMin(bad, (unsigned long long)i << 2 | BAD_END);
  }
  const uint32_t sg = seg[i];
  const int64_t local = (int64_t)(before[k] - c0) - OVERHANG + match[i].q_m_end;   // ctg_len - 500 + q_m_end
  put(k, c0 + (uint64_t)local, off[r.rid1] + (uint64_t)(int64_t)(r.e - (int)sg), sg, r.strand1);
  if (sg == 0) return;   // (an empty segment writes nothing wherever it lies)
  if (local < 0) atomicMin(bad, (unsigned long long)i << 2 | BAD_START);
  else if (local + (int64_t)sg > (int64_t)(c1 - c0)) atomicMin(bad, (unsigned long long)i << 2 | BAD_END);
}

// bits_to_base (shmr_utils.c:35-43) over four nibbles, one per byte of n: 1, 2, 4, 8 -> A, C, G, T; any other value -> N.
// v_perm_b32 picks byte sel (0 .. 3: of the second operand, 4 .. 7: of the first) per byte of the selector.
__device__ __forceinline__ uint32_t bases4(uint32_t n) {
  const uint32_t sel = n & 0x07070707u;
  const uint32_t lo = __builtin_amdgcn_perm(0x4E4E4E47u, 0x4E43414Eu, sel);   // nibbles 0 .. 7:  N A C N | G N N N
  const uint32_t hi = __builtin_amdgcn_perm(0x4E4E4E4Eu, 0x4E4E4E54u, sel);   // nibbles 8 .. 15: T N N N | N N N N
  const uint32_t m = ((n >> 3) & 0x01010101u) * 0xFFu;
  return (lo & ~m) | (hi & m);
}
__device__ __forceinline__ uint8_t base1(uint32_t nib) { return nib == 1 ? 'A' : nib == 2 ? 'C' : nib == 4 ? 'G' : nib == 8 ? 'T' : 'N'; }

__global__ __launch_bounds__(STITCH_THREADS) void k_stitch(const uint8_t *__restrict__ seq, const Seg *__restrict__ segs, uint32_t n_seg,
                                                          const uint64_t *__restrict__ end_max, const uint64_t *__restrict__ rev_start_max,
                                                          uint64_t total, uint8_t *__restrict__ text) {
  __shared__ __attribute__((aligned(16))) uint8_t img[TILE];
  const uint64_t a = (uint64_t)blockIdx.x * TILE, b = min(a + TILE, total);
  reinterpret_cast<uint4 *>(img)[threadIdx.x] = make_uint4(0x4E4E4E4Eu, 0x4E4E4E4Eu, 0x4E4E4E4Eu, 0x4E4E4E4Eu);
  // the segments that can touch [a, b): from the first k whose running furthest end passes a, up to the first k from which on every start
  // is at b or beyond (uniform over the workgroup)
  uint32_t lo = 0, hi = n_seg;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (end_max[mid] > a) hi = mid;
    else lo = mid + 1;
  }
  const uint32_t k0 = lo;
  lo = k0, hi = n_seg;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (~rev_start_max[n_seg - 1 - mid] >= b) hi = mid;
    else lo = mid + 1;
  }
  const uint32_t k1 = lo;
  __syncthreads();
  for (uint32_t k = k0; k < k1; ++k) {
    const Seg s = segs[k];
    const uint64_t g0 = max(a, s.dst), g1 = min(b, s.dst + s.len);
    if (!s.len || g0 >= g1) continue;   // (uniform)
    const uint32_t o0 = (uint32_t)(g0 - a), o1 = (uint32_t)(g1 - a);
    const uint8_t *src = seq + s.src + (a - s.dst);   // the source byte of tile byte 0 (only [o0, o1) of it is the segment's)
    const uint32_t shift = s.strand ? 4u : 0u;
    // 8-byte groups of the image, one per thread and round: whole groups with one 8-byte load and one 8-byte LDS store, the two ragged
    // ones at the segment's edges byte by byte
    for (uint32_t g = (o0 >> 3) + threadIdx.x; g <= ((o1 - 1) >> 3); g += STITCH_THREADS) {
      const uint32_t p = g << 3;
      if (p >= o0 && p + 8 <= o1) {
        uint2 v;
        __builtin_memcpy(&v, src + p, 8);
        uint2 r;
        r.x = bases4((v.x >> shift) & 0x0F0F0F0Fu), r.y = bases4((v.y >> shift) & 0x0F0F0F0Fu);
        *reinterpret_cast<uint2 *>(img + p) = r;
      } else {
        for (uint32_t j = max(p, o0); j < min(p + 8, o1); ++j) img[j] = base1((src[j] >> shift) & 15u);
      }
    }
    __syncthreads();   // the next segment may overwrite what this one wrote
  }
  // (the output buffer is a whole number of tiles: the last tile's stores beyond `total` land in its padding)
  reinterpret_cast<uint4 *>(text + a)[threadIdx.x] = reinterpret_cast<const uint4 *>(img)[threadIdx.x];
}

__global__ void k_key_rids(const pgx_align_key2 *__restrict__ keys, uint32_t n, uint32_t *__restrict__ rids) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) rids[2 * i] = keys[i].rid0, rids[2 * i + 1] = keys[i].rid1;
}

// The bytes the byte-wise kernels of a call read: the seqdb's, or -- released / compacted -- a view of the reads d_rids names
struct ByteSource {
  const uint8_t *seq = nullptr;
  const uint64_t *off = nullptr;
  ByteView view;
  ByteSource(const pgx_seqdb *db, const uint32_t *d_rids, uint32_t n) {
    if (db->d_seq.p) {
      seq = db->d_seq.p, off = db->d_roff.p;
      return;
    }
    PGX_REQUIRE(seq_packs_valid(db), PGX_ESTATE, "the seqdb's bytes are gone and it has no packs to rebuild them from");
    side_view_of_rids(db, d_rids, n, view);
    seq = view.seq, off = view.off;
  }
};

// row_name[i]: what a message calls row i (the file level: its line in the tiling path); nullptr: i
uint64_t name_of(const uint64_t *row_name, size_t i) { return row_name ? row_name[i] : (uint64_t)i; }

// the rows' checks that need no alignment (path_to_contig.py:58-88), and s, e transformed in place
void check_rows(const pgx_seqdb *db, std::vector<pgx_tile_row> &rows, size_t n_ctg, const uint64_t *row_name, std::vector<uint32_t> &first_row) {
  const size_t nr = db->rlen_by_rid.size(), n = rows.size();
  first_row.assign(n_ctg + 1, (uint32_t)n);
  for (size_t i = 0; i < n; ++i) {
    pgx_tile_row &r = rows[i];
    const unsigned long long nm = name_of(row_name, i);
    PGX_REQUIRE_PIECE(r.ctg < n_ctg && (i == 0 ? r.ctg == 0 : r.ctg == rows[i - 1].ctg || r.ctg == rows[i - 1].ctg + 1), PGX_EARG, nm,
                "tiling path row %llu: contig number %u (the rows of a contig must be consecutive, the contigs numbered 0 .. %zu in order)", nm, r.ctg,
                n_ctg - 1);
    if (i == 0 || r.ctg != rows[i - 1].ctg) first_row[r.ctg] = (uint32_t)i;
    PGX_REQUIRE_PIECE(r.rid0 < nr && db->rlen_by_rid[r.rid0] && r.rid1 < nr && db->rlen_by_rid[r.rid1], PGX_EARG, nm,
                "tiling path row %llu: read %u is not in the database", nm, r.rid0 < nr && db->rlen_by_rid[r.rid0] ? r.rid1 : r.rid0);
    const int64_t l0 = db->rlen_by_rid[r.rid0], l1 = db->rlen_by_rid[r.rid1];
    PGX_REQUIRE_PIECE(l0 >= OVERHANG, PGX_EARG, nm, "tiling path row %llu: read %u has %lld bases, fewer than the overhang of %d", nm, r.rid0, (long long)l0, OVERHANG);
    const int64_t span = std::llabs((int64_t)r.e - (int64_t)r.s);
    PGX_REQUIRE_PIECE(span + OVERHANG <= l1, PGX_EARG, nm, "tiling path row %llu: |e - s| + %d = %lld exceeds the %lld bases of read %u", nm, OVERHANG,
                (long long)(span + OVERHANG), (long long)l1, r.rid1);
    int64_t s = r.s, e = r.e;
    if (r.strand1) s = l1 - s, e = l1 - e;
    PGX_REQUIRE_PIECE(e > s, PGX_EARG, nm, "tiling path row %llu: e <= s (%lld <= %lld%s)", nm, (long long)e, (long long)s, r.strand1 ? ", after the strand transform" : "");
    r.s = (int32_t)s, r.e = (int32_t)e;   // (|s|, |e| <= 2 l1 < 2^31 for the reads the alignment kernels take; checked by the caller)
    r.strand0 = r.strand0 ? 1 : 0, r.strand1 = r.strand1 ? 1 : 0;
  }
  PGX_REQUIRE(n == 0 ? n_ctg == 0 : (size_t)rows[n - 1].ctg + 1 == n_ctg, PGX_EARG, "the rows name %zu contigs, n_ctg = %zu", n ? (size_t)rows[n - 1].ctg + 1 : 0,
              n_ctg);
}

// contig bytes of checked rows; text: out_alloc'd, total + 1 bytes (NUL-terminated)
void contigs_layout(pgx_seqdb *db, const std::vector<pgx_tile_row> &rows, const std::vector<uint32_t> &first_row, const uint64_t *row_name,
                    char **text, uint64_t *ctg_off, uint64_t *text_len) {
  const size_t n = rows.size(), n_ctg = first_row.size() - 1, n_seg = n + n_ctg;
  hipStream_t st = ctx().stream;
  *text = nullptr, *text_len = 0, ctg_off[0] = 0;
  if (n == 0) {
    *text = (char *)out_alloc(1), (*text)[0] = 0;
    return;
  }
  PGX_REQUIRE(n_seg < (1ULL << 31), PGX_EARG, "too many tiling path rows for one call (%zu)", n);
  MemTag mem_tag("contigs");
  std::vector<pgx_align_key2> keys(n);
  std::vector<uint32_t> rids;
  if (!db->d_seq.p) rids.reserve(2 * n);
  for (size_t i = 0; i < n; ++i) {
    const pgx_tile_row &r = rows[i];
    const uint32_t l0 = db->rlen_by_rid[r.rid0], l1 = db->rlen_by_rid[r.rid1];
    keys[i] = pgx_align_key2{r.rid0, r.rid1, l0 - OVERHANG, l1 - (uint32_t)(r.e - r.s) - OVERHANG, r.strand0, r.strand1, {0, 0}};
    if (!db->d_seq.p) rids.push_back(r.rid0), rids.push_back(r.rid1);
  }
  DevBuf<pgx_tile_row> d_rows(n);
  DevBuf<pgx_align_key2> d_keys(n);
  DevBuf<pgx_match> d_match(n);
  DevBuf<uint32_t> d_first(n_ctg + 1), d_seglen(n), d_rids(rids.size());
  DevBuf<uint64_t> d_step(n_seg + 1), d_before(n_seg + 1), d_end(n_seg), d_rev(n_seg), d_ctg_off(n_ctg + 1);
  DevBuf<unsigned long long> d_bad(1);
  DevBuf<Seg> d_segs(n_seg);
  d_rows.upload(rows.data(), n), d_keys.upload(keys.data(), n), d_first.upload(first_row.data(), n_ctg + 1), d_rids.upload(rids.data(), rids.size());
  PGX_HIP(hipMemsetAsync(d_bad.p, 0xFF, sizeof(unsigned long long), st));
  PGX_HIP(hipMemsetAsync(d_step.p + n_seg, 0, sizeof(uint64_t), st));
  ByteSource src(db, d_rids.p, (uint32_t)rids.size());
  dev_align2(db, src.seq, src.off, d_keys.p, n, BAND, d_match.p);
  unsigned long long bad = NO_BAD;
  uint64_t total = 0;
  {
    KernelTimer tm("tile_geom", n);
    hipLaunchKernelGGL(k_tile_geom, dim3(cdiv(n, 256)), dim3(256), 0, st, d_rows.p, d_match.p, (uint32_t)n, db->d_rlen.p, d_step.p, d_seglen.p, d_bad.p);
    exclusive_sum(d_step.p, d_before.p, n_seg + 1);   // (step[n_seg] = 0: before[n_seg] is the total)
  }
  // the placement checks run whatever the geometry pass found: a row with e - seg < 0 still has its seg and its step, so every other row's
  // place is defined, and k_tile_place only STORES the descriptor of such a row (nothing is read through it: k_stitch is not launched)
  hipLaunchKernelGGL(k_tile_place, dim3(cdiv(n, 256)), dim3(256), 0, st, d_rows.p, d_match.p, d_seglen.p, (uint32_t)n, (uint32_t)n_seg, d_first.p, d_before.p,
                     src.off, db->d_rlen.p, d_segs.p, d_end.p, d_rev.p, d_ctg_off.p, d_bad.p);
  PGX_HIP(hipGetLastError());
  PGX_HIP(hipMemcpyAsync(&total, d_before.p + n_seg, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  PGX_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof(bad), hipMemcpyDeviceToHost, st));
  sync();
  if (bad != NO_BAD) {
    const size_t i = (size_t)(bad >> 2);
    const unsigned kind = (unsigned)(bad & 3u);
    PGX_REQUIRE_PIECE(false, PGX_EARG, name_of(row_name, i), "tiling path row %llu: %s", (unsigned long long)name_of(row_name, i),
                kind == BAD_SOURCE  ? "the segment the alignment cuts starts before read w's first base (e - seg < 0)"
                : kind == BAD_START ? "the segment would start before its contig's first base"
                                    : "a segment ends beyond the end of its contig (a later row pulled the contig's length back)");
  }
  running_max(d_end.p, d_end.p, n_seg);
  running_max(d_rev.p, d_rev.p, n_seg);
  const size_t tiles = (total + TILE - 1) / TILE;
  PGX_REQUIRE(tiles < (1ULL << 31), PGX_EARG, "the contigs of one call exceed 8 TB");
  DevBuf<uint8_t> d_text(tiles * TILE);
  if (tiles) {
    KernelTimer tm("stitch", total);
    hipLaunchKernelGGL(k_stitch, dim3((unsigned)tiles), dim3(STITCH_THREADS), 0, st, src.seq, d_segs.p, (uint32_t)n_seg, d_end.p, d_rev.p, total, d_text.p);
    PGX_HIP(hipGetLastError());
  }
  char *out = (char *)out_alloc(total + 1);
  try {
    if (total) PGX_HIP(hipMemcpyAsync(out, d_text.p, total, hipMemcpyDeviceToHost, st));
    d_ctg_off.download(ctg_off, n_ctg + 1);
    sync();
  } catch (...) {
    out_free(out);
    throw;
  }
  out[total] = 0;
  *text = out, *text_len = total;
}

// ---- the file level --------------------------------------------------------------------------------------------------------------------
struct Mapped {   // a file, read-only
  const uint8_t *p = nullptr;
  size_t n = 0;
  ~Mapped() {
    if (p && n) munmap((void *)p, n);
  }
  bool open(const char *path) {
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return false;
    struct stat sb;
    bool ok = fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode);
    if (ok && sb.st_size) {
      void *m = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_SHARED, fd, 0);
      ok = m != MAP_FAILED;
      if (ok) p = (const uint8_t *)m, n = (size_t)sb.st_size;
    }
    close(fd);
    return ok;
  }
};
bool parse_int(const std::string &t, int64_t lo, int64_t hi, int64_t *out) {   // [+-]digits, as int() takes them
  size_t i = t.size() && (t[0] == '-' || t[0] == '+') ? 1 : 0;
  if (i == t.size() || t.size() - i > 18) return false;
  int64_t v = 0;
  for (; i < t.size(); ++i) {
    if (t[i] < '0' || t[i] > '9') return false;
    v = v * 10 + (t[i] - '0');
  }
  if (t[0] == '-') v = -v;
  *out = v;
  return v >= lo && v <= hi;
}
bool parse_node(const std::string &t, int64_t *rid, uint8_t *strand) {   // "rid:E" / "rid:B" (strand 0 for E, 1 for anything else)
  const size_t c = t.find(':');
  if (c == std::string::npos || !parse_int(t.substr(0, c), 0, 0xFFFFFFFFLL, rid)) return false;
  const size_t c2 = t.find(':', c + 1);
  *strand = t.substr(c + 1, c2 == std::string::npos ? std::string::npos : c2 - c - 1) == "E" ? 0 : 1;
  return true;
}
struct PathRow {
  uint32_t ctg, rid0, rid1;   // rid: the read's slot in the idx file
  int32_t s, e;
  uint8_t strand0, strand1;
  uint64_t line;
};

}  // namespace

// the layout of rows over a resident database, whoever made the rows (pgx_contigs_resident; the GFA segments of pgx_gfa.hip): the checks
// that need no alignment, then contigs_layout.  A refusal of a row throws a Fail that carries the row's index.
void contigs_resident_rows(const char *who, pgx_seqdb *db, std::vector<pgx_tile_row> &rows, size_t n_ctg, char **text, uint64_t *ctg_off, uint64_t *text_len) {
  PGX_REQUIRE(db->max_rlen < (1u << 30), PGX_EARG, "%s: a read of %u bases", who, db->max_rlen);
  std::vector<uint32_t> first_row;
  check_rows(db, rows, n_ctg, nullptr, first_row);
  contigs_layout(db, rows, first_row, nullptr, text, ctg_off, text_len);
}
}  // namespace pgx

namespace pgx {
namespace {
// the rows of a tiling path file, in file order (path_to_contig.py:32-39): where the text route and the row route of the layout part
void feed_path_text(const char *tiling_path, const TileRowFn &add) {
  Mapped path;
  PGX_REQUIRE(path.open(tiling_path), PGX_EIO, "cannot read %s", tiling_path);
  {
    const char *p = (const char *)path.p, *end = p + path.n;
    std::vector<std::string> f;
    for (uint64_t line = 0; p < end; ++line) {
      const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
      const char *le = nl ? nl : end;
      f.clear();
      for (const char *q = p; q < le;) {
        while (q < le && isspace((unsigned char)*q)) ++q;
        const char *t0 = q;
        while (q < le && !isspace((unsigned char)*q)) ++q;
        if (q > t0) f.emplace_back(t0, q);
      }
      p = nl ? nl + 1 : end;
      PGX_REQUIRE(f.size() == 10, PGX_EARG, "tiling path row %llu: %zu fields, not 10", (unsigned long long)line, f.size());
      int64_t r0 = 0, r1 = 0, s = 0, e = 0;
      uint8_t st0 = 0, st1 = 0;
      PGX_REQUIRE(parse_node(f[1], &r0, &st0) && parse_node(f[2], &r1, &st1), PGX_EARG, "tiling path row %llu: cannot read the nodes '%s' '%s' (rid:E or rid:B)",
                  (unsigned long long)line, f[1].c_str(), f[2].c_str());
      PGX_REQUIRE(parse_int(f[4], INT32_MIN, INT32_MAX, &s) && parse_int(f[5], INT32_MIN, INT32_MAX, &e), PGX_EARG,
                  "tiling path row %llu: cannot read s, e = '%s', '%s'", (unsigned long long)line, f[4].c_str(), f[5].c_str());
      add(f[0], r0, r1, s, e, st0, st1, line);
    }
  }
}
}  // namespace

ContigPieces::~ContigPieces() {
  for (auto &pc : pieces) out_free(pc.text);
}

// The layout behind pgx_contigs_chunk, pgx_tiling_contigs and the GFA's file level: feed hands over the rows in order (contig name, the two
// reads' ids as the idx names them, s, e, strands, the row's number for messages); every check runs in that order, then the batching and
// the layout: the batches' contig bytes as pieces (throws; the Fail of a refused row carries the row's number)
void contig_pieces_from_rows(const char *who, const char *seqdb_prefix, const TileRowFeed &feed, ContigPieces &out) {
  std::vector<ContigPieces::Piece> &pieces = out.pieces;
  std::vector<std::string> &ctg_names = out.names;
  {
    require_ready();
    PGX_REQUIRE(seqdb_prefix, PGX_EARG, "%s: null argument", who);
    const std::string prefix(seqdb_prefix);
    std::vector<uint32_t> rid, rlen;
    std::vector<uint64_t> roff;
    PGX_REQUIRE(load_idx((prefix + ".idx").c_str(), rid, rlen, roff) == 0, PGX_EIO, "cannot open %s.idx", seqdb_prefix);
    Mapped seqdb;
    PGX_REQUIRE(seqdb.open((prefix + ".seqdb").c_str()), PGX_EIO, "cannot read %s.seqdb", seqdb_prefix);
    std::unordered_map<uint32_t, uint32_t> slot_of;   // rid -> its LAST slot in the idx file (the script's dict keeps the last entry)
    slot_of.reserve(rid.size() * 2);
    for (size_t i = 0; i < rid.size(); ++i) {
      PGX_REQUIRE(roff[i] + rlen[i] <= seqdb.n, PGX_EARG, "read %u exceeds %s.seqdb (%zu bytes)", rid[i], seqdb_prefix, seqdb.n);
      slot_of[rid[i]] = (uint32_t)i;
    }
    // ---- the tiling path: rows by contig, contigs in order of first appearance (path_to_contig.py:32-39), every check in FILE order
    std::unordered_map<std::string, uint32_t> ctg_of;
    std::vector<std::vector<PathRow>> by_ctg;
    feed([&](const std::string &ctg, int64_t r0, int64_t r1, int64_t s, int64_t e, uint8_t st0, uint8_t st1, uint64_t line) {
      const auto i0 = slot_of.find((uint32_t)r0), i1 = slot_of.find((uint32_t)r1);
      PGX_REQUIRE_PIECE(i0 != slot_of.end() && i1 != slot_of.end(), PGX_EARG, line, "tiling path row %llu: read %lld is not in %s.idx", (unsigned long long)line,
                  (long long)(i0 == slot_of.end() ? r0 : r1), seqdb_prefix);
      auto it = ctg_of.find(ctg);
      if (it == ctg_of.end()) {
        it = ctg_of.emplace(ctg, (uint32_t)ctg_names.size()).first;
        ctg_names.push_back(ctg), by_ctg.emplace_back();
      }
      by_ctg[it->second].push_back(PathRow{it->second, i0->second, i1->second, (int32_t)s, (int32_t)e, st0, st1, line});
      // the checks of the row itself, here so that the FIRST bad row of the file is the one reported
      const int64_t l0 = rlen[i0->second], l1 = rlen[i1->second];
      PGX_REQUIRE_PIECE(l0 >= OVERHANG, PGX_EARG, line, "tiling path row %llu: read %lld has %lld bases, fewer than the overhang of %d", (unsigned long long)line,
                        (long long)r0, (long long)l0, OVERHANG);
      PGX_REQUIRE_PIECE(l1 < (1LL << 30) && std::llabs(e - s) + OVERHANG <= l1, PGX_EARG, line, "tiling path row %llu: |e - s| + %d = %lld exceeds the %lld bases of read %lld",
                        (unsigned long long)line, OVERHANG, (long long)(std::llabs(e - s) + OVERHANG), (long long)l1, (long long)r1);
      PGX_REQUIRE_PIECE(st1 ? l1 - e > l1 - s : e > s, PGX_EARG, line, "tiling path row %llu: e <= s%s", (unsigned long long)line, st1 ? " after the strand transform" : "");
    });
    // ---- batches of whole contigs: the reads a batch names gathered into a sub-database of their own, rids remapped to 0 .. m - 1
    size_t free_b = 0, total_b = 0;
    PGX_HIP(hipMemGetInfo(&free_b, &total_b));
    const uint64_t budget = (uint64_t)(free_b + dev_cache_free_bytes()) / 2;
    const char *be = getenv("PGX_CONTIGS_BATCH");
    const size_t max_ctg = be && atoll(be) > 0 ? (size_t)atoll(be) : SIZE_MAX;
    std::vector<uint32_t> local(rid.size()), stamp(rid.size(), 0);
    uint32_t batch_no = 0;
    uint64_t bases = 0;
    for (size_t c0 = 0; c0 < by_ctg.size();) {
      ++batch_no;
      std::vector<uint32_t> slots;   // the batch's reads, local rid = position
      std::vector<pgx_tile_row> rows;
      std::vector<uint64_t> names;
      uint64_t sub_bytes = 0, out_est = 0;
      size_t c1 = c0;
      for (; c1 < by_ctg.size() && c1 - c0 < max_ctg; ++c1) {
        // what the contig adds: its reads not yet in the batch, a row's share of the tables, and at most |e - s| + 500 output bytes per row
        uint64_t add_bytes = 0, add_out = rlen[by_ctg[c1][0].rid0];
        std::vector<uint32_t> fresh;
        for (const PathRow &r : by_ctg[c1]) {
          for (uint32_t sl : {r.rid0, r.rid1})
            if (stamp[sl] != batch_no) stamp[sl] = batch_no, fresh.push_back(sl), add_bytes += rlen[sl];
          add_out += (uint64_t)std::llabs((int64_t)r.e - r.s) + OVERHANG;
        }
        const uint64_t need = sub_bytes + add_bytes + out_est + add_out + 160ULL * (rows.size() + by_ctg[c1].size() + 2);
        if (c1 > c0 && need > budget) {
          for (uint32_t sl : fresh) stamp[sl] = 0;
          break;
        }
        PGX_REQUIRE(need <= budget, PGX_ENOMEM, "contig %s alone needs %.1f GB of HBM, %.1f GB are free", ctg_names[c1].c_str(), need / 1e9, budget / 1e9);
        for (uint32_t sl : fresh) local[sl] = (uint32_t)slots.size(), slots.push_back(sl);
        sub_bytes += add_bytes, out_est += add_out;
        for (const PathRow &r : by_ctg[c1]) {
          rows.push_back(pgx_tile_row{(uint32_t)(c1 - c0), local[r.rid0], local[r.rid1], r.s, r.e, r.strand0, r.strand1, {0, 0}});
          names.push_back(r.line);
        }
      }
      HostArray<uint8_t> sub(sub_bytes);
      std::vector<uint32_t> srid(slots.size()), srlen(slots.size());
      std::vector<uint64_t> sroff(slots.size());
      uint64_t at = 0;
      for (size_t i = 0; i < slots.size(); ++i) {
        srid[i] = (uint32_t)i, srlen[i] = rlen[slots[i]], sroff[i] = at;
        memcpy(sub.p + at, seqdb.p + roff[slots[i]], rlen[slots[i]]);
        at += rlen[slots[i]];
      }
      pgx_seqdb *sdb = nullptr;
      const int urc = pgx_seqdb_upload(sub.p, sub_bytes, srid.data(), srlen.data(), sroff.data(), (uint32_t)slots.size(), &sdb);
      if (urc) throw Fail{urc};   // (its message stands)
      std::unique_ptr<pgx_seqdb, void (*)(pgx_seqdb *)> hold(sdb, pgx_seqdb_free);
      sub.clear();
      std::vector<uint32_t> first_row;
      check_rows(sdb, rows, c1 - c0, names.data(), first_row);
      pieces.emplace_back();
      ContigPieces::Piece &pc = pieces.back();
      pc.ctg0 = c0, pc.off.assign(c1 - c0 + 1, 0);
      uint64_t len = 0;
      contigs_layout(sdb, rows, first_row, names.data(), &pc.text, pc.off.data(), &len);
      bases += len;
      if (getenv("PGX_TRACE"))
        fprintf(stderr, "[pgx] contigs: batch %u, contigs %zu .. %zu, %zu rows, %zu reads (%.3f MB) uploaded, %.3f MB out\n", batch_no, c0, c1, rows.size(),
                slots.size(), sub_bytes / 1e6, len / 1e6);
      c0 = c1;
    }
    out.bases = bases;
  }
}

// The layout behind pgx_contigs_chunk and pgx_tiling_contigs: the pieces, then the FASTA -- written only when every batch is through, so
// that an error in a later batch leaves nothing written
int contigs_from_rows(const char *who, const char *seqdb_prefix, const TileRowFeed &feed, const char *out_path, uint64_t *n_ctg_out, uint64_t *n_bases_out) {
  ContigPieces cp;
  return guarded([&]() -> int {
    contig_pieces_from_rows(who, seqdb_prefix, feed, cp);
    const std::vector<std::string> &ctg_names = cp.names;
    // ---- the FASTA (path_to_contig.py:109,115)
    FILE *f = out_path ? fopen(out_path, "wb") : stdout;
    PGX_REQUIRE(f, PGX_EIO, "cannot write %s", out_path);
    bool ok = true;
    for (const ContigPieces::Piece &pc : cp.pieces)
      for (size_t c = 0; c + 1 < pc.off.size() && ok; ++c) {
        const std::string &nm = ctg_names[pc.ctg0 + c];
        const uint64_t len = pc.off[c + 1] - pc.off[c];
        ok = fputc('>', f) != EOF && fwrite(nm.data(), 1, nm.size(), f) == nm.size() && fputc('\n', f) != EOF &&
             fwrite(pc.text + pc.off[c], 1, len, f) == len && fputc('\n', f) != EOF;
      }
    ok = (out_path ? fclose(f) == 0 : fflush(f) == 0) && ok;
    PGX_REQUIRE(ok, PGX_EIO, "writing %s failed", out_path ? out_path : "stdout");
    if (n_ctg_out) *n_ctg_out = ctg_names.size();
    if (n_bases_out) *n_bases_out = cp.bases;
    return PGX_OK;
  });
}

}  // namespace pgx

using namespace pgx;

extern "C" {

int pgx_align_batch2(pgx_seqdb *db, const pgx_align_key2 *keys, size_t n, int band, pgx_match *out) {
  return guarded([&]() -> int {
    require_ready();
    PGX_REQUIRE(db && (n == 0 || (keys && out)), PGX_EARG, "pgx_align_batch2: null argument");
    PGX_REQUIRE(band > 0 && band < (1 << 20), PGX_EARG, "bad band");
    PGX_REQUIRE(n < (1ULL << 30), PGX_EARG, "too many alignments for one call");
    for (size_t i = 0; i < n; ++i) {
      const auto &k = keys[i];
      PGX_REQUIRE(k.rid0 < db->rlen_by_rid.size() && k.rid1 < db->rlen_by_rid.size() && k.q_off <= db->rlen_by_rid[k.rid0] &&
                      k.t_off <= db->rlen_by_rid[k.rid1],
                  PGX_EARG, "alignment key %zu out of range", i);
    }
    if (n == 0) return PGX_OK;
    MemTag mem_tag("contigs");
    DevBuf<pgx_align_key2> d_keys(n);
    DevBuf<pgx_match> d_out(n);
    DevBuf<uint32_t> d_rids(db->d_seq.p ? 0 : 2 * n);
    d_keys.upload(keys, n);
    if (d_rids.n) hipLaunchKernelGGL(k_key_rids, dim3(cdiv(n, 256)), dim3(256), 0, ctx().stream, d_keys.p, (uint32_t)n, d_rids.p);
    ByteSource src(db, d_rids.p, (uint32_t)d_rids.n);
    dev_align2(db, src.seq, src.off, d_keys.p, n, band, d_out.p);
    d_out.download(out, n);
    pgx::sync();
    return PGX_OK;
  });
}

int pgx_contigs_resident(pgx_seqdb *db, const pgx_tile_row *rows, size_t n_rows, size_t n_ctg, char **text, uint64_t *ctg_off, uint64_t *text_len) {
  return guarded([&]() -> int {
    require_ready();
    PGX_REQUIRE(db && text && ctg_off && text_len && (n_rows == 0 || rows), PGX_EARG, "pgx_contigs_resident: null argument");
    std::vector<pgx_tile_row> r(rows, rows + n_rows);
    contigs_resident_rows("pgx_contigs_resident", db, r, n_ctg, text, ctg_off, text_len);
    return PGX_OK;
  });
}

int pgx_contigs_chunk(const char *seqdb_prefix, const char *tiling_path, const char *out_path, uint64_t *n_ctg_out, uint64_t *n_bases_out) {
  return contigs_from_rows("pgx_contigs_chunk", tiling_path ? seqdb_prefix : nullptr, [&](const TileRowFn &add) { feed_path_text(tiling_path, add); }, out_path, n_ctg_out, n_bases_out);
}

}  // extern "C"
