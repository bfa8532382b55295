// pgx_fasta.hip -- a FASTA text to a resident pgx_seqdb on the GPU: the record grammar of the reference's kseq reader
// (restated for a byte-serial reader in pgx_mkseqdb.hip: parse_some), the '\r' rule, the compaction of the sequence lines and the
// two-strand encoding of src/shmr_utils.c:44-51, each as per-byte / per-line predicates plus prefix sums.  Four passes:
//   marks  : k_fa_first (the first header marker m0, a min-reduction over wave64 ballots), k_fa_marks (line starts behind m0, their
//            number, the smallest line-start '+' -- the FASTQ refusal)
//   tables : the line starts (select), k_fa_lines (header / record / sequence-line flags), record of every line (scan), the sequence-line
//            table k_fa_seq_lines (start, kept length after the '\r' rule, record), pool offsets (scan), the record table k_fa_records
//            (header offset, name span, roff; rlen is the difference of consecutive roff, i.e. the segmented sum of the kept lengths)
//   gather : k_fa_gather, fixed tiles of TEXT bytes, a byte's line by search in the line table -> the ASCII pool
//   encode : k_fa_encode, fixed tiles of POOL bytes, a byte's record by search in roff -> the database's bytes, in place
// Only the names, roff and three numbers cross to the host.
#include <algorithm>

#include "pgx_fasta_k.h"

namespace pgx {
namespace {

// line j = [start[j], end): end is the '\n' in front of the next line start, or the end of the text (less its final '\n').  Line 0 is
// m0's header line.  is_rec: a header that starts a record (with eof_seen a marker that is the very last byte starts none); is_seq: a
// non-empty line that is no header.
__global__ void k_fa_lines(const uint8_t *__restrict__ b, uint64_t n, const uint64_t *__restrict__ start, uint64_t n_lines,
                           uint32_t eof_seen, uint32_t *__restrict__ is_rec, uint8_t *__restrict__ is_seq) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_lines) return;
  const uint64_t s = start[j];
  const uint64_t e = j + 1 < n_lines ? start[j + 1] - 1 : (b[n - 1] == '\n' ? n - 1 : n);
  const bool hdr = j == 0 || (e > s && fa_marker(b[s]));
  is_rec[j] = hdr && (s != n - 1 || !eof_seen) ? 1u : 0u;
  is_seq[j] = !hdr && e > s ? 1 : 0;
}

struct FastaOut {
  DevBuf<uint8_t> bytes;   // the database's bytes and their padding
  std::vector<uint64_t> roff;   // n_rec + 1
  std::vector<char> names;
};

// the passes, on d (n bytes of text on the device); throws the grammar's refusals
void fasta_passes(const uint8_t *d, uint64_t n, FastaOut &o) {
  hipStream_t st = ctx().stream;
  PrimWs tmp;
  // marks
  DevBuf<unsigned long long> acc(3);   // m0, number of line starts, smallest refused offset
  unsigned long long h_acc[3] = {NONE, 0, NONE};
  acc.upload(h_acc, 3);
  pgx::sync();   // (h_acc is read by the copy)
  if (n) hipLaunchKernelGGL(k_fa_first, dim3(cdiv(n, TILE)), dim3(TPB), 0, st, d, n, acc.p);
  acc.download(h_acc, 1);
  pgx::sync();
  const uint64_t m0 = h_acc[0];
  const uint32_t eof_seen = n % KS_BUF != 0;
  PGX_REQUIRE(m0 != NONE && (m0 != n - 1 || !eof_seen), PGX_EINVAL, "pgx_seqdb_from_fasta: no record in the text (%llu bytes)", (unsigned long long)n);
  DevBuf<uint64_t> start;
  uint64_t n_lines = 0;
  {
    DevBuf<uint8_t> ls(n);
    hipLaunchKernelGGL(k_fa_marks, dim3(cdiv(n, TILE)), dim3(TPB), 0, st, d, n, m0, ls.p, acc.p + 1);
    acc.download(h_acc, 3);
    pgx::sync();
    PGX_REQUIRE(h_acc[2] == NONE, PGX_EINVAL,
                "pgx_seqdb_from_fasta: a line starts with '+' at byte offset %llu: FASTQ records are not read here (use shmr_mkseqdb)", h_acc[2]);
    n_lines = h_acc[1];
    PGX_REQUIRE(n_lines < (1ull << 31), PGX_EINVAL, "pgx_seqdb_from_fasta: %llu lines (2^31 and more are not read here)", (unsigned long long)n_lines);
    start.alloc(n_lines + 1);
    // (the select takes at most 2^30 flags a call)
    uint64_t got = 0;
    for (uint64_t at = 0; at < n; at += 1ull << 30) {
      const uint64_t len = std::min<uint64_t>(n - at, 1ull << 30);
      const uint64_t c = select_indices(ls.p + at, len, start.p + got, &tmp);
      if (c && at) hipLaunchKernelGGL(k_fa_add_base, dim3(cdiv(c, 256)), dim3(256), 0, st, start.p + got, c, at);
      got += c;
      PGX_REQUIRE(got <= n_lines, PGX_EHIP, "pgx_seqdb_from_fasta: the line starts were counted as %llu and selected as more", (unsigned long long)n_lines);
    }
    PGX_REQUIRE(got == n_lines, PGX_EHIP, "pgx_seqdb_from_fasta: the line starts were counted as %llu and selected as %llu", (unsigned long long)n_lines,
                (unsigned long long)got);
  }
  // tables
  DevBuf<uint32_t> is_rec(n_lines + 1), rec_incl(n_lines + 2);
  DevBuf<uint8_t> is_seq(n_lines + 1);
  LAUNCH(k_fa_lines, n_lines, d, n, start.p, n_lines, eof_seen, is_rec.p, is_seq.p);
  const uint32_t n_rec = scan_to_total(is_rec.p, rec_incl.p, n_lines, &tmp);
  DevBuf<uint32_t> hl((size_t)n_rec + 1), sl(n_lines + 1);
  const uint32_t n_hl = select_indices(is_rec.p, n_lines, hl.p, &tmp);
  const uint32_t n_sl = select_indices(is_seq.p, n_lines, sl.p, &tmp);
  PGX_REQUIRE(n_hl == n_rec && n_rec >= 1, PGX_EHIP, "pgx_seqdb_from_fasta: %u record headers scanned, %u selected", n_rec, n_hl);
  is_rec.release(), is_seq.release();
  DevBuf<uint64_t> l_start((size_t)n_sl + 1), l_kept((size_t)n_sl + 1), pool_off((size_t)n_sl + 2);
  DevBuf<uint32_t> l_rec((size_t)n_sl + 1);
  if (n_sl) LAUNCH(k_fa_seq_lines, n_sl, d, n, start.p, n_lines, sl.p, n_sl, rec_incl.p, eof_seen, l_start.p, l_kept.p, l_rec.p);
  const uint64_t pool_size = scan_to_total(l_kept.p, pool_off.p, n_sl, &tmp);
  if (!n_sl) PGX_HIP(hipMemsetAsync(pool_off.p, 0, sizeof(uint64_t), st));
  DevBuf<uint64_t> hdr_off((size_t)n_rec + 1), name_len1((size_t)n_rec + 1), name_off((size_t)n_rec + 2), roff((size_t)n_rec + 1);
  LAUNCH(k_fa_records, (size_t)n_rec + 1, d, n, start.p, hl.p, n_rec, l_rec.p, n_sl, pool_off.p, hdr_off.p, name_len1.p, roff.p);
  const uint64_t names_size = scan_to_total(name_len1.p, name_off.p, n_rec, &tmp);
  DevBuf<char> names(names_size + 1);
  LAUNCH(k_fa_names, n_rec, d, hdr_off.p, name_off.p, n_rec, names.p);
  o.roff.resize((size_t)n_rec + 1);
  o.names.resize(names_size);
  roff.download(o.roff.data(), (size_t)n_rec + 1);
  names.download(o.names.data(), names_size);
  start.release(), sl.release(), hl.release(), rec_incl.release();
  // gather
  DevBuf<uint8_t> pool(pool_size + 1);
  if (pool_size) hipLaunchKernelGGL(k_fa_gather, dim3(cdiv(n, TILE)), dim3(TPB), 0, st, d, n, l_start.p, l_kept.p, pool_off.p, n_sl, pool.p, pool_size);
  // encode, into the database's own block
  {
    MemTag mem_tag("seqdb.bytes");
    o.bytes.alloc(pool_size + 1024);
  }
  PGX_HIP(hipMemsetAsync(o.bytes.p + pool_size, 0, 1024, st));
  if (pool_size) hipLaunchKernelGGL(k_fa_encode, dim3(cdiv(pool_size, TILE)), dim3(TPB), 0, st, pool.p, pool_size, roff.p, n_rec, o.bytes.p);
  PGX_HIP(hipGetLastError());
  pgx::sync();   // (the tables and the pool go back to the block cache behind this)
}

}  // namespace
}  // namespace pgx

using namespace pgx;

extern "C" int pgx_seqdb_from_fasta(const char *text, size_t len, int on_device, pgx_seqdb **out, char **names, size_t *names_len, uint64_t *n_reads,
                                    uint64_t *n_bases) {
  return guarded([&]() -> int {
    require_ready();
    PGX_REQUIRE(out && names && names_len && (text || len == 0), PGX_EARG, "pgx_seqdb_from_fasta: null argument");
    *out = nullptr, *names = nullptr, *names_len = 0;
    FastaOut o;
    int code = PGX_OK;
    try {
      MemTag mem_tag("fasta");
      KernelTimer tm("fasta", len);
      DevBuf<uint8_t> copy;
      const uint8_t *d = (const uint8_t *)text;
      if (!on_device) {
        copy.alloc(len + 1);
        copy.upload((const uint8_t *)text, len);
        d = copy.p;
      }
      fasta_passes(d, len, o);
    } catch (const Fail &f) {
      code = build_fail_code(f, "pgx_seqdb_from_fasta", "tables, pool and database", len, "bytes of text");
    }
    timing_flush();
    if (code != PGX_OK) return code;
    const size_t n_rec = o.roff.size() - 1;
    std::vector<uint32_t> rid(n_rec), rlen(n_rec);
    for (size_t r = 0; r < n_rec; ++r) {
      const uint64_t l = o.roff[r + 1] - o.roff[r];
      if (l >= (1ull << 32)) {
        size_t a = 0;
        for (size_t k = 0; k < r; ++k) a = (size_t)(std::find(o.names.begin() + a, o.names.end(), '\n') - o.names.begin()) + 1;
        const size_t e = (size_t)(std::find(o.names.begin() + a, o.names.end(), '\n') - o.names.begin());
        PGX_REQUIRE(false, PGX_EINVAL, "pgx_seqdb_from_fasta: record %zu ('%.*s') has %llu bases (2^32 and more do not fit the idx)", r, (int)std::min<size_t>(e - a, 200),
                    o.names.data() + a, (unsigned long long)l);
      }
      rid[r] = (uint32_t)r, rlen[r] = (uint32_t)l;
    }
    char *nm = (char *)malloc(o.names.size() + 1);
    if (!nm) throw std::bad_alloc();
    memcpy(nm, o.names.data(), o.names.size());
    nm[o.names.size()] = 0;
    const int rc = seqdb_take_dev(std::move(o.bytes), (size_t)o.roff[n_rec], rid.data(), rlen.data(), o.roff.data(), (uint32_t)n_rec, out);
    if (rc != PGX_OK) {
      free(nm);
      return rc;
    }
    *names = nm, *names_len = o.names.size();
    if (n_reads) *n_reads = n_rec;
    if (n_bases) *n_bases = o.roff[n_rec];
    return PGX_OK;
  });
}

extern "C" int pgx_seqdb_save(pgx_seqdb *db, const char *names, size_t names_len, const char *seqdb_prefix) {
  return guarded([&]() -> int {
    require_ready();
    PGX_REQUIRE(db && seqdb_prefix && (names || names_len == 0), PGX_EARG, "pgx_seqdb_save: null argument");
    PGX_REQUIRE(db->d_seq.p, PGX_ESTATE, "pgx_seqdb_save: the seqdb's bytes were released (pgx_seqdb_release_bytes / pgx_seqdb_compact_bytes)");
    const size_t nr = db->rid.size();
    std::vector<std::pair<size_t, size_t>> span;   // the names' [begin, end) in `names`
    for (size_t a = 0; a < names_len;) {
      const char *nl = (const char *)memchr(names + a, '\n', names_len - a);
      const size_t e = nl ? (size_t)(nl - names) : names_len;
      span.emplace_back(a, e);
      a = e + 1;
    }
    PGX_REQUIRE(span.size() == nr, PGX_EARG, "pgx_seqdb_save: %zu names for %zu reads", span.size(), nr);
    std::vector<uint8_t> bytes(db->nbytes);
    if (db->nbytes) PGX_HIP(hipMemcpyAsync(bytes.data(), db->d_seq.p, db->nbytes, hipMemcpyDeviceToHost, ctx().stream));
    pgx::sync();
    const std::string pre(seqdb_prefix);
    FILE *fdb = fopen((pre + ".seqdb").c_str(), "wb");
    PGX_REQUIRE(fdb, PGX_EIO, "cannot create %s.seqdb", seqdb_prefix);
    const bool ok_db = (!db->nbytes || fwrite(bytes.data(), 1, db->nbytes, fdb) == db->nbytes);
    const bool closed_db = fclose(fdb) == 0;
    PGX_REQUIRE(ok_db && closed_db, PGX_EIO, "short write to %s.seqdb", seqdb_prefix);
    FILE *fidx = fopen((pre + ".idx").c_str(), "w");
    PGX_REQUIRE(fidx, PGX_EIO, "cannot create %s.idx", seqdb_prefix);
    bool ok = true;
    for (size_t i = 0; i < nr && ok; ++i)
      ok = fprintf(fidx, "%09d %.*s %u %lu\n", (int)db->rid[i], (int)(span[i].second - span[i].first), names + span[i].first, (unsigned)db->rlen[i],
                   (unsigned long)db->roff[i]) > 0;
    ok = (fclose(fidx) == 0) && ok;
    PGX_REQUIRE(ok, PGX_EIO, "short write to %s.idx", seqdb_prefix);
    return PGX_OK;
  });
}
