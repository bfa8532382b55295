// pgx_mapmerge.hip -- the step between shmr_map and pg_asm_cns.py: `cat map-*.dat | LC_ALL=C sort -k 1 -g -k 2 -g` (pg_run.py:491-496) on
// the device.  The rule: by field 0 as a number, by field 1 as a number, then by the whole line bytewise -- which
// for canonical decimals is fields 2 .. 8 compared as decimal STRINGS.  A field's string order is the numeric order of
// (v * 10^(10 - ndigits(v)), ndigits(v)), 38 bits; the seven of them back to back are 266 bits, a row's tie key of five 64-bit words.
//
//   k_mm_key        ref_id << 32 | ref_bgn and the row's index; one stable 64-bit radix sort puts every row in its run of equal keys
//   k_mm_heads      run heads (select: where every run starts), k_mm_classify: a run's path by its length, the counts of the stats
//   k_mm_run_wave   a run of 2 .. 64 rows on one wavefront: a row per lane, its rank by counting over the lanes' keys (shuffles)
//   k_mm_run_group  a run of up to RUN_MAX rows on one workgroup: the keys in LDS word by word, a row's rank by counting
//   lsd_runs        longer runs: their rows selected, five stable passes over the tie key's words from the last, a sixth over the run
//   k_mm_gather     the rows in the final order
// and the file level: k_mm_lines (a thread per line: nine canonical decimals below 2^32, single blanks, nothing else) behind the line
// select the consensus job's parser uses (k_par_newlines), MapLines (the rows as text through the piece scheme of pgx_text.h).
#include <algorithm>
#include <string>

#include "pgx_internal.h"
#include "pgx_text.h"

namespace pgx {
namespace {

constexpr uint32_t WAVE_RUN = 64;       // rows of a run one wavefront ranks
constexpr uint32_t RUN_MAX = 1024;      // ... one workgroup: 5 x 8 x 1024 = 40 KiB of LDS, 4 K comparisons a thread
constexpr uint32_t KEY_WORDS = 5, GROUP_THREADS = 256;
enum { S_TIE_RUNS, S_LONGEST, S_WAVE, S_GROUP, S_LSD, S_SLOTS };

uint32_t run_max_hook() {
  const char *e = getenv("PGX_MERGE_RUN_MAX");
  const long v = e ? atol(e) : 0;
  return v > 0 ? (uint32_t)std::min<long>(v, RUN_MAX) : RUN_MAX;   // (below 64 it bounds the wavefront's runs too; 1: every tie run is a long one)
}
size_t piece_hook() {
  const char *e = getenv("PGX_MERGE_PIECE");
  return e && atol(e) > 0 ? (size_t)atol(e) : (size_t)64 << 20;
}

// the decimal string of v among decimal strings, as a number: the digits left-aligned in ten places, then the length
__device__ inline uint64_t field_key(uint32_t v) {
  const uint32_t nd = ndigits(v);
  uint64_t s = v;
  for (uint32_t k = nd; k < 10; ++k) s *= 10u;
  return s << 4 | nd;   // < 10^10 * 16 < 2^38
}
// fields 2 .. 8 of a row as one 266-bit number, most significant word first
__device__ inline void tie_key(const uint32_t *row, uint64_t w[KEY_WORDS]) {
#pragma unroll
  for (uint32_t k = 0; k < KEY_WORDS; ++k) w[k] = 0;
#pragma unroll
  for (int f = 0; f < 7; ++f) {
    const uint64_t k = field_key(row[2 + f]);
    const int pos = f * 38, wi = pos >> 6, left = 64 - (pos & 63) - 38;   // left: blanks behind the field in its first word
    if (left >= 0) {
      w[wi] |= k << left;
    } else {
      w[wi] |= k >> -left;
      w[wi + 1] |= k << (64 + left);
    }
  }
}

__global__ void k_mm_key(const uint32_t *__restrict__ rows, uint32_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ val) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  key[i] = (uint64_t)rows[(size_t)i * 9] << 32 | rows[(size_t)i * 9 + 1];
  val[i] = i;
}
__global__ void k_mm_heads(const uint64_t *__restrict__ skey, uint32_t n, uint8_t *__restrict__ head) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) head[j] = j == 0 || skey[j] != skey[j - 1];
}
__device__ inline uint32_t wave_sum(uint32_t v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
__device__ inline uint32_t wave_max(uint32_t v) {
  for (int d = 32; d > 0; d >>= 1) v = max(v, (uint32_t)__shfl_xor(v, d));
  return v;
}
// run r is the sorted positions [start[r], start[r + 1]) (start[n_runs] = n): which path orders it, and the stats (a wavefront adds
// its runs up before it touches the counters)
__global__ void k_mm_classify(const uint32_t *__restrict__ start, uint32_t n_runs, uint32_t n, uint32_t run_max, uint8_t *__restrict__ is_wave,
                              uint8_t *__restrict__ is_group, uint8_t *__restrict__ is_lsd, unsigned long long *__restrict__ stat) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t len = 0;
  if (r < n_runs) len = (r + 1 < n_runs ? start[r + 1] : n) - start[r];
  const bool on_wave = len > 1 && len <= min(WAVE_RUN, run_max), on_group = len > WAVE_RUN && len <= run_max, on_lsd = len > 1 && len > run_max;
  if (r < n_runs) is_wave[r] = on_wave, is_group[r] = on_group, is_lsd[r] = on_lsd;
  const uint32_t ties = wave_sum(len > 1), longest = wave_max(len);
  const uint32_t w = wave_sum(on_wave ? len : 0), g = wave_sum(on_group ? len : 0);
  // (a wavefront's long runs may hold 2^32 rows and more between them: summed in 64 bits)
  unsigned long long l = on_lsd ? len : 0;
  for (int d = 32; d > 0; d >>= 1) l += __shfl_xor(l, d);
  if ((threadIdx.x & 63) == 0) {
    if (ties) atomicAdd(&stat[S_TIE_RUNS], (unsigned long long)ties);
    if (w) atomicAdd(&stat[S_WAVE], (unsigned long long)w);
    if (g) atomicAdd(&stat[S_GROUP], (unsigned long long)g);
    if (l) atomicAdd(&stat[S_LSD], l);
    atomicMax(&stat[S_LONGEST], (unsigned long long)longest);
  }
}

__device__ inline bool key_less(const uint64_t a[KEY_WORDS], const uint64_t b[KEY_WORDS], bool a_first) {
#pragma unroll
  for (uint32_t k = 0; k < KEY_WORDS; ++k)
    if (a[k] != b[k]) return a[k] < b[k];
  return a_first;   // equal keys are identical lines: their places only have to differ
}
// a wavefront per run of list[]: lane l holds row l of the run, and counts the rows that come before its own
__global__ __launch_bounds__(256) void k_mm_run_wave(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ start,
                                                     uint32_t n_runs, uint32_t n, const uint32_t *__restrict__ list, uint32_t n_list,
                                                     uint32_t *__restrict__ order) {
  const uint32_t x = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (x >= n_list) return;   // (the whole wavefront)
  const uint32_t r = list[x], s = start[r], len = (r + 1 < n_runs ? start[r + 1] : n) - s;   // 2 <= len <= 64
  const bool have = lane < len;
  const uint32_t idx = have ? sidx[s + lane] : 0;
  uint64_t mine[KEY_WORDS] = {0, 0, 0, 0, 0};
  if (have) tie_key(rows + (size_t)idx * 9, mine);
  uint32_t rank = 0;
  for (uint32_t j = 0; j < len; ++j) {   // (len is the wavefront's: every lane takes part in every shuffle)
    uint64_t other[KEY_WORDS];
#pragma unroll
    for (uint32_t k = 0; k < KEY_WORDS; ++k) other[k] = __shfl(mine[k], (int)j);
    rank += key_less(other, mine, j < lane);
  }
  if (have) order[s + rank] = idx;
}
// a workgroup per run of list[]: the keys of its len <= cap rows in LDS, word k of row i at keys[k * cap + i]; a thread reads row j's
// words at the same address as its neighbours (a broadcast)
__global__ __launch_bounds__(GROUP_THREADS) void k_mm_run_group(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ sidx,
                                                                const uint32_t *__restrict__ start, uint32_t n_runs, uint32_t n,
                                                                const uint32_t *__restrict__ list, uint32_t cap, uint32_t *__restrict__ order) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];
  const uint32_t r = list[blockIdx.x], s = start[r];
  const uint32_t len = min((r + 1 < n_runs ? start[r + 1] : n) - s, cap);   // (<= cap by the list's making)
  for (uint32_t i = threadIdx.x; i < len; i += GROUP_THREADS) {
    uint64_t w[KEY_WORDS];
    tie_key(rows + (size_t)sidx[s + i] * 9, w);
#pragma unroll
    for (uint32_t k = 0; k < KEY_WORDS; ++k) keys[k * cap + i] = w[k];
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < len; i += GROUP_THREADS) {
    uint64_t mine[KEY_WORDS];
#pragma unroll
    for (uint32_t k = 0; k < KEY_WORDS; ++k) mine[k] = keys[k * cap + i];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < len; ++j) {
      bool less = j < i;
      for (uint32_t k = 0; k < KEY_WORDS; ++k) {   // (the later words are read only behind equal earlier ones)
        const uint64_t o = keys[k * cap + j];
        if (o != mine[k]) {
          less = o < mine[k];
          break;
        }
      }
      rank += less;
    }
    order[s + rank] = sidx[s + i];
  }
}

// ---- the runs no workgroup holds ------------------------------------------------------------------------------------------------------
__global__ void k_mm_mark(const uint32_t *__restrict__ start, uint32_t n_runs, uint32_t n, const uint32_t *__restrict__ list, uint8_t *__restrict__ flag) {
  const uint32_t r = list[blockIdx.x], s = start[r], e = r + 1 < n_runs ? start[r + 1] : n;
  for (uint32_t p = s + threadIdx.x; p < e; p += blockDim.x) flag[p] = 1;
}
// selected row t is sorted position pos[t]: word k of its tie key at kw[k * m + t]
__global__ void k_mm_lsd_keys(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ pos, uint32_t m,
                              uint64_t *__restrict__ kw, uint32_t *__restrict__ perm) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m) return;
  uint64_t w[KEY_WORDS];
  tie_key(rows + (size_t)sidx[pos[t]] * 9, w);
#pragma unroll
  for (uint32_t k = 0; k < KEY_WORDS; ++k) kw[(size_t)k * m + t] = w[k];
  perm[t] = t;
}
__global__ void k_mm_lsd_take(const uint64_t *__restrict__ word, const uint32_t *__restrict__ perm, uint32_t m, uint64_t *__restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < m) out[t] = word[perm[t]];
}
__global__ void k_mm_lsd_take_run(const uint64_t *__restrict__ skey, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ perm, uint32_t m,
                                  uint64_t *__restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < m) out[t] = skey[pos[perm[t]]];
}
__global__ void k_mm_lsd_place(const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ perm, uint32_t m,
                               uint32_t *__restrict__ order) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < m) order[pos[t]] = sidx[pos[perm[t]]];
}
__global__ void k_mm_gather(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ order, uint32_t n, uint32_t *__restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (n < 2^31: n * 9 needs 64 bits)
  if (t >= (uint64_t)n * 9) return;
  const uint32_t j = (uint32_t)(t / 9), f = (uint32_t)(t - (uint64_t)j * 9);
  out[t] = rows[(size_t)order[j] * 9 + f];
}

// The rows of the long runs alone through an LSD sort: the tie key's words from the last to the first, then the run's own key -- six
// stable passes, each over the m selected rows.  The selected positions are ascending, so the j-th row of the result belongs at pos[j].
void lsd_runs(const uint32_t *d_rows, const uint32_t *sidx, const uint64_t *skey, const uint32_t *start, uint32_t n_runs, uint32_t n, const uint32_t *list,
              uint32_t n_list, uint32_t *order, PrimWs *ws) {
  hipStream_t st = ctx().stream;
  DevBuf<uint8_t> flag(n);
  DevBuf<uint32_t> pos(n);
  PGX_HIP(hipMemsetAsync(flag.p, 0, n, st));
  hipLaunchKernelGGL(k_mm_mark, dim3(n_list), dim3(256), 0, st, start, n_runs, n, list, flag.p);
  const uint32_t m = select_indices(flag.p, n, pos.p, ws);
  flag.release();
  DevBuf<uint64_t> kw((size_t)KEY_WORDS * m), k_in(m), k_out(m);
  DevBuf<uint32_t> perm(m), perm2(m);
  LAUNCH(k_mm_lsd_keys, m, d_rows, sidx, pos.p, m, kw.p, perm.p);
  uint32_t *a = perm.p, *b = perm2.p;
  for (int k = (int)KEY_WORDS - 1; k >= 0; --k) {
    LAUNCH(k_mm_lsd_take, m, kw.p + (size_t)k * m, a, m, k_in.p);
    sort_pairs(k_in.p, k_out.p, a, b, m, k == (int)KEY_WORDS - 1 ? 54 : 0, 64, ws);   // (the last word holds the key's last 10 bits)
    std::swap(a, b);
  }
  LAUNCH(k_mm_lsd_take_run, m, skey, pos.p, a, m, k_in.p);
  sort_pairs(k_in.p, k_out.p, a, b, m, 0, 64, ws);
  LAUNCH(k_mm_lsd_place, m, sidx, pos.p, b, m, order);
  PGX_HIP(hipGetLastError());
  sync();   // (the temporaries go back to the block cache with this scope)
}

}  // namespace

// n > 0 rows (9 x u32, device) in the merge's order to d_out (device, not d_rows)
void map_merge_dev(const uint32_t *d_rows, uint32_t n, uint32_t *d_out, pgx_map_merge_stats *ms) {
  hipStream_t st = ctx().stream;
  PrimWs ws;
  const double t0 = wall_ms();
  DevBuf<uint64_t> key(n), skey(n);
  DevBuf<uint32_t> val(n), sidx(n), order(n);
  LAUNCH(k_mm_key, n, d_rows, n, key.p, val.p);
  sync();
  const double t1 = wall_ms();
  sort_pairs(key.p, skey.p, val.p, sidx.p, n, 0, 64, &ws);
  sync();
  const double t2 = wall_ms();
  key.release(), val.release();
  // the runs
  DevBuf<uint8_t> head(n);
  DevBuf<uint32_t> start(n);
  LAUNCH(k_mm_heads, n, skey.p, n, head.p);
  const uint32_t n_runs = select_indices(head.p, n, start.p, &ws);
  head.release();
  const uint32_t run_max = run_max_hook();
  DevBuf<uint8_t> is_wave(n_runs), is_group(n_runs), is_lsd(n_runs);
  DevBuf<uint32_t> wave_list(n_runs), group_list(n_runs), lsd_list(n_runs);
  DevBuf<unsigned long long> stat(S_SLOTS);
  PGX_HIP(hipMemsetAsync(stat.p, 0, S_SLOTS * sizeof(unsigned long long), st));
  LAUNCH(k_mm_classify, n_runs, start.p, n_runs, n, run_max, is_wave.p, is_group.p, is_lsd.p, stat.p);
  const uint32_t n_wave = select_indices(is_wave.p, n_runs, wave_list.p, &ws);
  const uint32_t n_group = select_indices(is_group.p, n_runs, group_list.p, &ws);
  const uint32_t n_lsd = select_indices(is_lsd.p, n_runs, lsd_list.p, &ws);
  // every run in place: a run of one row where the sort left it, the others by their paths
  PGX_HIP(hipMemcpyAsync(order.p, sidx.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  if (n_wave) LAUNCH(k_mm_run_wave, (size_t)n_wave * 64, d_rows, sidx.p, start.p, n_runs, n, wave_list.p, n_wave, order.p);
  if (n_group)
    hipLaunchKernelGGL(k_mm_run_group, dim3(n_group), dim3(GROUP_THREADS), (size_t)run_max * KEY_WORDS * sizeof(uint64_t), st, d_rows, sidx.p, start.p, n_runs, n,
                       group_list.p, run_max, order.p);
  if (n_lsd) lsd_runs(d_rows, sidx.p, skey.p, start.p, n_runs, n, lsd_list.p, n_lsd, order.p, &ws);
  LAUNCH(k_mm_gather, (size_t)n * 9, d_rows, order.p, n, d_out);
  PGX_HIP(hipGetLastError());
  unsigned long long h[S_SLOTS];
  stat.download(h, S_SLOTS);
  sync();
  const double t3 = wall_ms();
  if (ms) {
    ms->n_rows = n, ms->n_runs = n_runs, ms->n_tie_runs = h[S_TIE_RUNS], ms->longest_run = h[S_LONGEST];
    ms->rows_wave = h[S_WAVE], ms->rows_group = h[S_GROUP], ms->rows_lsd = h[S_LSD];
    ms->key_ms += t1 - t0, ms->sort_ms += t2 - t1, ms->ties_ms += t3 - t2;
  }
}

namespace {

// ---- rows of the host form: n x 9 int64 ---------------------------------------------------------------------------------------------
__global__ void k_mm_narrow(const int64_t *__restrict__ in, uint64_t n_vals, uint32_t *__restrict__ out, unsigned long long *__restrict__ bad) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_vals) return;
  const int64_t v = in[t];
  if (v < 0 || v > (int64_t)UINT32_MAX) atomicMin(bad, (unsigned long long)(t / 9));
  out[t] = (uint32_t)v;
}
__global__ void k_mm_widen(const uint32_t *__restrict__ in, uint64_t n_vals, int64_t *__restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_vals) out[t] = in[t];
}

// ---- text -> rows: a thread per line, line k is text[nlpos[k - 1] + 1, nlpos[k]) --------------------------------------------------------
__global__ void k_mm_lines(const char *__restrict__ text, const uint32_t *__restrict__ nlpos, uint32_t nl, uint32_t *__restrict__ rows, uint32_t *__restrict__ err) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nl) return;
  const uint32_t begin = k ? nlpos[k - 1] + 1 : 0, len = nlpos[k] - begin;
  const char *p = text + begin;
  uint32_t i = 0;
  bool ok = true;
  for (int f = 0; f < 9 && ok; ++f) {
    const uint32_t a = i;
    uint64_t v = 0;
    while (i < len && i - a < 11 && p[i] >= '0' && p[i] <= '9') v = v * 10 + (uint64_t)(p[i] - '0'), ++i;   // (11 digits: < 2^37)
    const uint32_t nd = i - a;
    ok = nd >= 1 && nd <= 10 && !(nd > 1 && p[a] == '0') && v <= UINT32_MAX;
    rows[(size_t)k * 9 + f] = (uint32_t)v;
    if (ok && f < 8) ok = i < len && p[i++] == ' ';
  }
  if (!ok || i != len) atomicMin(err, k);
}

// the rows as text, "%u %u %u %u %u %u %d %u %u\n" (src/shmr_map.c:153): a piece source of pgx_text.h, every line a piece
struct MapLines {
  const uint32_t *rows;
  uint32_t n;
  static constexpr uint32_t MAX = 112;   // nine numbers of <= 10 digits, eight blanks, a newline: 99
  template <bool WRITE>
  __device__ uint32_t piece(uint32_t j, char *dst) const {
    LineOut<WRITE> o{dst, 0};
    const uint32_t *r = rows + (size_t)j * 9;
#pragma unroll
    for (int f = 0; f < 9; ++f) o.u32(r[f]), o.ch(f == 8 ? '\n' : ' ');
    return o.n;
  }
};

struct FileHandle {
  FILE *f = nullptr;
  bool own = true;
  ~FileHandle() {
    if (f && own) fclose(f);
  }
};
struct StageHandle {
  TextStage ts;
  ~StageHandle() { ts.drop(); }
};

// the lines of one file as rows (device, 9 x u32), in pieces of the file that end at a line's end
void parse_file(const char *who, const char *path, size_t piece, std::vector<DevBuf<uint32_t>> &parts, std::vector<uint32_t> &part_n, uint64_t *n_rows, PrimWs *ws) {
  hipStream_t st = ctx().stream;
  const bool is_stdin = strcmp(path, "-") == 0;
  const char *name = is_stdin ? "<stdin>" : path;
  FileHandle in;
  in.f = is_stdin ? stdin : fopen(path, "rb"), in.own = !is_stdin;
  PGX_REQUIRE(in.f, PGX_EIO, "%s: cannot open %s", who, name);
  std::vector<char> buf;
  uint64_t lines_before = 0;
  bool eof = false;
  while (!eof) {
    const size_t had = buf.size();
    buf.resize(had + piece);
    const size_t got = fread(buf.data() + had, 1, piece, in.f);
    PGX_REQUIRE(got == piece || !ferror(in.f), PGX_EIO, "%s: cannot read %s", who, name);
    buf.resize(had + got);
    eof = got < piece;
    if (eof && !buf.empty() && buf.back() != '\n') buf.push_back('\n');   // a last line without its end is a line
    const char *last = buf.empty() ? nullptr : (const char *)memrchr(buf.data(), '\n', buf.size());
    if (!last) continue;   // (a line longer than a piece: read on)
    const size_t nb = (size_t)(last - buf.data()) + 1;
    PGX_REQUIRE(nb < (1ull << 31), PGX_EARG, "%s: a piece of %s of 2^31 bytes and more", who, name);
    const uint32_t n = (uint32_t)nb;
    DevBuf<char> d_text(n);
    DevBuf<uint8_t> flag(n);
    DevBuf<uint32_t> nlpos(n), err(1);
    PGX_HIP(hipMemcpyAsync(d_text.p, buf.data(), n, hipMemcpyHostToDevice, st));
    PGX_HIP(hipMemsetAsync(err.p, 0xFF, sizeof(uint32_t), st));
    LAUNCH(k_par_newlines, n, d_text.p, n, flag.p);
    const uint32_t nl = select_indices(flag.p, n, nlpos.p, ws);
    PGX_REQUIRE(*n_rows + nl < (1ull << 31), PGX_EARG, "%s: 2^31 lines and more", who);
    parts.emplace_back((size_t)nl * 9);
    part_n.push_back(nl);
    LAUNCH(k_mm_lines, nl, d_text.p, nlpos.p, nl, parts.back().p, err.p);
    uint32_t bad = 0;
    err.download(&bad, 1);
    sync();   // (the text and the line ends go back to the block cache with this scope)
    PGX_REQUIRE(bad == UINT32_MAX, PGX_EINVAL, "%s: %s: line %llu is not nine canonical decimals below 2^32 separated by single blanks", who, name,
                (unsigned long long)(lines_before + bad));
    *n_rows += nl, lines_before += nl;
    buf.erase(buf.begin(), buf.begin() + nb);
  }
}

// a Fail that is the device out of memory answers PGX_ENOMEM: the merge has no host spill
template <class F>
int merge_call(const char *who, const uint64_t *n, F &&body) {
  return guarded([&]() -> int {
    try {
      body();
    } catch (const Fail &f) {
      return build_fail_code(f, who, "merge", *n, "rows");
    }
    return PGX_OK;
  });
}

}  // namespace
}  // namespace pgx

using namespace pgx;

extern "C" {

int pgx_map_merge_dev(const uint32_t *d_rows, uint64_t n, uint32_t *d_out, pgx_map_merge_stats *stats) {
  return merge_call("pgx_map_merge_dev", &n, [&] {
    require_ready();
    const char *who = "pgx_map_merge_dev";
    if (stats) memset(stats, 0, sizeof(*stats));
    PGX_REQUIRE(n == 0 || (d_rows && d_out && d_rows != d_out), PGX_EARG, "%s: null argument, or the rows sorted onto themselves", who);
    PGX_REQUIRE(n < (1ull << 31), PGX_EARG, "%s: 2^31 rows and more", who);
    if (n == 0) return;
    MemTag mem_tag("map.merge");
    map_merge_dev(d_rows, (uint32_t)n, d_out, stats);
  });
}

int pgx_map_merge_rows(const int64_t *rows, size_t n, int64_t *out, pgx_map_merge_stats *stats) {
  uint64_t n64 = n;
  return merge_call("pgx_map_merge_rows", &n64, [&] {
    require_ready();
    const char *who = "pgx_map_merge_rows";
    if (stats) memset(stats, 0, sizeof(*stats));
    PGX_REQUIRE(n == 0 || (rows && out), PGX_EARG, "%s: null argument", who);
    PGX_REQUIRE(n < (1ull << 31), PGX_EARG, "%s: 2^31 rows and more", who);
    if (n == 0) return;
    MemTag mem_tag("map.merge");
    hipStream_t st = ctx().stream;
    const uint64_t nv = (uint64_t)n * 9;
    DevBuf<uint32_t> d_rows(nv), d_out(nv);
    DevBuf<unsigned long long> bad(1);
    {
      DevBuf<int64_t> wide(nv);
      wide.upload(rows, nv);
      PGX_HIP(hipMemsetAsync(bad.p, 0xFF, sizeof(unsigned long long), st));
      LAUNCH(k_mm_narrow, nv, wide.p, nv, d_rows.p, bad.p);
      unsigned long long b = 0;
      bad.download(&b, 1);
      sync();
      PGX_REQUIRE(b == ~0ull, PGX_EINVAL, "%s: row %llu holds a value outside [0, 2^32)", who, b);
    }
    map_merge_dev(d_rows.p, (uint32_t)n, d_out.p, stats);
    d_rows.release();
    DevBuf<int64_t> wide(nv);
    LAUNCH(k_mm_widen, nv, d_out.p, nv, wide.p);
    wide.download(out, nv);
    sync();
  });
}

int pgx_map_merge(const char *const *paths, size_t n_paths, const char *out_path, pgx_map_merge_stats *stats) {
  uint64_t n_rows = 0;
  return merge_call("pgx_map_merge", &n_rows, [&] {
    require_ready();
    const char *who = "pgx_map_merge";
    if (stats) memset(stats, 0, sizeof(*stats));
    PGX_REQUIRE(n_paths == 0 || paths, PGX_EARG, "%s: null argument", who);
    for (size_t k = 0; k < n_paths; ++k) PGX_REQUIRE(paths[k], PGX_EARG, "%s: null argument", who);
    MemTag mem_tag("map.merge");
    hipStream_t st = ctx().stream;
    pgx_map_merge_stats ms = {};
    PrimWs ws;
    const size_t piece = piece_hook();
    const double t0 = wall_ms();
    // every file to rows; nothing is written before the last line has passed
    std::vector<DevBuf<uint32_t>> parts;
    std::vector<uint32_t> part_n;
    for (size_t k = 0; k < n_paths; ++k) parse_file(who, paths[k], piece, parts, part_n, &n_rows, &ws);
    const uint32_t n = (uint32_t)n_rows;
    DevBuf<uint32_t> d_rows((size_t)n * 9), d_out;
    uint64_t at = 0;
    for (size_t k = 0; k < parts.size(); ++k) {
      if (part_n[k]) PGX_HIP(hipMemcpyAsync(d_rows.p + at * 9, parts[k].p, (size_t)part_n[k] * 9 * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
      at += part_n[k];
    }
    sync();
    parts.clear();
    ms.parse_ms = wall_ms() - t0;
    if (n) {
      d_out.alloc((size_t)n * 9);
      map_merge_dev(d_rows.p, n, d_out.p, &ms);
      d_rows.release();
    }
    // the text, in pieces of whole lines
    const double t1 = wall_ms();
    FileHandle out;
    out.f = out_path ? fopen(out_path, "wb") : stdout, out.own = out_path != nullptr;
    PGX_REQUIRE(out.f, PGX_EIO, "%s: cannot write %s", who, out_path ? out_path : "stdout");
    const uint32_t rows_per_piece = (uint32_t)std::min<size_t>(std::max<size_t>(piece / 100, 1), 1u << 24);
    StageHandle stage;
    std::vector<char> host;
    for (uint32_t r0 = 0; r0 < n; r0 += rows_per_piece) {
      const MapLines src{d_out.p + (size_t)r0 * 9, std::min(rows_per_piece, n - r0)};
      TextPlan plan;
      plan_text(src, (const uint32_t *)nullptr, src.n, &plan, &ws);
      uint64_t total = 0;
      PGX_HIP(hipMemcpyAsync(&total, plan.poff.p + src.n, sizeof(total), hipMemcpyDeviceToHost, st));
      sync();
      DevBuf<char> d_text(total + 16);
      hipLaunchKernelGGL(k_piece_format<MapLines>, dim3(cdiv(total, TEXT_TILE)), dim3(TEXT_THREADS), 0, st, src, plan.poff.p, (uint64_t)0, total, d_text.p);
      PGX_HIP(hipGetLastError());
      host.resize(total);
      text_download(stage.ts, d_text.p, total, host.data());
      sync();
      PGX_REQUIRE(fwrite(host.data(), 1, total, out.f) == total, PGX_EIO, "%s: cannot write %s", who, out_path ? out_path : "stdout");
    }
    PGX_REQUIRE(fflush(out.f) == 0, PGX_EIO, "%s: cannot write %s", who, out_path ? out_path : "stdout");
    ms.format_ms = wall_ms() - t1;
    if (stats) *stats = ms;
  });
}

}  // extern "C"
