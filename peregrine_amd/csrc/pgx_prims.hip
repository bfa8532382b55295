// pgx_prims.hip -- the device-wide sorts, scans, selects and reductions of libpgx.so: the one file that includes hipcub and so the one
// place where rocPRIM's kernels are instantiated (prototypes and their contract: pgx_internal.h, "device-wide primitives").
//
// Every function is hipcub's two-call idiom once: size query with a null workspace, a workspace, the run; those that answer a number
// copy it back and synchronise the stream.  n == 0 is settled here, before any of that.  The iterator and pointer types handed to
// hipcub are the ones the call sites had when each wrote the idiom out itself (mutable input pointers, the type of the slot the
// number of selected items lands in ...): they name the rocPRIM instantiation, and with it the tuned configuration that runs.
#include <hipcub/hipcub.hpp>

#include <climits>

#include "pgx_internal.h"

namespace pgx {
// The flags of the reads (uint32 per read; non-zero: the read is unfinished, the bits say why) as hipcub select flags
struct FlaggedFor {
  uint32_t skip_bits;
  __host__ __device__ bool operator()(uint32_t f) const { return f != 0 && !(f & skip_bits); }
};
namespace {
// hipcub's idiom for n > 0 items: call(workspace, bytes, n as hipcub takes it) is the hipcub function with everything else bound
template <class Call>
void run(const char *what, size_t n, PrimWs *tmp, Call &&call) {
  if (n == 0) return;
  PGX_REQUIRE(n <= (size_t)INT_MAX, PGX_EARG, "too many records for one call");
  PrimWs own;
  size_t bytes = 0;
  hipError_t e = call(nullptr, bytes, (int)n);
  if (e == hipSuccess) e = call((tmp ? *tmp : own).get(bytes), bytes, (int)n);
  if (e != hipSuccess) {
    set_error("%s failed: %s", what, hipGetErrorString(e));
    throw Fail{PGX_EHIP};
  }
}
template <typename T>
T number_back(const T *d_num, hipStream_t st) {
  T num = 0;
  PGX_HIP(hipMemcpyAsync(&num, d_num, sizeof(T), hipMemcpyDeviceToHost, st));
  PGX_HIP(hipStreamSynchronize(st));
  return num;
}
// ... for the primitives that leave a number of type T on the device (call's fourth argument: where), which is the answer
template <typename T, class Call>
T counted(const char *what, size_t n, PrimWs *tmp, hipStream_t st, Call &&call) {
  if (n == 0) return 0;
  DevBuf<T> d_num(1);
  run(what, n, tmp, [&](void *work, size_t &bytes, int ni) { return call(work, bytes, ni, d_num.p); });
  return number_back(d_num.p, st);
}
template <typename T>
T *as_mutable(const T *p) { return const_cast<T *>(p); }   // (read only all the same: see the head of the file)

using Iota32 = hipcub::CountingInputIterator<uint32_t, ptrdiff_t>;
using Iota64 = hipcub::CountingInputIterator<uint64_t, ptrdiff_t>;
struct MaxOp {
  __host__ __device__ int32_t operator()(int32_t a, int32_t b) const { return a > b ? a : b; }
};

template <typename K>
void sort_pairs_of(const K *k_in, K *k_out, const uint32_t *v_in, uint32_t *v_out, size_t n, int begin_bit, int end_bit, PrimWs *tmp, hipStream_t st) {
  run("radix sort of pairs", n, tmp, [&](void *work, size_t &bytes, int ni) {
    return hipcub::DeviceRadixSort::SortPairs(work, bytes, k_in, k_out, v_in, v_out, ni, begin_bit, end_bit, st);
  });
}
__global__ void k_prim_iota(uint32_t *__restrict__ d, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d[i] = i;
}
__global__ void k_prim_gather(const uint64_t *__restrict__ key, const uint32_t *__restrict__ idx, uint32_t n, uint64_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = key[idx[i]];
}
template <typename FlagIt>
uint32_t select_indices_of(FlagIt flags, size_t n, uint32_t *d_list, PrimWs *tmp, hipStream_t st) {
  return counted<uint32_t>("select", n, tmp, st, [&](void *work, size_t &bytes, int ni, uint32_t *d_num) {
    return hipcub::DeviceSelect::Flagged(work, bytes, Iota32(0), flags, d_list, d_num, ni, st);
  });
}
template <typename In, typename O>
void scan_offsets_of(In d_vals, O *d_offs, size_t n, PrimWs *tmp, hipStream_t st) {
  PGX_HIP(hipMemsetAsync(d_offs, 0, sizeof(O), st));
  run("inclusive sum", n, tmp, [&](void *work, size_t &bytes, int ni) { return hipcub::DeviceScan::InclusiveSum(work, bytes, d_vals, d_offs + 1, ni, st); });
}
template <typename In, typename O>
O scan_to_total_of(In d_vals, O *d_offs, size_t n, PrimWs *tmp, hipStream_t st) {
  scan_offsets_of(d_vals, d_offs, n, tmp, st);
  return n ? number_back(d_offs + n, st) : 0;
}
template <typename In, typename Out>
void exclusive_sum_of(In d_in, Out *d_out, size_t n, PrimWs *tmp, hipStream_t st) {
  run("exclusive sum", n, tmp, [&](void *work, size_t &bytes, int ni) { return hipcub::DeviceScan::ExclusiveSum(work, bytes, d_in, d_out, ni, st); });
}
template <typename In, typename Out, typename Op>
void running_max_of(In d_in, Out *d_out, Op op, size_t n, PrimWs *tmp, hipStream_t st) {
  run("running maximum", n, tmp, [&](void *work, size_t &bytes, int ni) { return hipcub::DeviceScan::InclusiveScan(work, bytes, d_in, d_out, op, ni, st); });
}
}  // namespace

#define TAIL PrimWs *tmp, hipStream_t st
// ---- sorts ---------------------------------------------------------------------------------------------------------------------------------
void sort_pairs(const uint64_t *k_in, uint64_t *k_out, const uint32_t *v_in, uint32_t *v_out, size_t n, int begin_bit, int end_bit, TAIL) {
  sort_pairs_of(k_in, k_out, v_in, v_out, n, begin_bit, end_bit, tmp, st);
}
void sort_pairs(const uint32_t *k_in, uint32_t *k_out, const uint32_t *v_in, uint32_t *v_out, size_t n, int begin_bit, int end_bit, TAIL) {
  sort_pairs_of(k_in, k_out, v_in, v_out, n, begin_bit, end_bit, tmp, st);
}
void sort_pairs(const uint8_t *k_in, uint8_t *k_out, const uint32_t *v_in, uint32_t *v_out, size_t n, int begin_bit, int end_bit, TAIL) {
  sort_pairs_of(k_in, k_out, v_in, v_out, n, begin_bit, end_bit, tmp, st);
}
void sort_keys(const uint64_t *k_in, uint64_t *k_out, size_t n, int begin_bit, int end_bit, TAIL) {
  run("radix sort of keys", n, tmp,
      [&](void *work, size_t &bytes, int ni) { return hipcub::DeviceRadixSort::SortKeys(work, bytes, k_in, k_out, ni, begin_bit, end_bit, st); });
}
void iota(uint32_t *d, size_t n, TAIL) {
  if (n == 0) return;
  PGX_REQUIRE(n <= (size_t)INT_MAX, PGX_EARG, "too many records for one call");
  LAUNCH(k_prim_iota, n, d, (uint32_t)n);
  PGX_HIP(hipGetLastError());
}
void gather(const uint64_t *key, const uint32_t *idx, size_t n, uint64_t *out, TAIL) {
  if (n == 0) return;
  PGX_REQUIRE(n <= (size_t)INT_MAX, PGX_EARG, "too many records for one call");
  LAUNCH(k_prim_gather, n, key, idx, (uint32_t)n, out);
  PGX_HIP(hipGetLastError());
}
void sort_order(std::initializer_list<SortKey> keys, size_t n, const uint32_t *order_in, uint32_t *order_out, uint64_t *first_out, PrimWs *tmp) {
  const int n_keys = (int)keys.size();
  if (n == 0 || n_keys == 0) return;
  hipStream_t st = ctx().stream;
  DevBuf<uint32_t> other;      // the orders alternate between this and order_out, the last lands in order_out
  DevBuf<uint64_t> col, junk;  // a key behind the order so far; the sorted keys nobody reads
  if (n_keys > 1 || !order_in) other.alloc(n);
  if (n_keys > 1 || order_in) col.alloc(n);
  if (n_keys > 2 || (n_keys > 1 && order_in)) junk.alloc(n);
  const uint32_t *cur = order_in;
  if (!cur) {
    uint32_t *first = n_keys & 1 ? other.p : order_out;
    iota(first, n, tmp, st);
    cur = first;
  }
  for (int k = n_keys - 1; k >= 0; --k) {
    const uint64_t *k_in = keys.begin()[k].key;
    if (order_in || k < n_keys - 1) gather(k_in, cur, n, col.p, tmp, st), k_in = col.p;
    uint32_t *next = k & 1 ? other.p : order_out;
    uint64_t *k_out = k == 0 ? first_out : k_in == col.p ? junk.p : col.p;
    sort_pairs(k_in, k_out, cur, next, n, 0, keys.begin()[k].bits, tmp, st);
    cur = next;
  }
}

// ---- selects -------------------------------------------------------------------------------------------------------------------------------
uint32_t select_indices(const uint8_t *d_flags, size_t n, uint32_t *d_list, TAIL) { return select_indices_of(as_mutable(d_flags), n, d_list, tmp, st); }
uint32_t select_indices(const uint32_t *d_flags, size_t n, uint32_t *d_list, TAIL) { return select_indices_of(as_mutable(d_flags), n, d_list, tmp, st); }
void select_indices_dev(const uint8_t *d_flags, size_t n, uint32_t *d_list, uint32_t *d_num, TAIL) {
  if (n == 0) PGX_HIP(hipMemsetAsync(d_num, 0, sizeof(uint32_t), st));
  run("select", n, tmp, [&](void *work, size_t &bytes, int ni) {
    return hipcub::DeviceSelect::Flagged(work, bytes, Iota32(0), as_mutable(d_flags), d_list, d_num, ni, st);
  });
}
uint64_t select_indices(const uint8_t *d_flags, size_t n, uint64_t *d_list, TAIL) {
  return counted<uint64_t>("select", n, tmp, st, [&](void *work, size_t &bytes, int ni, uint64_t *d_num) {
    return hipcub::DeviceSelect::Flagged(work, bytes, Iota64(0), as_mutable(d_flags), d_list, d_num, ni, st);
  });
}
uint32_t select_flagged(const uint32_t *d_flags, size_t n, uint32_t *d_list, uint32_t skip_bits, TAIL) {
  return select_indices_of(hipcub::TransformInputIterator<bool, FlaggedFor, const uint32_t *>(d_flags, FlaggedFor{skip_bits}), n, d_list, tmp, st);
}
uint64_t select_values(const pgx_mm128 *d_in, const uint8_t *d_flags, size_t n, pgx_mm128 *d_out, TAIL) {
  return counted<uint64_t>("select", n, tmp, st, [&](void *work, size_t &bytes, int ni, uint64_t *d_num) {
    return hipcub::DeviceSelect::Flagged(work, bytes, as_mutable(d_in), as_mutable(d_flags), d_out, d_num, ni, st);
  });
}

// ---- sums and running maxima ---------------------------------------------------------------------------------------------------------------
void exclusive_sum(const uint32_t *d_in, uint32_t *d_out, size_t n, TAIL) { exclusive_sum_of(as_mutable(d_in), d_out, n, tmp, st); }
void exclusive_sum(const uint64_t *d_in, uint64_t *d_out, size_t n, TAIL) { exclusive_sum_of(as_mutable(d_in), d_out, n, tmp, st); }
void scan_offsets(const uint32_t *d_vals, uint32_t *d_offs, size_t n, TAIL) { scan_offsets_of(as_mutable(d_vals), d_offs, n, tmp, st); }
uint32_t scan_to_total(const uint32_t *d_vals, uint32_t *d_offs, size_t n, TAIL) { return scan_to_total_of(as_mutable(d_vals), d_offs, n, tmp, st); }
uint64_t scan_to_total(const uint32_t *d_vals, uint64_t *d_offs, size_t n, TAIL) { return scan_to_total_of(d_vals, d_offs, n, tmp, st); }
uint64_t scan_to_total(const uint64_t *d_vals, uint64_t *d_offs, size_t n, TAIL) { return scan_to_total_of(d_vals, d_offs, n, tmp, st); }
void running_max(const int32_t *d_in, int32_t *d_out, size_t n, TAIL) { running_max_of(as_mutable(d_in), d_out, MaxOp(), n, tmp, st); }
void running_max(const uint64_t *d_in, uint64_t *d_out, size_t n, TAIL) { running_max_of(d_in, d_out, hipcub::Max(), n, tmp, st); }

// ---- reductions ----------------------------------------------------------------------------------------------------------------------------
void reduce_sum(const uint32_t *d_in, uint32_t *d_out, size_t n, TAIL) {
  if (n == 0) PGX_HIP(hipMemsetAsync(d_out, 0, sizeof(uint32_t), st));
  run("sum", n, tmp, [&](void *work, size_t &bytes, int ni) { return hipcub::DeviceReduce::Sum(work, bytes, as_mutable(d_in), d_out, ni, st); });
}
void reduce_max(const uint32_t *d_in, uint32_t *d_out, size_t n, TAIL) {
  if (n == 0) PGX_HIP(hipMemsetAsync(d_out, 0, sizeof(uint32_t), st));
  run("maximum", n, tmp, [&](void *work, size_t &bytes, int ni) { return hipcub::DeviceReduce::Max(work, bytes, as_mutable(d_in), d_out, ni, st); });
}
uint32_t sum_by_key(const uint64_t *d_keys, uint64_t *d_uniq, const uint32_t *d_vals, uint32_t *d_sums, size_t n, TAIL) {
  return counted<uint32_t>("reduce by key", n, tmp, st, [&](void *work, size_t &bytes, int ni, uint32_t *d_num) {
    return hipcub::DeviceReduce::ReduceByKey(work, bytes, as_mutable(d_keys), d_uniq, as_mutable(d_vals), d_sums, d_num, hipcub::Sum(), ni, st);
  });
}
uint64_t run_lengths(const uint64_t *d_in, uint64_t *d_uniq, uint32_t *d_counts, size_t n, TAIL) {
  return counted<uint64_t>("run-length encode", n, tmp, st, [&](void *work, size_t &bytes, int ni, uint64_t *d_num) {
    return hipcub::DeviceRunLengthEncode::Encode(work, bytes, as_mutable(d_in), d_uniq, d_counts, d_num, ni, st);
  });
}
#undef TAIL

}  // namespace pgx
