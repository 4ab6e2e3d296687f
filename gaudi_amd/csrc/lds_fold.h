// lds_fold.h -- ordered sums over the rows of a run with the loads batched: the rows of a batch are fetched first (independent
// reads, one latency), then folded in slot order.  The 4-wave family learned this for its segmented sums (device_common.h: SegSum,
// GAUDI_SEG_BATCH); this is the same lesson for the per-node sums of the 8-wave kernels, whose runs have run-time lengths -- hipcc
// cannot hoist a load out of such a loop, so each iteration was one LDS round trip (two where the row comes from an index list).
//
// The arithmetic is the plain loop's: a left fold from the caller's initial value, one addition (subtraction) per slot of the run
// in slot order.  A slot beyond the run is skipped by a select -- nothing is added for it, not even a zero -- and its load reads
// row 0 of the table (entry 0 of the index list), which every caller's table has: no branch goes around a load.
//
// Depends on nothing of the project, so the host side compiles alone (tests/test_lds_batch_cpu.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GAUDI_FOLD_HD __host__ __device__ __forceinline__
#else
#define GAUDI_FOLD_HD inline
#endif

namespace gaudi {

// B rows (values of type V: float or a float4 vector) of one batch of a run.  The run's slots are k = 0 .. n-1; the batch holds
// k0 .. k0 + B - 1.
template <int B, class V>
struct FoldBatch {
  V v[B];
  // table rows of the batch's slots -- a run of consecutive rows first, first + 1, ...
  GAUDI_FOLD_HD static void rows_of_run(int (&r)[B], int first, int k0, int n) {
#pragma unroll
    for (int k = 0; k < B; ++k) r[k] = k0 + k < n ? first + k0 + k : 0;
  }
  // ... or the rows idx[first], idx[first + 1], ...: the indices of a batch are fetched together, ahead of the rows they address
  GAUDI_FOLD_HD static void rows_of_list(int (&r)[B], const uint16_t* idx, int first, int k0, int n) {
#pragma unroll
    for (int k = 0; k < B; ++k) r[k] = (int)idx[k0 + k < n ? first + k0 + k : 0];
  }
  // row r of the table = the V at base + r * stride (floats)
  GAUDI_FOLD_HD void load(const float* base, int stride, const int (&r)[B]) {
#pragma unroll
    for (int k = 0; k < B; ++k) v[k] = *(const V*)(base + r[k] * stride);
  }
  GAUDI_FOLD_HD V add(V s, int k0, int n) const {
#pragma unroll
    for (int k = 0; k < B; ++k) s = k0 + k < n ? s + v[k] : s;
    return s;
  }
  GAUDI_FOLD_HD V sub(V s, int k0, int n) const {
#pragma unroll
    for (int k = 0; k < B; ++k) s = k0 + k < n ? s - v[k] : s;
    return s;
  }
};

// s (+|-)= row first, first + 1, ... first + n - 1, in that order
template <int B, class V, bool SUB = false>
GAUDI_FOLD_HD V fold_run(V s, const float* base, int stride, int first, int n) {
  for (int k0 = 0; k0 < n; k0 += B) {
    FoldBatch<B, V> b;
    int r[B];
    b.rows_of_run(r, first, k0, n);
    b.load(base, stride, r);
    s = SUB ? b.sub(s, k0, n) : b.add(s, k0, n);
  }
  return s;
}
// s (+|-)= row idx[first], idx[first + 1], ... idx[first + n - 1], in that order
template <int B, class V, bool SUB = false>
GAUDI_FOLD_HD V fold_list(V s, const float* base, int stride, const uint16_t* idx, int first, int n) {
  for (int k0 = 0; k0 < n; k0 += B) {
    FoldBatch<B, V> b;
    int r[B];
    b.rows_of_list(r, idx, first, k0, n);
    b.load(base, stride, r);
    s = SUB ? b.sub(s, k0, n) : b.add(s, k0, n);
  }
  return s;
}

}  // namespace gaudi
