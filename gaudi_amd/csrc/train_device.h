// train_device.h -- device helpers shared by the training kernels (kernt_pred_train.hip, kernt_edm_train.hip): the SiLU
// family and mm_rows, the fp32 row-block product over a torch-layout matrix.
#pragma once
#include <hip/hip_runtime.h>

namespace gaudi_train {

constexpr int kThreads = 256;
constexpr int kRows = 16;  // rows of X staged in LDS per round of mm_rows

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float silu(float x) { return x * sigm(x); }
__device__ __forceinline__ float dsilu(float x) {
  const float s = sigm(x);
  return s * (1.f + x * (1.f - s));
}

// Y[r][o] (+)= sum_k WT[k*ldw + o] X[r][k] (+ bias[o]),  r < R, o < Out <= 256, k < Kin <= 256.  Every thread calls it.
// Forward products pass a transposed matrix (WT[k][o] = W[o][k]); reverse products (W^T d) pass W itself with the
// roles of o and k swapped.
__device__ inline void mm_rows(const float* __restrict__ WT, int ldw, int Kin, int Out, const float* X, int ldx, int R, float* Y,
                        int ldy, const float* __restrict__ bias, bool acc, float* lds) {
  const int tid = threadIdx.x;
  for (int r0 = 0; r0 < R; r0 += kRows) {
    const int nr = min(kRows, R - r0);
    __syncthreads();
    for (int i = tid; i < kRows * Kin; i += kThreads) {
      const int r = i / Kin, k = i - r * Kin;
      lds[i] = r < nr ? X[(size_t)(r0 + r) * ldx + k] : 0.f;
    }
    __syncthreads();
    if (tid < Out) {
      float a[kRows];
#pragma unroll
      for (int r = 0; r < kRows; ++r) a[r] = 0.f;
      for (int k = 0; k < Kin; ++k) {
        const float w = WT[(size_t)k * ldw + tid];
#pragma unroll
        for (int r = 0; r < kRows; ++r) a[r] = fmaf(w, lds[r * Kin + k], a[r]);
      }
      const float bv = bias ? bias[tid] : 0.f;
      for (int r = 0; r < nr; ++r) {
        float* y = &Y[(size_t)(r0 + r) * ldy + tid];
        *y = acc ? *y + a[r] : a[r] + bv;
      }
    }
  }
  __syncthreads();
}

}  // namespace gaudi_train
