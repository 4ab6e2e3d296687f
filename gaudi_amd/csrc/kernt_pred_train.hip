// kernt_pred_train.hip -- the predictor's training kernels (pred_train.h): embedding, one GCL layer forward or reverse,
// the L1 readout seed, and the fixed-order weight-gradient reduction.  One workgroup (256 threads) per molecule for the
// network kernels; fp32 instructions throughout.  The pieces of a GCL it has in common with the EDM's kernels are
// train_device.h's; the reduction serves both passes.
#include "pred_train.h"

namespace gaudi_train {

__global__ void __launch_bounds__(kThreads) pt_embed_kernel(const PTBufs b) {
  __shared__ float lds[kRows * 256];
  const Mol m(b);
  const int N = m.N, F = b.F, F1 = F + 1, D = 3 + F, tid = threadIdx.x;
  const float* z = b.zt + (size_t)m.bg * N * D;
  float* hin = b.hin + (size_t)m.mb * N * F1;
  float* x = m.xstash(b, 0);
  for (int i = tid; i < N * F1; i += kThreads) {
    const int n = i / F1, k = i - n * F1;
    hin[i] = k < F ? z[n * D + 3 + k] * m.nm[n] : b.t[m.bg];  // h * node_mask | h_time (models.py:440-451)
  }
  for (int i = tid; i < N * 4; i += kThreads) {
    const int n = i / 4, k = i - n * 4;
    x[i] = k < 3 ? z[n * D + k] * m.nm[n] : 0.f;
  }
  __syncthreads();
  float* d0 = m.escal(b.d0);
  for (int e = tid; e < m.E; e += kThreads) {
    const int i = e / N, j = e - i * N;
    float r = 0.f;
    for (int k = 0; k < 3; ++k) {
      const float d = x[i * 4 + k] - x[j * 4 + k];
      r += d * d;
    }
    d0[e] = r;  // edge_attr (models.py:452)
  }
  mm_rows(b.wt + b.off[EMB_W], m.H, F1, m.H, hin, F1, N, m.hstash(b, 0), m.H, b.w + b.off[EMB_B], false, lds);
}

// The forward of GCL layer l (gcl.py:288-316) from the stash hs[l], xs[l], keeping every intermediate in the layer
// scratch; with `out`, also h_{l+1}, x_{l+1} into hs[l+1], xs[l+1].
__device__ void layer_forward(const PTBufs& b, const Mol& m, int l, bool out, float* lds) {
  const int N = m.N, E = m.E, H = m.H, tid = threadIdx.x;
  const int* o = b.off + NHEAD + NLAYER * l;
  const float* h = m.hstash(b, l);
  const float* x = m.xstash(b, l);
  float *P = m.node(b.P), *Q = m.node(b.Q);
  float *U = m.edge(b.U), *S = m.edge(b.Su), *V = m.edge(b.V), *M = m.edge(b.M), *EF = m.edge(b.EF), *CP = m.edge(b.CP),
        *C = m.edge(b.C);
  float *diff = m.escal(b.diff, 4), *rad = m.escal(b.rad), *phi = m.escal(b.phi), *ppre = m.escal(b.ppre);
  const float* d0 = m.escal(b.d0);
  const float* W1T = b.wt + o[E0W];  // [2H+2][H]
  // edge_mlp.0 over [h_i | h_j | radial | d0] = P_i + Q_j + c_r radial + c_d d0 (P carries the bias)
  mm_rows(W1T, H, H, H, h, H, N, P, H, b.w + o[E0B], false, lds);
  mm_rows(W1T + (size_t)H * H, H, H, H, h, H, N, Q, H, nullptr, false, lds);
  for (int e = tid; e < E; e += kThreads) {  // coord2radial (gcl.py:318-325)
    const int i = e / N, j = e - i * N;
    float r = 0.f;
    for (int k = 0; k < 3; ++k) {
      const float d = x[i * 4 + k] - x[j * 4 + k];
      diff[e * 4 + k] = d;
      r += d * d;
    }
    rad[e] = r;
    diff[e * 4 + 3] = sqrtf(r + 1e-8f);
  }
  __syncthreads();
  const float* cr = W1T + (size_t)2 * H * H;
  const float* cd = W1T + (size_t)(2 * H + 1) * H;
  for (int idx = tid; idx < E * H; idx += kThreads) {
    const int e = idx / H, k = idx - e * H, i = e / N, j = e - i * N;
    const float u = P[i * H + k] + Q[j * H + k] + cr[k] * rad[e] + cd[k] * d0[e];
    U[idx] = u;
    S[idx] = silu(u);
  }
  mm_rows(b.wt + o[E2W], H, H, H, S, H, E, V, H, b.w + o[E2B], false, lds);
  for (int idx = tid; idx < E * H; idx += kThreads) M[idx] = silu(V[idx]);
  __syncthreads();
  gate_edge_feat(b, m, o + AW);  // att_mlp (gcl.py:261-263)
  mm_rows(b.wt + o[C0W], H, H, H, EF, H, E, CP, H, b.w + o[C0B], false, lds);
  for (int idx = tid; idx < E * H; idx += kThreads) C[idx] = silu(CP[idx]);
  __syncthreads();
  for (int e = tid; e < E; e += kThreads) {  // coord_mlp.2 (+ tanh) (gcl.py:280-285)
    const float* wc2 = b.w + o[C2W];
    float p = 0.f;
    for (int k = 0; k < H; ++k) p = fmaf(wc2[k], C[e * H + k], p);
    ppre[e] = p;
    phi[e] = b.use_tanh ? tanhf(p) * b.coords_range_layer : p;
  }
  row_aggregate<false>(b, m, 1.f);  // unsorted_segment_sum over row (gcl.py:268-271): a plain sum
  if (out) {
    float* xo = m.xstash(b, l + 1);
    for (int i = tid; i < N; i += kThreads) {  // coord_model, 'sum' (gcl.py:276-300)
      float a[3] = {0.f, 0.f, 0.f};
      for (int j = 0; j < N; ++j) {
        const int e = i * N + j;
        const float s = phi[e] * m.em[e] / (diff[e * 4 + 3] + 1.f);
        for (int k = 0; k < 3; ++k) a[k] += diff[e * 4 + k] * s;
      }
      for (int k = 0; k < 3; ++k) xo[i * 4 + k] = (x[i * 4 + k] + a[k]) * m.nm[i];
      xo[i * 4 + 3] = 0.f;
    }
  }
  node_mlp_forward(b, m, h, o + N0W, out ? l + 1 : -1, lds);
}

// The reverse pass of GCL layer l: (dh_{l+1}, dx_{l+1}) in dh / dx become (dh_l, dx_l) in place, leaving the operands of
// every weight gradient of the layer in the scratch (pred_train_host.inc lists them).
__device__ void layer_reverse(const PTBufs& b, const Mol& m, int l, float* lds) {
  const int N = m.N, E = m.E, H = m.H, tid = threadIdx.x;
  const int* o = b.off + NHEAD + NLAYER * l;
  const bool coord = l < b.L - 1;  // the last layer's coordinate output never reaches h
  float *dx = m.dx(b), *dP = m.node(b.dP), *CP = m.edge(b.CP), *DE = m.edge(b.DE);
  float *diff = m.escal(b.diff, 4), *dcd = m.escal(b.dcd, 4), *phi = m.escal(b.phi), *ppre = m.escal(b.ppre),
        *dp = m.escal(b.dp);
  // h_out = (h + node_mlp([h | agg])) * nm ;  x_out = (x + sum_j trans_ij) * nm
  for (int idx = tid; idx < N * 4; idx += kThreads) dx[idx] = dx[idx] * m.nm[idx / 4];
  node_mlp_reverse(b, m, o + N0W, lds);
  // coordinate branch -> d phi -> d cpre (in CP), d edge_feat (DE)
  for (int e = tid; e < E; e += kThreads) {
    const int i = e / N;
    float g = 0.f, dt3[3] = {0.f, 0.f, 0.f};
    if (coord) {
      const float inv = 1.f / (diff[e * 4 + 3] + 1.f);
      for (int k = 0; k < 3; ++k) {
        const float dt = dx[i * 4 + k] * m.em[e];
        g += dt * diff[e * 4 + k] * inv;
        dt3[k] = dt * phi[e];
      }
      if (b.use_tanh) {
        const float th = tanhf(ppre[e]);
        g *= b.coords_range_layer * (1.f - th * th);
      }
    }
    dp[e] = g;
    for (int k = 0; k < 3; ++k) dcd[e * 4 + k] = dt3[k];
  }
  __syncthreads();
  if (coord) {
    const float* wc2 = b.w + o[C2W];
    for (int idx = tid; idx < E * H; idx += kThreads) {
      const int e = idx / H, k = idx - e * H;
      CP[idx] = dp[e] * wc2[k] * dsilu(CP[idx]);
    }
    mm_rows(b.w + o[C0W], H, H, H, CP, H, E, DE, H, nullptr, false, lds);  // DE = Wc1^T dc
  } else {
    for (int idx = tid; idx < E * H; idx += kThreads) DE[idx] = 0.f;
    __syncthreads();
  }
  for (int idx = tid; idx < E * H; idx += kThreads) {  // + dagg_i: edge_feat is summed into agg of its row
    const int e = idx / H, k = idx - e * H, i = e / N;
    DE[idx] += dP[i * H + k];
  }
  attention_reverse(b, m, o + AW);  // edge_feat = silu(v) * gate * em
  edge_mlp_reverse(b, m, o[E0W], o[E2W], true, lds, [&](int e, float dradial) {  // radial and coord_diff -> d diff
    const float w = diff[e * 4 + 3], inv = 1.f / (w + 1.f);
    float dot = 0.f;
    for (int k = 0; k < 3; ++k) dot += dcd[e * 4 + k] * diff[e * 4 + k];
    const float c = dot * inv * inv / w;
    for (int k = 0; k < 3; ++k)
      dcd[e * 4 + k] = dcd[e * 4 + k] * inv - diff[e * 4 + k] * c + 2.f * diff[e * 4 + k] * dradial;
  });
  scatter_dx(b, m);
}

__global__ void __launch_bounds__(kThreads) pt_layer_kernel(const PTBufs b, int l, int reverse) {
  __shared__ float lds[kRows * 256];
  const Mol m(b);
  layer_forward(b, m, l, !reverse, lds);
  if (reverse) layer_reverse(b, m, l, lds);
}

// L1 seed (torch.nn.functional.l1_loss, sign(0) = 0) through the readout  pred = mean_n (Wout h_n + bout) nm_n
__global__ void __launch_bounds__(kThreads) pt_readout_kernel(const PTBufs b) {
  __shared__ float lds[kRows * 256];
  const Mol m(b);
  const int N = m.N, K = b.K, tid = threadIdx.x;
  float* dho = b.dhout + (size_t)m.mb * N * K;
  for (int i = tid; i < N * K; i += kThreads) {
    const int n = i / K, k = i - n * K;
    const float d = b.pred[(size_t)m.bg * K + k] - b.y[(size_t)m.bg * K + k];
    const float s = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    dho[i] = s * b.dpred_scale * m.nm[n] / b.readout_div;
  }
  for (int i = tid; i < N * 4; i += kThreads) m.dx(b)[i] = 0.f;
  __syncthreads();
  mm_rows(b.w + b.off[OUT_W], m.H, K, m.H, dho, K, N, m.node(b.dh), m.H, nullptr, false, lds);
}

// G[m][k] += sum_r Y[r][m] X[r][k] over one 32 x 32 tile per workgroup on v_mfma_f32_16x16x4_f32 (A[m][r] = Y[r][m],
// B[r][k] = X[r][k]).  Split-K in a fixed order: wave w sums the w-th quarter of the rows (each MFMA is a k-ordered fp32
// fma chain), and the four partial tiles are added w = 0, 1, 2, 3 -- no atomics, the same bits on every call.
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(kThreads) pt_outer_kernel(const OuterJob* __restrict__ jobs, const int4* __restrict__ tiles) {
  __shared__ float part[4][32][33];
  const int4 tl = tiles[blockIdx.x];
  const OuterJob j = jobs[tl.x];
  const int m0 = tl.y, k0 = tl.z;
  const int w = threadIdx.x / 64, lane = threadIdx.x % 64, li = lane & 15, lk = lane >> 4;
  const int per = ((j.R + 15) / 16) * 4;  // rows per wave (a multiple of 4)
  const int rb = min(j.R, w * per), re = min(j.R, rb + per);
  const bool am0 = m0 + li < j.M, am1 = m0 + 16 + li < j.M, bk0 = k0 + li < j.Kc, bk1 = k0 + 16 + li < j.Kc;
  f32x4 c00 = {0.f, 0.f, 0.f, 0.f}, c01 = c00, c10 = c00, c11 = c00;
  for (int r = rb; r < re; r += 4) {
    const int row = r + lk;
    const bool rv = row < re;
    const float* yr = j.Y + (size_t)row * j.ldy + m0 + li;
    const float a0 = rv && am0 ? yr[0] : 0.f;
    const float a1 = rv && am1 ? yr[16] : 0.f;
    float b0 = 0.f, b1 = 0.f;
    if (rv) {
      if (j.X) {
        const float* xr = j.X + (size_t)row * j.ldx + k0 + li;
        b0 = bk0 ? xr[0] : 0.f;
        b1 = bk1 ? xr[16] : 0.f;
      } else {
        b0 = bk0 ? 1.f : 0.f;
      }
    }
    c00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, c00, 0, 0, 0);
    c01 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, c01, 0, 0, 0);
    c10 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, c10, 0, 0, 0);
    c11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, c11, 0, 0, 0);
  }
  for (int v = 0; v < 4; ++v) {  // C/D map: col = lane & 15, row = 4 (lane >> 4) + v
    const int i = 4 * lk + v;
    part[w][i][li] = c00[v];
    part[w][i][16 + li] = c01[v];
    part[w][16 + i][li] = c10[v];
    part[w][16 + i][16 + li] = c11[v];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 32 * 32; idx += kThreads) {
    const int mm = idx / 32, kk = idx % 32;
    if (m0 + mm < j.M && k0 + kk < j.Kc) {
      float s = part[0][mm][kk];
      s += part[1][mm][kk];
      s += part[2][mm][kk];
      s += part[3][mm][kk];
      float* g = &j.G[(size_t)(m0 + mm) * j.ldg + k0 + kk];
      *g += s;
    }
  }
}

}  // namespace gaudi_train

using namespace gaudi_train;

int gaudi_pt_embed(const PTBufs& b, int Bc, hipStream_t s) {
  hipLaunchKernelGGL(pt_embed_kernel, dim3(Bc), dim3(kThreads), 0, s, b);
  return (int)hipGetLastError();
}

int gaudi_pt_layer(const PTBufs& b, int Bc, int l, int reverse, hipStream_t s) {
  hipLaunchKernelGGL(pt_layer_kernel, dim3(Bc), dim3(kThreads), 0, s, b, l, reverse);
  return (int)hipGetLastError();
}

int gaudi_pt_readout(const PTBufs& b, int Bc, hipStream_t s) {
  hipLaunchKernelGGL(pt_readout_kernel, dim3(Bc), dim3(kThreads), 0, s, b);
  return (int)hipGetLastError();
}

int gaudi_pt_outer(const OuterJob* jobs, const int4* tiles, int n_tiles, hipStream_t s) {
  if (n_tiles <= 0) return 0;
  hipLaunchKernelGGL(pt_outer_kernel, dim3(n_tiles), dim3(kThreads), 0, s, jobs, tiles);
  return (int)hipGetLastError();
}
