// kernt_edm_train.hip -- the EDM's training kernels (edm_train.h): forward noising and embedding, one block forward, the
// loss readout and its seed, and the reverse passes of gcl_equiv and of one GCL sub-layer.  One workgroup (256 threads) per
// molecule; fp32 instructions throughout.  The pieces of a GCL it has in common with the
// predictor's kernels are train_device.h's; the weight-gradient reduction is gaudi_pt_outer (kernt_pred_train.hip).
#include "edm_train.h"
#include "edm_device.h"

namespace gaudi_etrain {

using namespace gaudi_train;

// stash: h at sub-layer s (s = S: the input of gcl_equiv) of block l; x at the input of block l is m.xstash(b, l)
__device__ inline float* hst(const ETBufs& b, const Mol& m, int l, int s) { return m.hstash(b, l * (b.S + 1) + s); }

// a sum over the nodes of one molecule in node order (thread 0), broadcast through LDS
__device__ float node_sum(const float* v, int N, float* cell) {
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int n = 0; n < N; ++n) s += v[n];
    *cell = s;
  }
  __syncthreads();
  const float r = *cell;
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(kThreads) et_embed_kernel(const ETBufs b) {
  __shared__ float lds[kRows * 256];
  __shared__ float mean[4];
  const Mol m(b);
  const int N = m.N, F = b.F, F1 = F + 1, D = 3 + F, A2 = b.A / 2, tid = threadIdx.x;
  float* eps = b.eps + (size_t)m.mb * N * D;
  float* hin = b.hin + (size_t)m.mb * N * F1;
  float* x = m.xstash(b, 0);
  // sample_combined_position_feature_noise (en_diffusion.py:937-956): raw draw 0, masked, x part mean-removed
  for (int i = tid; i < N * D; i += kThreads) {
    float raw;
    if (b.noise) {
      raw = b.noise[(size_t)m.bg * N * D + i];
    } else {
      const gaudi::f4 v = gaudi::philox_normal4(b.seed, (uint64_t)(b.sample_offset + m.bg), 0u, (uint32_t)(i >> 2));
      raw = v[i & 3];
    }
    eps[i] = raw * m.nm[i / D];
  }
  __syncthreads();
  if (tid < 3) {
    float s = 0.f, cnt = 0.f;
    for (int n = 0; n < N; ++n) {
      s += eps[n * D + tid];
      cnt += m.nm[n];
    }
    mean[tid] = s / fmaxf(cnt, 1.0f);
  }
  __syncthreads();
  for (int i = tid; i < N * 3; i += kThreads) {
    const int n = i / 3, d = i - n * 3;
    eps[n * D + d] = eps[n * D + d] - mean[d] * m.nm[n];
  }
  __syncthreads();
  // z_t = alpha_t * normalize([x | h]) + sigma_t * eps (:384-392, 676-684), then the dynamics' masking (models.py:88-96)
  const float a_t = b.as[2 * m.bg], s_t = b.as[2 * m.bg + 1];
  for (int i = tid; i < N * D; i += kThreads) {
    const int n = i / D, d = i - n * D;
    const float xh = d < 3 ? b.x[((size_t)m.bg * N + n) * 3 + d] / b.nv0
                           : (b.oh[((size_t)m.bg * N + n) * F + d - 3] - 0.0f) / b.nv1 * m.nm[n];
    const float z = (a_t * xh + s_t * eps[i]) * m.nm[n];
    if (d < 3) x[n * 4 + d] = z;
    else hin[n * F1 + d - 3] = z;
  }
  for (int n = tid; n < N; n += kThreads) {
    hin[n * F1 + F] = b.t[m.bg];  // h_time (models.py:98-106)
    x[n * 4 + 3] = 0.f;
  }
  __syncthreads();
  float* d0a = m.escal(b.d0a, A2);
  for (int e = tid; e < m.E; e += kThreads) {  // EGNN.forward: distances of the input x (egnn_new.py:298-301)
    const int i = e / N, j = e - i * N;
    float r = 0.f;
    for (int k = 0; k < 3; ++k) {
      const float d = x[i * 4 + k] - x[j * 4 + k];
      r += d * d;
    }
    if (b.sin) gaudi::sin_features(r, d0a + (size_t)e * A2);
    else d0a[e] = r;
  }
  mm_rows(b.wt + b.off[EMB_W], m.H, F1, m.H, hin, F1, N, hst(b, m, 0, 0), m.H, b.w + b.off[EMB_B], false, lds);
}

// coord2diff (egnn_new.py:394-400) of the block input x -> diff [E][4] (coord_diff, norm), radial, and the edge attributes
// [radial | d0] or their sinusoids (egnn_new.py:214-218)
__device__ void block_geo(const ETBufs& b, const Mol& m, int l) {
  const int N = m.N, A = b.A, A2 = A / 2, tid = threadIdx.x;
  const float* x = m.xstash(b, l);
  float *diff = m.escal(b.diff, 4), *rad = m.escal(b.rad), *ea = m.escal(b.ea, A);
  const float* d0a = m.escal(b.d0a, A2);
  for (int e = tid; e < m.E; e += kThreads) {
    const int i = e / N, j = e - i * N;
    float d[3], r = 0.f;
    for (int k = 0; k < 3; ++k) {
      d[k] = x[i * 4 + k] - x[j * 4 + k];
      r += d[k] * d[k];
    }
    const float norm = sqrtf(r + 1e-8f);
    for (int k = 0; k < 3; ++k) diff[e * 4 + k] = d[k] / (norm + b.norm_constant);
    diff[e * 4 + 3] = norm;
    rad[e] = r;
    float* o = ea + (size_t)e * A;
    if (b.sin) gaudi::sin_features(r, o);
    else o[0] = r;
    for (int k = 0; k < A2; ++k) o[A2 + k] = d0a[(size_t)e * A2 + k];
  }
  __syncthreads();
}

// the first two layers of an edge MLP over [h_i | h_j | edge_attr] (Linear(2H + A, H), SiLU, Linear(H, H), SiLU):
// P = A h + b1, Q = B h, U = P_i + Q_j + C ea, S = silu(U), V = W2 S + b2, M = silu(V)
__device__ void edge_mlp(const ETBufs& b, const Mol& m, const float* h, int w1, int b1, int w2, int b2, float* lds) {
  const int N = m.N, E = m.E, H = m.H, A = b.A, tid = threadIdx.x;
  float *P = m.node(b.P), *Q = m.node(b.Q), *U = m.edge(b.U), *S = m.edge(b.Su), *V = m.edge(b.V), *M = m.edge(b.M);
  const float* ea = m.escal(b.ea, A);
  const float* W1T = b.wt + w1;  // [2H + A][H]
  mm_rows(W1T, H, H, H, h, H, N, P, H, b.w + b1, false, lds);
  mm_rows(W1T + (size_t)H * H, H, H, H, h, H, N, Q, H, nullptr, false, lds);
  const float* C = W1T + (size_t)2 * H * H;
  for (int idx = tid; idx < E * H; idx += kThreads) {
    const int e = idx / H, k = idx - e * H, i = e / N, j = e - i * N;
    float u = P[i * H + k] + Q[j * H + k];
    for (int a = 0; a < A; ++a) u = fmaf(C[(size_t)a * H + k], ea[(size_t)e * A + a], u);
    U[idx] = u;
    S[idx] = silu(u);
  }
  mm_rows(b.wt + w2, H, H, H, S, H, E, V, H, b.w + b2, false, lds);
  for (int idx = tid; idx < E * H; idx += kThreads) M[idx] = silu(V[idx]);
  __syncthreads();
}

// GCL sub-layer s of block l (egnn_new.py:6-93) from the stash; with `out`, its output h into the stash
__device__ void gcl_forward(const ETBufs& b, const Mol& m, int l, int s, bool out, float* lds) {
  const float* h = hst(b, m, l, s);
  const int* o = b.off + gcl_slot(b.S, l, s, 0);
  edge_mlp(b, m, h, o[E0W], o[E0B], o[E2W], o[E2B], lds);
  gate_edge_feat(b, m, o + AW);  // att_mlp (egnn_new.py:50-52)
  __syncthreads();
  row_aggregate<true>(b, m, b.agg_div);  // unsorted_segment_sum over row (egnn_new.py:403-420)
  node_mlp_forward(b, m, h, o + N0W, out ? l * (b.S + 1) + s + 1 : -1, lds);
}

// gcl_equiv of block l (egnn_new.py:96-168); with `out`, x of block l + 1 and the block's output h = h * node_mask
__device__ void equiv_forward(const ETBufs& b, const Mol& m, int l, bool out, float* lds) {
  const int N = m.N, E = m.E, H = m.H, S = b.S, tid = threadIdx.x;
  const float* h = hst(b, m, l, S);
  float *M = m.edge(b.M), *diff = m.escal(b.diff, 4), *phi = m.escal(b.phi), *ppre = m.escal(b.ppre);
  const int o = equiv_slot(S, l, 0);
  edge_mlp(b, m, h, b.off[o + C0W], b.off[o + C0B], b.off[o + C2W], b.off[o + C2B], lds);
  const float* w4 = b.w + b.off[o + C4W];
  for (int e = tid; e < E; e += kThreads) {
    float p = 0.f;
    for (int k = 0; k < H; ++k) p = fmaf(w4[k], M[e * H + k], p);
    ppre[e] = p;
    phi[e] = b.use_tanh ? tanhf(p) * b.coords_range : p;
  }
  __syncthreads();
  if (out) {
    const float* x = m.xstash(b, l);
    float* xo = m.xstash(b, l + 1);
    for (int i = tid; i < N; i += kThreads) {
      float a[3] = {0.f, 0.f, 0.f};
      for (int j = 0; j < N; ++j) {
        const int e = i * N + j;
        for (int k = 0; k < 3; ++k) a[k] += diff[e * 4 + k] * phi[e] * m.em[e];
      }
      for (int k = 0; k < 3; ++k) xo[i * 4 + k] = (x[i * 4 + k] + a[k] / b.agg_div) * m.nm[i];
      xo[i * 4 + 3] = 0.f;
    }
    float* hn = hst(b, m, l + 1, 0);
    for (int idx = tid; idx < N * H; idx += kThreads) hn[idx] = h[idx] * m.nm[idx / H];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kThreads) et_block_kernel(const ETBufs b, int l) {
  __shared__ float lds[kRows * 256];
  const Mol m(b);
  block_geo(b, m, l);
  for (int s = 0; s < b.S; ++s) gcl_forward(b, m, l, s, true, lds);
  equiv_forward(b, m, l, true, lds);
}

// the reverse of an edge MLP's first two layers (train_device.h: edge_mlp_reverse); the radial column's C^T dU adds to drad,
// except with sin_embedding, which detaches the distance features (egnn_new.py:391)
__device__ void edge_reverse(const ETBufs& b, const Mol& m, int w1, int w2, float* lds) {
  float* drad = m.escal(b.drad);
  edge_mlp_reverse(b, m, w1, w2, !b.sin, lds, [&](int e, float g) { drad[e] += g; });
}

// gcl_equiv of block l, reverse: d (h_out, x_out) in (dh, dx) -> d h at its input in dh, d x through the residual in dx,
// and the block's d coord_diff / d radial (set here: gcl_equiv is the first of the block to run in reverse)
__global__ void __launch_bounds__(kThreads) et_equiv_rev_kernel(const ETBufs b, int l) {
  __shared__ float lds[kRows * 256];
  const Mol m(b);
  const int N = m.N, E = m.E, H = m.H, S = b.S, tid = threadIdx.x;
  block_geo(b, m, l);
  equiv_forward(b, m, l, false, lds);
  const int o = equiv_slot(S, l, 0);
  float *dh = m.node(b.dh), *dx = m.dx(b), *V = m.edge(b.V);
  float *diff = m.escal(b.diff, 4), *dcd = m.escal(b.dcd, 4), *phi = m.escal(b.phi), *ppre = m.escal(b.ppre),
        *dp = m.escal(b.dp), *drad = m.escal(b.drad);
  for (int idx = tid; idx < N * H; idx += kThreads) dh[idx] *= m.nm[idx / H];  // h_out = h * node_mask
  for (int idx = tid; idx < N * 4; idx += kThreads) dx[idx] *= m.nm[idx / 4];  // x_out = (x + agg) * node_mask
  __syncthreads();
  for (int e = tid; e < E; e += kThreads) {
    const int i = e / N;
    float g = 0.f;
    for (int k = 0; k < 3; ++k) {
      const float dt = dx[i * 4 + k] / b.agg_div * m.em[e];  // d trans
      g += dt * diff[e * 4 + k];
      dcd[e * 4 + k] = dt * phi[e];
    }
    dcd[e * 4 + 3] = 0.f;
    if (b.use_tanh) {
      const float th = tanhf(ppre[e]);
      g *= b.coords_range * (1.f - th * th);
    }
    dp[e] = g;
    drad[e] = 0.f;
  }
  __syncthreads();
  const float* w4 = b.w + b.off[o + C4W];
  for (int idx = tid; idx < E * H; idx += kThreads) {
    const int e = idx / H, k = idx - e * H;
    V[idx] = dp[e] * w4[k] * dsilu(V[idx]);  // V: dV
  }
  __syncthreads();
  edge_reverse(b, m, b.off[o + C0W], b.off[o + C2W], lds);
}

// GCL sub-layer s of block l, reverse: d h_out in dh -> d h_in in dh; after sub-layer 0 the block's d coord_diff and
// d radial become d x of the block input (coord2diff, egnn_new.py:394-400)
__global__ void __launch_bounds__(kThreads) et_gcl_rev_kernel(const ETBufs b, int l, int s) {
  __shared__ float lds[kRows * 256];
  const Mol m(b);
  const int N = m.N, E = m.E, H = m.H, tid = threadIdx.x;
  block_geo(b, m, l);
  gcl_forward(b, m, l, s, false, lds);
  const int* o = b.off + gcl_slot(b.S, l, s, 0);
  float *dP = m.node(b.dP), *DE = m.edge(b.DE);
  node_mlp_reverse(b, m, o + N0W, lds);
  for (int idx = tid; idx < E * H; idx += kThreads) {
    const int e = idx / H, k = idx - e * H, i = e / N;
    DE[idx] = dP[i * H + k] / b.agg_div;  // d edge_feat
  }
  attention_reverse(b, m, o + AW);
  __syncthreads();
  edge_reverse(b, m, o[E0W], o[E2W], lds);
  if (s > 0) return;
  // block input: x -> coord_diff = d / (|d| + norm_constant), radial = |d|^2
  const float* x = m.xstash(b, l);
  float *dcd = m.escal(b.dcd, 4), *drad = m.escal(b.drad);
  __syncthreads();
  for (int e = tid; e < E; e += kThreads) {
    const int i = e / N, j = e - i * N;
    float d[3], r = 0.f;
    for (int k = 0; k < 3; ++k) {
      d[k] = x[i * 4 + k] - x[j * 4 + k];
      r += d[k] * d[k];
    }
    const float norm = sqrtf(r + 1e-8f), den = norm + b.norm_constant;
    float dot = 0.f;
    for (int k = 0; k < 3; ++k) dot += dcd[e * 4 + k] * d[k];
    const float c = dot / (den * den * norm);
    for (int k = 0; k < 3; ++k) dcd[e * 4 + k] = dcd[e * 4 + k] / den - d[k] * c + 2.f * d[k] * drad[e];
  }
  __syncthreads();
  scatter_dx(b, m);
}

// net = [remove_mean_with_mask((x_L - x_0) nm) | (embedding_out(h_L) nm)[:, :F]] (models.py:108-152, egnn_new.py:306-312),
// the per-molecule sums of the loss (in the NLL kernel's order: per node over its columns, then over the nodes), and with
// `reverse` the seed dnet = coef (net - eps) back to d h_L (dh) and d x_L (dx)
__global__ void __launch_bounds__(kThreads) et_readout_kernel(const ETBufs b, int reverse) {
  __shared__ float lds[kRows * 256];
  __shared__ float red[3 * 256 + 8];
  const Mol m(b);
  const int N = m.N, F = b.F, F1 = F + 1, D = 3 + F, H = m.H, tid = threadIdx.x;
  const float* hf = hst(b, m, b.L, 0);
  const float *xf = m.xstash(b, b.L), *x0 = m.xstash(b, 0);
  const float* eps = b.eps + (size_t)m.mb * N * D;
  const float* hin = b.hin + (size_t)m.mb * N * F1;
  float* h3 = b.dhout + (size_t)m.mb * N * F1;
  float* net = b.net + (size_t)m.bg * N * D;
  mm_rows(b.wt + b.off[OUT_W], F1, H, F1, hf, H, N, h3, F1, b.w + b.off[OUT_B], false, lds);
  float* vn = red;  // [3][N]: masked velocity per column, then its sums
  for (int i = tid; i < N * 3; i += kThreads) {
    const int n = i / 3, d = i - n * 3;
    vn[d * N + n] = (xf[n * 4 + d] - x0[n * 4 + d]) * m.nm[n];
  }
  float cnt = node_sum(m.nm, N, &red[3 * 256]);
  cnt = fmaxf(cnt, 1.0f);
  float mean[3];
  for (int d = 0; d < 3; ++d) mean[d] = node_sum(vn + d * N, N, &red[3 * 256 + 1 + d]) / cnt;
  for (int i = tid; i < N * D; i += kThreads) {
    const int n = i / D, d = i - n * D;
    net[i] = d < 3 ? vn[d * N + n] - mean[d] * m.nm[n] : h3[n * F1 + d - 3] * m.nm[n];
  }
  __syncthreads();
  // per node: sum (eps - net)^2 over every column, over the x columns, and log p(h | z_0) of the true class (:600-642)
  float* part = red;
  for (int n = tid; n < N; n += kThreads) {
    float v0 = 0.f, vx = 0.f;
    for (int d = 0; d < D; ++d) {
      const float df = eps[n * D + d] - net[n * D + d];
      v0 += df * df;
      if (d == 2) vx = v0;
    }
    const float* zh = hin + n * F1;
    auto lp = [=](int k) {
      const float c = (zh[k] * b.nv1 + 0.0f) - 1.0f;
      const float hi = 0.5f * (1.0f + erff(((c + 0.5f) / b.sig_cat) / 1.41421356237309515f));
      const float lo = 0.5f * (1.0f + erff(((c - 0.5f) / b.sig_cat) / 1.41421356237309515f));
      return logf(hi - lo + 1e-10f);
    };
    float mx = -INFINITY;
    for (int k = 0; k < F; ++k) mx = fmaxf(mx, lp(k));
    float se = 0.f;
    for (int k = 0; k < F; ++k) se += expf(lp(k) - mx);
    const float logz = logf(se) + mx, mk = m.nm[n];
    float v1 = 0.f;
    for (int k = 0; k < F; ++k) {
      const float oh = ((b.oh[((size_t)m.bg * N + n) * F + k] - 0.0f) / b.nv1 * mk) * b.nv1 + 0.0f;
      v1 += (lp(k) - logz) * oh * mk;
    }
    part[n] = v0;
    part[N + n] = vx;
    part[2 * N + n] = v1;
  }
  __syncthreads();
  if (tid < 3) {
    float s = 0.f;
    for (int n = 0; n < N; ++n) s += part[tid * N + n];
    b.sums[(size_t)m.bg * 4 + tid] = s;
  }
  if (tid == 3) b.sums[(size_t)m.bg * 4 + 3] = 0.f;
  if (!reverse) return;
  __syncthreads();
  // seed: d net = coef (net - eps), x columns with coef[0], h columns with coef[1] (0 at t = 0)
  const float cx = b.coef[2 * m.bg], ch = b.coef[2 * m.bg + 1];
  float* dv = red;  // [3][N] d vel (after the projection)
  for (int i = tid; i < N * 3; i += kThreads) {
    const int n = i / 3, d = i - n * 3;
    dv[d * N + n] = cx * (net[n * D + d] - eps[n * D + d]);
  }
  for (int i = tid; i < N * F1; i += kThreads) {  // d h3 (the time column is dropped: exact zero), times node_mask
    const int n = i / F1, k = i - n * F1;
    h3[i] = k < F ? ch * (net[n * D + 3 + k] - eps[n * D + 3 + k]) * m.nm[n] : 0.f;
  }
  __syncthreads();
  float dm[3];
  for (int d = 0; d < 3; ++d) {
    float* tmp = lds;  // (lds is free until the product below)
    for (int n = tid; n < N; n += kThreads) tmp[n] = dv[d * N + n] * m.nm[n];
    dm[d] = node_sum(tmp, N, &red[3 * 256 + 4 + d]) / cnt;
  }
  float* dx = m.dx(b);
  for (int i = tid; i < N * 4; i += kThreads) {  // remove_mean_with_mask, then vel = (x_L - x_0) * node_mask
    const int n = i / 4, d = i - n * 4;
    dx[i] = d < 3 ? (dv[d * N + n] - dm[d]) * m.nm[n] : 0.f;
  }
  __syncthreads();
  mm_rows(b.w + b.off[OUT_W], H, F1, H, h3, F1, N, m.node(b.dh), H, nullptr, false, lds);
}

}  // namespace gaudi_etrain

using namespace gaudi_etrain;

int gaudi_et_embed(const ETBufs& b, int Bc, hipStream_t s) {
  hipLaunchKernelGGL(et_embed_kernel, dim3(Bc), dim3(kThreads), 0, s, b);
  return (int)hipGetLastError();
}

int gaudi_et_block(const ETBufs& b, int Bc, int l, hipStream_t s) {
  hipLaunchKernelGGL(et_block_kernel, dim3(Bc), dim3(kThreads), 0, s, b, l);
  return (int)hipGetLastError();
}

int gaudi_et_readout(const ETBufs& b, int Bc, int reverse, hipStream_t s) {
  hipLaunchKernelGGL(et_readout_kernel, dim3(Bc), dim3(kThreads), 0, s, b, reverse);
  return (int)hipGetLastError();
}

int gaudi_et_equiv_reverse(const ETBufs& b, int Bc, int l, hipStream_t s) {
  hipLaunchKernelGGL(et_equiv_rev_kernel, dim3(Bc), dim3(kThreads), 0, s, b, l);
  return (int)hipGetLastError();
}

int gaudi_et_gcl_reverse(const ETBufs& b, int Bc, int l, int sub, hipStream_t s) {
  hipLaunchKernelGGL(et_gcl_rev_kernel, dim3(Bc), dim3(kThreads), 0, s, b, l, sub);
  return (int)hipGetLastError();
}
