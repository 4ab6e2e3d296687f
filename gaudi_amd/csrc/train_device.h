// train_device.h -- the core the two training passes share (pred_train.h, edm_train.h; the host side is train_host.inc): the
// buffers both networks have, the weight-gradient job, and the device pieces of a GCL that kernt_pred_train.hip and
// kernt_edm_train.hip both call -- the SiLU family, mm_rows (the fp32 row-block product over a torch-layout matrix), the
// attention gate and edge_feat, the row aggregation, the node MLP forward and its reverse head, the attention reverse, the
// edge MLP's reverse tail and the antisymmetric scatter into dx.  A shared piece may take a switch where the networks differ;
// it keeps the sequence of float operations each had.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace gaudi_train {

constexpr int kThreads = 256;
constexpr int kRows = 16;  // rows of X staged in LDS per round of mm_rows

// float offsets of the head's tensors inside the flat buffer (-1: absent); each network's per-layer roles follow
enum Head { EMB_W, EMB_B, OUT_W, OUT_B, NHEAD };

// What both networks' kernels read and write.  Chunk arrays are array-major ([Bc][...]); E = N * N.
struct TrainBufs {
  // inputs (whole batch; the chunk's molecules start at b0)
  const float* t;      // [B]  t_int / T
  const float* nm;     // [B][N]
  const float* em;     // [B][N][N]
  // weights
  const float* w;      // flat, torch layout
  const float* wt;     // flat, every matrix transposed
  const int* off;      // float offset per role
  int F, H, L, N, A, attention, use_tanh;  // A: columns of an edge MLP's attribute block (W1 is [H][2H + A])
  int b0, bcap;  // first molecule of the chunk; molecules per chunk the scratch is laid out for (stride of hs / xs)
  // node stash: the input of every layer that is recomputed in reverse, and the final h / x
  float *hs, *xs;            // [stashes][Bc][N][H], [(L+1)][Bc][N][4]
  float* hin;                // [Bc][N][F+1]
  // scratch of one GCL, reused by every layer
  float *P, *Q, *agg, *qp, *q, *dr, *dP, *dQ, *dh;  // [Bc][N][H]  (qp: qpre -> dqpre; dh: the running gradient, in place)
  float* dx;                 // [Bc][N][4]  running gradient, in place
  float* dhout;              // [Bc][N][outputs of embedding_out]
  float *U, *Su, *V, *M, *EF, *DE;  // [Bc][E][H]  (U: u -> du, Su: silu(u), V: v -> dv, M: silu(v), EF: edge_feat, DE: its gradient)
  float *diff, *dcd;         // [Bc][E][4]  (diff: coord_diff, norm; dcd: d coord_diff)
  float *rad, *gate, *dap, *phi, *ppre, *dp;  // [Bc][E]
};

// one weight-gradient product: G[m][k] (+)= sum_r Y[r][m] * X[r][k]   (X == nullptr: X = 1, Kc = 1)
struct OuterJob {
  const float* Y;
  const float* X;
  float* G;
  int ldy, ldx, ldg, M, Kc, R;
};

// the molecule of this workgroup
struct Mol {
  int mb, bg, N, E, H;
  const float *nm, *em;
  __device__ Mol(const TrainBufs& b) {
    mb = blockIdx.x;
    bg = b.b0 + mb;
    N = b.N;
    E = N * N;
    H = b.H;
    nm = b.nm + (size_t)bg * N;
    em = b.em + (size_t)bg * E;
  }
  __device__ float* node(float* base) const { return base + (size_t)mb * N * H; }
  __device__ float* edge(float* base) const { return base + (size_t)mb * E * H; }
  __device__ float* escal(float* base, int w = 1) const { return base + (size_t)mb * E * w; }
  __device__ float* hstash(const TrainBufs& b, int slot) const { return b.hs + ((size_t)slot * b.bcap + mb) * N * H; }
  __device__ float* xstash(const TrainBufs& b, int slot) const { return b.xs + ((size_t)slot * b.bcap + mb) * N * 4; }
  __device__ float* dx(const TrainBufs& b) const { return b.dx + (size_t)mb * N * 4; }
};

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

// The pieces below are called by every thread of the workgroup, with M = silu(v) and the rest of the GCL's forward in the
// scratch.  att and nmlp point into b.off, at the consecutive slots AW, AB of att_mlp and N0W, N0B, N2W, N2B of node_mlp (the
// same order in both networks' enums): each float offset into b.w / b.wt is read where it is used, which keeps the scalar
// registers of the callers where they were (profiles/r12_train_ab.txt).  w1 and w2 are such offsets, already read.

// att_mlp: gate = sigmoid(wa . M + ba) (1 without attention; att is read with it only), then edge_feat
// EF = M * gate * edge_mask.  The caller synchronises before it reads EF.
__device__ inline void gate_edge_feat(const TrainBufs& b, const Mol& m, const int* att) {
  const int E = m.E, H = m.H, tid = threadIdx.x;
  const float* M = m.edge(b.M);
  float *EF = m.edge(b.EF), *gate = m.escal(b.gate);
  for (int e = tid; e < E; e += kThreads) {
    float g = 1.f;
    if (b.attention) {
      const float* wa = b.w + att[0];
      float a = b.w[att[1]];
      for (int k = 0; k < H; ++k) a = fmaf(wa[k], M[e * H + k], a);
      g = sigm(a);
    }
    gate[e] = g;
  }
  __syncthreads();
  for (int idx = tid; idx < E * H; idx += kThreads) {
    const int e = idx / H;
    EF[idx] = M[idx] * gate[e] * m.em[e];
  }
}

// unsorted_segment_sum of EF over the row, in column order; kDivide: divided by div (the EDM's normalization_factor or N --
// the predictor's plain sum must not become a division by 1)
template <bool kDivide>
__device__ inline void row_aggregate(const TrainBufs& b, const Mol& m, float div) {
  const int N = m.N, H = m.H;
  const float* EF = m.edge(b.EF);
  float* agg = m.node(b.agg);
  for (int idx = threadIdx.x; idx < N * H; idx += kThreads) {
    const int i = idx / H, k = idx - i * H;
    float a = 0.f;
    for (int j = 0; j < N; ++j) a += EF[(i * N + j) * H + k];
    agg[idx] = kDivide ? a / div : a;
  }
  __syncthreads();
}

// node_mlp over [h | agg]: qp = Wn1 [h | agg] + b, q = silu(qp); with out_slot >= 0, the h stash of that slot becomes
// (h + Wn2 q + b2) * node_mask
__device__ inline void node_mlp_forward(const TrainBufs& b, const Mol& m, const float* h, const int* nmlp, int out_slot, float* lds) {
  const int N = m.N, H = m.H, tid = threadIdx.x;
  float *agg = m.node(b.agg), *qp = m.node(b.qp), *q = m.node(b.q);
  const float* Wn1T = b.wt + nmlp[0];  // [2H][H]
  mm_rows(Wn1T, H, H, H, h, H, N, qp, H, b.w + nmlp[1], false, lds);
  mm_rows(Wn1T + (size_t)H * H, H, H, H, agg, H, N, qp, H, nullptr, true, lds);
  for (int idx = tid; idx < N * H; idx += kThreads) q[idx] = silu(qp[idx]);
  __syncthreads();
  if (out_slot >= 0) {
    float* ho = m.hstash(b, out_slot);
    mm_rows(b.wt + nmlp[2], H, H, H, q, H, N, ho, H, b.w + nmlp[3], false, lds);
    for (int idx = tid; idx < N * H; idx += kThreads) ho[idx] = (h[idx] + ho[idx]) * m.nm[idx / H];  // recurrent, mask
    __syncthreads();
  }
}

// h_out = (h + node_mlp([h | agg])) * nm, reverse: d h_out in dh -> dr = dh = dh * nm, qp <- dqpre, dh += Wn1h^T dqpre,
// dP <- d agg = Wn1a^T dqpre
__device__ inline void node_mlp_reverse(const TrainBufs& b, const Mol& m, const int* nmlp, float* lds) {
  const int N = m.N, H = m.H, tid = threadIdx.x;
  float *dh = m.node(b.dh), *dr = m.node(b.dr), *qp = m.node(b.qp), *dP = m.node(b.dP), *dQ = m.node(b.dQ);
  for (int idx = tid; idx < N * H; idx += kThreads) {
    const float v = dh[idx] * m.nm[idx / H];
    dr[idx] = v;
    dh[idx] = v;
  }
  __syncthreads();
  mm_rows(b.w + nmlp[2], H, H, H, dr, H, N, dQ, H, nullptr, false, lds);  // dq = Wn2^T dr
  for (int idx = tid; idx < N * H; idx += kThreads) qp[idx] = dQ[idx] * dsilu(qp[idx]);  // qp: dqpre
  const float* Wn1 = b.w + nmlp[0];  // [H][2H]
  mm_rows(Wn1, 2 * H, H, H, qp, H, N, dh, H, nullptr, true, lds);       // dh += Wn1h^T dqpre
  mm_rows(Wn1 + H, 2 * H, H, H, qp, H, N, dP, H, nullptr, false, lds);  // dP <- dagg
}

// edge_feat = silu(v) * gate * em, reverse: d edge_feat in DE (synchronised here) -> dap = d (att_mlp's pre-activation), and
// V <- dv.  The caller synchronises (or calls mm_rows) before it reads V.
__device__ inline void attention_reverse(const TrainBufs& b, const Mol& m, const int* att) {
  const int E = m.E, H = m.H, tid = threadIdx.x;
  float *V = m.edge(b.V), *M = m.edge(b.M), *DE = m.edge(b.DE), *gate = m.escal(b.gate), *dap = m.escal(b.dap);
  __syncthreads();
  for (int e = tid; e < E; e += kThreads) {
    float a = 0.f;
    if (b.attention) {
      for (int k = 0; k < H; ++k) a = fmaf(DE[e * H + k], M[e * H + k], a);
      a *= m.em[e] * gate[e] * (1.f - gate[e]);
    }
    dap[e] = a;
  }
  __syncthreads();
  const float* wa = b.attention ? b.w + att[0] : nullptr;
  for (int idx = tid; idx < E * H; idx += kThreads) {
    const int e = idx / H, k = idx - e * H;
    float dm = DE[idx] * gate[e] * m.em[e];
    if (wa) dm = fmaf(dap[e], wa[k], dm);
    V[idx] = dm * dsilu(V[idx]);  // V: dv
  }
}

// The reverse of an edge MLP's first two layers (W1 at w1: [H][2H + A], W2 at w2), from dv (in V): leaves du in U, its row /
// column sums in dP / dQ (d(A h_i): the edges of row i; d(B h_j): the edges of col j), adds A^T dP + B^T dQ to dh, and with
// `radial` calls per_edge(e, g) for every edge of this thread with g = the radial column's C^T du.
template <class PerEdge>
__device__ inline void edge_mlp_reverse(const TrainBufs& b, const Mol& m, int w1, int w2, bool radial, float* lds, PerEdge per_edge) {
  const int N = m.N, E = m.E, H = m.H, ld1 = 2 * H + b.A, tid = threadIdx.x;
  float *dP = m.node(b.dP), *dQ = m.node(b.dQ), *dh = m.node(b.dh);
  float *U = m.edge(b.U), *V = m.edge(b.V), *DE = m.edge(b.DE);
  mm_rows(b.w + w2, H, H, H, V, H, E, DE, H, nullptr, false, lds);  // DE <- ds = W2^T dv
  for (int idx = tid; idx < E * H; idx += kThreads) U[idx] = DE[idx] * dsilu(U[idx]);  // U: du
  __syncthreads();
  for (int idx = tid; idx < N * H; idx += kThreads) {
    const int i = idx / H, k = idx - i * H;
    float a = 0.f, c = 0.f;
    for (int j = 0; j < N; ++j) {
      a += U[(i * N + j) * H + k];
      c += U[(j * N + i) * H + k];
    }
    dP[idx] = a;
    dQ[idx] = c;
  }
  const float* W1 = b.w + w1;
  if (radial) {
    for (int e = tid; e < E; e += kThreads) {
      float g = 0.f;
      for (int k = 0; k < H; ++k) g = fmaf(W1[(size_t)k * ld1 + 2 * H], U[e * H + k], g);
      per_edge(e, g);
    }
  }
  __syncthreads();
  mm_rows(W1, ld1, H, H, dP, H, N, dh, H, nullptr, true, lds);      // dh += A^T dP
  mm_rows(W1 + H, ld1, H, H, dQ, H, N, dh, H, nullptr, true, lds);  // dh += B^T dQ
}

// coord_diff_ij = f(x_i - x_j): dx_i += sum_j (dcd_ij - dcd_ji), with dcd holding d (x_i - x_j)
__device__ inline void scatter_dx(const TrainBufs& b, const Mol& m) {
  const int N = m.N;
  const float* dcd = m.escal(b.dcd, 4);
  float* dx = m.dx(b);
  for (int i = threadIdx.x; i < N; i += kThreads) {
    float a[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < N; ++j)
      for (int k = 0; k < 3; ++k) a[k] += dcd[(i * N + j) * 4 + k] - dcd[(j * N + i) * 4 + k];
    for (int k = 0; k < 3; ++k) dx[i * 4 + k] += a[k];
  }
  __syncthreads();
}

}  // namespace gaudi_train

// the weight-gradient reduction (kernt_pred_train.hip); tiles: device array of (job index, m0, k0, -) 32 x 32 output tiles of
// the device job array `jobs`; returns the hipError_t of the launch
int gaudi_pt_outer(const gaudi_train::OuterJob* jobs, const int4* tiles, int n_tiles, hipStream_t s);
