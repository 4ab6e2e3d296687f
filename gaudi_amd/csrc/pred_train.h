// pred_train.h -- predictor training: the L1 loss gradient with respect to every EGNN_predictor parameter
// (cond_prediction/train_cond_predictor.py:64-81 compute_loss + loss.backward(); edm/egnn_predictor/gcl.py:225-316,
// edm/egnn_predictor/models.py:433-457,543-560).  Shared by the kernels (kernt_pred_train.hip) and the C ABI
// (pred_train_host.inc).
//
// The kernels run on fp32 instructions over the UNPADDED torch shapes: every tensor of the predictor lives in one flat
// buffer in the order the checkpoint names were passed to gaudi_load_predictor (the gradient comes back in that same
// layout), and a second buffer of the same size holds each matrix transposed (the forward products read W^T so that
// consecutive threads read consecutive floats; the reverse products read W itself).
//
// One workgroup = one molecule, over the dense N x N edge set of the reference (get_adj_matrix: edge e = i*N + j,
// row i, col j; masked slots carry edge_mask = 0 and contribute exact zeros).  Per call the batch is cut into chunks;
// per chunk, with E = N*N and H = hidden_nf:
//   per-layer node stash   (L+1) x { h [N][H] | x [N][4] } per molecule (the input of every layer)
//   layer scratch, reused by every layer: 8 edge arrays [E][H] (u->du, silu(u), v->dv, silu(v), edge_feat, cpre->dc,
//   silu(cpre), d edge_feat), 10 node arrays [N][H], 15 edge scalars
// i.e. about 4 (8 E H + (L + 11) N H + 16 E) bytes per molecule: 0.98 MB for a cata-11 molecule (N 11) at H 196 and
// 12 layers; chunks are sized to 1 GiB of scratch (about 1000 such molecules).  A layer's reverse pass recomputes that layer's forward from the stash instead of keeping the edge arrays
// of every layer (12 x the memory).  After each layer's reverse pass the weight-gradient reduction (pt_outer) sums
// dY (x) X over every (molecule, row) of the chunk on v_mfma_f32_16x16x4_f32, split over four waves in a fixed order, no atomics;
// chunks add into the gradient one after the other, so two identical calls give bit-identical gradients.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace gaudi_train {

// float offsets of the predictor's tensors inside the flat buffer (-1: absent).  Head, then 13 per layer.
enum Head { EMB_W, EMB_B, OUT_W, OUT_B, NHEAD };
enum Layer { E0W, E0B, E2W, E2B, AW, AB, C0W, C0B, C2W, N0W, N0B, N2W, N2B, NLAYER };

struct PTBufs {
  // inputs (whole batch; the chunk's molecules start at b0)
  const float* zt;     // [B][N][3+F]
  const float* t;      // [B]
  const float* nm;     // [B][N]
  const float* em;     // [B][N][N]
  const float* pred;   // [B][K]
  const float* y;      // [B][K]
  // weights
  const float* w;      // flat, torch layout
  const float* wt;     // flat, every matrix transposed
  const int* off;      // NHEAD + NLAYER * L
  int F, K, H, L, N, attention, use_tanh;
  float coords_range_layer, readout_div, dpred_scale;  // dpred = sign(pred - y) * dpred_scale  (= 1 / (B K))
  int b0, bcap;  // first molecule of the chunk; molecules per chunk the scratch is laid out for (stride of hs / xs)
  // chunk stash / scratch (array-major: [Bc][...])
  float *hs, *xs;           // [(L+1)][Bc][N][H], [(L+1)][Bc][N][4]
  float* hin;               // [Bc][N][F+1]
  float* d0;                // [Bc][E]
  float *P, *Q, *agg, *qp, *q, *dr, *dP, *dQ;  // [Bc][N][H]  (qp: qpre -> dqpre)
  float *dh0, *dh1;         // [Bc][N][H] ping-pong running dh
  float *dx0, *dx1;         // [Bc][N][4]
  float* dhout;             // [Bc][N][K]
  float *U, *S, *V, *M, *EFt, *CP, *C, *DE;  // [Bc][E][H]  (U: u -> du, V: v -> dv, CP: cpre -> dc, DE: d edge_feat)
  float *diff, *ddiff;      // [Bc][E][4]  (diff: x_i - x_j, w = |diff|)
  float *rad, *gate, *phi, *ppre, *dp, *dap;  // [Bc][E]
};

// one weight-gradient product: G[m][k] (+)= sum_r Y[r][m] * X[r][k]   (X == nullptr: X = 1, Kc = 1)
struct OuterJob {
  const float* Y;
  const float* X;
  float* G;
  int ldy, ldx, ldg, M, Kc, R;
};

}  // namespace gaudi_train

// launchers (kernt_pred_train.hip); return the hipError_t of the launch
int gaudi_pt_embed(const gaudi_train::PTBufs& b, int Bc, hipStream_t s);
int gaudi_pt_layer(const gaudi_train::PTBufs& b, int Bc, int l, int reverse, hipStream_t s);
int gaudi_pt_readout(const gaudi_train::PTBufs& b, int Bc, hipStream_t s);
// tiles: device array of (job index, m0, k0, -) 32 x 32 output tiles of the device job array `jobs`
int gaudi_pt_outer(const gaudi_train::OuterJob* jobs, const int4* tiles, int n_tiles, hipStream_t s);
