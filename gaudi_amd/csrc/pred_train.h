// pred_train.h -- predictor training: the L1 loss gradient with respect to every EGNN_predictor parameter
// (cond_prediction/train_cond_predictor.py:64-81 compute_loss + loss.backward(); edm/egnn_predictor/gcl.py:225-316,
// edm/egnn_predictor/models.py:433-457,543-560).  Shared by the kernels (kernt_pred_train.hip) and the C ABI
// (pred_train_host.inc).  What the predictor has in common with the EDM's pass (edm_train.h) -- the buffers of a GCL, the
// weight-gradient job and the device pieces of a GCL -- is train_device.h; this file holds what the predictor adds.
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
//   silu(cpre), d edge_feat), 9 node arrays [N][H] (the running gradient dh among them: each layer's reverse pass
//   updates it, and dx [N][4], in place), 15 edge scalars
// i.e. about 4 (8 E H + (L + 10) N H + 15 E) bytes per molecule: 0.96 MB for a cata-11 molecule (N 11) at H 196 and
// 12 layers; chunks are sized to 1 GiB of scratch (about 1100 such molecules).  The host lists the arrays once
// (train_host.inc: Carver) and takes both the size and the pointers from that list.  A layer's reverse pass recomputes
// that layer's forward from the stash instead of keeping the edge arrays
// of every layer (12 x the memory).  After each layer's reverse pass the weight-gradient reduction (pt_outer) sums
// dY (x) X over every (molecule, row) of the chunk on v_mfma_f32_16x16x4_f32, split over four waves in a fixed order, no atomics;
// chunks add into the gradient one after the other, so two identical calls give bit-identical gradients.
#pragma once
#include "train_device.h"

namespace gaudi_train {

// float offsets of the predictor's tensors inside the flat buffer (-1: absent).  Head (train_device.h), then 13 per layer.
enum Layer { E0W, E0B, E2W, E2B, AW, AB, C0W, C0B, C2W, N0W, N0B, N2W, N2B, NLAYER };

// TrainBufs (A = 2: radial and the input distance d0; hs holds L+1 stashes; dhout is [Bc][N][K]) and what the predictor adds
struct PTBufs : TrainBufs {
  // inputs (whole batch)
  const float* zt;     // [B][N][3+F]
  const float* pred;   // [B][K]
  const float* y;      // [B][K]
  int K;
  float coords_range_layer, readout_div, dpred_scale;  // dpred = sign(pred - y) * dpred_scale  (= 1 / (B K))
  // chunk scratch
  float* d0;           // [Bc][E]
  float *CP, *C;       // [Bc][E][H]  (CP: cpre -> dc, C: silu(cpre))
};

}  // namespace gaudi_train

// launchers (kernt_pred_train.hip); return the hipError_t of the launch
int gaudi_pt_embed(const gaudi_train::PTBufs& b, int Bc, hipStream_t s);
int gaudi_pt_layer(const gaudi_train::PTBufs& b, int Bc, int l, int reverse, hipStream_t s);
int gaudi_pt_readout(const gaudi_train::PTBufs& b, int Bc, hipStream_t s);
