// edm_train.h -- EDM training: the per-molecule loss of EnVariationalDiffusion in train mode and its gradient with respect
// to every dynamics.egnn parameter (train_edm.py:36-50 compute_loss + loss.backward(); en_diffusion.py:644-805 with
// t0_always = False; edm/egnn/models.py:83-152, edm/egnn/egnn_new.py).  Shared by the kernels (kernt_edm_train.hip) and
// the C ABI (edm_train_host.inc).  What the EDM has in common with the predictor's pass (pred_train.h) -- the buffers of a
// GCL, the weight-gradient job and the device pieces of a GCL -- is train_device.h; this file holds what the EDM adds.
//
// As for the predictor, the kernels run on fp32 instructions over the UNPADDED torch shapes: every tensor
// lives in one flat buffer in the order of the names passed to gaudi_load_edm (the gradient comes back in that layout),
// and a second buffer of the same size holds each matrix transposed.  These copies are separate from the sampler's packed
// images: gaudi_edm_set_train_weights replaces them alone.
//
// One workgroup = one molecule over the dense N x N edge set (edge e = i*N + j).  Per chunk of molecules:
//   node stash  (L (S+1) + 1) x h [N][H]: the input of every GCL sub-layer and of every gcl_equiv, and the final h;
//               (L+1) x x [N][4]: the input of every block, and the final x
//   block scratch: the edge attributes [E][A] and those of the input distances [E][A/2], coord_diff / norm [E][4],
//   radial and d radial [E], d coord_diff [E][4]
//   sub-layer scratch (reused by every sub-layer): 6 edge arrays [E][H], 9 node arrays [N][H], 5 edge scalars
// The host lists these arrays once (train_host.inc: Carver) and takes both the size of a chunk and the pointers from that list.
// Launches per chunk: embed, one forward launch per block, the readout (loss sums + seed), then per block in reverse
// gcl_equiv and each GCL sub-layer (each recomputes its forward from the stash) with the weight-gradient reduction
// (train_device.h: gaudi_pt_outer) after each, and the embedding's reduction last.  No atomics: two identical calls give
// bit-identical results.
#pragma once
#include "train_device.h"

namespace gaudi_etrain {

// float offsets of the tensors inside the flat buffer (-1: absent).  Head (train_device.h), then per block S GCLs and gcl_equiv.
using gaudi_train::EMB_B;
using gaudi_train::EMB_W;
using gaudi_train::NHEAD;
using gaudi_train::OUT_B;
using gaudi_train::OUT_W;
enum Gcl { E0W, E0B, E2W, E2B, AW, AB, N0W, N0B, N2W, N2B, NGCL };
enum Equiv { C0W, C0B, C2W, C2B, C4W, NEQ };

__host__ __device__ inline int block_stride(int S) { return S * NGCL + NEQ; }
__host__ __device__ inline int gcl_slot(int S, int l, int s, int r) { return NHEAD + l * block_stride(S) + s * NGCL + r; }
__host__ __device__ inline int equiv_slot(int S, int l, int r) { return NHEAD + l * block_stride(S) + S * NGCL + r; }
inline int n_slots(int S, int L) { return NHEAD + L * block_stride(S); }

// TrainBufs (A = 2, or 24 with sin_embedding; hs holds L (S+1) + 1 stashes; dhout is [Bc][N][F+1]) and what the EDM adds
struct ETBufs : gaudi_train::TrainBufs {
  // inputs (whole batch; the chunk's molecules start at b0)
  const float* x;      // [B][N][3]  un-normalised
  const float* oh;     // [B][N][F]
  const float* as;     // [B][2]  alpha_t, sigma_t
  const float* coef;   // [B][2]  seed coefficient of the x columns, of the h columns: dnet = coef * (net - eps)
  const float* noise;  // [B][N][3+F] raw draws, or nullptr: Philox draw 0 of (seed, sample_offset + b)
  uint64_t seed;
  int64_t sample_offset;
  // outputs (whole batch)
  float* net;          // [B][N][3+F]
  float* sums;         // [B][4]: sum (eps - net)^2 over every entry, over the x columns, log p(h | z_0) (true classes)
  int S, sin;          // (off holds n_slots(S, L) offsets)
  float coords_range, norm_constant, agg_div, nv0, nv1, sig_cat;  // agg_div: normalization_factor, or N for 'mean'
  // chunk scratch of a block
  float* eps;          // [Bc][N][3+F]
  float* d0a;          // [Bc][E][A/2]  edge attributes of the input distances
  float* ea;           // [Bc][E][A]
  float* drad;         // [Bc][E]
};

}  // namespace gaudi_etrain

// launchers (kernt_edm_train.hip); return the hipError_t of the launch
int gaudi_et_embed(const gaudi_etrain::ETBufs& b, int Bc, hipStream_t s);
int gaudi_et_block(const gaudi_etrain::ETBufs& b, int Bc, int l, hipStream_t s);            // forward of block l
int gaudi_et_readout(const gaudi_etrain::ETBufs& b, int Bc, int reverse, hipStream_t s);   // loss sums (+ seed)
int gaudi_et_equiv_reverse(const gaudi_etrain::ETBufs& b, int Bc, int l, hipStream_t s);
int gaudi_et_gcl_reverse(const gaudi_etrain::ETBufs& b, int Bc, int l, int sub, hipStream_t s);
