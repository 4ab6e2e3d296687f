// edm_train.h -- EDM training: the per-molecule loss of EnVariationalDiffusion in train mode and its gradient with respect
// to every dynamics.egnn parameter (train_edm.py:36-50 compute_loss + loss.backward(); en_diffusion.py:644-805 with
// t0_always = False; edm/egnn/models.py:83-152, edm/egnn/egnn_new.py).  Shared by the kernels (kernt_edm_train.hip) and
// the C ABI (edm_train_host.inc).
//
// As for the predictor (pred_train.h), the kernels run on fp32 instructions over the UNPADDED torch shapes: every tensor
// lives in one flat buffer in the order of the names passed to gaudi_load_edm (the gradient comes back in that layout),
// and a second buffer of the same size holds each matrix transposed.  These copies are separate from the sampler's packed
// images: gaudi_edm_set_train_weights replaces them alone.
//
// One workgroup = one molecule over the dense N x N edge set (edge e = i*N + j).  Per chunk of molecules:
//   node stash  (L (S+1) + 1) x h [N][H]: the input of every GCL sub-layer and of every gcl_equiv, and the final h;
//               (L+1) x x [N][4]: the input of every block, and the final x
//   block scratch: the edge attributes [E][A], coord_diff / norm [E][4], d radial [E], d coord_diff [E][4]
//   sub-layer scratch (reused by every sub-layer): 6 edge arrays [E][H], 9 node arrays [N][H], 5 edge scalars
// Launches per chunk: embed, one forward launch per block, the readout (loss sums + seed), then per block in reverse
// gcl_equiv and each GCL sub-layer (each recomputes its forward from the stash) with the weight-gradient reduction of
// pred_train.h (gaudi_pt_outer) after each, and the embedding's reduction last.  No atomics: two identical calls give
// bit-identical results.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace gaudi_etrain {

// float offsets of the tensors inside the flat buffer (-1: absent).  Head, then per block S GCLs and gcl_equiv.
enum Head { EMB_W, EMB_B, OUT_W, OUT_B, NHEAD };
enum Gcl { E0W, E0B, E2W, E2B, AW, AB, N0W, N0B, N2W, N2B, NGCL };
enum Equiv { C0W, C0B, C2W, C2B, C4W, NEQ };

__host__ __device__ inline int block_stride(int S) { return S * NGCL + NEQ; }
__host__ __device__ inline int gcl_slot(int S, int l, int s, int r) { return NHEAD + l * block_stride(S) + s * NGCL + r; }
__host__ __device__ inline int equiv_slot(int S, int l, int r) { return NHEAD + l * block_stride(S) + S * NGCL + r; }
inline int n_slots(int S, int L) { return NHEAD + L * block_stride(S); }

struct ETBufs {
  // inputs (whole batch; the chunk's molecules start at b0)
  const float* x;      // [B][N][3]  un-normalised
  const float* oh;     // [B][N][F]
  const float* t;      // [B]  t_int / T
  const float* as;     // [B][2]  alpha_t, sigma_t
  const float* coef;   // [B][2]  seed coefficient of the x columns, of the h columns: dnet = coef * (net - eps)
  const float* nm;     // [B][N]
  const float* em;     // [B][N][N]
  const float* noise;  // [B][N][3+F] raw draws, or nullptr: Philox draw 0 of (seed, sample_offset + b)
  uint64_t seed;
  int64_t sample_offset;
  // outputs (whole batch)
  float* net;          // [B][N][3+F]
  float* sums;         // [B][4]: sum (eps - net)^2 over every entry, over the x columns, log p(h | z_0) (true classes)
  // weights
  const float* w;      // flat, torch layout
  const float* wt;     // flat, every matrix transposed
  const int* off;      // n_slots(S, L)
  int F, H, L, S, N, A, attention, use_tanh, sin;
  float coords_range, norm_constant, agg_div, nv0, nv1, sig_cat;  // agg_div: normalization_factor, or N for 'mean'
  int b0, bcap;
  // chunk stash / scratch (array-major: [Bc][...])
  float *hs, *xs;            // [(L (S+1) + 1)][Bc][N][H], [(L+1)][Bc][N][4]
  float* hin;                // [Bc][N][F+1]
  float* eps;                // [Bc][N][3+F]
  float* d0a;                // [Bc][E][A/2]  edge attributes of the input distances
  float* ea;                 // [Bc][E][A]
  float *diff, *dcd;         // [Bc][E][4]  (diff: coord_diff, norm)
  float *rad, *drad;         // [Bc][E]
  float *P, *Q, *agg, *qp, *q, *dr, *dP, *dQ, *dh;  // [Bc][N][H]
  float* dx;                 // [Bc][N][4]
  float* dhout;              // [Bc][N][F+1]
  float *U, *Sx, *V, *M, *EF, *DE;  // [Bc][E][H]
  float *gate, *dap, *phi, *ppre, *dp;  // [Bc][E]
};

}  // namespace gaudi_etrain

// launchers (kernt_edm_train.hip); return the hipError_t of the launch
int gaudi_et_embed(const gaudi_etrain::ETBufs& b, int Bc, hipStream_t s);
int gaudi_et_block(const gaudi_etrain::ETBufs& b, int Bc, int l, hipStream_t s);            // forward of block l
int gaudi_et_readout(const gaudi_etrain::ETBufs& b, int Bc, int reverse, hipStream_t s);   // loss sums (+ seed)
int gaudi_et_equiv_reverse(const gaudi_etrain::ETBufs& b, int Bc, int l, hipStream_t s);
int gaudi_et_gcl_reverse(const gaudi_etrain::ETBufs& b, int Bc, int l, int sub, hipStream_t s);
