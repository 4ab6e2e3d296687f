/*
 * gaudi_hip.h -- C ABI of libgaudi_hip.so: MI355X (gfx950) guided-diffusion sampler for GaUDI.
 *
 * The reference (tomer196/GaUDI) has no FFI/plugin layer: its boundary for this path is a set
 * of Python call signatures plus an on-disk checkpoint.  This header is
 * therefore the boundary a maintainer would bind with ctypes; each entry
 * point names the reference function it replaces.  Conventions:
 *   - every function returns 0 on success or a negative GAUDI_E_* code; nothing throws across
 *     the ABI; gaudi_last_error(h) returns a human-readable message for the last failure;
 *   - all pointers are HOST pointers to caller-owned, contiguous fp32/int buffers; the handle
 *     owns all device memory and one HIP stream; one handle per device, not thread-safe;
 *   - tensors use the reference's layouts: z/eps/grad [B,N,3+F] (x first), node_mask [B,N],
 *     edge_mask [B,N,N] (row i = receiving node, as edm/egnn/models.py:154-175).
 */
#ifndef GAUDI_HIP_H
#define GAUDI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GAUDI_OK 0
#define GAUDI_E_INVALID (-1)   /* bad argument / unsupported configuration      */
#define GAUDI_E_HIP (-2)       /* HIP runtime error                              */
#define GAUDI_E_STATE (-3)     /* e.g. sampling before weights are loaded        */
#define GAUDI_E_MISSING (-4)   /* a required checkpoint tensor was not supplied  */
#define GAUDI_E_CAPACITY (-5)  /* problem does not fit the kernel's LDS budget   */

typedef struct gaudi_handle gaudi_handle;

/* Architecture of EnVariationalDiffusion(EGNN_dynamics): models_edm.py:67-96 / utils/args_edm.py. */
typedef struct {
  int32_t in_node_nf;          /* F: dataset.num_node_features (cata 1, hetro 12)            */
  int32_t hidden_nf;           /* args.nf                                                      */
  int32_t n_layers;            /* args.n_layers (EquivariantBlocks)                            */
  int32_t inv_sublayers;       /* args.inv_sublayers (GCLs per block)                          */
  int32_t attention;           /* args.attention                                               */
  int32_t tanh;                /* args.tanh                                                    */
  float coords_range;          /* args.coords_range (NOT divided by n_layers, egnn_new.py:290) */
  float norm_constant;         /* args.norm_constant                                           */
  float normalization_factor;  /* args.normalization_factor of aggregation_method "sum"; 0 = aggregation_method "mean": divide by the
                                  number of edges of the dense list per row, masked ones included = the call's padded node
                                  count N (unsorted_segment_sum, edm/egnn/egnn_new.py:403-421)   */
  int32_t diffusion_steps;     /* args.diffusion_steps (T)                                     */
  float noise_power;           /* p of "polynomial_<p>" (en_diffusion.py:47-61); 0 = the "cosine" schedule (:64-81,196-197) */
  float noise_precision;       /* args.diffusion_noise_precision                               */
  float norm_values[3];        /* args.normalize_factors                                       */
  int32_t sin_embedding;       /* args.sin_embedding (egnn_new.py:269-273,378-391): the first Linear of every edge / coordinate MLP
                                  takes 2 x 12 sinusoids of sqrt(r), sqrt(d0) instead of (r, d0).  Such a denoiser runs on the
                                  4-wave kernels (about 0.4 x the 8-wave rate; fused with the predictor at the tiny and the default
                                  width pairs, two launches per guided step elsewhere)   (ABI 7)   */
} gaudi_edm_config;

/* Architecture of EGNN_predictor: cond_prediction/train_cond_predictor.py:183-196. */
typedef struct {
  int32_t in_nf;        /* F                                                      */
  int32_t out_nf;       /* K = dataset.num_targets                                */
  int32_t hidden_nf;    /* args.nf                                                */
  int32_t n_layers;     /* args.n_layers                                          */
  int32_t attention;
  int32_t tanh;
  float coords_range;   /* divided by n_layers inside (egnn_predictor/models.py:515) */
} gaudi_pred_config;

/* Per-call diagnostics replacing the reference's per-step asserts
 * (edm/equivariant_diffusion/utils.py:52-65, sampling_edm.py:167-168,222-223). */
typedef struct {
  float max_masked_leak;   /* max |x * (1-node_mask)|                     */
  float max_cog_rel;       /* max |sum_n x| / (max|x| + 1e-10)            */
  float max_cog_abs;       /* max |sum_n x| before the final re-projection */
  int32_t nan_count;       /* NaNs scrubbed inside the chain              */
  int32_t reprojected;     /* 1 if the 5e-2 CoG re-projection fired (en_diffusion.py:1000-1006) */
} gaudi_diag;

int gaudi_create(int device, gaudi_handle** out);
void gaudi_destroy(gaudi_handle* h);
const char* gaudi_last_error(const gaudi_handle* h);
/* The last NON-fatal condition of the handle a caller should know about ("" if none): e.g. a weight set the fp16-pair images
 * cannot carry (an infinite weight, a matrix far below the others), whose calls therefore run the fp32-instruction kernels at
 * about 0.55 x the speed.  gaudi_amd.engine turns it into a Python warning at load time and into diag["edge_math_fallback"]. */
const char* gaudi_last_warning(const gaudi_handle* h);
/* The kernel the most recent launch of the handle ran, as its kernel-table key ("waves=8 SP=1 MR=0 GN=0 FR=0 PG=0 N1=1 EF=2 HPE=192
 * HPP=208 VT=0": csrc/kernel_table.h), NUL-terminated and cut to n bytes; "" before the first launch.  For tests and tooling: which
 * instantiation a plan picked (GAUDI_NO_FR / GAUDI_NO_N1 at gaudi_create keep the resident full-ring kernel on its plain form).
 * A launch in which the kernel's last wave ran its side job (GAUDI_NO_SIDE at gaudi_create: never) has " SD=1" behind the key. */
int gaudi_last_kernel_key(const gaudi_handle* h, char* buf, int n);
/* Every distinct key the handle has launched since gaudi_create, in first-launch order, one per line (each line ends in '\n'),
 * NUL-terminated and cut to n bytes.  gaudi_last_kernel_key names one launch; a call that makes two (a guided step on the 4-wave
 * global-node-buffer kernels, a sin_embedding width without a fused entry) shows both here.  Returns the bytes the whole text needs
 * (its NUL included), so (h, NULL, 0) sizes the buffer; GAUDI_E_INVALID for a null handle or n < 0. */
int gaudi_kernel_key_log(const gaudi_handle* h, char* buf, int n);
/* The key of every entry the library's kernel table holds (csrc/kernel_table.h), sorted, in the same form and with the same
 * return value.  Needs no device: tests/test_kernel_census_cpu.py holds the list against the cases of tests/kernel_census.py. */
int gaudi_host_kernel_keys(char* buf, int n);
/* Bumped whenever an exported signature or a config struct changes (round 6: 6; 7: gaudi_edm_config.sin_embedding appended).  gaudi_amd/_lib.py refuses to bind the host-side packers of a
 * diagnostic library (GAUDI_LIB) whose version differs: round 5 inserted an argument into gaudi_host_pack_matrix_split. */
/* (Entry points ADDED since -- the NLL / training calls, the time grids, the value targets, gaudi_rings_to_atoms, gaudi_host_eigh3, gaudi_atoms_to_rings, gaudi_bond_orders, gaudi_kernel_key_log, gaudi_host_kernel_keys, gaudi_canonical_order, gaudi_circular_fingerprint, gaudi_host_circular_fingerprint, gaudi_fp_library_set, gaudi_fp_nearest, gaudi_fp_common, gaudi_host_fp_nearest, gaudi_fp_profile_get, gaudi_substructure_search, gaudi_host_substructure_search, gaudi_host_substructure_root_steps, gaudi_substructure_profile_get, gaudi_huckel, gaudi_host_huckel, gaudi_huckel_profile_get, gaudi_ppp, gaudi_host_ppp, gaudi_ppp_profile_get, gaudi_fp_neighbours, gaudi_fp_cluster, gaudi_fp_pick_diverse, gaudi_host_fp_neighbours, gaudi_host_fp_cluster, gaudi_host_fp_pick_diverse, gaudi_fp_select_stages_get, gaudi_ppp_open, gaudi_host_ppp_open, gaudi_ppp_open_profile_get, gaudi_ppp_scf, gaudi_host_ppp_scf, gaudi_ppp_scf_profile_get -- change no existing
 * signature and keep the version.) */
#define GAUDI_ABI_VERSION 7
int gaudi_abi_version(void);

/* Load a state dict (reference key names WITHOUT the "module." prefix).
 * names[i] is the key, tensors[i] its fp32 data, numel[i] its element count.  Unknown keys are
 * ignored ("buffer", "gamma.gamma": the schedule is rebuilt from the config exactly as
 * PredefinedNoiseSchedule does); missing ones fail with GAUDI_E_MISSING.
 * Replaces models_edm.get_model / load_state_dict (models_edm.py:61-104). */
int gaudi_load_edm(gaudi_handle* h, const gaudi_edm_config* cfg, int n, const char* const* names,
                   const float* const* tensors, const int64_t* numel);
/* Replaces get_cond_predictor_model (cond_prediction/train_cond_predictor.py:183-203). */
int gaudi_load_predictor(gaudi_handle* h, const gaudi_pred_config* cfg, int n, const char* const* names,
                         const float* const* tensors, const int64_t* numel);

/* gamma table [T+1] as PredefinedNoiseSchedule builds it (en_diffusion.py:191-218). */
int gaudi_get_gamma(gaudi_handle* h, float* gamma_out /* [T+1] */);
/* Per-step scalars (en_diffusion.py:433-457, 811-821): coef_out[s] = {alpha_t|s, sigma2_t|s/alpha_t|s/sigma_t,
 * sigma_t|s*sigma_s/sigma_t, t=(s+1)/T} for s in [0,T). */
int gaudi_get_step_coefficients(gaudi_handle* h, float* coef_out /* [T][4] */);

/* eps_hat = EGNN_dynamics._forward(t, z, node_mask, edge_mask)  (edm/egnn/models.py:83-152). */
int gaudi_phi(gaudi_handle* h, int B, int N, const float* z, const float* t /* [B] */,
              const float* node_mask, const float* edge_mask, float* eps_out);

/* pred = EGNN_predictor.forward(z, node_mask, edge_mask, t)  (edm/egnn_predictor/models.py:433-457). */
int gaudi_predictor_fwd(gaudi_handle* h, int B, int N, const float* z, const float* t /* [B] */,
                        const float* node_mask, const float* edge_mask, float* pred_out /* [B,K] */);
/* grad = d(sum_b dpred[b].pred[b])/dz: the hand-written reverse pass replacing
 * torch.autograd.grad at en_diffusion.py:900-903. */
int gaudi_predictor_grad(gaudi_handle* h, int B, int N, const float* z, const float* t, const float* node_mask,
                         const float* edge_mask, const float* dpred /* [B,K] */, float* pred_out /* [B,K] or NULL */,
                         float* grad_out /* [B,N,3+F] */);

/* Forward noising + predictor evaluation at noise level t: sample_edm_t (cond_prediction/train_cond_predictor.py:47-61)
 * followed by the predictor forward of compute_loss (:64-81) / eval_cond_predictor.val_epoch (eval_cond_predictor.py:34-60).
 * x [B,N,3] (un-normalised, masked, mean-free) and onehot [B,N,F] are normalised as EnVariationalDiffusion.normalize does,
 * z_t = alpha_t * xh + sigma_t * eps with gamma looked up at t_int[b] in 0..T and eps = the combined position/feature noise
 * (injected raw draws `noise` [B,N,3+F], or Philox draw 0 of (seed, sample_offset + b) when NULL);
 * pred = predictor(z_t, t_int/T).  Either output may be NULL. */
int gaudi_predict_noised(gaudi_handle* h, int B, int N, const float* x, const float* onehot, const int32_t* t_int,
                         const float* node_mask, const float* edge_mask, uint64_t seed, int64_t sample_offset,
                         const float* noise, float* zt_out /* [B,N,3+F] or NULL */, float* pred_out /* [B,K] or NULL */);

/* The predictor's training step: cond_prediction/train_cond_predictor.py compute_loss (:64-81) followed by loss.backward().
 * Inputs as gaudi_predict_noised, plus y [B,K] (the targets).  z_t and pred come from the same launch as gaudi_predict_noised
 * (pred_out [B,K] or NULL receives the numbers it returns); loss_out [1] = l1_loss(pred, y) = mean |pred - y|.
 * grad_out receives d loss / d w for every predictor tensor, in the order and the row-major shape of the names passed to
 * gaudi_load_predictor, concatenated (gaudi_predictor_grad_size gives the float count).  has_grad_out [n names] = 1 where the
 * tensor has a gradient path, 0 where it has none (the last layer's coord_mlp, whose coordinate output is never read, and any
 * name the predictor does not use): those entries of grad_out are not written -- torch leaves .grad at None for them.
 * The seed dpred = sign(pred - y) / (B K) (sign(0) = 0) runs back through a separate fp32 reverse pass over the unpadded
 * weights (pred_train.h); the weight gradients are reduced on the fp32 matrix instruction in a fixed order without atomics,
 * so two identical calls give bit-identical gradients.  Every kernel family is accepted on purpose (4-wave, V4G / V8G,
 * GAUDI_EDGE_MATH=fp32, refused fp16-pair images): the forward is whatever gaudi_predict_noised runs, and the reverse pass
 * does not depend on it.  N up to 128 (GAUDI_E_CAPACITY beyond); the batch is processed in slices of at most 1 GiB of
 * scratch. */
int gaudi_predictor_loss_grad(gaudi_handle* h, int B, int N, const float* x, const float* onehot, const int32_t* t_int,
                              const float* node_mask, const float* edge_mask, const float* y /* [B,K] */, uint64_t seed,
                              int64_t sample_offset, const float* noise /* [B,N,3+F] or NULL */, float* loss_out /* [1] */,
                              float* pred_out /* [B,K] or NULL */, float* grad_out, int32_t* has_grad_out);
/* Floats of gaudi_predictor_loss_grad's grad_out: the summed numel of the tensors passed to gaudi_load_predictor. */
int gaudi_predictor_grad_size(gaudi_handle* h, int64_t* n_floats);

/* EDM training: EnVariationalDiffusion in train mode (train_edm.py:36-50; en_diffusion.py:644-805 with t0_always = False)
 * and the gradient of its per-molecule loss with respect to every dynamics.egnn tensor.  Inputs as gaudi_edm_nll, except
 * t_int [B] in 0..T and noise = ONE draw [B,N,3+F] (or NULL: Philox draw 0 of (seed, sample_offset + b)).  loss_type 0 = l2,
 * 1 = vlb.  loss_out [B] = the per-molecule loss (before compute_loss's .mean(0)); net_out [B,N,3+F] (or NULL) = phi(z_t, t).
 * grad_out (or NULL: forward only) = sum_b weight_b d loss_b / d w (weight NULL: 1 each) in the layout of the names given to
 * gaudi_load_edm (gaudi_edm_grad_size floats); has_grad_out [n names] = 1 for every dynamics.egnn tensor, 0 for the others
 * (gamma.gamma, buffer), whose entries are not written.  The reverse pass is separate fp32 HIP over the torch-layout weights
 * (edm_train.h) with a fixed-order reduction: two identical calls give bit-identical results.  N up to 128
 * (GAUDI_E_CAPACITY beyond); the batch runs in slices of at most 1 GiB of scratch. */
int gaudi_edm_loss_grad(gaudi_handle* h, int B, int N, const float* x, const float* onehot, const int32_t* t_int,
                        const float* node_mask, const float* edge_mask, uint64_t seed, int64_t sample_offset,
                        const float* noise /* [B,N,3+F] or NULL */, int loss_type, const float* weight /* [B] or NULL */,
                        float* loss_out /* [B] */, float* net_out /* [B,N,3+F] or NULL */, float* grad_out /* or NULL */,
                        int32_t* has_grad_out);
/* Floats of gaudi_edm_loss_grad's grad_out: the summed numel of the tensors passed to gaudi_load_edm. */
int gaudi_edm_grad_size(gaudi_handle* h, int64_t* n_floats);
/* Replace only the torch-layout copy (and its transposes) that gaudi_edm_loss_grad reads; names, order and sizes must be
 * those of gaudi_load_edm.  No repack: the sampler's weight images become stale, and every entry point that runs the
 * sampler kernels (gaudi_phi, gaudi_step, gaudi_decode, gaudi_sample and its callback / chain forms, gaudi_edm_nll) fails with
 * GAUDI_E_STATE, naming gaudi_load_edm, until gaudi_load_edm rebuilds both copies. */
int gaudi_edm_set_train_weights(gaudi_handle* h, int n, const char* const* names, const float* const* tensors,
                                const int64_t* numel);

/* The EDM's negative log-likelihood of data: EnVariationalDiffusion.forward in eval mode (en_diffusion.py:777-805, compute_loss
 * with t0_always = True).  x [B,N,3] (un-normalised, masked, mean-free), onehot [B,N,F], t_int [B] in 1..T (refused otherwise).
 * One launch of the EDM-only kernels evaluates the network twice per molecule: at z_t = alpha_t * xh + sigma_t * eps and
 * t = t_int/T, and at z_0 = alpha_0 * xh + sigma_0 * eps_0 and t = 0.  eps / eps_0 = combined position/feature noise from the
 * injected raw draws `noise` [2,B,N,3+F], or Philox draws 0 / 1 of (seed, sample_offset + b) when NULL.
 * nll_out [B] = kl_prior + loss_t + neg_log_constants + loss_term_0 - delta_log_px; terms_out [B][6] = those five terms in
 * that order, then error = sum (eps - phi(z_t, t))^2.  Either output may be NULL. */
int gaudi_edm_nll(gaudi_handle* h, int B, int N, const float* x, const float* onehot, const int32_t* t_int, const float* node_mask,
                  const float* edge_mask, uint64_t seed, int64_t sample_offset, const float* noise /* [2,B,N,3+F] or NULL */,
                  float* nll_out /* [B] or NULL */, float* terms_out /* [B][6] or NULL */);

/* One teacher-forced reverse step z_t -> z_s with s = s_idx/T, t = (s_idx+1)/T:
 * sample_p_zs_given_zt (en_diffusion.py:807-852) when target_w == NULL, else
 * sample_p_zs_given_zt_guidance (:854-935) for the target  T(pred) = target_w . pred  scaled by `scale`.
 * eps_raw [B,N,3+F] are the raw N(0,1) draws (x part first). */
int gaudi_step(gaudi_handle* h, int B, int N, int s_idx, const float* z_t, const float* node_mask,
               const float* edge_mask, const float* eps_raw, const float* target_w /* [K] or NULL */,
               float scale, float* zs_out);

/* x, one_hot = sample_p_xh_given_z0(z0)  (en_diffusion.py:533-560 + unnormalize :406-415). */
int gaudi_decode(gaudi_handle* h, int B, int N, const float* z0, const float* node_mask, const float* edge_mask,
                 const float* eps_raw, float* x_out /* [B,N,3] */, float* onehot_out /* [B,N,F] */);

/* Whole chain: EnVariationalDiffusion.sample (en_diffusion.py:958-1008) when target_w == NULL, else
 * .sample_guidance (:1010-1067).  noise: NULL -> on-device Philox4x32-10 keyed by
 * (seed, sample_offset + b, draw, element) so results do not depend on how samples are sharded;
 * otherwise injected raw N(0,1) draws [T+2,B,N,3+F] (draw 0 -> z_T, 1+k -> k-th step, T+1 -> decode).
 * Shards of one logical batch must all use the batch-wide padded N (sample_guidance pads to the
 * batch max, sampling_edm.py:177): pad the masks to that N before calling. */
int gaudi_sample(gaudi_handle* h, int B, int N, const float* node_mask, const float* edge_mask, uint64_t seed,
                 int64_t sample_offset, const float* noise, float std, const float* target_w /* [K] or NULL */,
                 float scale, float* x_out /* [B,N,3] */, float* onehot_out /* [B,N,F] */,
                 float* z0_out /* [B,N,3+F] or NULL */, gaudi_diag* diag /* or NULL */);

/* ---- Chains on a chosen time grid, from the prior or from given molecules. ----
 * A grid is n_grid >= 2 strictly descending time indices g[0] > g[1] > ... > g[n_grid-1] = 0 with g[0] <= T.  Step k moves z
 * from g[k] to g[k+1] with the reference's own formulas for that pair -- sample_p_zs_given_zt(s, t) and
 * sample_p_zs_given_zt_guidance(s, t) take any s < t (en_diffusion.py:807-935); only the reference's loops fix t = s + 1 --
 * and the networks (and a callback) see t = g[k] / T.  After the last step the usual decode p(x, h | z_0) runs.
 *
 * Start: x0 == onehot0 == NULL -> the prior z_T ~ N(0, std), legal only with g[0] == T.  Otherwise both are given
 * (x0 [B,N,3] mean-free over live nodes, onehot0 [B,N,F], un-normalised as gaudi_predict_noised takes them) and the chain
 * starts from  z_{g[0]} = alpha * normalize([x0 | onehot0]) + sigma * eps  (sample_edm_t, train_cond_predictor.py:47-61),
 * computed by the first launch exactly as gaudi_predict_noised computes its z_t; zt_out [B,N,3+F] (or NULL) receives it.
 * `std` scales the prior draw only.
 *
 * Noise is keyed by TIME INDEX, not by step count: draw 0 is the start (the prior draw, or eps of the forward noising), the
 * step that lands on time index s takes draw T - s, the decode draw T + 1.  An injected buffer keeps the layout
 * [T+2,B,N,3+F] and a coarse grid reads a subset of its rows; the Philox keys (global sample index, node, draw) are those of
 * gaudi_sample.  So the unit grid T, T-1, ..., 0 reproduces gaudi_sample bit for bit, and a molecule's result does not
 * depend on sharding or packing on any grid.
 *
 * GAUDI_E_INVALID (with gaudi_last_error) for: fewer than two entries, not strictly descending, last entry != 0, g[0] > T,
 * a prior start with g[0] != T, only one of x0 / onehot0, a start from given molecules while fix_noise is set.
 * gaudi_sample_chain takes no grid: its frame rule is defined on the unit grid only. */
int gaudi_sample_grid(gaudi_handle* h, int B, int N, const float* node_mask, const float* edge_mask, uint64_t seed,
                      int64_t sample_offset, const float* noise, float std, const float* target_w /* [K] or NULL */, float scale,
                      int n_grid, const int32_t* grid, const float* x0 /* or NULL */, const float* onehot0 /* or NULL */,
                      float* x_out, float* onehot_out, float* z0_out /* or NULL */, float* zt_out /* or NULL */,
                      gaudi_diag* diag /* or NULL */);

/* ---- Value-seeking targets, per-molecule guidance, a guidance window and a guidance trace, fused. ----
 * One target per molecule b over the predictor outputs p[k], k < K:
 *   T_b(p) = sum_k w[b,k] p[k] + sum_k q[b,k] a(p[k] - c[b,k], side[b,k])^2
 *   a(d, 0) = d  (aim at the value c);  a(d, +1) = d if d > 0 else 0  (upper bound c);  a(d, -1) = d if d < 0 else 0  (lower bound c)
 * and the energy of sample_p_zs_given_zt_guidance (en_diffusion.py:899-903) is scale[b] * T_b.  The kernels seed the predictor's
 * reverse pass with  d(scale T)/dp[k] = (w + (q + q) * a) * scale  in fp32, every operation rounded on its own, in that order
 * (gaudi_host_target_seed is the same function on the host).  Each array is shared ([K]; scale: one float) or per molecule
 * ([B,K]; scale [B]) as its *_per_mol flag says; a NULL array means 0 (w, q, c, side) or 1 (scale).
 * Window: the step that STARTS at time index t is guided iff t_lo <= t <= t_hi (both 0: every step, 1..T).  Outside it the step
 * is the guided step with a zero gradient -- eps_t.nan_to_num and the final NaN scrub stay -- and the predictor is not run. */
typedef struct {
  int32_t K;                 /* must equal the predictor's number of outputs (<= 16) */
  const float* w;            /* linear weights        [K] or [B,K], or NULL */
  const float* q;            /* curvatures            [K] or [B,K], or NULL */
  const float* c;            /* centres / bounds      [K] or [B,K], or NULL */
  const int32_t* side;       /* -1 / 0 / +1           [K] or [B,K], or NULL */
  const float* scale;        /* guidance strength     [1] or [B],   or NULL */
  int32_t w_per_mol, q_per_mol, c_per_mol, side_per_mol, scale_per_mol;
  int32_t t_lo, t_hi;        /* guidance window in time indices; 0, 0 = 1..T */
} gaudi_target_spec;

/* gaudi_sample_grid with the spec in place of (target_w, scale).  grid == NULL: the unit grid T, T-1, ..., 0 (n_grid ignored).
 * trace_out (or NULL) [n_grid-1][B][K+2]: for every step in chain order and every molecule, the K predictions at (z_s, t), the
 * 2-norm of the gradient before the clip, and the clip coefficient min(1, 10 / (norm + 1e-6)) (en_diffusion.py:905-909); rows of
 * steps outside the window are zero.  Noise keys, sample_offset, fix_noise, grids and seeded starts as in gaudi_sample_grid.
 * Every molecule runs alone in its workgroup (no packed or wide groups: a shared workgroup has one readout and one seed), so
 * molecule i's result depends on molecule i's parameters only, bit for bit, and equals gaudi_sample_cb with the same
 * dT/dpred bit for bit.  GAUDI_E_INVALID (with gaudi_last_error) for: K mismatch, a side outside {-1, 0, 1}, a window outside
 * 1..T or empty, a non-finite parameter, and what gaudi_sample_grid refuses. */
int gaudi_sample_target(gaudi_handle* h, int B, int N, const float* node_mask, const float* edge_mask, uint64_t seed,
                        int64_t sample_offset, const float* noise, float std, const gaudi_target_spec* spec, int n_grid,
                        const int32_t* grid /* or NULL */, const float* x0 /* or NULL */, const float* onehot0 /* or NULL */,
                        float* x_out, float* onehot_out, float* z0_out /* or NULL */, float* zt_out /* or NULL */,
                        float* trace_out /* or NULL */, gaudi_diag* diag /* or NULL */);
/* gaudi_step_pair with the spec; trace_out (or NULL) [B][K+2] = the step's trace row. */
int gaudi_step_target(gaudi_handle* h, int B, int N, int s_idx, int t_idx, const float* z_t, const float* node_mask,
                      const float* edge_mask, const float* eps_raw, const gaudi_target_spec* spec, float* zs_out,
                      float* trace_out /* or NULL */);
/* The seed the kernels compute, on the host (no device): out [B,K] = d(scale_b T_b)/dp at pred [B,K].  GAUDI_E_INVALID for a
 * spec whose K differs, a side outside {-1, 0, 1} or a non-finite parameter. */
int gaudi_host_target_seed(const gaudi_target_spec* spec, int B, int K, const float* pred, float* out);

/* One teacher-forced step z_t -> z_s for ANY pair 0 <= s_idx < t_idx <= T (gaudi_step is t_idx = s_idx + 1, bit for bit).
 * eps_raw stands for raw draw T - s_idx. */
int gaudi_step_pair(gaudi_handle* h, int B, int N, int s_idx, int t_idx, const float* z_t, const float* node_mask,
                    const float* edge_mask, const float* eps_raw, const float* target_w /* [K] or NULL */, float scale,
                    float* zs_out);

/* The step table of a grid, as the chains above build it per call: coef_out [n_grid-1][4], row k = (alpha_t|s,
 * sigma2_t|s / alpha_t|s / sigma_t, sigma, t) of step g[k] -> g[k+1]; land_out [n_grid-1] (or NULL) the time index each
 * step lands on.  Same float operations as gaudi_host_schedule's [T][4] table: on the unit grid row k equals that table's
 * row T-1-k bit for bit.  Needs no device.  GAUDI_E_INVALID for a malformed grid. */
int gaudi_host_grid_coefficients(int T, float noise_power /* 0 = cosine */, float noise_precision, int n_grid,
                                 const int32_t* grid, float* coef_out, int32_t* land_out);

/* sample_guidance for an ARBITRARY differentiable target T(pred, t) (the reference accepts any closure over the
 * predictor, generation_guidance.py:187-205).  Each reverse step runs in two launches: (A) denoise + predictor forward,
 * (B) predictor reverse pass + guidance update; in between, target_grad receives pred [B,K] and t and must write
 * dT/dpred [B,K] (the energy is scale * sum_b T(pred_b), en_diffusion.py:899).  Both networks stay on the device;
 * only the K-vector per molecule crosses the boundary (pinned host buffers, one event wait per step).  With target_grad
 * returning a constant w this equals gaudi_sample(target_w = w) bit for bit.  Molecules beyond the LDS limit (the V4G
 * kernels: node buffers in global memory) run phase A as two launches -- the reference has no size cap,
 * sampling_edm.py:172-209 -- so a step there is three launches. */
typedef void (*gaudi_target_cb)(void* user, int B, int K, const float* pred, float t, float* dT_dpred_out);
int gaudi_sample_cb(gaudi_handle* h, int B, int N, const float* node_mask, const float* edge_mask, uint64_t seed,
                    int64_t sample_offset, const float* noise, float std, gaudi_target_cb target_grad, void* user,
                    float scale, float* x_out, float* onehot_out, float* z0_out, gaudi_diag* diag);

/* The same for a target that ALSO depends on z outside the predictor -- the reference differentiates any function of z_s
 * (autograd at en_diffusion.py:899-903).  Between the two phases the callback receives z_s [B,N,D] (D = 3 + F, before the
 * guidance update) beside pred and t and writes dT/dpred [B,K] and the DIRECT part dT/dz [B,N,D] (pred held fixed); the
 * library scales it, masks it with node_mask (the reference asserts that the coordinate gradient of masked nodes is zero,
 * utils.py:33-44) and adds it to the reverse pass's gradient before the clip (en_diffusion.py:905-909). */
typedef void (*gaudi_target_cbz)(void* user, int B, int N, int D, int K, const float* z_s, const float* pred, float t,
                                 float* dT_dpred_out, float* dT_dz_out);
int gaudi_sample_cbz(gaudi_handle* h, int B, int N, const float* node_mask, const float* edge_mask, uint64_t seed,
                     int64_t sample_offset, const float* noise, float std, gaudi_target_cbz target_grad, void* user,
                     float scale, float* x_out, float* onehot_out, float* z0_out, gaudi_diag* diag);

/* gaudi_sample_cb / gaudi_sample_cbz on a time grid (see gaudi_sample_grid for the grid, the start and the noise keying):
 * exactly one of target_grad / target_grad_z is set; the callback receives t = g[k] / T. */
int gaudi_sample_cb_grid(gaudi_handle* h, int B, int N, const float* node_mask, const float* edge_mask, uint64_t seed,
                         int64_t sample_offset, const float* noise, float std, gaudi_target_cb target_grad,
                         gaudi_target_cbz target_grad_z, void* user, float scale, int n_grid, const int32_t* grid,
                         const float* x0, const float* onehot0, float* x_out, float* onehot_out, float* z0_out, float* zt_out,
                         gaudi_diag* diag);

/* EnVariationalDiffusion.sample_chain (en_diffusion.py:1118-1174): the unguided chain with `keep_frames`
 * intermediate states: chain_out [keep_frames,B,N,3+F], frame (s*keep_frames)//T = unnormalize_z(z_s) of the last
 * step s mapping to it, frame 0 = the final [x | one_hot].  (The reference returns the same data viewed as
 * [keep_frames*B, N, 3+F].) */
int gaudi_sample_chain(gaudi_handle* h, int B, int N, const float* node_mask, const float* edge_mask, uint64_t seed,
                       int64_t sample_offset, const float* noise, float std, int keep_frames, float* chain_out);

/* ---- Graph-of-rings stability check: the step that follows sampling (eval_validity.py:49, sampling_edm.py:96). ----
 * Geometry tables of one dataset, indexed by ring-type index (= class index of the one-hot node features,
 * data/aromatic_dataloader.py:31-35).  Raw values of utils/helpers.py:11-157 in double; the library applies `tol`
 * as the reference does ((1 - tol) on lower, (1 + tol) on upper bounds, then fp32). */
typedef struct {
  int32_t n_types;          /* len(RINGS_LIST[dataset]) <= 16                                               */
  int32_t orientation;      /* 1 if dataset != "cata": nodes [n/2, n) are orientation nodes of type n_types-1 */
  int32_t check_dihedrals;  /* 0 for "hetro" (check_angels4 returns True, analyze/analyze.py:40)              */
  double tol;               /* 0.1 in every reference call                                                    */
  double min_dist;          /* min over ring_distances[dataset] of the lower bound                            */
  double dist_lo[16][16], dist_hi[16][16]; /* ring_distances window of the type pair; hi == 0: never bonded   */
  int32_t a3_count[16];     /* number of 3-ring angle windows of the centre type (<= 4)                       */
  double a3_lo[16][4], a3_hi[16][4];       /* angels3_dict[dataset][type]                                     */
  double a4_0, a4_180;      /* angels4_dict[dataset]                                                          */
} gaudi_ring_tables;

typedef struct {
  int32_t n_rings;       /* rings tested (orientation nodes excluded)              */
  int32_t n_edges;       /* bonded ring pairs                                      */
  int32_t n_triplets;    /* de-duplicated 3-ring paths the reference enumerates    */
  int32_t n_nan_angles;  /* 3-ring angles that came out NaN (acos of 1 + 1 ulp)    */
  float a3_min, a3_max;  /* range of the 3-ring angles (degrees; +-inf when none)  */
  float a4_min, a4_max;  /* range of the 4-ring dihedrals tested                   */
} gaudi_stability_aux;

/* check_stability (analyze/analyze.py:50-100) for B molecules at once: x [B,N,3] and ring_type [B,N] hold each
 * molecule's n_nodes[b] valid nodes first (the reference compacts with node_mask before the call).
 * flags_out [B,5] = {orientation_nodes, dist_stable, connected, angels3, angels4}; a molecule is stable when all
 * five are 1.  Optional outputs: dist_out / adj_out [B,N,N] = positions2adj (utils/helpers.py:167-190) of the ring
 * block, zero elsewhere; aux_out [B]. */
int gaudi_check_stability(gaudi_handle* h, const gaudi_ring_tables* tables, int B, int N, const float* x,
                          const int32_t* ring_type, const int32_t* n_nodes, uint8_t* flags_out,
                          float* dist_out /* or NULL */, float* adj_out /* or NULL */,
                          gaudi_stability_aux* aux_out /* or NULL */);
/* Number of stability-kernel launches since gaudi_profile_reset(h, 1) and their summed duration (HIP events). */
int gaudi_stability_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms);

/* ---- Graph of rings -> graph of atoms: data/gor2goa.py:133-261 (gor2goa) for B molecules in one launch. ----
 * Constants of the conversion for one dataset, indexed by ring-type index as gaudi_ring_tables: the 2-D ring templates
 * (data/gor2goa.py:18-51), the elements of the ring atoms (RINGS_DICT, data/ring.py:6-18) as indices into ATOMS_LIST[dataset]
 * (data/aromatic_dataloader.py:26-30), and the per-type rules written out in gor2goa's body. */
#define GAUDI_ATOMS_MAX_ATOMS 384  /* 32 rings x (6 ring atoms + 2 template H + 4 placed H) */
#define GAUDI_ATOMS_MAX_BONDS 384
typedef struct {
  int32_t n_types;                 /* as gaudi_ring_tables.n_types                                                   */
  int32_t ring_size[16];           /* ring atoms of the type: 4, 5 or 6; 0 = not a ring (the orientation type ".")   */
  int32_t ring_elem[16][6];        /* element of ring atom k, index into ATOMS_LIST[dataset]                         */
  double templ[16][6][2];          /* template position of ring atom k around the ring centre (Angstrom)             */
  int32_t no_orientation[16];      /* 1: NO_ORIENTATION_RINGS -- turned towards the lowest-index fused ring           */
  double extra_angle[16];          /* added to that angle: pi/6 for Bn, pi/4 for Cbd (gor2goa.py:161-164)             */
  int32_t n_template_h[16];        /* template H's of the type: Bl / Pl 1, DhDb 2 (gor2goa.py:189-198)                */
  int32_t template_h_parent[16][2];/* ring atom each of them is bonded to                                             */
  int32_t h_elem, c_elem;          /* ATOMS_LIST[dataset].index("H") / .index("C")                                   */
  double h_bond;                   /* X-H distance of place_hydrogens (Angstrom); no reference counterpart           */
} gaudi_atom_tables;

#define GAUDI_ATOMS_PLACE_H 1      /* flags of gaudi_rings_to_atoms */
#define GAUDI_ATOMS_FINGERPRINT 2
/* status_out codes: 0 = built; otherwise the reference raises for this input and the molecule has n_atoms = n_bonds = 0. */
#define GAUDI_ATOMS_BUILT 0
#define GAUDI_ATOMS_NO_NEIGHBOUR 1 /* a NO_ORIENTATION ring without a fused ring in a multi-ring molecule (nonzero()[0, 0])      */
#define GAUDI_ATOMS_BAD_TYPE 2     /* the orientation type "." or a type outside the table among the rings (KeyError / IndexError) */
#define GAUDI_ATOMS_NO_RINGS 3     /* no ring at all: a lone orientation node (np.stack of an empty list)                          */
#define GAUDI_ATOMS_OVERFLOW 4     /* NOT a reference error: more than max_atoms / max_bonds results, more than 96 fused pairs or
                                      more than 256 atoms before hydrogens are placed                                              */

/* x [B,N,3], ring_type [B,N], n_nodes [B] as gaudi_check_stability takes them (`tables` gives the fused pairs: the same
 * positions2adj, bit for bit).  One 64-lane wave per molecule restates gor2goa in the reference's order of operations and
 * ATOM ORDER (bonds are index pairs): align_to_xy_plane (inertia tensor about the origin over all nodes, "centre of mass" = sum / 3,
 * eigenvectors of the symmetric 3 x 3 in ascending-eigenvalue order WITH THE SIGNS numpy.linalg.eigh returns -- the atom order
 * depends on them, so the kernel restates LAPACK's dsyevd path for n = 3, see gaudi_host_eigh3), ring templates
 * turned towards the orientation node or the lowest-index fused ring, template H's at the origin, per fused pair (np.triu order)
 * the closest ring atom to the centre-to-centre segment on either side (the `> 0` / `< 0` masks, first minimum), merged into
 * midpoint atoms appended at the end, originals deleted, bonds renumbered and de-duplicated.  Geometry in double.
 * A hetero molecule with an odd node count is built as the reference builds it: n // 2 rings, node n // 2 + i orients ring i.
 * Outputs, rows of max_atoms <= GAUDI_ATOMS_MAX_ATOMS / max_bonds <= GAUDI_ATOMS_MAX_BONDS entries per molecule:
 *   n_atoms_out [B], atom_type_out [B][max_atoms] (index into ATOMS_LIST[dataset]);
 *   xy_out [B][max_atoms][2]: the aligned frame, what the reference returns;
 *   xyz_out [B][max_atoms][3]: the same points in the input frame, sum / 3 + E[:, :2] . xy;
 *   n_bonds_out [B], bonds_out [B][max_bonds][2]: each pair i <= j, the list sorted; status_out [B];
 *   fingerprint_out [B] (needed with GAUDI_ATOMS_FINGERPRINT, else may be NULL).
 * GAUDI_ATOMS_PLACE_H: every template H moves from the origin to h_bond from its ring atom, on the outward direction
 * -(sum of unit vectors to the heavy neighbours) in the molecular plane, and every carbon with two heavy neighbours gets an H by
 * the same construction (the reference adds those without coordinates, build_molecule_aromatic, gor2goa.py:288-293); the added
 * H's follow all other atoms in ascending parent index.
 * GAUDI_ATOMS_FINGERPRINT: a 64-bit key of the heavy-atom graph, equal for isomorphic molecules (stands in for the InChI of
 * analyze_rdkit_validity_for_molecules, analyze/analyze.py:180-231): initial colour (element, heavy degree, attached H count
 * with the H of a two-neighbour carbon counted whether placed or not, histogram of shortest-path lengths to the other heavy
 * atoms), Weisfeiler-Lehman rounds until the number of colour classes stops growing, hash of the colour multiset and the
 * counts.  Integer arithmetic only.  Equal keys do not prove isomorphism.  0 for a molecule that was not built.
 * GAUDI_E_CAPACITY for more than 32 rings in one molecule. */
int gaudi_rings_to_atoms(gaudi_handle* h, const gaudi_ring_tables* tables, const gaudi_atom_tables* atom_tables, int B, int N,
                         const float* x, const int32_t* ring_type, const int32_t* n_nodes, int flags, int max_atoms,
                         int max_bonds, int32_t* n_atoms_out, int32_t* atom_type_out, double* xy_out, double* xyz_out,
                         int32_t* n_bonds_out, int32_t* bonds_out, int32_t* status_out, uint64_t* fingerprint_out);

/* Number of gaudi_rings_to_atoms launches since gaudi_profile_reset(h, 1) and their summed duration (HIP events). */
int gaudi_atoms_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms);

/* ---- Graph of atoms -> graph of rings: the inverse of gaudi_rings_to_atoms, for B molecules in one launch. ----
 * What data/aromatic_dataloader.py:131-152 (AromaticDataset.get_rings) computes per molecule in Python: bonds from covalent radii
 * (utils/molgraph.py:37-80), the rings, their types, centres and orientation candidates (utils/ring_graph.py:12-93) and the
 * ring-ring adjacency (:120-128).  Constants for one dataset: */
#define GAUDI_RINGS_MAX_ATOMS 384  /* atoms of one molecule: everything gaudi_rings_to_atoms can emit fits */
#define GAUDI_RINGS_MAX_HEAVY 192  /* non-hydrogen atoms */
#define GAUDI_RINGS_MAX_RINGS 32
typedef struct {
  int32_t n_elems;                 /* len(ATOMS_LIST[dataset]) <= 8                                                    */
  double cov_radius[8];            /* covalent radius of each element (utils/const.py), Angstrom                       */
  int32_t h_elem, c_elem, b_elem;  /* ATOMS_LIST[dataset].index("H") / ("C") / ("B"); b_elem = -1 where there is no B  */
  int32_t n_types;                 /* len(RINGS_LIST[dataset]) <= 16                                                   */
  int32_t ring_size[16];           /* ring atoms of the type: 4, 5 or 6; 0 = not a ring (".")                          */
  int32_t ring_elem[16][6];        /* its elements (RINGS_DICT) as indices into ATOMS_LIST[dataset], in any order       */
  int32_t no_orientation[16];      /* 1: NO_ORIENTATION_RINGS -- the orientation candidate is the centre itself         */
  int32_t db_type, dhdb_type;      /* the two types that share CCBCCB, told apart by the H on B; -1 / -1 where absent   */
} gaudi_perception_tables;

#define GAUDI_RINGS_USE_H 1        /* flag: hydrogens count when Db / DhDb is decided (skip_hydrogen=False); default: they
                                      take no part at all (the dataset path, skip_hydrogen=True), and CCBCCB is Db      */
/* status_out codes: 0 = perceived; otherwise the molecule has n_rings = 0. */
#define GAUDI_RINGS_OK 0
#define GAUDI_RINGS_NO_RINGS 1     /* no heavy atom, or a heavy-atom graph without a cycle                                        */
#define GAUDI_RINGS_BAD_TYPE 2     /* a ring whose element multiset is no ring type of the dataset (NotImplementedError / ValueError) */
#define GAUDI_RINGS_NOT_A_BASIS 3  /* the chordless cycles of 4..6 atoms are not THE minimum cycle basis: the reference's answer
                                      depends on networkx's tie-breaking or holds a ring it cannot type                           */
#define GAUDI_RINGS_OVERFLOW 4     /* NOT a reference error: more than 384 atoms, 192 heavy atoms or max_rings rings              */

/* xyz [B][A][3] float64, elem [B][A] (indices into ATOMS_LIST[dataset]), n_atoms [B] in 0..A.  One 64-lane wave per molecule:
 *  - heavy atoms i < j are bonded iff sqrt(dx^2 + dy^2 + dz^2) <= (r_i + r_j) * covalency_factor, in float64 without contraction;
 *    the adjacency is kept as bit rows, so a heavy atom may have any number of neighbours;
 *  - the rings are the chordless cycles of 4 to 6 heavy atoms.  There must be no triangle, they must number E - V + C
 *    (C = components) and be independent over GF(2); then every minimum cycle basis consists of exactly these cycles, and networkx.minimum_cycle_basis returns them as
 *    a set.  Otherwise GAUDI_RINGS_NOT_A_BASIS;
 *  - rings are ordered ascending by their sorted tuple of atom indices (the reference's order is networkx's);
 *  - type: the first type of RINGS_LIST[dataset] with the ring's element multiset; CCBCCB is Db, and DhDb only with
 *    GAUDI_RINGS_USE_H when a B atom of the ring has an H within (r_B + r_H) * covalency_factor.  (The reference looks at the
 *    first B in networkx's cycle order only.)
 * Outputs, rows of max_rings <= GAUDI_RINGS_MAX_RINGS entries per molecule, zero beyond n_rings:
 *   status_out [B], n_rings_out [B], ring_size_out [B][max_rings], ring_type_out [B][max_rings];
 *   ring_atoms_out [B][max_rings][6]: atom indices ascending, padded with -1 (all -1 beyond n_rings);
 *   centre_out [B][max_rings][3]: the float64 mean of the ring atoms, summed in ascending atom index;
 *   n_orient_out [B][max_rings], orient_out [B][max_rings][2][3]: the centre for a NO_ORIENTATION type, otherwise the
 *     coordinates of the ring's non-carbon atoms in ascending index (at most 2);
 *   adj_out [B][max_rings][max_rings]: 1 where two different rings share an atom (get_rings_adj).
 * A molecule that fails never disturbs the others of the batch. */
int gaudi_atoms_to_rings(gaudi_handle* h, const gaudi_perception_tables* tables, int B, int A, const double* xyz,
                         const int32_t* elem, const int32_t* n_atoms, int flags, double covalency_factor, int max_rings,
                         int32_t* status_out, int32_t* n_rings_out, int32_t* ring_size_out, int32_t* ring_atoms_out,
                         int32_t* ring_type_out, double* centre_out, int32_t* n_orient_out, double* orient_out, uint8_t* adj_out);
/* Number of gaudi_atoms_to_rings launches since gaudi_profile_reset(h, 1) and their summed duration (HIP events). */
int gaudi_rings_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms);

/* ---- Bond orders and formal charges of a graph of atoms, for B molecules in one launch. ----
 * What the reference asks of xyz2mol.AC2BO inside rdkit_valid (data/gor2goa.py:298-324, data/xyz2mol.py:538-634), as a rule of
 * this library's own (the reference's answer depends on the atom numbering): an atom's sigma degree d is its number of bonds,
 * one more for a carbon with exactly two (the H build_molecule_aromatic adds); its options are the (added bonds, formal charge)
 * pairs of its (element, d) below; a molecule is valid when its bond graph is connected, every atom has an option, and one option
 * per atom can be chosen such that the charges sum to zero and the atoms that add a bond have a perfect matching among themselves
 * -- the double bonds.  Returned: such a structure with the fewest charged atoms. */
#define GAUDI_BONDS_MAX_ATOMS 384  /* as GAUDI_RINGS_MAX_ATOMS / _MAX_HEAVY: everything gaudi_rings_to_atoms emits fits */
#define GAUDI_BONDS_MAX_HEAVY 192
#define GAUDI_BONDS_MAX_BONDS 384
#define GAUDI_BONDS_MAX_CHARGED 4     /* a returned structure has at most this many charged atoms */
#define GAUDI_BONDS_SEARCH_CHARGED 6  /* ... and whether one exists at all is searched up to this many */
typedef struct {
  int32_t n_elems;                 /* len(ATOMS_LIST[dataset]) <= 8                                                       */
  int32_t n_options[8][5];         /* options of (element, sigma degree 0..4): 0, 1 or 2; a degree above 4 has none      */
  int32_t option[8][5][2][2];      /* (added bonds 0 / 1, formal charge); of two, the first is neutral, the second charged */
  int32_t h_elem, c_elem;          /* ATOMS_LIST[dataset].index("H") / .index("C")                                      */
} gaudi_valence_tables;
/* status_out codes; anything but OK leaves the molecule's orders, charges and n_charged zero. */
#define GAUDI_BONDS_OK 0
#define GAUDI_BONDS_NO_STRUCTURE 1   /* no choice of options works with up to GAUDI_BONDS_SEARCH_CHARGED charged atoms (a proof
                                        that none exists whenever fewer than 7 atoms can carry a charge at all)                 */
#define GAUDI_BONDS_CAPPED 2         /* none within GAUDI_BONDS_MAX_CHARGED, but one with 5 or 6 charged atoms exists             */
#define GAUDI_BONDS_NOT_CONNECTED 3
#define GAUDI_BONDS_BAD_VALENCE 4    /* an atom without an option, e.g. a carbon with five bonds                               */
#define GAUDI_BONDS_BAD_INPUT 5      /* a bond index outside 0..n_atoms-1, a bond from an atom to itself or listed twice, an
                                        element outside the table                                                              */
#define GAUDI_BONDS_OVERFLOW 6       /* more than 384 atoms, 192 non-hydrogen atoms or 384 bonds                               */
#define GAUDI_BONDS_EMPTY 7          /* n_atoms = 0: what a molecule gaudi_rings_to_atoms did not build looks like             */
#define GAUDI_BONDS_GAVE_UP 8        /* undecided: one subset size of the atoms with two options would have taken more than 16 384
                                        subsets (pruned ones included).  A structure within the cap may exist, and this status --
                                        unlike every other, and unlike n_charged -- can depend on the atom numbering: another
                                        numbering may reach a structure first.  It cannot occur within the cap with at most 25
                                        two-option atoms (sizes 1..4 are then at most 15 275 subsets); with 26 it can           */
/* elem [B][A] (indices into ATOMS_LIST[dataset]), n_atoms [B] in 0..A, bonds [B][M][2], n_bonds [B] in 0..M, as
 * gaudi_rings_to_atoms returns them, with or without placed hydrogens.  One 64-lane wave per molecule, integer arithmetic only.
 * order_out [B][M]: 1 or 2 for every listed bond; charge_out [B][A]; n_charged_out [B] = atoms with a nonzero charge;
 * status_out [B].  Which of several structures with equally few charges comes back is a function of the molecule's own arrays
 * (never of its place in the batch), and bit for bit what gaudi_host_bond_orders returns.  A molecule that fails never disturbs
 * the others of the batch. */
int gaudi_bond_orders(gaudi_handle* h, const gaudi_valence_tables* tables, int B, int A, int M, const int32_t* elem,
                      const int32_t* n_atoms, const int32_t* bonds, const int32_t* n_bonds, uint8_t* order_out,
                      int8_t* charge_out, int32_t* n_charged_out, int32_t* status_out);
/* Number of gaudi_bond_orders launches since gaudi_profile_reset(h, 1) and their summed duration (HIP events). */
int gaudi_bonds_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms);

/* ---- Canonical numbering of a graph of atoms, for B molecules in one launch. ----
 * The identity of a built molecule that does not depend on its atom numbering (what the reference takes from the InChI string,
 * analyze/analyze.py:180-231).  The labelled graph: vertices = the non-hydrogen atoms; vertex label = element * 8 + H count, the
 * H count being the listed H neighbours plus one for a carbon with exactly two bonds (the H build_molecule_aromatic adds), so a
 * molecule has the same graph with and without placed hydrogens; edges = the bonds between non-hydrogen atoms, unlabelled (bond
 * orders and formal charges belong to one resonance structure, not to the molecule).  The code of a numbering is n_heavy, the
 * labels in rank order and the edges as sorted (lo, hi) pairs of ranks; the canonical numbering is the one with the
 * lexicographically smallest code over the leaves of an individualisation-refinement search (csrc/canon.inc, DESIGN.md section
 * 8i).  Two molecules get equal codes if and only if their labelled graphs are isomorphic. */
#define GAUDI_CANON_MAX_ATOMS 384   /* as GAUDI_BONDS_MAX_*: everything gaudi_rings_to_atoms emits fits */
#define GAUDI_CANON_MAX_HEAVY 192
#define GAUDI_CANON_MAX_BONDS 384
#define GAUDI_CANON_MAX_DEGREE 8    /* bonds of one atom */
#define GAUDI_CANON_MAX_NODES 4096  /* search-tree nodes per molecule; one node = one refinement to an equitable colouring */
#define GAUDI_CANON_MAX_DEPTH 16    /* individualisations on one path of the tree */
/* status_out codes; BAD_INPUT, OVERFLOW and EMPTY leave every output of the molecule zero. */
#define GAUDI_CANON_OK 0
#define GAUDI_CANON_GAVE_UP 1    /* the tree has more than GAUDI_CANON_MAX_NODES nodes or a path deeper than GAUDI_CANON_MAX_DEPTH
                                    (many identical disconnected pieces: three benzenes need 16 903 nodes).  The outputs are a
                                    valid numbering and its code, but NOT canonical: they may differ under renumbering */
#define GAUDI_CANON_BAD_INPUT 2  /* as GAUDI_BONDS_BAD_INPUT: a bond index outside 0..n_atoms-1, a bond from an atom to itself or
                                    listed twice, an element outside 0..n_elems-1                                            */
#define GAUDI_CANON_OVERFLOW 3   /* more than 384 atoms, 192 non-hydrogen atoms or 384 bonds; an atom with more than 8 bonds or a
                                    non-hydrogen atom with more than 7 hydrogens                                             */
#define GAUDI_CANON_EMPTY 4      /* n_atoms = 0: what a molecule gaudi_rings_to_atoms did not build looks like                */
/* Inputs as gaudi_bond_orders takes them; n_elems = len(ATOMS_LIST[dataset]) <= 8, h_elem / c_elem = the indices of H and C.
 * One 64-lane wave per molecule, integer arithmetic only, one launch.  rank_out [B][A]: the canonical index of a non-hydrogen
 * atom, -1 for hydrogens and padding; n_heavy_out [B]; label_out [B][A]: element * 8 + H count in rank order; n_hbonds_out [B]:
 * bonds between non-hydrogen atoms; cbonds_out [B][M][2]: those bonds as (lo, hi) rank pairs, sorted; nodes_out [B]: search-tree
 * nodes spent; status_out [B].  The outputs are a function of the molecule's own arrays (never of its place in the batch) and
 * bit for bit what gaudi_host_canonical_order returns.  A molecule that fails never disturbs the others of the batch. */
int gaudi_canonical_order(gaudi_handle* h, int n_elems, int h_elem, int c_elem, int B, int A, int M, const int32_t* elem,
                          const int32_t* n_atoms, const int32_t* bonds, const int32_t* n_bonds, int32_t* rank_out,
                          int32_t* n_heavy_out, uint8_t* label_out, int32_t* n_hbonds_out, uint16_t* cbonds_out,
                          int32_t* nodes_out, int32_t* status_out);
/* Number of gaudi_canonical_order launches since gaudi_profile_reset(h, 1) and their summed duration (HIP events). */
int gaudi_canon_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms);

/* ---- Circular count fingerprints and their similarity (csrc/fp.inc). ----
 * How ALIKE two built molecules are, where the canonical code says whether they are the same.  The graph is the one of
 * gaudi_canonical_order: label(v) = element * 8 + H count, deg(v) = non-hydrogen neighbours; bond orders are no part of it, and a
 * molecule has the same fingerprint with and without placed hydrogens.  With uint32_t arithmetic that wraps and
 *   mix(x):  x ^= x >> 16;  x *= 0x85ebca6b;  x ^= x >> 13;  x *= 0xc2b2ae35;  x ^= x >> 16
 *   id_0(v) = mix(0x9e3779b9 + label(v) * 16 + deg(v))
 *   id_r(v), r = 1..radius:  h = mix(r);  h = mix(h ^ id_{r-1}(v));  for the neighbours' id_{r-1} in ascending order: h = mix(h ^ id)
 * the features are the multiset { id_r(v) : v, r = 0..radius }, fp[bin] = min(255, features with (id & (n_bins - 1)) == bin) and
 * total = the sum of the stored bytes.  radius 0..3, n_bins 256, 512 or 1024 (GAUDI_E_INVALID otherwise).  Inputs as
 * gaudi_canonical_order takes them; one 64-lane wave per molecule, integer arithmetic only, one launch.  fp_out [B][n_bins],
 * total_out [B], status_out [B]: GAUDI_CANON_OK, or GAUDI_CANON_BAD_INPUT / OVERFLOW / EMPTY with their meaning there, a zero row
 * and total 0.  The outputs are a function of the molecule's own arrays (never of its place in the batch) and bit for bit what
 * gaudi_host_circular_fingerprint returns.  A molecule that fails never disturbs the others of the batch. */
int gaudi_circular_fingerprint(gaudi_handle* h, int n_elems, int h_elem, int c_elem, int B, int A, int M, const int32_t* elem,
                               const int32_t* n_atoms, const int32_t* bonds, const int32_t* n_bonds, int radius, int n_bins,
                               uint8_t* fp_out, int32_t* total_out, int32_t* status_out);
/* Similarity of rows a, b: common = sum min(a_i, b_i), union = total_a + total_b - common, similarity = common / union, and 0 when
 * union = 0.  The entry points return the two INTEGERS; the caller forms the quotient.  The total order of library rows for one
 * query, used everywhere: x is ahead of y when common_x * union_y > common_y * union_x in 64-bit integers, a union of 0 counting
 * as similarity 0; equal similarity goes to the smaller library index.
 * gaudi_fp_library_set keeps lib [M][n_bins] on the device, replacing the previous library; M = 0 frees it. */
int gaudi_fp_library_set(gaudi_handle* h, int n_bins, int M, const uint8_t* lib);
/* The k (1..16) library rows most similar to each of the B queries q [B][n_bins], in that order.  lib [M][n_bins], or NULL for the
 * resident library (then M and n_bins must be its; GAUDI_E_STATE without one).  idx_out, common_out, union_out: each [B][k];
 * entries beyond M rows are -1, 0, 0.  The result does not depend on how the library is split over workgroups (GAUDI_FP_SPLITS,
 * read per call, forces the number of splits: a test knob) nor on the query's place in the batch, and is exactly what
 * gaudi_host_fp_nearest returns. */
int gaudi_fp_nearest(gaudi_handle* h, int n_bins, int B, const uint8_t* q, int M, const uint8_t* lib, int k, int32_t* idx_out,
                     int32_t* common_out, int32_t* union_out);
/* common_out [B][M] for every pair; B * M <= 2^28 (GAUDI_E_CAPACITY beyond).  lib as for gaudi_fp_nearest. */
int gaudi_fp_common(gaudi_handle* h, int n_bins, int B, const uint8_t* q, int M, const uint8_t* lib, int32_t* common_out);
/* Number of fingerprint / nearest / common calls since gaudi_profile_reset(h, 1) and the summed duration of their kernels (HIP
 * events; uploads and downloads are outside). */
int gaudi_fp_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms);

/* ---- Diverse subsets and Butina clusters of fingerprint batches (csrc/fp_select.inc). ----
 * Which of a batch to take on: what RDKit users get from MaxMinPicker and Butina clustering.  rows [N][n_bins] of uint8, n_bins
 * 256, 512 or 1024; total_i = the sum of row i's bytes and a row is LIVE when total_i > 0.  Rows that are not live (the refused or
 * unbuilt molecules) are never picked, never clustered, have no neighbours and are nobody's neighbour.  common and union are the
 * ones above and every comparison of two similarities is the cross product above, in 64-bit integers.  A threshold is the
 * rational thr_num / thr_den with 0 <= thr_num <= thr_den <= 65536: the pair i, j is AT LEAST THR when union_ij > 0 and
 * common_ij * thr_den >= thr_num * union_ij.  No float is compared anywhere, and every output is exactly what the gaudi_host_
 * twin of the entry point returns.  N <= 2^20 and at most 2^28 neighbour entries (GAUDI_E_CAPACITY with a message beyond); N = 0
 * is GAUDI_OK with nothing written.  The launches are counted (one by one) and timed in gaudi_fp_profile_get's log.
 *
 * gaudi_fp_neighbours: count_out [N] = for a live row i the number of live j at least thr to it, i itself included, and 0 for a
 * row that is not live; offsets_out [N + 1] = the exclusive prefix of the counts; list_out = those j, ascending, row after row
 * (CSR).  list_out may be NULL with capacity 0: counts and offsets only.  A capacity below offsets_out[N] returns
 * GAUDI_E_CAPACITY after count_out and offsets_out are written, so the caller sizes the buffer and calls again.  The batch is
 * compared with itself in splits of whole tiles as gaudi_fp_nearest does it (GAUDI_FP_SPLITS forces their number); no output
 * depends on the number of splits. */
int gaudi_fp_neighbours(gaudi_handle* h, int n_bins, int N, const uint8_t* rows, int thr_num, int thr_den, int32_t* count_out,
                        int64_t capacity, int64_t* offsets_out, int32_t* list_out);
/* Butina clustering on those lists, which stay on the device.  The rows are ordered by count descending, then index ascending; along
 * that order a live row not yet assigned becomes the centroid of the next cluster (0, 1, ...) and claims every not yet assigned
 * row of its list, itself included.  cluster_out [N]: the cluster of row i, -1 for a row that is not live.  centroid_out [N],
 * size_out [N]: by cluster number, -1 and 0 from *n_clusters_out on.  count_out [N] as above. */
int gaudi_fp_cluster(gaudi_handle* h, int n_bins, int N, const uint8_t* rows, int thr_num, int thr_den, int32_t* cluster_out,
                     int32_t* centroid_out, int32_t* size_out, int32_t* count_out, int32_t* n_clusters_out);
/* MaxMin picking of up to k rows.  seeds [S][n_bins]: rows chosen before (NULL with S > 0: the resident library of
 * gaudi_fp_library_set, which must have S rows of n_bins; a seed row of zeros has similarity 0 to every row).  Every live row i
 * carries near(i) = (common, union, owner): the most similar chosen element so far, among equally similar ones the earliest
 * chosen -- seeds in index order, then picks in pick order.  Pick t: with S = 0 and t = 0 the row `first` (-1: the live row with
 * the smallest index; out of range or not live: GAUDI_E_INVALID; `first` is read only when S = 0); otherwise the live unpicked
 * row whose near is LEAST similar, equal similarity to the smaller row index.  pick_common_out[t], pick_union_out[t] = that
 * row's near when it is picked (0, 0 for a first pick without seeds).  Picking stops after k picks, when no live unpicked row is
 * left, or -- thr_den > 0 -- when the candidate's near is at least thr already: it is not picked, and the picks cover the batch
 * at that radius.  thr_den = 0: no threshold.  After a pick every live row strictly more similar to it than to its near takes it
 * as owner, and the picked row owns itself with common = union = total.  picked_out, pick_common_out, pick_union_out: each [k],
 * -1, 0, 0 from *n_picked_out on.  owner_out [N]: the row index of the owning pick, -2 - s for seed s, -1 for a row that is not
 * live or when nothing was chosen; owner_common_out, owner_union_out [N]: its near (0, 0 with owner -1).  One launch per pick, with
 * no host synchronisation inside a chunk of 256 picks; GAUDI_FP_SPLITS forces the number of workgroups a round cuts the rows
 * into, and no output depends on it. */
int gaudi_fp_pick_diverse(gaudi_handle* h, int n_bins, int N, const uint8_t* rows, int S, const uint8_t* seeds, int first, int k,
                          int thr_num, int thr_den, int32_t* picked_out, int32_t* pick_common_out, int32_t* pick_union_out,
                          int32_t* n_picked_out, int32_t* owner_out, int32_t* owner_common_out, int32_t* owner_union_out);
/* The kernel times of the most recent of the three calls above that ran with profiling on (gaudi_profile_reset(h, 1)), by stage,
 * in milliseconds (HIP events): ms_out [8] = the COUNT pass, the offsets, the FILL pass, the sort, the walk, the set-up of a pick
 * call (the seed search, the cleared state, the round that makes no pick), all its rounds together, and fp_totals_kernel over
 * the same rows (a pick call with profiling on launches it once more as the yardstick of a round: it reads every byte once).
 * Stages the call did not run are 0.  With profiling on these calls synchronise the stream where a stage ends. */
int gaudi_fp_select_stages_get(gaudi_handle* h, double* ms_out);

/* ---- Substructure search over graphs of atoms (csrc/sub.inc). ----
 * Does a molecule contain a motif, where, and how often: what a SMARTS match without bond primitives answers.
 * Graphs, on both sides, are the one of gaudi_canonical_order: vertices = the non-hydrogen atoms; a vertex carries its element and
 * its H count (the listed H neighbours plus one for a carbon with exactly two bonds); edges = the bonds between non-hydrogen atoms,
 * unlabelled.  Bond orders and charges are no part of it.
 * A PATTERN is such a graph with 1..GAUDI_SUB_MAX_QUERY vertices, connected, given as (elem, bonds) arrays exactly as molecules
 * are (p_elem [P][QA], p_n_atoms [P], p_bonds [P][QM][2], p_n_bonds [P]).  Anything else -- empty, no non-hydrogen atom, not
 * connected, more than 32 vertices, n_atoms > QA or n_bonds > QM, a bad index or element, a self bond, a duplicate bond, more than
 * 8 bonds at an atom, an unknown flag -- gives GAUDI_SUB_BAD_PATTERN in every cell of that pattern's column (whatever the molecule
 * is) and never disturbs the other patterns.
 * Per-pattern flags p_flags [P]: GAUDI_SUB_H_EXACT -- the target vertex's H count equals the pattern vertex's; GAUDI_SUB_CLOSED --
 * the target vertex's heavy degree equals the pattern vertex's (nothing else is attached).  With neither only elements and edges
 * count.
 * An EMBEDDING is an injective map of pattern vertices to target vertices with equal elements, every pattern edge on a target edge
 * and the flags holding at every vertex: a monomorphism, not an induced subgraph.
 * Outputs per (molecule b, pattern p):
 *   count_out [B][P]: the embeddings found.
 *   first_out [B][P][QA] (or NULL: not wanted): the embedding that is lexicographically smallest when written as target ATOM indices
 *     in the pattern's own atom order; -1 at pattern hydrogens and padding, and everywhere when count is 0.
 *   covered_out [B][P][A] (or NULL): 1 for every target atom some embedding found uses.
 *   steps_out [B][P]: candidate tests spent, summed over roots, saturating at 2^31 - 1.
 *   status_out [B][P]: GAUDI_SUB_OK; GAUDI_SUB_GAVE_UP -- the budget ran out: count is a lower bound, first the smallest among
 *     those found, covered a subset, and a count of 0 means undecided; GAUDI_SUB_BAD_INPUT / OVERFLOW / EMPTY with the meaning of
 *     their GAUDI_CANON_* namesakes for the molecule; GAUDI_SUB_BAD_PATTERN.  Where the molecule or the pattern was refused the
 *     other outputs are zero and -1.
 * The budget is counted per ROOT (a target vertex tried as the image of the first pattern vertex of the match order; the test of
 * the root itself is the first step): GAUDI_SUB_MAX_STEPS candidate tests.  A root that needs more is abandoned with what it found
 * and the status becomes GAVE_UP.  The budget never depends on which lane ran the root, so the device and the host build cut a
 * search at the same step and agree bit for bit even when they give up.  The match order is fixed per pattern by host code
 * (csrc/sub.inc: sub_plan states the rule); count, first and covered do not depend on it when the status is OK.
 * One 64-lane wave per molecule, integer arithmetic only, one launch.  P <= GAUDI_SUB_MAX_PATTERNS per call and B * P * max(A, QA)
 * <= 2^31 (GAUDI_E_CAPACITY beyond).  The outputs are a function of the molecule's and the patterns' own arrays (never of the
 * molecule's place in the batch) and bit for bit what gaudi_host_substructure_search returns. */
#define GAUDI_SUB_MAX_QUERY 32      /* vertices of a pattern */
#define GAUDI_SUB_MAX_PATTERNS 64   /* patterns of one call */
#define GAUDI_SUB_MAX_STEPS 8192    /* candidate tests per root: DESIGN.md section 8k has the measurement behind it */
#define GAUDI_SUB_H_EXACT 1
#define GAUDI_SUB_CLOSED 2
#define GAUDI_SUB_OK 0
#define GAUDI_SUB_GAVE_UP 1
#define GAUDI_SUB_BAD_INPUT 2
#define GAUDI_SUB_OVERFLOW 3
#define GAUDI_SUB_EMPTY 4
#define GAUDI_SUB_BAD_PATTERN 5
int gaudi_substructure_search(gaudi_handle* h, int n_elems, int h_elem, int c_elem, int B, int A, int M, const int32_t* elem,
                              const int32_t* n_atoms, const int32_t* bonds, const int32_t* n_bonds, int P, int QA, int QM,
                              const int32_t* p_elem, const int32_t* p_n_atoms, const int32_t* p_bonds, const int32_t* p_n_bonds,
                              const int32_t* p_flags, int32_t* count_out, int32_t* first_out, uint8_t* covered_out,
                              int32_t* steps_out, int32_t* status_out);
/* Number of gaudi_substructure_search launches since gaudi_profile_reset(h, 1) and their summed duration (HIP events; uploads and
 * downloads are outside). */
int gaudi_substructure_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms);

/* ---- Hueckel molecular-orbital levels, gap, pi charges and pi bond orders (csrc/huckel.inc). ----
 * The graph is the one of gaudi_canonical_order: vertices = the non-hydrogen atoms, each with its element, its H count (the listed H
 * neighbours plus one for a carbon with exactly two bonds) and its heavy degree.  coordination = heavy degree + H count.
 * tables->site_class[element][coordination 0..4] names a site class or -1: not a pi centre (left out of the matrix, counted in
 * n_excluded; a coordination above 4 is never one).  A class has a Coulomb term h, an electron count n_e in {0, 1, 2} and a bond
 * factor k.  In units of |beta| with alpha = 0, over the pi centres in ascending atom index: M_rr = h_r and, for bonded centres,
 * M_rs = k_pair[class r][class s] where that is not NaN, else k_r * k_s.  An orbital's energy is alpha + x beta with beta < 0: the
 * larger x, the lower the level.  n_electrons = sum of n_e - charge[b] (charge NULL: all zero); levels fill from the lowest energy,
 * two to a level.
 * Outputs per molecule b:
 *   levels_out [B][GAUDI_HUCKEL_MAX_PI] fp32: x by ascending energy (descending x), zero padded; occupation_out the same shape, uint8.
 *   n_pi_out, n_electrons_out, n_excluded_out, sweeps_out (Jacobi sweeps run), flags_out, status_out: [B] int32.
 *   homo_out, lumo_out: for an even count, x of the last doubly occupied level and of the level after it; gap_out = homo - lumo in
 *     |beta| (>= 0);
 *     e_pi_out = sum of occupation * x.  An odd count leaves one singly occupied level: homo = lumo = that level, gap = 0,
 *     GAUDI_HUCKEL_OPEN_SHELL.  With no electron at all both names go to the lowest level, with no empty level both to the highest.
 *   GAUDI_HUCKEL_DEGENERATE: the last level holding an electron and the next level (which holds fewer) are closer than 1e-3: charges
 *     and bond orders are returned but not unique.
 *   pi_charge_out [B][A] fp32: n_e(r) - sum of occupation * v_r^2; zero on hydrogens and excluded atoms.
 *   pi_bond_order_out [B][M] fp32: sum of occupation * v_r * v_s per listed bond; zero on bonds not between pi centres.
 *   site_class_out [B][A] int8: -1 on hydrogens and excluded atoms.
 * status: GAUDI_HUCKEL_OK; NOT_CONVERGED -- GAUDI_HUCKEL_MAX_SWEEPS sweeps left an off-diagonal element above 2^-24 (the results are
 * what the last sweep left); BAD_INPUT / OVERFLOW / EMPTY with the meaning of their GAUDI_CANON_* namesakes, BAD_INPUT also for a
 * charge that leaves fewer than 0 or more than 2 n_pi electrons, OVERFLOW also for more than GAUDI_HUCKEL_MAX_PI pi centres; NO_PI --
 * no atom is a pi centre; BAD_TABLE -- n_classes outside 1..GAUDI_HUCKEL_MAX_CLASSES, a class index outside -1..n_classes-1, an n_e
 * outside 0..2, a non-finite h or k, or k_pair[i][j] != k_pair[j][i] (every molecule of the call gets it).  Where a molecule is
 * refused (every status but OK and NOT_CONVERGED) its rows are zero.
 * One 64-lane wave per molecule; capacity tiers of 32, 64 and 128 pi centres by the molecule's heavy-atom count, one launch per tier
 * present.  Individually rounded fp32 in a fixed order: the outputs are a function of the molecule's own arrays (never of the tier,
 * the batch or its place in it) and bit for bit what gaudi_host_huckel returns.  B * max(A, M, 128) <= 2^31. */
#define GAUDI_HUCKEL_MAX_PI 128
#define GAUDI_HUCKEL_MAX_CLASSES 16
#define GAUDI_HUCKEL_MAX_SWEEPS 30
#define GAUDI_HUCKEL_OK 0
#define GAUDI_HUCKEL_NOT_CONVERGED 1
#define GAUDI_HUCKEL_BAD_INPUT 2
#define GAUDI_HUCKEL_OVERFLOW 3
#define GAUDI_HUCKEL_EMPTY 4
#define GAUDI_HUCKEL_NO_PI 5
#define GAUDI_HUCKEL_BAD_TABLE 6
#define GAUDI_HUCKEL_OPEN_SHELL 1
#define GAUDI_HUCKEL_DEGENERATE 2
typedef struct gaudi_huckel_tables {
  int32_t n_elems, h_elem, c_elem; /* the element list of the call's elem arrays; which entries are H and C */
  int32_t n_classes;
  int32_t site_class[8][5];        /* [element][coordination] -> class, -1: not a pi centre */
  float h[GAUDI_HUCKEL_MAX_CLASSES];
  int32_t n_e[GAUDI_HUCKEL_MAX_CLASSES];
  float k[GAUDI_HUCKEL_MAX_CLASSES];
  float k_pair[GAUDI_HUCKEL_MAX_CLASSES][GAUDI_HUCKEL_MAX_CLASSES]; /* NaN: use k[i] * k[j] */
} gaudi_huckel_tables;
int gaudi_huckel(gaudi_handle* h, const gaudi_huckel_tables* tables, int B, int A, int M, const int32_t* elem,
                 const int32_t* n_atoms, const int32_t* bonds, const int32_t* n_bonds, const int32_t* charge, float* levels_out,
                 uint8_t* occupation_out, int32_t* n_pi_out, int32_t* n_electrons_out, int32_t* n_excluded_out,
                 int32_t* sweeps_out, int32_t* flags_out, int32_t* status_out, float* homo_out, float* lumo_out, float* gap_out,
                 float* e_pi_out, float* pi_charge_out, float* pi_bond_order_out, int8_t* site_class_out);
/* gaudi_huckel without a handle: the same source text (csrc/huckel.inc: huckel_molecule) compiled for the host and run serially.
 * Test surface for the CPU suite, not a CPU fallback: gaudi_amd never calls it on its own. */
int gaudi_host_huckel(const gaudi_huckel_tables* tables, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                      const int32_t* bonds, const int32_t* n_bonds, const int32_t* charge, float* levels_out,
                      uint8_t* occupation_out, int32_t* n_pi_out, int32_t* n_electrons_out, int32_t* n_excluded_out,
                      int32_t* sweeps_out, int32_t* flags_out, int32_t* status_out, float* homo_out, float* lumo_out,
                      float* gap_out, float* e_pi_out, float* pi_charge_out, float* pi_bond_order_out, int8_t* site_class_out);
/* Number of gaudi_huckel launches (one per capacity tier present in a call) since gaudi_profile_reset(h, 1) and their summed
 * duration (HIP events; uploads and downloads are outside). */
int gaudi_huckel_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms);

/* ---- Pariser-Parr-Pople self-consistent pi levels, gap and charges in eV (csrc/ppp.inc). ----
 * The pi centres are those of gaudi_huckel: the same graph, the same coordination rule, tables->site_class as there.  A class has a
 * valence-state ionisation energy I (eV), a one-centre repulsion gamma (eV, > 0), a core charge z in {0, 1, 2} (the electrons it
 * contributes) and a bond factor k.  Over the pi centres in ascending atom index, with xyz [B][A][3] fp32 in Angstrom:
 *   beta_rs  = beta_pair[class r][class s] where that is not NaN, else beta0 * k_r * k_s, for bonded centres; 0 otherwise
 *   gamma_rr = gamma_r;  a_rs = 2 * 14.397 / (gamma_r + gamma_s);  d2 = (dx * dx + dy * dy) + dz * dz
 *   gamma_rs = 14.397 / (sqrt(d2) + a_rs)        repulsion = GAUDI_PPP_MATAGA_NISHIMOTO
 *            = 14.397 / sqrt(d2 + a_rs * a_rs)   repulsion = GAUDI_PPP_OHNO
 *   F_rr = -I_r + 1/2 P_rr gamma_rr + sum over s != r of (P_ss - z_s) gamma_rs;   F_rs = beta_rs - 1/2 P_rs gamma_rs
 *   H_rr = -I_r - sum over s != r of z_s gamma_rs;   H_rs = beta_rs
 * Closed shell: n_electrons = sum of z - charge[b] (charge NULL: all zero) must be even.  P starts as diag(z).  One iteration
 * builds F(P), diagonalises it (the Jacobi routine of gaudi_huckel, its threshold 2^-24 times the largest |F_rr| of the first F
 * rounded up to a power of two), ranks the levels by counting (ties: the smaller index first), fills the lowest n_electrons / 2,
 * forms P_new = 2 sum over the occupied v v^T and delta_p = max |P_new - P|, and stops when delta_p <= 2^-16; otherwise
 * P = (1 - damping) * P_new + damping * P.  GAUDI_PPP_MAX_ITERATIONS iterations without getting there is NOT_CONVERGED.
 * Results, from the eigenvectors v of the last iteration (columns normalised) and F = F(their P_new):
 *   levels_out [B][GAUDI_HUCKEL_MAX_PI] fp32: v^T F v in eV, ascending, zero padded; occupation_out the same shape, uint8 (0 or 2).
 *   homo_out, lumo_out: the last filled level and the one after it (no electron: both the lowest level; no empty level: both the
 *     highest); gap_out = lumo - homo >= 0.
 *   e_electronic_out = 1/2 sum over r, s of P_rs (H_rs + F_rs);  e_core_out = sum over r < s of z_r z_s gamma_rs.
 *   pi_charge_out [B][A] = z_r - P_rr, zero on hydrogens and excluded atoms; pi_bond_order_out [B][M] = P_rs per listed bond, zero
 *     on bonds not between pi centres; site_class_out [B][A] int8, -1 on hydrogens and excluded atoms.
 *   n_pi_out, n_electrons_out, n_excluded_out, iterations_out (SCF iterations run), sweeps_out (Jacobi sweeps, all iterations),
 *     flags_out, status_out [B] int32; delta_p_out [B] fp32: the last iteration's.
 *   flags: GAUDI_PPP_DEGENERATE -- lumo - homo below 1e-3 eV: charges and bond orders are returned but not unique;
 *     GAUDI_PPP_SCF_CAP / GAUDI_PPP_JACOBI_CAP -- why the status is NOT_CONVERGED: the iteration cap, or a diagonalisation that
 *     used GAUDI_HUCKEL_MAX_SWEEPS sweeps.
 * status: the GAUDI_HUCKEL_* values with their meaning there, and GAUDI_PPP_OPEN_SHELL -- an odd electron count;
 * GAUDI_PPP_BAD_GEOMETRY -- a non-finite coordinate on a pi centre, or two pi centres closer than 0.5 Angstrom (atoms that are
 * not pi centres, template hydrogens at the origin among them, are not looked at).  BAD_TABLE (every molecule of the call) also for
 * a non-finite or non-positive gamma, a non-finite I, k, beta0 or listed beta_pair, a z outside 0..2, damping outside [0, 1), and a
 * repulsion that is neither formula.  Where a molecule is refused (every status but OK and NOT_CONVERGED) its rows are zero.
 * One 64-lane wave per molecule, tiers and launches as gaudi_huckel; a, v in LDS, the density matrix in a per-workgroup row of
 * global scratch that a lane reads only where it wrote.  Individually rounded fp32 in a fixed order: the outputs are a function
 * of the molecule's own arrays and bit for bit what gaudi_host_ppp returns.  B * max(A, M, 128) <= 2^31. */
#define GAUDI_PPP_MAX_ITERATIONS 64
#define GAUDI_PPP_OPEN_SHELL 7
#define GAUDI_PPP_BAD_GEOMETRY 8
#define GAUDI_PPP_DEGENERATE 2
#define GAUDI_PPP_SCF_CAP 4
#define GAUDI_PPP_JACOBI_CAP 8
#define GAUDI_PPP_MATAGA_NISHIMOTO 0
#define GAUDI_PPP_OHNO 1
typedef struct gaudi_ppp_tables {
  int32_t n_elems, h_elem, c_elem; /* as gaudi_huckel_tables */
  int32_t n_classes;
  int32_t site_class[8][5];
  float I[GAUDI_HUCKEL_MAX_CLASSES];
  float gamma[GAUDI_HUCKEL_MAX_CLASSES];
  int32_t z[GAUDI_HUCKEL_MAX_CLASSES];
  float k[GAUDI_HUCKEL_MAX_CLASSES];
  float beta0;
  float beta_pair[GAUDI_HUCKEL_MAX_CLASSES][GAUDI_HUCKEL_MAX_CLASSES]; /* NaN: use beta0 * k[i] * k[j] */
} gaudi_ppp_tables;
int gaudi_ppp(gaudi_handle* h, const gaudi_ppp_tables* tables, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
              const int32_t* bonds, const int32_t* n_bonds, const float* xyz, const int32_t* charge, int repulsion, float damping,
              float* levels_out, uint8_t* occupation_out, float* pi_charge_out, float* pi_bond_order_out, int8_t* site_class_out,
              int32_t* n_pi_out, int32_t* n_electrons_out, int32_t* n_excluded_out, int32_t* iterations_out, int32_t* sweeps_out,
              int32_t* flags_out, int32_t* status_out, float* homo_out, float* lumo_out, float* gap_out, float* e_electronic_out,
              float* e_core_out, float* delta_p_out);
/* gaudi_ppp without a handle: the same source text (csrc/ppp.inc: ppp_molecule) compiled for the host and run serially.  Test
 * surface for the CPU suite, not a CPU fallback: gaudi_amd never calls it on its own. */
int gaudi_host_ppp(const gaudi_ppp_tables* tables, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                   const int32_t* bonds, const int32_t* n_bonds, const float* xyz, const int32_t* charge, int repulsion,
                   float damping, float* levels_out, uint8_t* occupation_out, float* pi_charge_out, float* pi_bond_order_out,
                   int8_t* site_class_out, int32_t* n_pi_out, int32_t* n_electrons_out, int32_t* n_excluded_out,
                   int32_t* iterations_out, int32_t* sweeps_out, int32_t* flags_out, int32_t* status_out, float* homo_out,
                   float* lumo_out, float* gap_out, float* e_electronic_out, float* e_core_out, float* delta_p_out);
/* Number of gaudi_ppp launches (one per capacity tier present in a call) since gaudi_profile_reset(h, 1) and their summed duration
 * (HIP events; uploads and downloads are outside). */
int gaudi_ppp_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms);

/* ---- PPP for open shells: radical ions, delta-SCF IP / EA and triplets (csrc/ppp_open.inc). ----
 * Dewar's half-electron method on gaudi_ppp's machinery.  Everything of gaudi_ppp stays: sites, table, beta, gamma_rs, H, the Fock
 * formula, P0 = diag(z), damping, the 2^-16 stopping rule, the iteration cap, the Jacobi threshold rule, ranking by counting with
 * ties going to the smaller index.  What is new:
 *   A row is (molecule, charge, multiplicity).  multiplicity [B] int32 (NULL: all zero) is 1, 2 or 3; 0 means the lowest the parity
 *   allows (1 for even n_electrons, 2 for odd).  n_open = multiplicity - 1, n_c = (n_electrons - n_open) / 2.  BAD_INPUT where
 *   n_electrons - n_open is odd or negative, where n_c + n_open > n_pi, or where the multiplicity is outside 0..3 (after the
 *   refusals of the graph, NO_PI and OVERFLOW).  GAUDI_PPP_OPEN_SHELL is never returned.
 *   Density: P = sum over the ranked columns of occ_k v_k v_k^T, occ = 2 for ranks below n_c, 1 for the next n_open, 0 above --
 *   in the loop (ranks of the rotated diagonal) and in the result (ranks of the Rayleigh quotients).  F(P) is gaudi_ppp's formula
 *   unchanged: the half-electron operator.
 *   Energy: E_he = 1/2 sum over r, s of P_rs (H_rs + F_rs).  For an open orbital m: J_mm = sum over r, s of v_rm^2 v_sm^2 gamma_rs
 *   (gamma_rr on the diagonal); for two open orbitals K_mn = sum over r, s of v_rm v_rn v_sm v_sn gamma_rs.
 *     doublet: E = E_he - J_mm / 4;    triplet: E = E_he - (J_mm + J_nn) / 4 - K_mn / 2;    e_state = E + e_core.
 *   (So a single pi centre with one electron has e_state = -I, and triplet ethylene e_state = -2 I_C.)
 *   E_he, the J and K sums and e_core are accumulated in fp64 from the fp32 elements (P_rs, H_rs + F_rs, v, gamma_rs, z_r z_s
 *   gamma_rs), by columns over r ascending and then over the columns ascending; nothing is rounded to fp32.
 * Outputs: the eighteen of gaudi_ppp -- occupation_out holds 2 / 1 / 0; homo_out is the highest occupied level (the open one when
 * there is one) and lumo_out the first empty one -- and then
 *   spin_density_out [B][A] fp32 = sum over the open orbitals of v_rm^2, zero on hydrogens and excluded atoms;
 *   e_state_out, he_correction_out [B] fp64: E + e_core and E - E_he in eV;
 *   n_open_out [B] int32;  somo_out [B][2] int32: the ranks of the open levels, -1 where there is none.
 * flags gains GAUDI_PPP_OPEN_TIE (rows with n_open > 0 only): in some iteration's ranking or in the result the two levels on
 * either boundary of the open set (ranks n_c - 1 | n_c, or n_c + n_open - 1 | n_c + n_open) differ by less than 1e-3 eV -- the
 * choice of singly occupied orbital was arbitrary within a degenerate pair (the benzene cation); the values are still returned, and
 * per-atom quantities depend on that choice.  GAUDI_PPP_DEGENERATE is lumo - homo below 1e-3 eV as in gaudi_ppp.
 * On a row of multiplicity 1 the eighteen outputs are gaudi_ppp's bit for bit and the flag is never set.  A refused row is zero.
 * Tiers, launches, LDS and scratch as gaudi_ppp; bit for bit what gaudi_host_ppp_open returns, the doubles included.
 * Not here: UHF and ROHF coupling operators, open-shell singlets, CIS / ring currents / localization on an open-shell reference. */
#define GAUDI_PPP_OPEN_TIE 256
int gaudi_ppp_open(gaudi_handle* h, const gaudi_ppp_tables* tables, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                   const int32_t* bonds, const int32_t* n_bonds, const float* xyz, const int32_t* charge,
                   const int32_t* multiplicity, int repulsion, float damping, float* levels_out, uint8_t* occupation_out,
                   float* pi_charge_out, float* pi_bond_order_out, int8_t* site_class_out, int32_t* n_pi_out,
                   int32_t* n_electrons_out, int32_t* n_excluded_out, int32_t* iterations_out, int32_t* sweeps_out,
                   int32_t* flags_out, int32_t* status_out, float* homo_out, float* lumo_out, float* gap_out,
                   float* e_electronic_out, float* e_core_out, float* delta_p_out, float* spin_density_out, double* e_state_out,
                   double* he_correction_out, int32_t* n_open_out, int32_t* somo_out);
/* gaudi_ppp_open without a handle: the same source text compiled for the host and run serially.  Test surface, not a fallback. */
int gaudi_host_ppp_open(const gaudi_ppp_tables* tables, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                        const int32_t* bonds, const int32_t* n_bonds, const float* xyz, const int32_t* charge,
                        const int32_t* multiplicity, int repulsion, float damping, float* levels_out, uint8_t* occupation_out,
                        float* pi_charge_out, float* pi_bond_order_out, int8_t* site_class_out, int32_t* n_pi_out,
                        int32_t* n_electrons_out, int32_t* n_excluded_out, int32_t* iterations_out, int32_t* sweeps_out,
                        int32_t* flags_out, int32_t* status_out, float* homo_out, float* lumo_out, float* gap_out,
                        float* e_electronic_out, float* e_core_out, float* delta_p_out, float* spin_density_out,
                        double* e_state_out, double* he_correction_out, int32_t* n_open_out, int32_t* somo_out);
/* Number of gaudi_ppp_open launches (one per capacity tier present in a call) since gaudi_profile_reset(h, 1) and their summed
 * duration. */
int gaudi_ppp_open_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms);

/* ---- The PPP SCF with Pulay's DIIS (csrc/ppp_scf.inc). ----
 * gaudi_ppp_open's model, rows, statuses and outputs; the self-consistent iteration extrapolates the Fock matrix.  Opt-in: no other
 * entry point changes.  Per iteration k (1-based), after F = F(P) of the input density P:
 *   While k >= diis_start the commutator e = F P - P F (fp32; G = F P with every sum over the inner index ascending, e = G - G^T)
 *   and F enter a ring of diis_size entries (the oldest leaves a full ring); diis_error = max |e_rc| in eV.  P0 = diag(z) never
 *   enters (diis_start >= 2): it commutes with every F of an all-carbon molecule.
 *   B_ij = sum over r, c of e_i e_j in fp64 from the fp32 elements (by columns over r ascending, then over the columns ascending),
 *   computed once per pair; B is scaled by its largest diagonal element and [[B, 1], [1^T, 0]] (c, lambda) = (0, 1) is solved by
 *   Gaussian elimination with partial pivoting (the first largest element of a column) in fp64.  A pivot below 2^-40 (or B = 0)
 *   drops the oldest entry for good and the rest is solved again; one entry left: F goes on as it is.
 *   F <- sum over the entries, oldest to newest, of c_i F_i (fp32 elements, the coefficients rounded once to fp32).  Then gaudi_ppp's
 *   path unchanged: Jacobi, normalise, rank, P_new, delta_p = max |P_new - P|.
 *   From iteration diis_start on P = P_new (no damping); before it, the damped update.
 *   Stop: delta_p <= 2^-16 and diis_error <= GAUDI_PPP_DIIS_ERROR (the second condition only rejects a stagnant history, which
 *   reads delta_p = 0 while the commutator is of order 0.1 eV), or GAUDI_PPP_MAX_ITERATIONS.
 * The levels, energies, charges and the fp64 state energy are those of F(P_new) of the last eigenvectors, never of an extrapolated
 * matrix, exactly as in gaudi_ppp_open.
 * diis_size outside 2..GAUDI_PPP_DIIS_MAX or diis_start outside 2..GAUDI_PPP_MAX_ITERATIONS: every row GAUDI_HUCKEL_BAD_INPUT and
 * zero (behind BAD_TABLE, which a table, damping or repulsion formula that cannot be used gives every row); 0 does not select the
 * damped iteration.  Every other refusal and its order are gaudi_ppp_open's.
 * Outputs: the twenty-three of gaudi_ppp_open and then
 *   diis_error_out [B] fp32: the last iteration's max |e_rc| in eV (0 where the iteration ended before diis_start);
 *   n_extrapolated_out [B] int32: the iterations whose F was a combination of two or more entries (<= iterations - diis_start + 1).
 * A row of multiplicity 1 solves gaudi_ppp's model but is not gaudi_ppp's bits: it stops elsewhere on the way to the same fixed point.
 * Tiers and LDS as gaudi_ppp; the scratch row is (1 + 2 diis_size) P^2 floats, and a tier's rows are split into launches that hold at
 * most 512 MiB of it.  Bit for bit what gaudi_host_ppp_scf returns, the doubles included.
 * Not here: DIIS for gaudi_ppp_cis's ground state, ring currents and localization energies; level shifting, EDIIS / ADIIS,
 * second-order SCF; stability analysis (DIIS can stop on a saddle); following a state through exact ties; UHF / ROHF. */
#define GAUDI_PPP_DIIS_MAX 8
#define GAUDI_PPP_DIIS_ERROR 9.765625e-4f /* 2^-10 eV (DESIGN.md section 8t says where it comes from) */
int gaudi_ppp_scf(gaudi_handle* h, const gaudi_ppp_tables* tables, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                  const int32_t* bonds, const int32_t* n_bonds, const float* xyz, const int32_t* charge, const int32_t* multiplicity,
                  int repulsion, int32_t diis_size, int32_t diis_start, float damping, float* levels_out, uint8_t* occupation_out,
                  float* pi_charge_out, float* pi_bond_order_out, int8_t* site_class_out, int32_t* n_pi_out,
                  int32_t* n_electrons_out, int32_t* n_excluded_out, int32_t* iterations_out, int32_t* sweeps_out,
                  int32_t* flags_out, int32_t* status_out, float* homo_out, float* lumo_out, float* gap_out,
                  float* e_electronic_out, float* e_core_out, float* delta_p_out, float* spin_density_out, double* e_state_out,
                  double* he_correction_out, int32_t* n_open_out, int32_t* somo_out, float* diis_error_out,
                  int32_t* n_extrapolated_out);
/* gaudi_ppp_scf without a handle: the same source text compiled for the host and run serially.  Test surface, not a fallback. */
int gaudi_host_ppp_scf(const gaudi_ppp_tables* tables, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                       const int32_t* bonds, const int32_t* n_bonds, const float* xyz, const int32_t* charge,
                       const int32_t* multiplicity, int repulsion, int32_t diis_size, int32_t diis_start, float damping,
                       float* levels_out, uint8_t* occupation_out, float* pi_charge_out, float* pi_bond_order_out,
                       int8_t* site_class_out, int32_t* n_pi_out, int32_t* n_electrons_out, int32_t* n_excluded_out,
                       int32_t* iterations_out, int32_t* sweeps_out, int32_t* flags_out, int32_t* status_out, float* homo_out,
                       float* lumo_out, float* gap_out, float* e_electronic_out, float* e_core_out, float* delta_p_out,
                       float* spin_density_out, double* e_state_out, double* he_correction_out, int32_t* n_open_out,
                       int32_t* somo_out, float* diis_error_out, int32_t* n_extrapolated_out);
/* Number of gaudi_ppp_scf launches (one per capacity tier present in a call, more where a tier's scratch is split) since
 * gaudi_profile_reset(h, 1) and their summed duration. */
int gaudi_ppp_scf_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms);

/* ---- PPP-CIS excited states: S1, T1 and oscillator strengths (csrc/ppp_cis.inc). ----
 * gaudi_ppp, then configuration interaction over single excitations on its ground state.  After a solve with status OK: the levels
 * eps by rank, the normalised eigenvector columns C, n_occ = n_electrons / 2, n = n_pi, the centres' coordinates and gamma.
 * Active window: window = W in 1..8 (any other value: BAD_TABLE for every molecule).  n_o = min(n_occ, W) highest occupied ranks,
 * n_v = min(n - n_occ, W) lowest empty ranks, D = n_o * n_v <= 64 configurations (i -> a) ordered by (i ascending, a ascending).
 * D = 0 (no electron, or no empty level): status OK, n_states = 0.
 *   (ia|jb) = sum_r C_ri C_ra (sum_s gamma_rs C_sj C_sb);  (ij|ab) = sum_r C_ri C_rj (sum_s gamma_rs C_sa C_sb)
 *   (gamma_rs as gaudi_ppp forms it, gamma_rr = gamma_r; r and s ascending; computed for ia <= jb and mirrored)
 *   triplet matrix T[ia,jb] = delta_ij delta_ab (eps_a - eps_i) - (ij|ab);  singlet matrix S = T + 2 (ia|jb)
 * Each is diagonalised by the Jacobi routine of gaudi_huckel on a 64-wide work space (threshold: 2^-24 of its largest |diagonal|
 * rounded up to a power of two); the excitation energies are the dense Rayleigh quotients X^T M X of the normalised columns,
 * ranked by counting (ties: the smaller index first):
 *   singlet_out, triplet_out [B][64] fp32, eV, ascending, zero beyond n_states.
 *   dipole_out [B][64][3], e Angstrom, of singlet k: sqrt2 sum_ia X_ia,k sum_r C_ri C_ra (x_r - x_0), x_0 the first pi centre.
 *   osc_out [B][64] = (2 / 3) (E_k / 27.211386) |mu_k|^2 / 0.52917721^2.
 *   lead_out [B][64][2] uint8: the (occupied rank, empty rank) of the largest X^2 of singlet k (ties: the smaller configuration),
 *     lead_weight_out [B][64] that X^2.
 *   n_states_out = D, n_active_occ_out = n_o, n_active_virt_out = n_v, cis_sweeps_out (both solves) [B] int32.
 * The eighteen outputs of gaudi_ppp are written as gaudi_ppp writes them, bit for bit, except that flags_out gains
 *   GAUDI_PPP_CIS_JACOBI_CAP -- a CIS solve used GAUDI_HUCKEL_MAX_SWEEPS sweeps; status_out becomes NOT_CONVERGED;
 *   GAUDI_PPP_CIS_TRUNCATED -- D < n_occ * (n - n_occ): the window is smaller than the single-excitation space;
 *   GAUDI_PPP_CIS_WINDOW_EDGE -- a level just outside the window within 1e-3 eV of the window's edge level: the results depend on
 *     how the solver oriented a degenerate pair;
 *   GAUDI_PPP_CIS_TRIPLET_UNSTABLE -- triplet[0] <= 0: the closed-shell ground state is not the lowest state (information).
 * A molecule whose gaudi_ppp status is not OK keeps that status and has zero CIS rows.  One more launch after gaudi_ppp's, one
 * 64-lane wave per molecule for all tiers; individually rounded fp32 in a fixed order: bit for bit what gaudi_host_ppp_cis returns. */
#define GAUDI_PPP_CIS_MAX_WINDOW 8
#define GAUDI_PPP_CIS_MAX_STATES 64
#define GAUDI_PPP_CIS_JACOBI_CAP 16
#define GAUDI_PPP_CIS_TRUNCATED 32
#define GAUDI_PPP_CIS_WINDOW_EDGE 64
#define GAUDI_PPP_CIS_TRIPLET_UNSTABLE 128
int gaudi_ppp_cis(gaudi_handle* h, const gaudi_ppp_tables* tables, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                  const int32_t* bonds, const int32_t* n_bonds, const float* xyz, const int32_t* charge, int repulsion,
                  float damping, float* levels_out, uint8_t* occupation_out, float* pi_charge_out, float* pi_bond_order_out,
                  int8_t* site_class_out, int32_t* n_pi_out, int32_t* n_electrons_out, int32_t* n_excluded_out,
                  int32_t* iterations_out, int32_t* sweeps_out, int32_t* flags_out, int32_t* status_out, float* homo_out,
                  float* lumo_out, float* gap_out, float* e_electronic_out, float* e_core_out, float* delta_p_out, int window,
                  float* singlet_out, float* triplet_out, float* osc_out, float* dipole_out, uint8_t* lead_out,
                  float* lead_weight_out, int32_t* n_states_out, int32_t* n_active_occ_out, int32_t* n_active_virt_out,
                  int32_t* cis_sweeps_out);
/* gaudi_ppp_cis without a handle: the same source text compiled for the host and run serially.  Test surface, not a fallback. */
int gaudi_host_ppp_cis(const gaudi_ppp_tables* tables, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                       const int32_t* bonds, const int32_t* n_bonds, const float* xyz, const int32_t* charge, int repulsion,
                       float damping, float* levels_out, uint8_t* occupation_out, float* pi_charge_out, float* pi_bond_order_out,
                       int8_t* site_class_out, int32_t* n_pi_out, int32_t* n_electrons_out, int32_t* n_excluded_out,
                       int32_t* iterations_out, int32_t* sweeps_out, int32_t* flags_out, int32_t* status_out, float* homo_out,
                       float* lumo_out, float* gap_out, float* e_electronic_out, float* e_core_out, float* delta_p_out, int window,
                       float* singlet_out, float* triplet_out, float* osc_out, float* dipole_out, uint8_t* lead_out,
                       float* lead_weight_out, int32_t* n_states_out, int32_t* n_active_occ_out, int32_t* n_active_virt_out,
                       int32_t* cis_sweeps_out);
/* Number of CIS launches (one per gaudi_ppp_cis call that reaches the device) since gaudi_profile_reset(h, 1) and their summed
 * duration; the SCF launches of those calls are counted by gaudi_ppp_profile_get. */
int gaudi_ppp_cis_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms);

/* ---- All Kekule structures: their count, Pauling bond orders, sextets, Fries and Clar numbers (csrc/kekule.inc, DESIGN.md
 * section 8o), for B molecules in one launch. ----
 * gaudi_bond_orders returns one Kekule structure; this enumerates them all.  Atoms, bonds, the sigma degree (bonds, one more for a
 * carbon with exactly two) and the valence table are those of gaudi_bond_orders.  Every atom takes its FIRST option, which must be
 * neutral; `sel` is the set of atoms whose option adds a bond, G[sel] the graph of the bonds with both ends in sel; a Kekule
 * structure is a perfect matching of G[sel] and K their number (0 when |sel| is odd; 1 when sel is empty).  The molecule must be
 * connected.  Exact integer combinatorics: no parameter, no floating point.
 * The search tree, which defines the budget: the root is the empty matching; at a node v is the lowest-index unmatched atom of sel;
 * without one the node is a structure; otherwise it has one child per unmatched sel neighbour of v, in ascending order; a node
 * without a child is a dead end.  n_nodes_out counts every node.
 * Hexagons: the chordless 6-cycles of the heavy-atom graph whose six atoms are all in sel (pyridine-type rings included; a
 * five-ring whose heteroatom gives a lone pair is not a sextet here), ordered by their sorted atom tuple and each reported in
 * cycle order from its smallest atom towards the smaller of that atom's two ring neighbours.  A hexagon is a sextet of a structure
 * in which three of its six bonds are double.  fries = the most sextets of one structure; clar = the most pairwise atom-disjoint
 * sextets of one structure, which is the Clar number.
 * Not here: counts beyond the budget (no factorisation over components, no determinant method), charged resonance forms,
 * lone-pair sextets of five-rings, resonance energies in eV. */
#define GAUDI_KEKULE_BUDGET (1 << 20)  /* nodes of the search tree per molecule */
#define GAUDI_KEKULE_MAX_SEL 128       /* atoms in sel (the largest tier of gaudi_huckel) */
#define GAUDI_KEKULE_MAX_EDGES 192     /* bonds of G[sel] */
/* status_out codes; anything but OK leaves every other output of the molecule zero. */
#define GAUDI_KEKULE_OK 0
#define GAUDI_KEKULE_NO_KEKULE 1      /* K = 0: |sel| is odd, or G[sel] has no perfect matching                              */
#define GAUDI_KEKULE_NOT_NEUTRAL 2    /* an atom has options but no neutral one (its only option is charged)                 */
#define GAUDI_KEKULE_NOT_CONNECTED 3
#define GAUDI_KEKULE_BAD_VALENCE 4    /* an atom without an option, as GAUDI_BONDS_BAD_VALENCE                                */
#define GAUDI_KEKULE_BAD_INPUT 5      /* as GAUDI_BONDS_BAD_INPUT                                                            */
#define GAUDI_KEKULE_OVERFLOW 6       /* beyond gaudi_bond_orders' capacities, or more than 128 atoms in sel, 192 bonds in G[sel],
                                         GAUDI_RINGS_MAX_RINGS hexagons, or a sel atom with more than three sel neighbours     */
#define GAUDI_KEKULE_EMPTY 7          /* n_atoms = 0                                                                         */
#define GAUDI_KEKULE_UNDECIDED 8      /* the tree has more than GAUDI_KEKULE_BUDGET nodes.  Like GAUDI_BONDS_GAVE_UP, and unlike every
                                         other status and every count, this can depend on the atom numbering                 */
/* Inputs as gaudi_bond_orders takes them.  One 64-lane wave per molecule; the tree is expanded level by level until 64 nodes are
 * open, then every lane walks subtrees depth-first; sums and maxima commute, so the outputs are bit for bit those of
 * gaudi_host_kekule wherever the molecule stands in the batch.
 * k_out [B]; double_count_out [B][M]: structures in which the listed bond is double, 0 for a bond outside G[sel] (the Pauling bond
 * order is double_count / K); n_hex_out [B]; hex_atoms_out [B][GAUDI_RINGS_MAX_RINGS][6]: atom indices; sextet_count_out
 * [B][GAUDI_RINGS_MAX_RINGS]: structures in which the hexagon is a sextet; fries_out, clar_out, n_nodes_out, status_out [B]. */
int gaudi_kekule(gaudi_handle* h, const gaudi_valence_tables* tables, int B, int A, int M, const int32_t* elem,
                 const int32_t* n_atoms, const int32_t* bonds, const int32_t* n_bonds, int64_t* k_out, uint32_t* double_count_out,
                 int32_t* n_hex_out, int32_t* hex_atoms_out, uint32_t* sextet_count_out, int32_t* fries_out, int32_t* clar_out,
                 int64_t* n_nodes_out, int32_t* status_out);
/* gaudi_kekule without a handle: the same source text compiled for the host and run serially.  Test surface, not a fallback. */
int gaudi_host_kekule(const gaudi_valence_tables* tables, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                      const int32_t* bonds, const int32_t* n_bonds, int64_t* k_out, uint32_t* double_count_out, int32_t* n_hex_out,
                      int32_t* hex_atoms_out, uint32_t* sextet_count_out, int32_t* fries_out, int32_t* clar_out,
                      int64_t* n_nodes_out, int32_t* status_out);
/* Number of gaudi_kekule launches since gaudi_profile_reset(h, 1) and their summed duration (HIP events). */
int gaudi_kekule_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms);

/* ---- Hueckel-London ring currents: the pi current a perpendicular magnetic field induces in every bond and every ring
 * (csrc/ring_current.inc), for B molecules. ----
 * The graph, the pi centres, the classes, the matrix M, the electron count, `charge` and the level filling are gaudi_huckel's; the
 * energy matrix is E = -M (units |beta|), the orbital energies eps = -x.  xyz [B][A][3] fp32 in Angstrom as gaudi_ppp takes it; only
 * pi centres are looked at.
 *   plane     c = the centroid of the pi centres, n = the unit eigenvector of the smallest eigenvalue of sum (r-c)(r-c)^T, its
 *             component of largest magnitude positive (the lower index wins a tie); rms_out_of_plane = the root mean square of n.(r-c).
 *   areas     s_rs = n.((r_r-c) x (r_s-c)) / 2.
 *   response  A_rs = E_rs s_rs on bonds, a_lk = v_l^T A v_k, W_lk = 2 a_lk / (eps_k - eps_l) for k occupied and l empty,
 *             Q = sum W_lk (v_l v_k^T - v_k v_l^T), P = 2 sum_occ v v^T, J_rs = 2 E_rs (s_rs P_rs + Q_sr).
 *   units     c0 = 2 A0 / 9, A0 = (3 sqrt(3) / 2) (1.40)^2: bond_current of listed bond (i, j) = -J_ij / c0 in the direction i -> j; it is
 *             +1 in benzene (a regular hexagon of 1.40 Angstrom, k = 1), counter-clockwise seen from the tip of n: positive is
 *             diatropic.  Zero on bonds that are not between pi centres, and exactly zero on a bond that lies on none of the
 *             rings when the ring currents are defined (it lies on no cycle: Kirchhoff's law).
 *   rings     the chordless cycles of 4, 5 or 6 pi centres of the graph of pi centres, ordered by sorted atom tuple, each reported
 *             from its smallest atom in the direction whose area projected along n (ring_area) is positive.
 *   currents  the ring currents I solve C I = b (b the bond currents, C[e][r] = +-1 where ring r runs along or against listed bond
 *             e) through the normal equations (C^T C) I = C^T b; residual = max |C I - b|.  They are defined when n_rings equals
 *             bonds - centres + components of the pi graph, n_rings <= 32, every ring_area > 1e-3 and the elimination meets no pivot
 *             <= 0; otherwise flags has GAUDI_RING_CURRENT_RINGS_UNDEFINED, n_rings and the ring rows are zero and the bond currents
 *             stay valid.
 * status, in this order: the GAUDI_HUCKEL_* refusals with their meaning there; GAUDI_PPP_OPEN_SHELL -- an odd electron count;
 * NOT_CONVERGED; GAUDI_RING_CURRENT_SMALL_GAP -- x_HOMO - x_LUMO < 1e-3 (the paramagnetic term diverges), also no occupied or no
 * empty level; a pi graph without a cycle is then OK with every current, the normal and rms_out_of_plane zero, whatever its
 * coordinates; GAUDI_PPP_BAD_GEOMETRY -- the rule of gaudi_ppp.  Every status but OK leaves every other output of the molecule zero.
 * Outputs: bond_current_out [B][M]; n_rings_out [B]; ring_atoms_out [B][32][6] atom indices in cycle order, -1 padded (a solved
 * molecule's rows beyond n_rings are -1 too); ring_size_out, ring_current_out, ring_area_out [B][32]; normal_out [B][3];
 * rms_out_of_plane_out, gap_out (x_HOMO - x_LUMO), residual_out [B] fp32; n_pi_out, n_electrons_out, sweeps_out, flags_out,
 * status_out [B].
 * One 64-lane wave per molecule, tiers and launches as gaudi_huckel, whose Jacobi routine and Rayleigh pass it runs.  Individually
 * rounded fp32 in a fixed order, no atomics: the outputs are a function of the molecule's own arrays and bit for bit what
 * gaudi_host_ring_currents returns.  B * max(A, M, 192) <= 2^31.
 * Not here: coupled (PPP) currents, ring currents of open shells, current-density maps, NICS, non-planar corrections. */
#define GAUDI_RING_CURRENT_MAX_RINGS 32
#define GAUDI_RING_CURRENT_MAX_SIZE 6
#define GAUDI_RING_CURRENT_SMALL_GAP 9       /* a status, after GAUDI_PPP_BAD_GEOMETRY */
#define GAUDI_RING_CURRENT_RINGS_UNDEFINED 1 /* a flag */
int gaudi_ring_currents(gaudi_handle* h, const gaudi_huckel_tables* tables, int B, int A, int M, const int32_t* elem,
                        const int32_t* n_atoms, const int32_t* bonds, const int32_t* n_bonds, const float* xyz, const int32_t* charge,
                        float* bond_current_out, int32_t* n_rings_out, int32_t* ring_atoms_out, int32_t* ring_size_out,
                        float* ring_current_out, float* ring_area_out, float* normal_out, float* rms_out_of_plane_out, float* gap_out,
                        float* residual_out, int32_t* n_pi_out, int32_t* n_electrons_out, int32_t* sweeps_out, int32_t* flags_out,
                        int32_t* status_out);
/* gaudi_ring_currents without a handle: the same source text (csrc/ring_current.inc: ring_current_molecule) compiled for the host
 * and run serially.  Test surface for the CPU suite, not a CPU fallback: gaudi_amd never calls it on its own. */
int gaudi_host_ring_currents(const gaudi_huckel_tables* tables, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                             const int32_t* bonds, const int32_t* n_bonds, const float* xyz, const int32_t* charge,
                             float* bond_current_out, int32_t* n_rings_out, int32_t* ring_atoms_out, int32_t* ring_size_out,
                             float* ring_current_out, float* ring_area_out, float* normal_out, float* rms_out_of_plane_out,
                             float* gap_out, float* residual_out, int32_t* n_pi_out, int32_t* n_electrons_out, int32_t* sweeps_out,
                             int32_t* flags_out, int32_t* status_out);
/* Number of gaudi_ring_currents launches (one per capacity tier present in a call) since gaudi_profile_reset(h, 1) and their
 * summed duration (HIP events). */
int gaudi_ring_currents_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms);

/* ---- Hueckel localization energies: where a conjugated molecule reacts and how easily (csrc/reactivity.inc, DESIGN.md section
 * 8r), for B molecules. ----
 * The graph, the pi centres, the classes, the matrix M, the electron count n_el, `charge` and the level filling are gaudi_huckel's,
 * and so is E_pi: the sum of occupation * x in |beta| (the larger x, the lower the level).  The parent has n centres.  Deleting
 * centres removes their rows, columns and bonds from M; h, k and the pair values of what survives stay as the table gives them.  A
 * residual system is filled as the parent is: two electrons per level from the lowest energy, the last level may hold one; an
 * empty residual system has E_pi = 0.
 *   atom localization (Wheland), per pi centre r and kind q = the pi electrons that stay localized on r (2 electrophilic, 1
 *     radical, 0 nucleophilic attack):  L_q(r) = E_pi(parent) - [E_pi(parent without r, n_el - q electrons) + q h_r];
 *     undefined where n_el - q < 0 or n_el - q > 2 (n - 1).
 *   para localization (Brown), per chordless six-ring c[0..5] of pi centres and pair k = 0..2 of opposite positions (c[k], c[k+3]):
 *     L = E_pi(parent) - [E_pi(parent without both, n_el - 2 electrons) + h_r + h_s]; undefined where n_el - 2 < 0 or > 2 (n - 2).
 *   ortho (bond) localization, per listed bond between two pi centres: the same with the bonded pair (with_bonds != 0 only).
 *   free valence, per pi centre: 1.7320508f less the pi bond orders (gaudi_huckel's) to its pi neighbours: the carbon scale.
 *   rings: the chordless cycles of 4, 5 or 6 pi centres of the graph of pi centres, ordered by sorted atom tuple, each in cycle
 *     order from its smallest atom towards the smaller of that atom's two ring neighbours.  At most 32: the rings are taken in the
 *     order of their smallest centre, and those of a smallest centre are kept while the count through that centre stays within
 *     32; when any is dropped, flags has GAUDI_REACTIVITY_RINGS_TRUNCATED and the para values are those of the kept rings.
 * One molecule costs n + 3 (six-rings) + (pi bonds) diagonalisations beside the parent's: its jobs, in this fixed order.  A residual
 * diagonalisation that uses GAUDI_HUCKEL_MAX_SWEEPS sweeps without converging leaves its entries undefined and sets
 * GAUDI_REACTIVITY_SWEEP_CAP in flags.
 * Outputs: atom_localization_out [B][3][A] (kinds q = 0, 1, 2); free_valence_out [B][A]; rings_out [B][32][6] atom indices, -1 padded;
 * n_rings_out [B]; para_localization_out [B][32][3]; ortho_localization_out [B][M]; e_pi_out [B] (gaudi_huckel's e_pi, bit for
 * bit); n_pi_out, n_electrons_out, n_jobs_out, sweeps_out (the parent's and every residual solve's), flags_out, status_out [B].
 * In a molecule with status OK every fp32 entry that carries no value holds the quiet NaN 0x7fc00000: a hydrogen, an excluded
 * atom, the padding beyond n_atoms / n_bonds / n_rings, a four- or five-ring, a bond to an atom that is no pi centre, an undefined
 * kind, every ortho entry when with_bonds = 0.  status: the GAUDI_HUCKEL_* values with their meaning there; NOT_CONVERGED is the
 * parent's diagonalisation.  Every status but OK leaves every other output of the molecule zero.
 * One launch per capacity tier present (tiers as gaudi_huckel); the grid is (molecule, slice), one 64-lane wave per workgroup:
 * every wave solves the parent, then the jobs j = slice (mod slices).  slices: 1..16, or 0 to have the entry point choose
 * ceil(2 * compute units / molecules of the tier) clamped to 1..16 (gaudi_host_reactivity: 1).  Individually rounded fp32 in a
 * fixed order, no atomics: the outputs do not depend on `slices`, the tier, the batch or the molecule's place in it, and are bit
 * for bit what gaudi_host_reactivity returns.  B * max(3 A, 224 + M) <= 2^31.
 * Not here: PPP-level (self-consistent) localization, transition states, steric effects, regioselectivity beyond these indices. */
#define GAUDI_REACTIVITY_KINDS 3
#define GAUDI_REACTIVITY_MAX_SLICES 16
#define GAUDI_REACTIVITY_SWEEP_CAP 1       /* flags */
#define GAUDI_REACTIVITY_RINGS_TRUNCATED 2
int gaudi_reactivity(gaudi_handle* h, const gaudi_huckel_tables* tables, int B, int A, int M, const int32_t* elem,
                     const int32_t* n_atoms, const int32_t* bonds, const int32_t* n_bonds, const int32_t* charge, int with_bonds,
                     int slices, float* atom_localization_out, float* free_valence_out, int32_t* rings_out, int32_t* n_rings_out,
                     float* para_localization_out, float* ortho_localization_out, float* e_pi_out, int32_t* n_pi_out,
                     int32_t* n_electrons_out, int32_t* n_jobs_out, int32_t* sweeps_out, int32_t* flags_out, int32_t* status_out);
/* gaudi_reactivity without a handle: the same source text (csrc/reactivity.inc: reactivity_molecule) compiled for the host and run
 * serially, slice after slice.  Test surface for the CPU suite, not a CPU fallback: gaudi_amd never calls it on its own. */
int gaudi_host_reactivity(const gaudi_huckel_tables* tables, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                          const int32_t* bonds, const int32_t* n_bonds, const int32_t* charge, int with_bonds, int slices,
                          float* atom_localization_out, float* free_valence_out, int32_t* rings_out, int32_t* n_rings_out,
                          float* para_localization_out, float* ortho_localization_out, float* e_pi_out, int32_t* n_pi_out,
                          int32_t* n_electrons_out, int32_t* n_jobs_out, int32_t* sweeps_out, int32_t* flags_out,
                          int32_t* status_out);
/* Number of gaudi_reactivity launches (one per capacity tier present in a call) since gaudi_profile_reset(h, 1) and their summed
 * duration (HIP events; uploads, downloads and the host-side fold are outside). */
int gaudi_reactivity_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms);

/* Device Philox stream used when noise == NULL, exposed for tests: out[draw][b][e], e < n_elem. */
int gaudi_philox_normal(gaudi_handle* h, uint64_t seed, int64_t sample_offset, int B, int n_elem, int draw0,
                        int n_draws, float* out);

/* ---- Device-free host logic (no handle, no GPU): exposed so the CPU test suite can check it. ----
 * gamma [T+1] and (optionally) the per-step table [T][4] exactly as gaudi_load_edm builds them. */
int gaudi_host_schedule(int T, float noise_power /* 0 = cosine */, float noise_precision, float* gamma_out, float* coef_out);
/* The symmetric 3 x 3 eigensolver of gaudi_rings_to_atoms (align_to_xy_plane), the same source text compiled for the host:
 * a [n][3][3] (the lower triangles are read) -> e_out [n][3][3], e_out[q][c][k] = component c of the eigenvector of the k-th
 * smallest eigenvalue, with the signs numpy.linalg.eigh (LAPACK dsyevd, 'L') returns. */
int gaudi_host_eigh3(int n, const double* a, double* e_out);
/* gaudi_atoms_to_rings without a handle: the same source text (csrc/rings.inc: perceive_rings) compiled for the host and run
 * serially, one molecule after the other.  Test surface for the CPU suite, not a CPU fallback: gaudi_amd never calls it on its own. */
int gaudi_host_atoms_to_rings(const gaudi_perception_tables* tables, int B, int A, const double* xyz, const int32_t* elem,
                              const int32_t* n_atoms, int flags, double covalency_factor, int max_rings, int32_t* status_out,
                              int32_t* n_rings_out, int32_t* ring_size_out, int32_t* ring_atoms_out, int32_t* ring_type_out,
                              double* centre_out, int32_t* n_orient_out, double* orient_out, uint8_t* adj_out);
/* gaudi_bond_orders without a handle: the same source text (csrc/bonds.inc: assign_bond_orders) compiled for the host and run
 * serially.  Test surface for the CPU suite, not a CPU fallback: gaudi_amd never calls it on its own. */
int gaudi_host_bond_orders(const gaudi_valence_tables* tables, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                           const int32_t* bonds, const int32_t* n_bonds, uint8_t* order_out, int8_t* charge_out,
                           int32_t* n_charged_out, int32_t* status_out);
/* gaudi_canonical_order without a handle: the same source text (csrc/canon.inc: canonical_order) compiled for the host and run
 * serially.  Test surface for the CPU suite, not a CPU fallback: gaudi_amd never calls it on its own. */
int gaudi_host_canonical_order(int n_elems, int h_elem, int c_elem, int B, int A, int M, const int32_t* elem,
                               const int32_t* n_atoms, const int32_t* bonds, const int32_t* n_bonds, int32_t* rank_out,
                               int32_t* n_heavy_out, uint8_t* label_out, int32_t* n_hbonds_out, uint16_t* cbonds_out,
                               int32_t* nodes_out, int32_t* status_out);
/* gaudi_circular_fingerprint without a handle: the same source text (csrc/fp.inc: circular_fingerprint) compiled for the host and
 * run serially.  Test surface for the CPU suite, not a CPU fallback: gaudi_amd never calls it on its own. */
int gaudi_host_circular_fingerprint(int n_elems, int h_elem, int c_elem, int B, int A, int M, const int32_t* elem,
                                    const int32_t* n_atoms, const int32_t* bonds, const int32_t* n_bonds, int radius, int n_bins,
                                    uint8_t* fp_out, int32_t* total_out, int32_t* status_out);
/* gaudi_substructure_search without a handle: the same source text (csrc/sub.inc: substructure_search) compiled for the host, every
 * root walked in turn through the same step function.  Test surface for the CPU suite, not a CPU fallback. */
int gaudi_host_substructure_search(int n_elems, int h_elem, int c_elem, int B, int A, int M, const int32_t* elem,
                                   const int32_t* n_atoms, const int32_t* bonds, const int32_t* n_bonds, int P, int QA, int QM,
                                   const int32_t* p_elem, const int32_t* p_n_atoms, const int32_t* p_bonds,
                                   const int32_t* p_n_bonds, const int32_t* p_flags, int32_t* count_out, int32_t* first_out,
                                   uint8_t* covered_out, int32_t* steps_out, int32_t* status_out);
/* The largest number of candidate tests ONE root took in gaudi_host_substructure_search since the last call with reset != 0: the
 * figure GAUDI_SUB_MAX_STEPS is sized with.  A process-wide counter, not thread-safe: tooling only. */
int gaudi_host_substructure_root_steps(int reset);
/* gaudi_fp_nearest without a handle: plain loops over every pair with the same comparison function (csrc/fp.inc: fp_ahead).  Test
 * surface for the CPU suite, not a CPU fallback. */
int gaudi_host_fp_nearest(int n_bins, int B, const uint8_t* q, int M, const uint8_t* lib, int k, int32_t* idx_out,
                          int32_t* common_out, int32_t* union_out);
/* gaudi_fp_neighbours, gaudi_fp_cluster and gaudi_fp_pick_diverse without a handle (and so without a resident library: seeds must
 * be given when S > 0): plain loops over every pair with the same comparison functions (csrc/fp_select.inc).  Test surface, not a
 * CPU fallback. */
int gaudi_host_fp_neighbours(int n_bins, int N, const uint8_t* rows, int thr_num, int thr_den, int32_t* count_out, int64_t capacity,
                             int64_t* offsets_out, int32_t* list_out);
int gaudi_host_fp_cluster(int n_bins, int N, const uint8_t* rows, int thr_num, int thr_den, int32_t* cluster_out,
                          int32_t* centroid_out, int32_t* size_out, int32_t* count_out, int32_t* n_clusters_out);
int gaudi_host_fp_pick_diverse(int n_bins, int N, const uint8_t* rows, int S, const uint8_t* seeds, int first, int k, int thr_num,
                               int thr_den, int32_t* picked_out, int32_t* pick_common_out, int32_t* pick_union_out,
                               int32_t* n_picked_out, int32_t* owner_out, int32_t* owner_common_out, int32_t* owner_union_out);
/* The layout gaudi_predictor_loss_grad reads the predictor in (pred_train_host.inc: pt_layout): off_out[4 + 13 L] = float
 * offset of each role inside the names-order flat buffer (-1: absent; head: embedding w/b, embedding_out w/b; per layer:
 * edge_mlp.0 w/b, edge_mlp.2 w/b, att_mlp.0 w/b, coord_mlp.0 w/b, coord_mlp.2 w, node_mlp.0 w/b, node_mlp.2 w/b),
 * has_grad_out[n] = the no-gradient-path rule, wt_out (or NULL) = the flat buffer with every matrix transposed.
 * GAUDI_E_MISSING when a known name has the wrong size. */
int gaudi_host_pred_train_layout(const gaudi_pred_config* cfg, int n, const char* const* names, const float* const* tensors,
                                 const int64_t* numel, int32_t* off_out, int32_t* has_grad_out, float* wt_out);
/* The layout gaudi_edm_loss_grad reads the denoiser in (edm_train_host.inc: et_layout): off_out[4 + L (10 S + 5)] = float
 * offset of each role (head: embedding w/b, embedding_out w/b; per block, per GCL: edge_mlp.0 w/b, edge_mlp.2 w/b, att_mlp.0
 * w/b, node_mlp.0 w/b, node_mlp.2 w/b; then gcl_equiv.coord_mlp.0 w/b, .2 w/b, .4 w; -1: absent), has_grad_out[n], and
 * wt_out (or NULL) = the flat buffer with every matrix transposed.  GAUDI_E_MISSING when a known name has the wrong size. */
int gaudi_host_edm_train_layout(const gaudi_edm_config* cfg, int n, const char* const* names, const float* const* tensors,
                                const int64_t* numel, int32_t* off_out, int32_t* has_grad_out, float* wt_out);
/* The chunk scratch per molecule, in floats, of gaudi_predictor_loss_grad (net 0) or gaudi_edm_loss_grad (net 1), counted by
 * the list that carves it (train_host.inc: Carver): the number that, with the scratch budget, sizes a call's chunks.  N padded
 * nodes, H hidden_nf, L n_layers, S inv_sublayers (EDM), F node features without the time column, K out_nf (predictor),
 * A = 24 with sin_embedding, else 2 (EDM; the predictor's is 2). */
int gaudi_host_train_floats_per_mol(int net, int N, int H, int L, int S, int F, int K, int A, int64_t* floats_out);
/* The seed of gaudi_edm_loss_grad's reverse pass, by the function the call uses: d loss_b / d net = coef (net - eps), with
 * coef_out [B][2] = (x columns, h columns) for loss_type (0 l2, 1 vlb), t_int [B] in 0..T, snr_w [B] = SNR(s - t) - 1 (read
 * for vlb at t > 0 only), D = 3 + F, padded N, and weight [B] (or NULL: 1 each). */
int gaudi_host_edm_seed_coef(int loss_type, int B, int T, int D, int N, const int32_t* t_int, const float* snr_w,
                             const float* weight, float* coef_out);
/* The network-free terms of gaudi_edm_nll, computed by the same function: terms_out [B][4] = kl_prior, neg_log_constants,
 * delta_log_px and the SNR weight SNR(gamma_s - gamma_t) - 1 of t_int[b] (1..T) for the schedule of gaudi_host_schedule and
 * normalize_factors (norm_x, norm_h). */
int gaudi_host_nll_terms(int T, float noise_power, float noise_precision, float norm_x, float norm_h, int B, int N, int F,
                         const float* x, const float* onehot, const float* node_mask, const int32_t* t_int, float* terms_out);
/* The live-edge metadata gaudi_* calls derive from (node_mask, edge_mask): per-wave capacity EW (multiple of 32),
 * launch order [B] (heaviest first), 32-edge passes per wave [B][4], per-node segment word [B][N]
 * (wave<<30 | start<<15 | len), the padded per-wave edge lists [B][4][EW] (i | j<<8) with their mask values, and
 * ncols [B] = 1 + the last node that is live or touches a live edge (node-level GEMMs stop there).  Live = mask != 0 and
 * not both endpoints masked (the reference's unmasked "padded ring <-> orientation node" identity edges reach no live
 * node).  edges_capacity = number of entries edges_out / emask_out can hold (B*4*EW needed). */
int gaudi_host_graph_meta(int B, int N, const float* node_mask, const float* edge_mask, int32_t* ew_out,
                          int32_t* order_out, int32_t* npairs_out, uint32_t* seg_out, uint32_t* edges_out,
                          float* emask_out, int32_t edges_capacity, int32_t* ncols_out /* [B] or NULL */);
/* The metadata of the 8-wave kernels (default): per molecule ONE flat slot list = its live edges sorted by receiving node
 * (then sending node), padded to whole 16-slot tiles (tile tau -> wave tau & 7 of the workgroup, round tau >> 3).
 * slots_out = slot capacity of the batch (multiple of 16); ntiles [B]; seg [B][N] = first_slot << 16 | run length of the
 * edges RECEIVED by a node; edge words [B][slots] = i | j << 8 | run_start_column << 16 | run_end << 20 | partial << 21
 * (a node's run touches at most two tiles; partial = 1 for its second tile) with their mask values; soff [B][N+1] / sidx
 * [B][slots] = CSR lists of the slots whose SENDING node is n (ascending), which the reverse pass sums over. */
int gaudi_host_graph_meta8(int B, int N, const float* node_mask, const float* edge_mask, int32_t* slots_out,
                           int32_t* order_out, int32_t* ntiles_out, uint32_t* seg_out, uint32_t* edges_out, float* emask_out,
                           uint16_t* soff_out, uint16_t* sidx_out, int32_t edges_capacity, int32_t* ncols_out);
/* Kernel family of a handle: 8 = eight waves per molecule, two per SIMD (default); 4 = four waves, one per SIMD
 * (environment GAUDI_WAVES=4 at gaudi_create, and the per-call fallback of an 8-wave handle for graphs beyond the 8-wave
 * kernels' limits: more than 128 edge slots with guidance, a node with more than 32 live edges, LDS).  last_call = what the
 * most recent call ran on. */
int gaudi_kernel_variant(const gaudi_handle* h, int32_t* configured, int32_t* last_call);
/* Arithmetic of the GEMMs (edge level: the W2 / Wc1 contractions and their transposes, edm/egnn/egnn_new.py:42-47 and
 * edm/egnn_predictor/gcl.py:225-231; since round 5 the node-level Linears too) on the 8-wave kernels: 1 = every fp32 operand
 * as a pair of fp16 pieces behind exact power-of-two scales, three piece products accumulated in fp32 on the fp16 matrix pipe
 * (rounds 2-4: three bf16 pieces, six products; error against float64 at or below the fp32 matrix instruction's:
 * tests/test_gpu_split.py, tests/test_gpu_round5.py); 0 = v_mfma_f32_16x16x4_f32 (environment GAUDI_EDGE_MATH=fp32 at gaudi_create,
 * the 4-wave kernels, and the per-call fallback when the LDS weight ring of the split form does not fit).  last_call: 1 =
 * split with the full ring (a 32-input chunk of all output tiles per trip), 2 = split with the half ring (two trips per
 * chunk: molecules whose node buffers leave less LDS), 0 = fp32 instructions. */
int gaudi_edge_math(const gaudi_handle* h, int32_t* configured, int32_t* last_call);
/* Where the most recent call kept its [N][hidden] node buffers: 0 = LDS (the resident kernels), 1 = a per-workgroup global
 * scratch -- molecules beyond the LDS limit (about 22 graph nodes at the default widths; the reference has no cap,
 * sampling_edm.py:172-209): the V8G kernels (8 waves, round 4) or, for graphs outside the 8-wave kernels' limits and with
 * GAUDI_GN8=0, the V4G kernels (4 waves; gaudi_kernel_variant tells which); 2 = the V8G kernels' hybrid form (round 6): the global
 * scratch holds three of the five buffers, P and Q stay in LDS (taken where that plan fits; GAUDI_GN8_PQ=0 turns it off); 3 = a WIDE
 * group (two molecules per workgroup) on the full weight ring: everything in LDS except one of the predictor's five buffers
 * (round 6; GAUDI_WIDE_FULL=0: the half ring with all five in LDS, as in round 5 -- the same bits). */
int gaudi_node_buffers(const gaudi_handle* h, int32_t* last_call);
/* Workgroups the most recent kernel launch of the handle ran: the molecules of the call (or of its last sub-batch), or the
 * groups they were packed into; node_slots (may be NULL): node slots per workgroup -- the call's N, or more when the launch
 * ran WIDE groups (below).  bench.py prices its roofline with these figures, not with the host-side plan. */
int gaudi_last_workgroups(const gaudi_handle* h, int32_t* workgroups, int32_t* node_slots);
/* Shader clock (MHz) the chip held during the most recent PROFILED sampler launch (gaudi_profile_reset(h, 1)): cycles of the
 * shader clock over ticks of the constant 100 MHz counter, both read by workgroup 0 at kernel entry and at the end of its last
 * step.  0 if no profiled launch has run.  The roofline peaks in bench.py assume the nominal 2.4 GHz; under this kernel's load
 * the chip runs at 1.7-2.0 GHz. */
int gaudi_profile_clock(gaudi_handle* h, double* shader_mhz);
/* Floats of LDS the most recent call gave to a KEPT split copy of h (round 6; 0: none -- no room in 160 KiB, a kernel family
 * without fp16-pair node GEMMs, or GAUDI_KEEP_H=0 at gaudi_create).  With it the node GEMMs that read h (P, Q, the node MLP's first
 * Linear: edm/egnn/egnn_new.py:59-73,119-128, edm/egnn_predictor/gcl.py:240-250) split it into fp16 pairs once per change of h
 * instead of once per GEMM; the copy is a function of h alone, results do not change by a bit. */
int gaudi_last_keep_h(const gaudi_handle* h, int32_t* lds_floats);
/* Per-molecule kernel family (round 6).  gaudi_sample sorts a request whose padded N is beyond the resident kernels' LDS limit
 * into the molecules that fit those kernels on their own (at most as many live nodes as the widest resident group takes, one round
 * of eight edge tiles -- a function of the molecule's own graph and the hidden sizes, so the choice does not depend on the rest of
 * the batch or on how it is sharded) and the rest; the first bucket runs packed on the resident kernels, the second on the V8G
 * kernels, both with noise keyed by the molecule's index in the request.  resident_molecules: how many molecules of the most
 * recent gaudi_sample call ran in the first bucket (0: the call ran one family).  Matches sampling_edm.py:172-209 (no size cap,
 * mixed sizes in one call).  OPT-IN (environment GAUDI_FAMILY_SPLIT=1 at gaudi_create): the two buckets are two launches per 25
 * steps on one stream, each with its own tail of idle CUs, and BASELINE config 4 read literally measures 76.8 mol/s this way
 * against 84.3 in one family (round 6); results are bit-identical per molecule either way of sharding. */
int gaudi_last_family_split(const gaudi_handle* h, int32_t* resident_molecules);
/* The same plan for WIDE groups (device-free): groups of up to node_slots (>= N) node slots and `tiles` edge tiles.  Opt-in
 * (environment GAUDI_PAIRS at gaudi_create: 0 never = default, 1 for batches of at least two molecules per CU, 2 always): a
 * sampling call then gives a workgroup more node slots than a molecule has -- two 11-ring cata molecules, three or four small
 * hetero ones -- and two rounds of eight edge tiles, so that every node-level weight matrix is streamed from L2 once for all of
 * them.  Results do not depend on the grouping, bit for bit (tests/test_gpu_round4.py); the guided path measured 2 % slower
 * this way at 1024 molecules, which is why it is not the default. */
int gaudi_host_pack_plan_wide(int B, int N, int node_slots, int tiles, const float* node_mask, const float* edge_mask,
                              int32_t* groups_out, int32_t* group_of_out, int32_t* ntiles_out, int32_t* ncols_out);
/* How a sampling call of the 8-wave kernels packs a batch (device-free): small molecules share a workgroup as the components
 * of one disjoint graph -- at most 4 molecules, N node slots and 8 edge tiles of 16 slots per group; a molecule keeps its own
 * tiles, node order, noise stream and per-molecule reductions, so its result does not depend on the packing (tested bit for
 * bit; GAUDI_PACK=0 at gaudi_create turns it off).  groups_out = G; group_of_out[B] = group of every molecule; ntiles_out /
 * ncols_out [>= G] = edge tiles and node columns of each group (what bench.py counts the issued matrix instructions from).
 * No reference counterpart (the reference batches dense N x N tensors, sampling_edm.py:172-209). */
int gaudi_host_pack_plan(int B, int N, const float* node_mask, const float* edge_mask, int32_t* groups_out, int32_t* group_of_out,
                         int32_t* ntiles_out, int32_t* ncols_out);
/* Plan hint for shards of a larger logical batch (gaudi_amd/dist.py; no reference counterpart: the reference runs one
 * process).  The kernel family and the edge-GEMM arithmetic of a call are chosen from batch-wide maxima -- the largest
 * number of 16-edge slots of a molecule (gaudi_host_graph_meta8: slots_out) and whether any node has more than 32 live edges
 * (gaudi_host_graph_meta8 returns GAUDI_E_CAPACITY) -- so two shards of one batch could otherwise run different arithmetic
 * and the gathered result would depend on the cut.  min_slots: plan every following call as if its batch held a molecule
 * with that many slots (0 = no hint); force_waves: 4 = run every following call on the 4-wave kernels, 0 = automatic.
 * gaudi_sample applies the same rule by itself to the sub-batches it cuts a large request into. */
int gaudi_set_plan_hint(gaudi_handle* h, int32_t min_slots, int32_t force_waves);
/* Tile packing of a weight block W[o][col0+k] (o,k < H, row stride ldw) into [HP/16][HP/16][16][16]
 * (k-chunk major), optionally transposed: the layout every GEMM of the kernels streams. */
int gaudi_host_pack_matrix(int H, int ldw, int col0, int HP, int transpose, const float* W, float* packed_out);
/* Split image of the same block (what the default 8-wave EDGE GEMMs stream; csrc/w8_split.h, round 5: fp16 pairs): packed_out
 * holds ceil(T/2) * T * 2 units of 1 KiB (T = HP/16), unit (m, t, p) = piece p of output tile t against the 32-input chunk m:
 * piece 0 = fp16(w * scale), piece 1 = fp16(w * scale - piece 0), round to nearest even (|w * scale - p0 - p1| <= 2^-22 |w * scale|
 * while piece 1 is a normal fp16 number; scale = a power of two, gaudi_host_weight_scale); lane L = (row L & 15, group g = L >> 4)
 * holds 8 fp16: slots 0-3 = inputs 16(2m) + 4g .. +3, slots 4-7 = inputs 16(2m+1) + 4g .. +3.  ktail != 0 and H % 16 == 4 with
 * an odd T >= 3: the last chunk holds the 4 tail inputs as T fp32 tiles of w * scale instead (float4 index (k % 16) * 16 + o % 16
 * of tile t, element 0). */
int gaudi_host_pack_matrix_split(int H, int ldw, int col0, int HP, int transpose, int ktail, float scale, const float* W,
                                 float* packed_out);
/* fp16-pair image of a NODE-GEMM matrix (csrc/w8_nodes_f16.h): packed_out holds HP * HP floats = (T / 2) * T * 2 units of 1 KiB,
 * unit (m, t, p) as above but lane L = (row L & 15, group g = L >> 4) holds inputs 32 m + 8 g .. +7, piece 0 = fp16(w * scale),
 * piece 1 = fp16((w * scale - piece 0) * 2^11); an odd T leaves the last 16 inputs as a trailing block of T * 256 fp32 values,
 * UNSCALED, [tile][k-step q][lane (row, g)] = w[row][16 (T - 1) + 4 q + g]. */
int gaudi_host_pack_matrix_f16(int H, int ldw, int col0, int HP, int transpose, float scale, const float* W, float* packed_out);
/* The power-of-two scale gaudi_load_edm / gaudi_load_predictor give a network's weight images: the largest finite |w| of the n
 * blocks (rows[i] x cols[i], row stride ldw[i]) lands in [2^13, 2^14).  0: refused -- an infinite weight, or a block whose largest
 * entry lies more than 2^17 below the largest of all (the blocks are judged as edge-level matrices; node-level ones may lie 2^25
 * below: round 6, through round 5 the rule was 2^12 for all) -- such a network runs the fp32-instruction kernels, and the load
 * leaves a warning (gaudi_last_warning). */
int gaudi_host_weight_scale(int n, const float* const* blocks, const int32_t* rows, const int32_t* cols, const int32_t* ldw,
                            float* scale_out);
/* LDS layout of the fp16-pair node GEMMs' activation copies (csrc/w8_nodes_f16.h; no reference counterpart: the reference's
 * node-level nn.Linear calls, egnn_new.py:42-89 / models.py:520-551, have no operand staging).  Float offset, inside the copy of
 * `column_tiles` tiles of 16 node columns, of the 16 bytes that hold inputs 32 chunk + 8 g .. + 7 of node column c (piece 0; piece 1
 * lies 256 floats further).  The layout is a performance contract the CPU suite checks: the 16 lanes (c = 0..15) of one g read 256
 * consecutive bytes, and the 32 lanes of one store pass of a row's split (4 chunks x 4 g x 2 halves) hit 64 different banks. */
int gaudi_host_node_operand_offset(int column_tiles, int chunk, int tile, int c, int g, int32_t* float_offset_out);

/* Kernel timing with HIP events on the handle's own stream (bench.py roofline).
 * gaudi_profile_reset enables collection; gaudi_profile_get returns the number of step-kernel
 * launches since the reset and their summed duration. */
int gaudi_profile_reset(gaudi_handle* h, int enable);
int gaudi_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms, int64_t* steps_done);

/* Override the node count the predictor readout divides by (EGNN_predictor.forward takes the mean over
 * the PADDED N, egnn_predictor/models.py:457).  0 (default) = the N of each call. */
int gaudi_set_readout_nodes(gaudi_handle* h, int n_pad);

/* fix_noise=True of EnVariationalDiffusion.sample / sample_guidance (en_diffusion.py:562-566, 972-978, 1022-1028): while
 * enabled, every molecule of a gaudi_sample / gaudi_sample_cb / gaudi_sample_chain call receives the raw N(0,1) draws of ONE
 * sample -- the Philox stream of global sample index key_sample, or, with injected noise, a buffer [T+2][1][N][3+F] --
 * masked and mean-centred per molecule exactly as the reference broadcasts its [1,N,.] randn over the batch. */
int gaudi_set_fix_noise(gaudi_handle* h, int enable, int64_t key_sample);

/* Tuning knob: reverse steps fused into one kernel launch (default 25). */
int gaudi_set_steps_per_launch(gaudi_handle* h, int steps);

#ifdef __cplusplus
}
#endif
#endif /* GAUDI_HIP_H */
