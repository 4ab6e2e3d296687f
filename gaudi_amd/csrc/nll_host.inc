// nll_host.inc -- the EDM's negative log-likelihood of data (included at the end of gaudi_hip.hip): EnVariationalDiffusion.forward
// in eval mode (en_diffusion.py:777-805 -> compute_loss with t0_always = True, :646-775).  The two network passes and their sums
// run in one MODE_NLL launch of the EDM-only kernels (sampler_kernel.h); everything that does not need the network is computed
// here, by the one function the CPU tests call through gaudi_host_nll_terms.

// Network-free terms of molecule b -> out[b][4] = kl_prior, neg_log_constants, delta_log_px, SNR weight (SNR(gamma_s - gamma_t) - 1).
// fp32 in the reference's order of operations: kl_prior is a difference of nearly equal numbers (sigma_T is 1 - 5e-6 at the
// default precision), so it is only reproducible as the same sequence of float operations.
static int nll_host_terms(const float* gamma, int T, float nv0, float nv1, int B, int N, int F, const float* x, const float* onehot,
                          const float* node_mask, const int32_t* t_int, float* out, std::string& err) {
  const float gT = gamma[T], g0 = gamma[0];
  const float alpha_T = sqrtf(sigmoid_host(-gT)), sigma_T = sqrtf(sigmoid_host(gT));  // alpha / sigma (:365-377) at gamma(1)
  const float log_nv0 = (float)std::log((double)nv0);
  const float half_log_2pi = (float)(0.5 * std::log(2.0 * 3.14159265358979323846));
  for (int b = 0; b < B; ++b) {
    if (t_int[b] < 1 || t_int[b] > T) {
      err = "t_int[" + std::to_string(b) + "] = " + std::to_string(t_int[b]) + ": the NLL draws t from 1..T (t0_always, en_diffusion.py:657-659)";
      return GAUDI_E_INVALID;
    }
    const float* m = node_mask + (size_t)b * N;
    float n = 0.f;
    for (int i = 0; i < N; ++i) n += m[i];
    const float dof = (n - 1.0f) * 3.0f;  // subspace_dimensionality (:380-382)
    // kl_prior (:459-491): h part gaussian_KL against N(0, 1), masked (:90-108) ...
    float kl_h = 0.f;
    for (int i = 0; i < N; ++i)
      for (int k = 0; k < F; ++k) {
        const float xh = (onehot[((size_t)b * N + i) * F + k] - 0.0f) / nv1 * m[i];
        const float mu = alpha_T * xh;
        kl_h += (logf(1.0f / sigma_T) + 0.5f * (sigma_T * sigma_T + mu * mu) / 1.0f - 0.5f) * m[i];
      }
    // ... x part on the (n - 1) * 3 dimensional subspace (:111-129)
    float mu2 = 0.f;
    for (int i = 0; i < N; ++i)
      for (int d = 0; d < 3; ++d) {
        const float mu = alpha_T * (x[((size_t)b * N + i) * 3 + d] / nv0);
        mu2 += mu * mu;
      }
    const float kl_x = dof * logf(1.0f / sigma_T) + 0.5f * (dof * (sigma_T * sigma_T) + mu2) / 1.0f - 0.5f * dof;
    out[4 * b + 0] = kl_x + kl_h;
    out[4 * b + 1] = -(dof * (-(0.5f * g0) - half_log_2pi));  // -log_constants_p_x_given_z0 (:517-531)
    out[4 * b + 2] = -dof * log_nv0;                           // normalize (:384-387)
    out[4 * b + 3] = expf(-(gamma[t_int[b] - 1] - gamma[t_int[b]])) - 1.0f;  // (:701-703)
  }
  return GAUDI_OK;
}

static int run_edm_nll(gaudi_handle* h, int B, int N, const float* x, const float* onehot, const int32_t* t_int,
                       const float* node_mask, const float* edge_mask, uint64_t seed, int64_t sample_offset, const float* noise,
                       float* nll_out, float* terms_out) {
  if (!h->has_edm) return fail(h, GAUDI_E_STATE, "EDM weights not loaded");
  if (h->edm_stale) return fail(h, GAUDI_E_STATE, kEdmStale);
  if (B <= 0 || N <= 0) return fail(h, GAUDI_E_INVALID, "B and N must be positive");
  if (N > 255) return fail(h, GAUDI_E_CAPACITY, "N must be at most 255");  // (one node slot per thread in the MODE_NLL sums)
  HIPCHECK(h, hipSetDevice(h->device));
  const int T = h->ecfg.diffusion_steps, F = h->ecfg.in_node_nf, D = 3 + F;
  const float nv0 = h->ecfg.norm_values[0], nv1 = h->ecfg.norm_values[1];
  std::vector<float> host((size_t)B * 4);
  std::string err;
  int rc = nll_host_terms(h->gamma.data(), T, nv0, nv1, B, N, F, x, onehot, node_mask, t_int, host.data(), err);
  if (rc) return fail(h, rc, err);
  std::vector<float> as((size_t)B * 2), tval(B), xh((size_t)B * N * D);
  for (int b = 0; b < B; ++b) {
    const float g = h->gamma[t_int[b]];
    as[2 * b] = sqrtf(sigmoid_host(-g));
    as[2 * b + 1] = sqrtf(sigmoid_host(g));
    tval[b] = (float)t_int[b] / (float)T;
    for (int n = 0; n < N; ++n) {
      float* dst = &xh[((size_t)b * N + n) * D];
      for (int d = 0; d < 3; ++d) dst[d] = x[((size_t)b * N + n) * 3 + d];
      for (int k = 0; k < F; ++k) dst[3 + k] = onehot[((size_t)b * N + n) * F + k];
    }
  }
  KParams P{};
  // (the default hints do not pack: one EDM pass takes one t per workgroup, molecules with different t cannot share one)
  rc = stage_graph(h, B, N, node_mask, edge_mask, P, h->HPE, 0, CallHints{});
  if (rc) return rc;
  fill_edm(h, P);
  const size_t zb = sizeof(float) * B * N * D;
  HIPCHECK(h, h->d_zin.reserve(zb));
  HIPCHECK(h, h->d_zout.reserve(zb));
  HIPCHECK(h, h->d_t.reserve(sizeof(float) * B));
  HIPCHECK(h, h->d_as.reserve(sizeof(float) * 2 * B));
  HIPCHECK(h, h->d_pred.reserve(sizeof(float) * 4 * B));
  HIPCHECK(h, hipMemcpyAsync(h->d_zin.p, xh.data(), zb, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(h->d_t.p, tval.data(), sizeof(float) * B, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(h->d_as.p, as.data(), sizeof(float) * 2 * B, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemsetAsync(h->d_pred.p, 0, sizeof(float) * 4 * B, h->stream));
  if (noise) {  // [2][B][N][D]: draw 0 = eps, draw 1 = eps_0
    HIPCHECK(h, h->d_noise.reserve(2 * zb));
    HIPCHECK(h, hipMemcpyAsync(h->d_noise.p, noise, 2 * zb, hipMemcpyHostToDevice, h->stream));
    P.noise = h->d_noise.as<float>();
  }
  P.draw_base = 0;
  P.draw_stride = (long long)B * N * D;
  P.seed = seed;
  P.sample_offset = sample_offset;
  P.mode = MODE_NLL;
  P.z_in = h->d_zin.as<float>();
  P.z_out = h->d_zout.as<float>();
  P.alpha_sigma = h->d_as.as<float>();
  P.t_in = h->d_t.as<float>();
  P.pred_out = h->d_pred.as<float>();
  rc = launch(h, P, h->HPE, 0, 0);
  if (rc) return rc;
  std::vector<float> sums((size_t)B * 4);
  HIPCHECK(h, hipMemcpyAsync(sums.data(), h->d_pred.p, sizeof(float) * 4 * B, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  for (int b = 0; b < B; ++b) {
    const float kl = host[4 * b], nlc = host[4 * b + 1], dlp = host[4 * b + 2], snr = host[4 * b + 3];
    const float error = sums[4 * b], err0 = sums[4 * b + 1], log_ph_cat = sums[4 * b + 2];
    const float loss_t = (float)T * (0.5f * snr * error);             // num_terms * loss_t (:737-739)
    const float log_pxh = -0.5f * err0 + (0.0f + log_ph_cat);         // (:597-599, 639-642; no integer part)
    const float loss_0 = -log_pxh;
    if (nll_out) nll_out[b] = (((kl + loss_t) + nlc) + loss_0) - dlp;  // (:756, 803)
    if (terms_out) {
      float* o = terms_out + (size_t)b * 6;
      o[0] = kl; o[1] = loss_t; o[2] = nlc; o[3] = loss_0; o[4] = dlp; o[5] = error;
    }
  }
  return GAUDI_OK;
}

extern "C" {

int gaudi_edm_nll(gaudi_handle* h, int B, int N, const float* x, const float* onehot, const int32_t* t_int, const float* node_mask,
                  const float* edge_mask, uint64_t seed, int64_t sample_offset, const float* noise, float* nll_out, float* terms_out) {
  if (!h || !x || !onehot || !t_int || !node_mask || !edge_mask || (!nll_out && !terms_out)) return GAUDI_E_INVALID;
  return run_edm_nll(h, B, N, x, onehot, t_int, node_mask, edge_mask, seed, sample_offset, noise, nll_out, terms_out);
}

int gaudi_host_nll_terms(int T, float noise_power, float noise_precision, float norm_x, float norm_h, int B, int N, int F,
                         const float* x, const float* onehot, const float* node_mask, const int32_t* t_int, float* terms_out) {
  if (T < 1 || B <= 0 || N <= 0 || F <= 0 || !(noise_power >= 0.f) || !x || !onehot || !node_mask || !t_int || !terms_out)
    return GAUDI_E_INVALID;
  const std::vector<float> g = make_gamma(T, noise_power, noise_precision);
  std::string err;
  return nll_host_terms(g.data(), T, norm_x, norm_h, B, N, F, x, onehot, node_mask, t_int, terms_out, err);
}

}  // extern "C"
