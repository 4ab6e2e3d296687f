// edm_train_host.inc -- EDM training half of the C ABI (included at the end of gaudi_hip.hip after train_host.inc, the core it
// shares with the predictor's half): the denoiser's role table, what its state and scratch add, gaudi_edm_set_train_weights
// and gaudi_edm_loss_grad (edm_train.h describes the kernels).  The torch-layout copy is kept next to the sampler's packed
// images.
#include "edm_train.h"

struct EdmTrainState : TrainState {
  DevBuf in, net, sums;
  void release() {
    TrainState::release();
    DevBuf* bufs[] = {&in, &net, &sums};
    for (DevBuf* b : bufs) b->release();
  }
};

static void et_release(gaudi_handle* h) {
  if (h->et) {
    h->et->release();
    delete h->et;
    h->et = nullptr;
  }
}

// The name -> role table of EGNN_dynamics_QM9's state dict (edm/egnn/models.py:29-45, egnn_new.py:6-312) and the rule for
// which tensors have a gradient path: every dynamics.egnn.* role (gamma.gamma is an nn.Parameter with requires_grad=False,
// en_diffusion.py:216-218, and buffer is a buffer; neither is a role).  Host only (train_host.inc: tr_layout).  Returns 0,
// or the name of a tensor whose size does not match its role.
static const char* et_layout(const gaudi_edm_config* cfg, int n, const char* const* names, const float* const* tensors,
                             const int64_t* numel, std::vector<int64_t>& start, std::vector<int>& off,
                             std::vector<int32_t>& has_grad, float* wt) {
  using namespace gaudi_etrain;
  const int H = cfg->hidden_nf, L = cfg->n_layers, S = cfg->inv_sublayers, F1 = cfg->in_node_nf + 1;
  const int A = cfg->sin_embedding ? 24 : 2, ld1 = 2 * H + A;
  const std::string p = "dynamics.egnn.";
  std::vector<TrainRole> t = {{EMB_W, p + "embedding.weight", H, F1, true},
                              {EMB_B, p + "embedding.bias", H, 1, true},
                              {OUT_W, p + "embedding_out.weight", F1, H, true},
                              {OUT_B, p + "embedding_out.bias", F1, 1, true}};
  for (int l = 0; l < L; ++l) {
    const std::string blk = p + "e_block_" + std::to_string(l) + ".";
    for (int s = 0; s < S; ++s) {
      const std::string q = blk + "gcl_" + std::to_string(s) + ".";
      tr_edge_roles(t, q, H, ld1, cfg->attention, gcl_slot(S, l, s, E0W));
      tr_node_roles(t, q, H, gcl_slot(S, l, s, N0W));
    }
    const std::string q = blk + "gcl_equiv.coord_mlp.";
    const int o = equiv_slot(S, l, 0);
    t.push_back({o + C0W, q + "0.weight", H, ld1, true});
    t.push_back({o + C0B, q + "0.bias", H, 1, true});
    t.push_back({o + C2W, q + "2.weight", H, H, true});
    t.push_back({o + C2B, q + "2.bias", H, 1, true});
    t.push_back({o + C4W, q + "4.weight", 1, H, true});
  }
  return tr_layout(t, n_slots(S, L), n, names, tensors, numel, start, off, has_grad, wt);
}

// gaudi_load_edm's check before it replaces anything: 0, or the name of a tensor whose size does not match its role
static const char* et_check(const gaudi_edm_config* cfg, int n, const char* const* names, const int64_t* numel) {
  std::vector<int64_t> start;
  std::vector<int> off;
  std::vector<int32_t> has;
  return et_layout(cfg, n, names, nullptr, numel, start, off, has, nullptr);
}

// every role the network reads is present (att_mlp only with attention)
static bool et_complete(const gaudi_edm_config* cfg, const std::vector<int>& off) {
  using namespace gaudi_etrain;
  const int S = cfg->inv_sublayers;
  for (int i = 0; i < (int)off.size(); ++i) {
    if (off[i] >= 0 || i < NHEAD) {
      if (off[i] < 0) return false;
      continue;
    }
    const int r = (i - NHEAD) % block_stride(S);
    const bool att = r < S * NGCL && (r % NGCL == AW || r % NGCL == AB);
    if (!(att && !cfg->attention)) return false;
  }
  return true;
}

// the torch-layout copy (and its transposes) the training kernels read; the sampler's images are not touched
static int et_upload(gaudi_handle* h, const gaudi_edm_config* cfg, int n, const char* const* names, const float* const* tensors,
                     const int64_t* numel) {
  if (!h->et) h->et = new EdmTrainState();
  return tr_upload(h, *h->et, "EDM", n, names, tensors, numel,
                   [&](std::vector<int64_t>& start, std::vector<int>& off, std::vector<int32_t>& has, float* wt) {
                     return et_layout(cfg, n, names, tensors, numel, start, off, has, wt);
                   });
}

// the chunk scratch of the EDM, from b's N, H, L, S, F, A (train_host.inc: Carver -- run once to count, once to carve)
static void et_carve(gaudi_etrain::ETBufs& b, Carver& c) {
  const int64_t N = b.N, E = N * N;
  tr_carve(b, c, (int64_t)b.L * (b.S + 1) + 1, b.F + 1, b.F + 1);
  b.eps = c.take(N * (3 + b.F));
  b.d0a = c.take(E * (b.A / 2));
  b.ea = c.take(E * b.A);
  b.drad = c.take(E);
}

// d loss_b / d net = coef (net - eps): coef_out[0] for the x columns, coef_out[1] for the h columns (en_diffusion.py:507-515,
// 694-767 in train mode).  l2: error / (D N) at every t, its x part alone at t = 0; vlb: (T + 1) (SNR(s - t) - 1) at t > 0,
// (T + 1) on the x part at t = 0 (the SNR weight of s = -1 is not read there).
static void et_seed_coef(int loss_type, int t, int T, int D, int N, float snr_w, float weight, float* coef_out) {
  float c;
  if (loss_type == 0) c = weight / ((float)D * (float)N);
  else c = weight * (float)(T + 1) * (t > 0 ? snr_w : 1.0f);
  coef_out[0] = c;
  coef_out[1] = t > 0 ? c : 0.0f;
}

// the per-molecule loss of compute_loss (t0_always = False) minus delta_log_px (en_diffusion.py:694-805) from the kernel sums
// and the network-free terms of nll_host_terms (terms: kl_prior, neg_log_constants, delta_log_px, SNR weight)
static float et_loss(int loss_type, int t, int T, int D, int N, const float* terms, const float* sums) {
  const bool l2 = loss_type == 0;
  const float denom = (float)(D * N);
  const float error = l2 ? sums[0] / denom : sums[0];
  const float error_x = l2 ? sums[1] / denom : sums[1];
  const float snr_w = l2 ? 1.0f : (t > 0 ? terms[3] : 0.0f);
  const float loss_t_gt0 = 0.5f * snr_w * error;
  const float log_pxh = -0.5f * error_x + (0.0f + sums[2]);  // (:585-642; no integer part)
  const float loss_term_0 = -log_pxh;
  const float tz = t == 0 ? 1.0f : 0.0f;
  const float loss_t = t == 0 ? loss_term_0 * tz : (1.0f - tz) * loss_t_gt0;  // (:750-755; the unselected term is not read)
  const float est = l2 ? loss_t : (float)(T + 1) * loss_t;
  const float nlc = l2 ? 0.0f : terms[1];
  const float dlp = l2 ? 0.0f : terms[2];
  return ((terms[0] + est) + nlc) - dlp;
}

const char* const kEdmStale =
    "the sampler's weight images are stale after gaudi_edm_set_train_weights: call gaudi_load_edm with the current weights";

extern "C" {

int gaudi_host_edm_train_layout(const gaudi_edm_config* cfg, int n, const char* const* names, const float* const* tensors,
                                const int64_t* numel, int32_t* off_out, int32_t* has_grad_out, float* wt_out) {
  if (!cfg || n < 0 || (n && (!names || !numel)) || !off_out || !has_grad_out || cfg->n_layers < 1 ||
      cfg->inv_sublayers < 1 || cfg->hidden_nf < 1 || cfg->in_node_nf < 1)
    return GAUDI_E_INVALID;
  std::vector<int64_t> start;
  std::vector<int> off;
  std::vector<int32_t> has;
  if (et_layout(cfg, n, names, tensors, numel, start, off, has, wt_out)) return GAUDI_E_MISSING;
  std::copy(off.begin(), off.end(), off_out);
  std::copy(has.begin(), has.end(), has_grad_out);
  return GAUDI_OK;
}

int gaudi_host_edm_seed_coef(int loss_type, int B, int T, int D, int N, const int32_t* t_int, const float* snr_w,
                             const float* weight, float* coef_out) {
  if ((loss_type != 0 && loss_type != 1) || B < 1 || T < 1 || D < 1 || N < 1 || !t_int || !snr_w || !coef_out)
    return GAUDI_E_INVALID;
  for (int b = 0; b < B; ++b) et_seed_coef(loss_type, t_int[b], T, D, N, snr_w[b], weight ? weight[b] : 1.0f, coef_out + 2 * b);
  return GAUDI_OK;
}

int gaudi_edm_grad_size(gaudi_handle* h, int64_t* n_floats) {
  if (!h || !n_floats) return GAUDI_E_INVALID;
  if (!h->has_edm || !h->et) return fail(h, GAUDI_E_STATE, "EDM weights not loaded");
  *n_floats = h->et->total;
  return GAUDI_OK;
}

int gaudi_edm_set_train_weights(gaudi_handle* h, int n, const char* const* names, const float* const* tensors,
                                const int64_t* numel) {
  if (!h || n < 0 || (n && (!names || !tensors || !numel))) return GAUDI_E_INVALID;
  if (!h->has_edm || !h->et) return fail(h, GAUDI_E_STATE, "EDM weights not loaded: call gaudi_load_edm first");
  const EdmTrainState& s = *h->et;
  if (n != (int)s.names.size()) return fail(h, GAUDI_E_INVALID, "gaudi_edm_set_train_weights: the names of gaudi_load_edm are expected");
  for (int i = 0; i < n; ++i)
    if (s.names[i] != names[i] || s.numel[i] != numel[i])
      return fail(h, GAUDI_E_INVALID, std::string("gaudi_edm_set_train_weights: tensor ") + names[i] +
                                          " differs in name, order or size from gaudi_load_edm's");
  HIPCHECK(h, hipSetDevice(h->device));
  const int rc = et_upload(h, &h->ecfg, n, names, tensors, numel);
  if (rc) return rc;
  h->edm_stale = true;
  return GAUDI_OK;
}

int gaudi_edm_loss_grad(gaudi_handle* h, int B, int N, const float* x, const float* onehot, const int32_t* t_int,
                        const float* node_mask, const float* edge_mask, uint64_t seed, int64_t sample_offset,
                        const float* noise, int loss_type, const float* weight, float* loss_out, float* net_out,
                        float* grad_out, int32_t* has_grad_out) {
  using namespace gaudi_etrain;
  if (!h || !x || !onehot || !t_int || !node_mask || !edge_mask || !loss_out || (grad_out && !has_grad_out))
    return GAUDI_E_INVALID;
  if (!h->has_edm || !h->et) return fail(h, GAUDI_E_STATE, "EDM weights not loaded");
  if (B < 1 || N < 1) return fail(h, GAUDI_E_INVALID, "B and N must be positive");
  if (loss_type != 0 && loss_type != 1) return fail(h, GAUDI_E_INVALID, "loss_type must be 0 (l2) or 1 (vlb)");
  if (N > 128)
    return fail(h, GAUDI_E_CAPACITY, "gaudi_edm_loss_grad: N = " + std::to_string(N) +
                                         " exceeds the training kernels' 128 nodes (dense N x N edge scratch)");
  const gaudi_edm_config& c = h->ecfg;
  const int H = c.hidden_nf, L = c.n_layers, S = c.inv_sublayers, F = c.in_node_nf, F1 = F + 1, D = 3 + F;
  const int A = c.sin_embedding ? 24 : 2, T = c.diffusion_steps, E = N * N;
  for (int b = 0; b < B; ++b)
    if (t_int[b] < 0 || t_int[b] > T)
      return fail(h, GAUDI_E_INVALID, "t_int[" + std::to_string(b) + "] = " + std::to_string(t_int[b]) + " is outside 0..T");
  EdmTrainState& s = *h->et;
  if (!et_complete(&c, s.off)) return fail(h, GAUDI_E_MISSING, "EDM tensor missing for training");
  HIPCHECK(h, hipSetDevice(h->device));
  // network-free terms: the NLL's function; its SNR weight needs t >= 1, so t = 0 asks for t = 1 and does not read it
  std::vector<float> terms((size_t)B * 4), as((size_t)B * 2), tval(B), coef((size_t)B * 2);
  {
    std::vector<int32_t> tq(t_int, t_int + B);
    for (int32_t& t : tq) t = std::max(t, 1);
    std::string err;
    const int rc = nll_host_terms(h->gamma.data(), T, c.norm_values[0], c.norm_values[1], B, N, F, x, onehot, node_mask,
                                  tq.data(), terms.data(), err);
    if (rc) return fail(h, rc, err);
  }
  for (int b = 0; b < B; ++b) {
    const float g = h->gamma[t_int[b]];
    as[2 * b] = sqrtf(sigmoid_host(-g));
    as[2 * b + 1] = sqrtf(sigmoid_host(g));
    tval[b] = (float)t_int[b] / (float)T;
    et_seed_coef(loss_type, t_int[b], T, D, N, terms[4 * b + 3], weight ? weight[b] : 1.0f, &coef[2 * b]);
  }
  const bool rev = grad_out != nullptr;
  ETBufs b{};
  b.F = F;
  b.H = H;
  b.L = L;
  b.S = S;
  b.N = N;
  b.A = A;
  Carver count{nullptr, 0};
  et_carve(b, count);
  const int Bc = tr_chunk(B, count.per, "GAUDI_EDM_TRAIN_SCRATCH_KB");
  HIPCHECK(h, s.scratch.reserve(sizeof(float) * (size_t)count.per * Bc));
  HIPCHECK(h, s.net.reserve(sizeof(float) * (size_t)B * N * D));
  HIPCHECK(h, s.sums.reserve(sizeof(float) * (size_t)B * 4));
  // inputs: x, onehot, t, alpha / sigma, coef, node_mask, edge_mask, noise
  const size_t n_in = (size_t)B * N * 3 + (size_t)B * N * F + B + 2 * B + 2 * B + (size_t)B * N + (size_t)B * E +
                      (noise ? (size_t)B * N * D : 0);
  HIPCHECK(h, s.in.reserve(sizeof(float) * n_in));
  float* p = s.in.as<float>();
  auto put = [&](const float* src, size_t cnt) -> const float* {
    float* dst = p;
    p += cnt;
    return hipMemcpyAsync(dst, src, sizeof(float) * cnt, hipMemcpyHostToDevice, h->stream) == hipSuccess ? dst : nullptr;
  };
  b.x = put(x, (size_t)B * N * 3);
  b.oh = put(onehot, (size_t)B * N * F);
  b.t = put(tval.data(), B);
  b.as = put(as.data(), 2 * B);
  b.coef = put(coef.data(), 2 * B);
  b.nm = put(node_mask, (size_t)B * N);
  b.em = put(edge_mask, (size_t)B * E);
  b.noise = noise ? put(noise, (size_t)B * N * D) : nullptr;
  if (!b.x || !b.oh || !b.t || !b.as || !b.coef || !b.nm || !b.em || (noise && !b.noise))
    return fail(h, GAUDI_E_HIP, "gaudi_edm_loss_grad: input upload failed");
  b.seed = seed;
  b.sample_offset = sample_offset;
  b.net = s.net.as<float>();
  b.sums = s.sums.as<float>();
  b.w = s.w.as<float>();
  b.wt = s.wt.as<float>();
  b.off = s.doff.as<int>();
  b.attention = c.attention;
  b.use_tanh = c.tanh;
  b.sin = c.sin_embedding;
  b.coords_range = c.coords_range;
  b.norm_constant = c.norm_constant;
  b.agg_div = c.normalization_factor > 0.f ? c.normalization_factor : (float)N;
  b.nv0 = c.norm_values[0];
  b.nv1 = c.norm_values[1];
  b.sig_cat = sqrtf(sigmoid_host(h->gamma[0])) * c.norm_values[1];
  b.bcap = Bc;
  Carver carve{s.scratch.as<float>(), Bc};
  et_carve(b, carve);

  // the weight-gradient products per reverse launch: per block from the last, gcl_equiv, then the GCLs from the last; then
  // the head
  OuterPlan plan;
  if (rev) {
    HIPCHECK(h, s.grad.reserve(sizeof(float) * (size_t)std::max<int64_t>(s.total, 1)));
    HIPCHECK(h, hipMemsetAsync(s.grad.p, 0, sizeof(float) * (size_t)s.total, h->stream));
    plan.G = s.grad.as<float>();
    const int* o0 = s.off.data();
    auto hst = [&](int l, int sub) { return b.hs + (size_t)(l * (S + 1) + sub) * Bc * N * H; };
    plan.build(B, Bc, [&](int bc) {
      const int Rn = bc * N, Re = bc * E;
      for (int l = L - 1; l >= 0; --l) {
        plan.begin();
        const int* o = o0 + equiv_slot(S, l, 0);
        plan.edge_jobs(b, hst(l, S), o[C0W], o[C0B], o[C2W], o[C2B], A, Rn, Re, {{b.ea, A}});
        plan.job(b.dp, 1, 1, b.M, H, H, o[C4W], H, Re);
        plan.end();
        for (int sub = S - 1; sub >= 0; --sub) {
          plan.begin();
          const int* g = o0 + gcl_slot(S, l, sub, 0);
          const float* hl = hst(l, sub);
          plan.edge_jobs(b, hl, g[E0W], g[E0B], g[E2W], g[E2B], A, Rn, Re, {{b.ea, A}});
          if (c.attention) plan.att_jobs(b, g[AW], g[AB], Re);
          plan.node_jobs(b, hl, g[N0W], g[N0B], g[N2W], g[N2B], Rn);
          plan.end();
        }
      }
      plan.begin();
      plan.head_jobs(b, hst(L, 0), F1, F1, o0, Rn);
      plan.end();
    });
    const int rc = plan.upload(h, s);
    if (rc) return rc;
  }

  for (int b0 = 0; b0 < B; b0 += Bc) {
    const int bc = std::min(Bc, B - b0);
    b.b0 = b0;
    HIPCHECK(h, (hipError_t)gaudi_et_embed(b, bc, h->stream));
    for (int l = 0; l < L; ++l) HIPCHECK(h, (hipError_t)gaudi_et_block(b, bc, l, h->stream));
    HIPCHECK(h, (hipError_t)gaudi_et_readout(b, bc, rev ? 1 : 0, h->stream));
    if (!rev) continue;
    plan.select(bc);
    size_t li = 0;
    for (int l = L - 1; l >= 0; --l) {
      HIPCHECK(h, (hipError_t)gaudi_et_equiv_reverse(b, bc, l, h->stream));
      HIPCHECK(h, plan.launch(li++, h->stream));
      for (int sub = S - 1; sub >= 0; --sub) {
        HIPCHECK(h, (hipError_t)gaudi_et_gcl_reverse(b, bc, l, sub, h->stream));
        HIPCHECK(h, plan.launch(li++, h->stream));
      }
    }
    HIPCHECK(h, plan.launch(li, h->stream));
  }
  std::vector<float> sums((size_t)B * 4);
  HIPCHECK(h, hipMemcpyAsync(sums.data(), s.sums.p, sizeof(float) * B * 4, hipMemcpyDeviceToHost, h->stream));
  if (net_out) HIPCHECK(h, hipMemcpyAsync(net_out, s.net.p, sizeof(float) * (size_t)B * N * D, hipMemcpyDeviceToHost, h->stream));
  if (rev) {
    const int rc = tr_grads_out(h, s, grad_out, has_grad_out);
    if (rc) return rc;
  } else {
    HIPCHECK(h, hipStreamSynchronize(h->stream));
  }
  for (int b0 = 0; b0 < B; ++b0) loss_out[b0] = et_loss(loss_type, t_int[b0], T, D, N, &terms[4 * b0], &sums[4 * b0]);
  return GAUDI_OK;
}

// The chunk scratch per molecule, in floats, as the carver counts it for a network (0: the predictor, 1: the EDM) of the
// given shape -- the number that sizes a call's chunks.  Defined here, after both networks' lists.
int gaudi_host_train_floats_per_mol(int net, int N, int H, int L, int S, int F, int K, int A, int64_t* floats_out) {
  if ((net != 0 && net != 1) || N < 1 || H < 1 || L < 1 || S < 1 || F < 0 || K < 1 || A < 2 || !floats_out)
    return GAUDI_E_INVALID;
  Carver count{nullptr, 0};
  if (net == 0) {
    gaudi_train::PTBufs b{};
    b.N = N, b.H = H, b.L = L, b.F = F, b.K = K, b.A = 2;
    pt_carve(b, count);
  } else {
    gaudi_etrain::ETBufs b{};
    b.N = N, b.H = H, b.L = L, b.S = S, b.F = F, b.A = A;
    et_carve(b, count);
  }
  *floats_out = count.per;
  return GAUDI_OK;
}

}  // extern "C"
