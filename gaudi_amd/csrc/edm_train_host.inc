// edm_train_host.inc -- EDM training half of the C ABI (included at the end of gaudi_hip.hip): the denoiser in torch layout
// kept next to the sampler's packed images, gaudi_edm_set_train_weights and gaudi_edm_loss_grad (edm_train.h describes the
// kernels).
#include "edm_train.h"

struct EdmTrainState {
  std::vector<std::string> names;     // the names passed to gaudi_load_edm, in order
  std::vector<int64_t> numel, start;  // per tensor
  std::vector<int32_t> has_grad;
  std::vector<int> off;               // gaudi_etrain::n_slots(S, L) float offsets (-1 absent)
  int64_t total = 0;
  DevBuf w, wt, doff, grad, scratch, jobs, tiles, in, net, sums;
  void release() {
    DevBuf* bufs[] = {&w, &wt, &doff, &grad, &scratch, &jobs, &tiles, &in, &net, &sums};
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
// en_diffusion.py:216-218, and buffer is a buffer; neither is a role).  Host only: start / off / has_grad per tensor, and
// wt = the flat buffer with every matrix transposed (NULL: skip).  Returns 0, or the name of a tensor whose size does not
// match its role.
static const char* et_layout(const gaudi_edm_config* cfg, int n, const char* const* names, const float* const* tensors,
                             const int64_t* numel, std::vector<int64_t>& start, std::vector<int>& off,
                             std::vector<int32_t>& has_grad, float* wt) {
  using namespace gaudi_etrain;
  const int H = cfg->hidden_nf, L = cfg->n_layers, S = cfg->inv_sublayers, F1 = cfg->in_node_nf + 1;
  const int A = cfg->sin_embedding ? 24 : 2, ld1 = 2 * H + A;
  start.resize(n);
  has_grad.assign(n, 0);
  off.assign(n_slots(S, L), -1);
  int64_t total = 0;
  std::map<std::string, int> idx;
  for (int i = 0; i < n; ++i) {
    start[i] = total;
    total += numel[i];
    idx[names[i]] = i;
    if (wt && tensors) std::copy(tensors[i], tensors[i] + numel[i], wt + start[i]);
  }
  const char* bad = nullptr;
  auto see = [&](int slot, const std::string& name, int rows, int cols) {
    auto it = idx.find(name);
    if (it == idx.end()) return;
    const int i = it->second;
    if (numel[i] != (int64_t)rows * cols) {
      if (!bad) bad = names[i];
      return;
    }
    off[slot] = (int)start[i];
    has_grad[i] = 1;
    if (wt && tensors && rows > 1 && cols > 1)
      for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) wt[start[i] + (int64_t)c * rows + r] = tensors[i][(int64_t)r * cols + c];
  };
  const std::string p = "dynamics.egnn.";
  see(EMB_W, p + "embedding.weight", H, F1);
  see(EMB_B, p + "embedding.bias", H, 1);
  see(OUT_W, p + "embedding_out.weight", F1, H);
  see(OUT_B, p + "embedding_out.bias", F1, 1);
  for (int l = 0; l < L; ++l) {
    const std::string blk = p + "e_block_" + std::to_string(l) + ".";
    for (int s = 0; s < S; ++s) {
      const std::string q = blk + "gcl_" + std::to_string(s) + ".";
      const int o = gcl_slot(S, l, s, 0);
      see(o + E0W, q + "edge_mlp.0.weight", H, ld1);
      see(o + E0B, q + "edge_mlp.0.bias", H, 1);
      see(o + E2W, q + "edge_mlp.2.weight", H, H);
      see(o + E2B, q + "edge_mlp.2.bias", H, 1);
      if (cfg->attention) {
        see(o + AW, q + "att_mlp.0.weight", 1, H);
        see(o + AB, q + "att_mlp.0.bias", 1, 1);
      }
      see(o + N0W, q + "node_mlp.0.weight", H, 2 * H);
      see(o + N0B, q + "node_mlp.0.bias", H, 1);
      see(o + N2W, q + "node_mlp.2.weight", H, H);
      see(o + N2B, q + "node_mlp.2.bias", H, 1);
    }
    const std::string q = blk + "gcl_equiv.coord_mlp.";
    const int o = equiv_slot(S, l, 0);
    see(o + C0W, q + "0.weight", H, ld1);
    see(o + C0B, q + "0.bias", H, 1);
    see(o + C2W, q + "2.weight", H, H);
    see(o + C2B, q + "2.bias", H, 1);
    see(o + C4W, q + "4.weight", 1, H);
  }
  return bad;
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
  EdmTrainState& s = *h->et;
  std::vector<int64_t> start;
  std::vector<int> off;
  std::vector<int32_t> has;
  int64_t total = 0;
  for (int i = 0; i < n; ++i) total += numel[i];
  std::vector<float> w((size_t)total), wt((size_t)total);
  const char* bad = et_layout(cfg, n, names, tensors, numel, start, off, has, wt.data());
  if (bad) return fail(h, GAUDI_E_MISSING, std::string("EDM tensor mis-shaped: ") + bad);
  for (int i = 0; i < n; ++i) std::copy(tensors[i], tensors[i] + numel[i], w.begin() + start[i]);
  s.names.assign(names, names + n);
  s.numel.assign(numel, numel + n);
  s.start = start;
  s.off = off;
  s.has_grad = has;
  s.total = total;
  HIPCHECK(h, s.w.reserve(sizeof(float) * std::max<size_t>(w.size(), 1)));
  HIPCHECK(h, s.wt.reserve(sizeof(float) * std::max<size_t>(wt.size(), 1)));
  HIPCHECK(h, s.doff.reserve(sizeof(int) * s.off.size()));
  HIPCHECK(h, hipMemcpy(s.w.p, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice));
  HIPCHECK(h, hipMemcpy(s.wt.p, wt.data(), sizeof(float) * wt.size(), hipMemcpyHostToDevice));
  HIPCHECK(h, hipMemcpy(s.doff.p, s.off.data(), sizeof(int) * s.off.size(), hipMemcpyHostToDevice));
  return GAUDI_OK;
}

// floats of chunk scratch per molecule (edm_train.h)
static int64_t et_floats_per_mol(int N, int H, int L, int S, int F, int A) {
  const int64_t E = (int64_t)N * N, F1 = F + 1, D = 3 + F;
  return ((int64_t)L * (S + 1) + 1) * N * H + (int64_t)(L + 1) * N * 4 + N * F1 + N * D + E * (A / 2) + E * A + 8 * E +
         2 * E + 9LL * N * H + 4LL * N + N * F1 + 6 * E * H + 5 * E;
}

// chunk size: the largest batch slice whose scratch fits in 1 GiB, or in GAUDI_EDM_TRAIN_SCRATCH_KB (tests of the chunked path)
static int64_t et_scratch_bytes() {
  if (const char* e = getenv("GAUDI_EDM_TRAIN_SCRATCH_KB")) {
    const long long kb = atoll(e);
    if (kb > 0) return kb * 1024LL;
  }
  return 1LL << 30;
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
  using gaudi_train::OuterJob;
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
  const int64_t per = et_floats_per_mol(N, H, L, S, F, A);
  const int Bc = (int)std::max<int64_t>(1, std::min<int64_t>(B, et_scratch_bytes() / (int64_t)sizeof(float) / per));
  HIPCHECK(h, s.scratch.reserve(sizeof(float) * (size_t)per * Bc));
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
  ETBufs b{};
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
  b.F = F;
  b.H = H;
  b.L = L;
  b.S = S;
  b.N = N;
  b.A = A;
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
  {
    float* q = s.scratch.as<float>();
    auto take = [&](int64_t cnt) {
      float* r = q;
      q += cnt * Bc;
      return r;
    };
    b.hs = take(((int64_t)L * (S + 1) + 1) * N * H);
    b.xs = take((int64_t)(L + 1) * N * 4);
    b.hin = take((int64_t)N * F1);
    b.eps = take((int64_t)N * D);
    b.d0a = take((int64_t)E * (A / 2));
    b.ea = take((int64_t)E * A);
    b.diff = take(4LL * E);
    b.dcd = take(4LL * E);
    b.rad = take(E);
    b.drad = take(E);
    float** node[] = {&b.P, &b.Q, &b.agg, &b.qp, &b.q, &b.dr, &b.dP, &b.dQ, &b.dh};
    for (float** r : node) *r = take((int64_t)N * H);
    b.dx = take(4LL * N);
    b.dhout = take((int64_t)N * F1);
    float** edge[] = {&b.U, &b.Sx, &b.V, &b.M, &b.EF, &b.DE};
    for (float** r : edge) *r = take((int64_t)E * H);
    float** sc[] = {&b.gate, &b.dap, &b.phi, &b.ppre, &b.dp};
    for (float** r : sc) *r = take(E);
  }

  // the weight-gradient products per reverse launch (gcl_equiv, then the GCLs from the last, per block from the last;
  // then the head), per chunk size
  std::vector<OuterJob> jobs;
  std::vector<int4> tiles;
  std::vector<std::pair<int, int>> launches;
  if (rev) {
    HIPCHECK(h, s.grad.reserve(sizeof(float) * (size_t)std::max<int64_t>(s.total, 1)));
    HIPCHECK(h, hipMemsetAsync(s.grad.p, 0, sizeof(float) * (size_t)s.total, h->stream));
    float* G = s.grad.as<float>();
    const int* o0 = s.off.data();
    const int ld1 = 2 * H + A;
    auto job = [&](const float* Yp, int ldy, int M, const float* Xp, int ldx, int Kc, int off, int ldg, int R) {
      jobs.push_back(OuterJob{Yp, Xp, G + off, ldy, ldx, ldg, M, Kc, R});
      for (int m0 = 0; m0 < M; m0 += 32)
        for (int k0 = 0; k0 < Kc; k0 += 32) tiles.push_back(make_int4((int)jobs.size() - 1, m0, k0, 0));
    };
    auto hst = [&](int l, int sub) { return b.hs + (size_t)(l * (S + 1) + sub) * Bc * N * H; };
    // the first two layers of an edge MLP: W1 = [A | B | C] over [h_i | h_j | ea], b1, W2, b2
    auto edge_jobs = [&](const float* hl, int w1, int b1, int w2, int b2, int Rn, int Re) {
      job(b.dP, H, H, hl, H, H, w1, ld1, Rn);
      job(b.dQ, H, H, hl, H, H, w1 + H, ld1, Rn);
      job(b.U, H, H, b.ea, A, A, w1 + 2 * H, ld1, Re);
      job(b.dP, H, H, nullptr, 0, 1, b1, 1, Rn);
      job(b.V, H, H, b.Sx, H, H, w2, H, Re);
      job(b.V, H, H, nullptr, 0, 1, b2, 1, Re);
    };
    auto plan = [&](int bc) {
      const int Rn = bc * N, Re = bc * E;
      for (int l = L - 1; l >= 0; --l) {
        int first = (int)tiles.size();
        const int* o = o0 + equiv_slot(S, l, 0);
        edge_jobs(hst(l, S), o[C0W], o[C0B], o[C2W], o[C2B], Rn, Re);
        job(b.dp, 1, 1, b.M, H, H, o[C4W], H, Re);
        launches.push_back({first, (int)tiles.size() - first});
        for (int sub = S - 1; sub >= 0; --sub) {
          first = (int)tiles.size();
          const int* g = o0 + gcl_slot(S, l, sub, 0);
          const float* hl = hst(l, sub);
          edge_jobs(hl, g[E0W], g[E0B], g[E2W], g[E2B], Rn, Re);
          if (c.attention) {
            job(b.dap, 1, 1, b.M, H, H, g[AW], H, Re);
            job(b.dap, 1, 1, nullptr, 0, 1, g[AB], 1, Re);
          }
          job(b.qp, H, H, hl, H, H, g[N0W], 2 * H, Rn);
          job(b.qp, H, H, b.agg, H, H, g[N0W] + H, 2 * H, Rn);
          job(b.qp, H, H, nullptr, 0, 1, g[N0B], 1, Rn);
          job(b.dr, H, H, b.q, H, H, g[N2W], H, Rn);
          job(b.dr, H, H, nullptr, 0, 1, g[N2B], 1, Rn);
          launches.push_back({first, (int)tiles.size() - first});
        }
      }
      const int first = (int)tiles.size();
      job(b.dhout, F1, F1, hst(L, 0), H, H, o0[OUT_W], H, Rn);
      job(b.dhout, F1, F1, nullptr, 0, 1, o0[OUT_B], 1, Rn);
      job(b.dh, H, H, b.hin, F1, F1, o0[EMB_W], F1, Rn);
      job(b.dh, H, H, nullptr, 0, 1, o0[EMB_B], 1, Rn);
      launches.push_back({first, (int)tiles.size() - first});
    };
    plan(Bc);
    if (B % Bc) plan(B % Bc);
    HIPCHECK(h, s.jobs.reserve(sizeof(OuterJob) * jobs.size()));
    HIPCHECK(h, s.tiles.reserve(sizeof(int4) * tiles.size()));
    HIPCHECK(h, hipMemcpyAsync(s.jobs.p, jobs.data(), sizeof(OuterJob) * jobs.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHECK(h, hipMemcpyAsync(s.tiles.p, tiles.data(), sizeof(int4) * tiles.size(), hipMemcpyHostToDevice, h->stream));
  }
  const OuterJob* djobs = s.jobs.as<OuterJob>();
  const int4* dtiles = s.tiles.as<int4>();
  const size_t per_plan = (size_t)L * (S + 1) + 1;  // reverse launches of one chunk's plan

  for (int b0 = 0; b0 < B; b0 += Bc) {
    const int bc = std::min(Bc, B - b0);
    b.b0 = b0;
    HIPCHECK(h, (hipError_t)gaudi_et_embed(b, bc, h->stream));
    for (int l = 0; l < L; ++l) HIPCHECK(h, (hipError_t)gaudi_et_block(b, bc, l, h->stream));
    HIPCHECK(h, (hipError_t)gaudi_et_readout(b, bc, rev ? 1 : 0, h->stream));
    if (!rev) continue;
    size_t li = bc == Bc ? 0 : per_plan;
    for (int l = L - 1; l >= 0; --l) {
      HIPCHECK(h, (hipError_t)gaudi_et_equiv_reverse(b, bc, l, h->stream));
      HIPCHECK(h, (hipError_t)gaudi_pt_outer(djobs, dtiles + launches[li].first, launches[li].second, h->stream));
      ++li;
      for (int sub = S - 1; sub >= 0; --sub) {
        HIPCHECK(h, (hipError_t)gaudi_et_gcl_reverse(b, bc, l, sub, h->stream));
        HIPCHECK(h, (hipError_t)gaudi_pt_outer(djobs, dtiles + launches[li].first, launches[li].second, h->stream));
        ++li;
      }
    }
    HIPCHECK(h, (hipError_t)gaudi_pt_outer(djobs, dtiles + launches[li].first, launches[li].second, h->stream));
  }
  std::vector<float> sums((size_t)B * 4);
  HIPCHECK(h, hipMemcpyAsync(sums.data(), s.sums.p, sizeof(float) * B * 4, hipMemcpyDeviceToHost, h->stream));
  if (net_out) HIPCHECK(h, hipMemcpyAsync(net_out, s.net.p, sizeof(float) * (size_t)B * N * D, hipMemcpyDeviceToHost, h->stream));
  std::vector<float> g(rev ? (size_t)s.total : 0);
  if (rev) HIPCHECK(h, hipMemcpyAsync(g.data(), s.grad.p, sizeof(float) * (size_t)s.total, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  for (int b0 = 0; b0 < B; ++b0) loss_out[b0] = et_loss(loss_type, t_int[b0], T, D, N, &terms[4 * b0], &sums[4 * b0]);
  if (rev)
    for (size_t i = 0; i < s.numel.size(); ++i) {
      has_grad_out[i] = s.has_grad[i];
      if (s.has_grad[i]) std::copy(g.begin() + s.start[i], g.begin() + s.start[i] + s.numel[i], grad_out + s.start[i]);
    }
  return GAUDI_OK;
}

}  // extern "C"
