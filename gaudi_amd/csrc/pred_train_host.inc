// pred_train_host.inc -- predictor training half of the C ABI (included at the end of gaudi_hip.hip): the weights in
// torch layout kept by gaudi_load_predictor, and gaudi_predictor_loss_grad (pred_train.h describes the kernels).
#include "pred_train.h"

struct PredTrainState {
  std::vector<int64_t> numel, start;  // per checkpoint tensor, in the order of the names passed to gaudi_load_predictor
  std::vector<int32_t> has_grad;
  std::vector<int> off;               // gaudi_train::NHEAD + NLAYER * L float offsets (-1 absent)
  int64_t total = 0;
  DevBuf w, wt, doff, grad, scratch, jobs, tiles, y, t, masks;
  void release() {
    DevBuf* bufs[] = {&w, &wt, &doff, &grad, &scratch, &jobs, &tiles, &y, &t, &masks};
    for (DevBuf* b : bufs) b->release();
  }
};

static void pt_release(gaudi_handle* h) {
  if (h->pt) {
    h->pt->release();
    delete h->pt;
    h->pt = nullptr;
  }
}

// The name -> role table of EGNN_predictor's state dict (edm/egnn_predictor/models.py:480-537, gcl.py:181-215) and the
// rule for which parameters have a gradient path: all but the last layer's coord_mlp (its coordinate output is never
// read).  Host only: start / off / has_grad per tensor, and wt = the flat buffer with every matrix transposed (NULL: skip).
// Returns 0, or the name of a tensor whose size does not match its role.
static const char* pt_layout(const gaudi_pred_config* cfg, int n, const char* const* names, const float* const* tensors,
                             const int64_t* numel, std::vector<int64_t>& start, std::vector<int>& off,
                             std::vector<int32_t>& has_grad, float* wt) {
  using namespace gaudi_train;
  const int H = cfg->hidden_nf, L = cfg->n_layers, K = cfg->out_nf, F1 = cfg->in_nf + 1;
  start.resize(n);
  has_grad.assign(n, 0);
  off.assign(NHEAD + NLAYER * L, -1);
  int64_t total = 0;
  std::map<std::string, int> idx;
  for (int i = 0; i < n; ++i) {
    start[i] = total;
    total += numel[i];
    idx[names[i]] = i;
    if (wt && tensors) std::copy(tensors[i], tensors[i] + numel[i], wt + start[i]);
  }
  const char* bad = nullptr;
  auto see = [&](int slot, const std::string& name, int rows, int cols, bool grad) {
    auto it = idx.find(name);
    if (it == idx.end()) return;
    const int i = it->second;
    if (numel[i] != (int64_t)rows * cols) {
      if (!bad) bad = names[i];
      return;
    }
    off[slot] = (int)start[i];
    has_grad[i] = grad;
    if (wt && tensors && rows > 1 && cols > 1)
      for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) wt[start[i] + (int64_t)c * rows + r] = tensors[i][(int64_t)r * cols + c];
  };
  const std::string p = "egnn.";
  see(EMB_W, p + "embedding.weight", H, F1, true);
  see(EMB_B, p + "embedding.bias", H, 1, true);
  see(OUT_W, p + "embedding_out.weight", K, H, true);
  see(OUT_B, p + "embedding_out.bias", K, 1, true);
  for (int l = 0; l < L; ++l) {
    const std::string q = p + "gcl_" + std::to_string(l) + ".";
    const int o = NHEAD + NLAYER * l;
    const bool coord = l < L - 1;
    see(o + E0W, q + "edge_mlp.0.weight", H, 2 * H + 2, true);
    see(o + E0B, q + "edge_mlp.0.bias", H, 1, true);
    see(o + E2W, q + "edge_mlp.2.weight", H, H, true);
    see(o + E2B, q + "edge_mlp.2.bias", H, 1, true);
    if (cfg->attention) {
      see(o + AW, q + "att_mlp.0.weight", 1, H, true);
      see(o + AB, q + "att_mlp.0.bias", 1, 1, true);
    }
    see(o + C0W, q + "coord_mlp.0.weight", H, H, coord);
    see(o + C0B, q + "coord_mlp.0.bias", H, 1, coord);
    see(o + C2W, q + "coord_mlp.2.weight", 1, H, coord);
    see(o + N0W, q + "node_mlp.0.weight", H, 2 * H, true);
    see(o + N0B, q + "node_mlp.0.bias", H, 1, true);
    see(o + N2W, q + "node_mlp.2.weight", H, H, true);
    see(o + N2B, q + "node_mlp.2.bias", H, 1, true);
  }
  return bad;
}

static int pt_load(gaudi_handle* h, const gaudi_pred_config* cfg, int n, const char* const* names, const float* const* tensors,
                   const int64_t* numel) {
  if (!h->pt) h->pt = new PredTrainState();
  PredTrainState& s = *h->pt;
  s.numel.assign(numel, numel + n);
  s.total = 0;
  for (int i = 0; i < n; ++i) s.total += numel[i];
  std::vector<float> w((size_t)s.total), wt((size_t)s.total);
  const char* bad = pt_layout(cfg, n, names, tensors, numel, s.start, s.off, s.has_grad, wt.data());
  if (bad) return fail(h, GAUDI_E_MISSING, std::string("predictor tensor mis-shaped: ") + bad);
  for (int i = 0; i < n; ++i) std::copy(tensors[i], tensors[i] + numel[i], w.begin() + s.start[i]);
  HIPCHECK(h, s.w.reserve(sizeof(float) * w.size()));
  HIPCHECK(h, s.wt.reserve(sizeof(float) * wt.size()));
  HIPCHECK(h, s.doff.reserve(sizeof(int) * s.off.size()));
  HIPCHECK(h, hipMemcpy(s.w.p, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice));
  HIPCHECK(h, hipMemcpy(s.wt.p, wt.data(), sizeof(float) * wt.size(), hipMemcpyHostToDevice));
  HIPCHECK(h, hipMemcpy(s.doff.p, s.off.data(), sizeof(int) * s.off.size(), hipMemcpyHostToDevice));
  return GAUDI_OK;
}

// floats of chunk scratch per molecule (pred_train.h)
static int64_t pt_floats_per_mol(int N, int H, int L, int F1, int K) {
  const int64_t E = (int64_t)N * N;
  return (int64_t)(L + 1) * N * (H + 4) + (int64_t)N * F1 + E + 10LL * N * H + 8LL * N + (int64_t)N * K + 8LL * E * H +
         8LL * E + 6LL * E;
}

// chunk size: the largest batch slice whose scratch fits in 1 GiB, or in GAUDI_PRED_TRAIN_SCRATCH_KB (tests of the chunked path)
static int64_t pt_scratch_bytes() {
  if (const char* e = getenv("GAUDI_PRED_TRAIN_SCRATCH_KB")) {
    const long long kb = atoll(e);
    if (kb > 0) return kb * 1024LL;
  }
  return 1LL << 30;
}

extern "C" {

int gaudi_host_pred_train_layout(const gaudi_pred_config* cfg, int n, const char* const* names, const float* const* tensors,
                                 const int64_t* numel, int32_t* off_out, int32_t* has_grad_out, float* wt_out) {
  if (!cfg || n < 0 || (n && (!names || !numel)) || !off_out || !has_grad_out || cfg->n_layers < 1) return GAUDI_E_INVALID;
  std::vector<int64_t> start;
  std::vector<int> off;
  std::vector<int32_t> has;
  if (pt_layout(cfg, n, names, tensors, numel, start, off, has, wt_out)) return GAUDI_E_MISSING;
  std::copy(off.begin(), off.end(), off_out);
  std::copy(has.begin(), has.end(), has_grad_out);
  return GAUDI_OK;
}

int gaudi_predictor_grad_size(gaudi_handle* h, int64_t* n_floats) {
  if (!h || !n_floats) return GAUDI_E_INVALID;
  if (!h->has_pred || !h->pt) return fail(h, GAUDI_E_STATE, "predictor weights not loaded");
  *n_floats = h->pt->total;
  return GAUDI_OK;
}

int gaudi_predictor_loss_grad(gaudi_handle* h, int B, int N, const float* x, const float* onehot, const int32_t* t_int,
                              const float* node_mask, const float* edge_mask, const float* y, uint64_t seed,
                              int64_t sample_offset, const float* noise, float* loss_out, float* pred_out, float* grad_out,
                              int32_t* has_grad_out) {
  using namespace gaudi_train;
  if (!h || !x || !onehot || !t_int || !node_mask || !edge_mask || !y || !loss_out || !grad_out || !has_grad_out)
    return GAUDI_E_INVALID;
  if (!h->has_pred || !h->pt) return fail(h, GAUDI_E_STATE, "predictor weights not loaded");
  if (B < 1 || N < 1) return fail(h, GAUDI_E_INVALID, "B and N must be positive");
  const gaudi_pred_config& c = h->pcfg;
  const int H = c.hidden_nf, L = c.n_layers, K = c.out_nf, F = c.in_nf, F1 = F + 1;
  if (N > 128)
    return fail(h, GAUDI_E_CAPACITY, "gaudi_predictor_loss_grad: N = " + std::to_string(N) +
                                         " exceeds the training kernels' 128 nodes (dense N x N edge scratch)");
  PredTrainState& s = *h->pt;
  for (int i = 0; i < NHEAD + NLAYER * L; ++i) {
    const int r = i < NHEAD ? -1 : (i - NHEAD) % NLAYER;
    if (s.off[i] < 0 && !(r == AW || r == AB)) return fail(h, GAUDI_E_MISSING, "predictor tensor missing for training");
  }
  // forward noising + the predictor forward: the same launch as gaudi_predict_noised, so pred (and the loss) are its
  // numbers; z_t stays on the device in d_zout
  std::vector<float> pred((size_t)B * K);
  int rc = run_predict_noised(h, B, N, x, onehot, t_int, node_mask, edge_mask, seed, sample_offset, noise, nullptr,
                              pred.data());
  if (rc) return rc;
  double acc = 0.0;
  for (size_t i = 0; i < pred.size(); ++i) acc += std::fabs((double)pred[i] - (double)y[i]);
  *loss_out = (float)(acc / (double)pred.size());
  if (pred_out) std::copy(pred.begin(), pred.end(), pred_out);

  const int E = N * N, T = h->ecfg.diffusion_steps;
  std::vector<float> tval(B);
  for (int b = 0; b < B; ++b) tval[b] = (float)t_int[b] / (float)T;
  const int64_t per = pt_floats_per_mol(N, H, L, F1, K);
  const int Bc = (int)std::max<int64_t>(1, std::min<int64_t>(B, pt_scratch_bytes() / (int64_t)sizeof(float) / per));
  HIPCHECK(h, s.scratch.reserve(sizeof(float) * (size_t)per * Bc));
  HIPCHECK(h, s.grad.reserve(sizeof(float) * (size_t)std::max<int64_t>(s.total, 1)));
  HIPCHECK(h, s.y.reserve(sizeof(float) * (size_t)B * K));
  HIPCHECK(h, s.t.reserve(sizeof(float) * (size_t)B));
  // d_mask / d_emask hold the STAGED graph of the launch above, not the dense masks: upload those here
  HIPCHECK(h, s.masks.reserve(sizeof(float) * (size_t)B * N * (1 + N)));
  float* d_nm = s.masks.as<float>();
  float* d_em = d_nm + (size_t)B * N;
  HIPCHECK(h, hipMemcpyAsync(d_nm, node_mask, sizeof(float) * B * N, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(d_em, edge_mask, sizeof(float) * (size_t)B * E, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(s.y.p, y, sizeof(float) * B * K, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(s.t.p, tval.data(), sizeof(float) * B, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemsetAsync(s.grad.p, 0, sizeof(float) * (size_t)s.total, h->stream));

  PTBufs b{};
  b.zt = h->d_zout.as<float>();
  b.t = s.t.as<float>();
  b.nm = d_nm;
  b.em = d_em;
  b.pred = h->d_pred.as<float>();
  b.y = s.y.as<float>();
  b.w = s.w.as<float>();
  b.wt = s.wt.as<float>();
  b.off = s.doff.as<int>();
  b.F = F;
  b.K = K;
  b.H = H;
  b.L = L;
  b.N = N;
  b.attention = c.attention;
  b.use_tanh = c.tanh;
  b.coords_range_layer = c.coords_range / (float)L;
  b.readout_div = (float)(h->readout_n > 0 ? h->readout_n : N);
  b.dpred_scale = 1.f / ((float)B * (float)K);
  b.bcap = Bc;
  {
    float* p = s.scratch.as<float>();
    auto take = [&](int64_t n) {
      float* r = p;
      p += n * Bc;
      return r;
    };
    b.hs = take((int64_t)(L + 1) * N * H);
    b.xs = take((int64_t)(L + 1) * N * 4);
    b.hin = take((int64_t)N * F1);
    b.d0 = take(E);
    float** node[] = {&b.P, &b.Q, &b.agg, &b.qp, &b.q, &b.dr, &b.dP, &b.dQ, &b.dh0, &b.dh1};
    for (float** q : node) *q = take((int64_t)N * H);
    b.dx0 = take(4LL * N);
    b.dx1 = take(4LL * N);
    b.dhout = take((int64_t)N * K);
    float** edge[] = {&b.U, &b.S, &b.V, &b.M, &b.EFt, &b.CP, &b.C, &b.DE};
    for (float** q : edge) *q = take((int64_t)E * H);
    b.diff = take(4LL * E);
    b.ddiff = take(4LL * E);
    float** sc[] = {&b.rad, &b.gate, &b.phi, &b.ppre, &b.dp, &b.dap};
    for (float** q : sc) *q = take(E);
  }
  const int par0 = (L - 1) & 1;  // the half of the dh ping-pong pair that holds dh_0 after layer 0's reverse pass

  // the weight-gradient products, per layer and for the head: (Y, X, G) in the order they are launched
  float* G = s.grad.as<float>();
  const int* o0 = s.off.data();
  std::vector<OuterJob> jobs;
  std::vector<int4> tiles;
  std::vector<std::pair<int, int>> launches;  // (first tile, tiles): L layer launches then the head, per chunk size
  auto job = [&](const float* Yp, int ldy, int M, const float* Xp, int ldx, int Kc, int off, int ldg, int R) {
    jobs.push_back(OuterJob{Yp, Xp, G + off, ldy, ldx, ldg, M, Kc, R});
    for (int m0 = 0; m0 < M; m0 += 32)
      for (int k0 = 0; k0 < Kc; k0 += 32) tiles.push_back(make_int4((int)jobs.size() - 1, m0, k0, 0));
  };
  auto plan = [&](int bc) {  // one chunk of bc molecules
    const int Rn = bc * N, Re = bc * E;
    for (int l = L - 1; l >= 0; --l) {
      const int first = (int)tiles.size();
      const int* o = o0 + NHEAD + NLAYER * l;
      const float* hl = b.hs + (size_t)l * Bc * N * H;
      const int ld1 = 2 * H + 2;
      job(b.dP, H, H, hl, H, H, o[E0W], ld1, Rn);
      job(b.dQ, H, H, hl, H, H, o[E0W] + H, ld1, Rn);
      job(b.U, H, H, b.rad, 1, 1, o[E0W] + 2 * H, ld1, Re);
      job(b.U, H, H, b.d0, 1, 1, o[E0W] + 2 * H + 1, ld1, Re);
      job(b.dP, H, H, nullptr, 0, 1, o[E0B], 1, Rn);
      job(b.V, H, H, b.S, H, H, o[E2W], H, Re);
      job(b.V, H, H, nullptr, 0, 1, o[E2B], 1, Re);
      if (c.attention) {
        job(b.dap, 1, 1, b.M, H, H, o[AW], H, Re);
        job(b.dap, 1, 1, nullptr, 0, 1, o[AB], 1, Re);
      }
      if (l < L - 1) {
        job(b.CP, H, H, b.EFt, H, H, o[C0W], H, Re);
        job(b.CP, H, H, nullptr, 0, 1, o[C0B], 1, Re);
        job(b.dp, 1, 1, b.C, H, H, o[C2W], H, Re);
      }
      job(b.qp, H, H, hl, H, H, o[N0W], 2 * H, Rn);
      job(b.qp, H, H, b.agg, H, H, o[N0W] + H, 2 * H, Rn);
      job(b.qp, H, H, nullptr, 0, 1, o[N0B], 1, Rn);
      job(b.dr, H, H, b.q, H, H, o[N2W], H, Rn);
      job(b.dr, H, H, nullptr, 0, 1, o[N2B], 1, Rn);
      launches.push_back({first, (int)tiles.size() - first});
    }
    const int first = (int)tiles.size();
    const float* dh0 = par0 ? b.dh0 : b.dh1;
    job(b.dhout, K, K, b.hs + (size_t)L * Bc * N * H, H, H, o0[OUT_W], H, Rn);
    job(b.dhout, K, K, nullptr, 0, 1, o0[OUT_B], 1, Rn);
    job(dh0, H, H, b.hin, F1, F1, o0[EMB_W], F1, Rn);
    job(dh0, H, H, nullptr, 0, 1, o0[EMB_B], 1, Rn);
    launches.push_back({first, (int)tiles.size() - first});
  };
  plan(Bc);
  const int last = B % Bc;
  if (last) plan(last);
  HIPCHECK(h, s.jobs.reserve(sizeof(OuterJob) * jobs.size()));
  HIPCHECK(h, s.tiles.reserve(sizeof(int4) * tiles.size()));
  HIPCHECK(h, hipMemcpyAsync(s.jobs.p, jobs.data(), sizeof(OuterJob) * jobs.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(s.tiles.p, tiles.data(), sizeof(int4) * tiles.size(), hipMemcpyHostToDevice, h->stream));
  const OuterJob* djobs = s.jobs.as<OuterJob>();
  const int4* dtiles = s.tiles.as<int4>();

  for (int b0 = 0; b0 < B; b0 += Bc) {
    const int bc = std::min(Bc, B - b0);
    const size_t li = bc == Bc ? 0 : (size_t)(L + 1);  // the plan of a full chunk, or of the short last one
    b.b0 = b0;
    HIPCHECK(h, (hipError_t)gaudi_pt_embed(b, bc, h->stream));
    for (int l = 0; l < L; ++l) HIPCHECK(h, (hipError_t)gaudi_pt_layer(b, bc, l, 0, h->stream));
    HIPCHECK(h, (hipError_t)gaudi_pt_readout(b, bc, h->stream));
    for (int l = L - 1; l >= 0; --l) {
      HIPCHECK(h, (hipError_t)gaudi_pt_layer(b, bc, l, 1, h->stream));
      const auto& ln = launches[li + (size_t)(L - 1 - l)];
      HIPCHECK(h, (hipError_t)gaudi_pt_outer(djobs, dtiles + ln.first, ln.second, h->stream));
    }
    const auto& ln = launches[li + (size_t)L];
    HIPCHECK(h, (hipError_t)gaudi_pt_outer(djobs, dtiles + ln.first, ln.second, h->stream));
  }
  // gradients out: torch layout, names order; tensors without a gradient path are left untouched
  std::vector<float> g((size_t)s.total);
  HIPCHECK(h, hipMemcpyAsync(g.data(), s.grad.p, sizeof(float) * (size_t)s.total, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < s.numel.size(); ++i) {
    has_grad_out[i] = s.has_grad[i];
    if (s.has_grad[i]) std::copy(g.begin() + s.start[i], g.begin() + s.start[i] + s.numel[i], grad_out + s.start[i]);
  }
  return GAUDI_OK;
}

}  // extern "C"
