// pred_train_host.inc -- predictor training half of the C ABI (included at the end of gaudi_hip.hip after train_host.inc, the
// core it shares with the EDM's half): the predictor's role table, what its state and scratch add, and
// gaudi_predictor_loss_grad (pred_train.h describes the kernels).
#include "pred_train.h"

struct PredTrainState : TrainState {
  DevBuf y, t, masks;
  void release() {
    TrainState::release();
    DevBuf* bufs[] = {&y, &t, &masks};
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
// read).  Host only (train_host.inc: tr_layout).  Returns 0, or the name of a tensor whose size does not match its role.
static const char* pt_layout(const gaudi_pred_config* cfg, int n, const char* const* names, const float* const* tensors,
                             const int64_t* numel, std::vector<int64_t>& start, std::vector<int>& off,
                             std::vector<int32_t>& has_grad, float* wt) {
  using namespace gaudi_train;
  const int H = cfg->hidden_nf, L = cfg->n_layers, K = cfg->out_nf, F1 = cfg->in_nf + 1;
  const std::string p = "egnn.";
  std::vector<TrainRole> t = {{EMB_W, p + "embedding.weight", H, F1, true},
                              {EMB_B, p + "embedding.bias", H, 1, true},
                              {OUT_W, p + "embedding_out.weight", K, H, true},
                              {OUT_B, p + "embedding_out.bias", K, 1, true}};
  for (int l = 0; l < L; ++l) {
    const std::string q = p + "gcl_" + std::to_string(l) + ".";
    const int o = NHEAD + NLAYER * l;
    const bool coord = l < L - 1;
    tr_edge_roles(t, q, H, 2 * H + 2, cfg->attention, o + E0W);
    t.push_back({o + C0W, q + "coord_mlp.0.weight", H, H, coord});
    t.push_back({o + C0B, q + "coord_mlp.0.bias", H, 1, coord});
    t.push_back({o + C2W, q + "coord_mlp.2.weight", 1, H, coord});
    tr_node_roles(t, q, H, o + N0W);
  }
  return tr_layout(t, NHEAD + NLAYER * L, n, names, tensors, numel, start, off, has_grad, wt);
}

static int pt_load(gaudi_handle* h, const gaudi_pred_config* cfg, int n, const char* const* names, const float* const* tensors,
                   const int64_t* numel) {
  if (!h->pt) h->pt = new PredTrainState();
  return tr_upload(h, *h->pt, "predictor", n, names, tensors, numel,
                   [&](std::vector<int64_t>& start, std::vector<int>& off, std::vector<int32_t>& has, float* wt) {
                     return pt_layout(cfg, n, names, tensors, numel, start, off, has, wt);
                   });
}

// the chunk scratch of the predictor, from b's N, H, L, F, K (train_host.inc: Carver -- run once to count, once to carve)
static void pt_carve(gaudi_train::PTBufs& b, Carver& c) {
  const int64_t E = (int64_t)b.N * b.N;
  tr_carve(b, c, b.L + 1, b.F + 1, b.K);
  b.d0 = c.take(E);
  b.CP = c.take(E * b.H);
  b.C = c.take(E * b.H);
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
  PTBufs b{};
  b.F = F;
  b.K = K;
  b.H = H;
  b.L = L;
  b.N = N;
  b.A = 2;
  Carver count{nullptr, 0};
  pt_carve(b, count);
  const int Bc = tr_chunk(B, count.per, "GAUDI_PRED_TRAIN_SCRATCH_KB");
  HIPCHECK(h, s.scratch.reserve(sizeof(float) * (size_t)count.per * Bc));
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

  b.zt = h->d_zout.as<float>();
  b.t = s.t.as<float>();
  b.nm = d_nm;
  b.em = d_em;
  b.pred = h->d_pred.as<float>();
  b.y = s.y.as<float>();
  b.w = s.w.as<float>();
  b.wt = s.wt.as<float>();
  b.off = s.doff.as<int>();
  b.attention = c.attention;
  b.use_tanh = c.tanh;
  b.coords_range_layer = c.coords_range / (float)L;
  b.readout_div = (float)(h->readout_n > 0 ? h->readout_n : N);
  b.dpred_scale = 1.f / ((float)B * (float)K);
  b.bcap = Bc;
  Carver carve{s.scratch.as<float>(), Bc};
  pt_carve(b, carve);

  // the weight-gradient products: one launch per layer from the last, then the head
  OuterPlan plan;
  plan.G = s.grad.as<float>();
  const int* o0 = s.off.data();
  plan.build(B, Bc, [&](int bc) {
    const int Rn = bc * N, Re = bc * E;
    for (int l = L - 1; l >= 0; --l) {
      plan.begin();
      const int* o = o0 + NHEAD + NLAYER * l;
      const float* hl = b.hs + (size_t)l * Bc * N * H;
      plan.edge_jobs(b, hl, o[E0W], o[E0B], o[E2W], o[E2B], 2, Rn, Re, {{b.rad, 1}, {b.d0, 1}});
      if (c.attention) plan.att_jobs(b, o[AW], o[AB], Re);
      if (l < L - 1) {
        plan.job(b.CP, H, H, b.EF, H, H, o[C0W], H, Re);
        plan.job(b.CP, H, H, nullptr, 0, 1, o[C0B], 1, Re);
        plan.job(b.dp, 1, 1, b.C, H, H, o[C2W], H, Re);
      }
      plan.node_jobs(b, hl, o[N0W], o[N0B], o[N2W], o[N2B], Rn);
      plan.end();
    }
    plan.begin();
    plan.head_jobs(b, b.hs + (size_t)L * Bc * N * H, K, F1, o0, Rn);
    plan.end();
  });
  rc = plan.upload(h, s);
  if (rc) return rc;

  for (int b0 = 0; b0 < B; b0 += Bc) {
    const int bc = std::min(Bc, B - b0);
    plan.select(bc);
    b.b0 = b0;
    HIPCHECK(h, (hipError_t)gaudi_pt_embed(b, bc, h->stream));
    for (int l = 0; l < L; ++l) HIPCHECK(h, (hipError_t)gaudi_pt_layer(b, bc, l, 0, h->stream));
    HIPCHECK(h, (hipError_t)gaudi_pt_readout(b, bc, h->stream));
    for (int l = L - 1; l >= 0; --l) {
      HIPCHECK(h, (hipError_t)gaudi_pt_layer(b, bc, l, 1, h->stream));
      HIPCHECK(h, plan.launch((size_t)(L - 1 - l), h->stream));
    }
    HIPCHECK(h, plan.launch((size_t)L, h->stream));
  }
  return tr_grads_out(h, s, grad_out, has_grad_out);
}

}  // extern "C"
