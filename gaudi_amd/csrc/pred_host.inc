// pred_host.inc -- predictor half of the C ABI (included at the end of gaudi_hip.hip).

static void fill_pred_common(gaudi_handle* h, KParams& P, int B, int N) {
  const gaudi_pred_config& c = h->pcfg;
  P.pred.w = (h->variant == 8 && h->plan.waves == 4) ? h->pred_w4.as<float>() : h->pred_w.as<float>();
  P.pred.w_bytes = (unsigned)h->pred_w_bytes;
  P.pred.F = c.in_nf;
  P.pred.K = c.out_nf;
  P.pred.L = c.n_layers;
  P.pred.attention = c.attention;
  P.pred.use_tanh = c.tanh;
  P.pred.coords_range_layer = c.coords_range / (float)c.n_layers;
  P.pred.ktail = h->plan.waves == 8 && has_ktail(c.hidden_nf, h->HPP);
  P.pred.ws = h->pred_ws.as<float>();
  P.pred.ws_bytes = (unsigned)h->pred_ws_bytes;
  P.pred.hinv = h->pred_hinv;
  // the stash is per WORKGROUP (P.B of them, P.N node slots each: more than a molecule's N in a wide-group launch); the
  // readout divides by the molecule's padded N (egnn_predictor/models.py:457)
  P.stash_stride = h->plan.waves == 8 ? w8::pred_stash_floats8(P.N, h->HPP, c.n_layers, P.EW)
                                       : pred_stash_floats(P.N, h->HPP, c.n_layers, P.EW);
  P.readout_div = (float)(h->readout_n > 0 ? h->readout_n : N);
  (void)B;
}

static int fill_pred(gaudi_handle* h, KParams& P, const float* target_w, int B, int N) {
  if (!h->has_pred) return fail(h, GAUDI_E_STATE, "predictor weights not loaded");
  if (h->pcfg.in_nf != h->ecfg.in_node_nf) return fail(h, GAUDI_E_INVALID, "EDM and predictor disagree on in_node_nf");
  fill_pred_common(h, P, B, N);
  HIPCHECK(h, h->d_stash.reserve(sizeof(float) * (size_t)P.stash_stride * (size_t)P.B));
  HIPCHECK(h, h->d_tw.reserve(sizeof(float) * 16));
  HIPCHECK(h, hipMemcpyAsync(h->d_tw.p, target_w, sizeof(float) * h->pcfg.out_nf, hipMemcpyHostToDevice, h->stream));
  P.stash = h->d_stash.as<float>();
  P.target_w = h->d_tw.as<float>();
  return GAUDI_OK;
}

static int run_predictor(gaudi_handle* h, int B, int N, const float* z, const float* t, const float* node_mask,
                         const float* edge_mask, const float* dpred, float* pred_out, float* grad_out) {
  if (!h->has_pred) return fail(h, GAUDI_E_STATE, "predictor weights not loaded");
  HIPCHECK(h, hipSetDevice(h->device));
  KParams P{};
  int rc = stage_graph(h, B, N, node_mask, edge_mask, P, 0, h->HPP, CallHints{});
  if (rc) return rc;
  P.F = h->pcfg.in_nf;
  fill_pred_common(h, P, B, N);
  const int D = 3 + P.F, K = h->pcfg.out_nf;
  const size_t zb = sizeof(float) * B * N * D;
  HIPCHECK(h, h->d_zin.reserve(zb));
  HIPCHECK(h, h->d_zout.reserve(zb));
  HIPCHECK(h, h->d_t.reserve(sizeof(float) * B));
  HIPCHECK(h, h->d_pred.reserve(sizeof(float) * B * K));
  HIPCHECK(h, h->d_dpred.reserve(sizeof(float) * B * K));
  HIPCHECK(h, h->d_stash.reserve(sizeof(float) * (size_t)P.stash_stride * B));
  HIPCHECK(h, hipMemcpyAsync(h->d_zin.p, z, zb, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(h->d_t.p, t, sizeof(float) * B, hipMemcpyHostToDevice, h->stream));
  if (dpred) HIPCHECK(h, hipMemcpyAsync(h->d_dpred.p, dpred, sizeof(float) * B * K, hipMemcpyHostToDevice, h->stream));
  P.mode = dpred ? MODE_PRED_GRAD : MODE_PRED_FWD;
  P.z_in = h->d_zin.as<float>();
  P.z_out = h->d_zout.as<float>();
  P.t_in = h->d_t.as<float>();
  P.pred_out = h->d_pred.as<float>();
  P.dpred_in = dpred ? h->d_dpred.as<float>() : nullptr;
  P.stash = h->d_stash.as<float>();
  rc = launch(h, P, 0, h->HPP, 0);
  if (rc) return rc;
  if (pred_out) HIPCHECK(h, hipMemcpyAsync(pred_out, h->d_pred.p, sizeof(float) * B * K, hipMemcpyDeviceToHost, h->stream));
  if (grad_out) HIPCHECK(h, hipMemcpyAsync(grad_out, h->d_zout.p, zb, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  return GAUDI_OK;
}

// sample_edm_t + predictor forward (cond_prediction/train_cond_predictor.py:47-81, eval_cond_predictor.py:34-60)
static int run_predict_noised(gaudi_handle* h, int B, int N, const float* x, const float* onehot, const int32_t* t_int,
                              const float* node_mask, const float* edge_mask, uint64_t seed, int64_t sample_offset,
                              const float* noise, float* zt_out, float* pred_out) {
  if (!h->has_edm) return fail(h, GAUDI_E_STATE, "EDM weights not loaded (the noise schedule and normalisation come from the EDM)");
  if (!h->has_pred) return fail(h, GAUDI_E_STATE, "predictor weights not loaded");
  if (h->pcfg.in_nf != h->ecfg.in_node_nf) return fail(h, GAUDI_E_INVALID, "EDM and predictor disagree on in_node_nf");
  HIPCHECK(h, hipSetDevice(h->device));
  const int T = h->ecfg.diffusion_steps, F = h->pcfg.in_nf, D = 3 + F, K = h->pcfg.out_nf;
  std::vector<float> as((size_t)B * 2), tval(B), xh((size_t)B * N * D);
  for (int b = 0; b < B; ++b) {
    if (t_int[b] < 0 || t_int[b] > T) return fail(h, GAUDI_E_INVALID, "t_int must be in 0..T");
    const float g = h->gamma[t_int[b]];                 // gamma(t) lookup: round(t * T) (en_diffusion.py:220-223)
    as[2 * b] = sqrtf(sigmoid_host(-g));                // alpha (en_diffusion.py:375-377)
    as[2 * b + 1] = sqrtf(sigmoid_host(g));             // sigma (:370-373)
    tval[b] = (float)t_int[b] / (float)T;
    for (int n = 0; n < N; ++n) {
      float* dst = &xh[((size_t)b * N + n) * D];
      for (int d = 0; d < 3; ++d) dst[d] = x[((size_t)b * N + n) * 3 + d];
      for (int k = 0; k < F; ++k) dst[3 + k] = onehot[((size_t)b * N + n) * F + k];
    }
  }
  KParams P{};
  int rc = stage_graph(h, B, N, node_mask, edge_mask, P, 0, h->HPP, CallHints{});
  if (rc) return rc;
  P.F = F;
  fill_pred_common(h, P, B, N);
  const size_t zb = sizeof(float) * B * N * D;
  HIPCHECK(h, h->d_zin.reserve(zb));
  HIPCHECK(h, h->d_zout.reserve(zb));
  HIPCHECK(h, h->d_t.reserve(sizeof(float) * B));
  HIPCHECK(h, h->d_as.reserve(sizeof(float) * 2 * B));
  HIPCHECK(h, h->d_pred.reserve(sizeof(float) * B * K));
  HIPCHECK(h, h->d_stash.reserve(sizeof(float) * (size_t)P.stash_stride * B));
  HIPCHECK(h, hipMemcpyAsync(h->d_zin.p, xh.data(), zb, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(h->d_t.p, tval.data(), sizeof(float) * B, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(h->d_as.p, as.data(), sizeof(float) * 2 * B, hipMemcpyHostToDevice, h->stream));
  if (noise) {
    HIPCHECK(h, h->d_noise.reserve(zb));
    HIPCHECK(h, hipMemcpyAsync(h->d_noise.p, noise, zb, hipMemcpyHostToDevice, h->stream));
    P.noise = h->d_noise.as<float>();
  }
  P.draw_base = 0;
  P.draw_stride = (long long)B * N * D;
  P.seed = seed;
  P.sample_offset = sample_offset;
  P.nv0 = h->ecfg.norm_values[0];
  P.nv1 = h->ecfg.norm_values[1];
  P.mode = MODE_PRED_FWD;
  P.z_in = h->d_zin.as<float>();
  P.z_out = h->d_zout.as<float>();
  P.zt_out = h->d_zout.as<float>();
  P.alpha_sigma = h->d_as.as<float>();
  P.t_in = h->d_t.as<float>();
  P.pred_out = h->d_pred.as<float>();
  P.stash = h->d_stash.as<float>();
  rc = launch(h, P, 0, h->HPP, 0);
  if (rc) return rc;
  if (pred_out) HIPCHECK(h, hipMemcpyAsync(pred_out, h->d_pred.p, sizeof(float) * B * K, hipMemcpyDeviceToHost, h->stream));
  if (zt_out) HIPCHECK(h, hipMemcpyAsync(zt_out, h->d_zout.p, zb, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  return GAUDI_OK;
}

extern "C" {

int gaudi_predict_noised(gaudi_handle* h, int B, int N, const float* x, const float* onehot, const int32_t* t_int,
                         const float* node_mask, const float* edge_mask, uint64_t seed, int64_t sample_offset,
                         const float* noise, float* zt_out, float* pred_out) {
  if (!h || !x || !onehot || !t_int || !node_mask || !edge_mask || (!zt_out && !pred_out)) return GAUDI_E_INVALID;
  return run_predict_noised(h, B, N, x, onehot, t_int, node_mask, edge_mask, seed, sample_offset, noise, zt_out, pred_out);
}

int gaudi_load_predictor(gaudi_handle* h, const gaudi_pred_config* cfg, int n, const char* const* names,
                         const float* const* tensors, const int64_t* numel) {
  if (!h || !cfg) return GAUDI_E_INVALID;
  HIPCHECK(h, hipSetDevice(h->device));
  const int H = cfg->hidden_nf, F = cfg->in_nf, F1 = F + 1, L = cfg->n_layers, K = cfg->out_nf;
  if (H <= 0 || H > 256) return fail(h, GAUDI_E_INVALID, "hidden_nf must be in 1..256");
  if (F < 1 || F > 15) return fail(h, GAUDI_E_INVALID, "in_nf must be in 1..15");
  if (K < 1 || K > 16) return fail(h, GAUDI_E_INVALID, "out_nf must be in 1..16");
  if (L < 1) return fail(h, GAUDI_E_INVALID, "bad n_layers");
  const int HP = round_hidden(H);
  if (!HP) return fail(h, GAUDI_E_INVALID, "no kernel instantiated for this hidden size");
  Tensors T;
  for (int i = 0; i < n; ++i) T.m[names[i]] = {tensors[i], numel[i]};
  if (h->warn.rfind("predictor weights:", 0) == 0) h->warn.clear();  // a reload reports the weights it loads, not the last ones
  PredLayout lay{HP, F1, K, L};
  const std::string p = "egnn.";
  const int PK = HP * HP;
  float hscale = 0.f;  // the exponent of the fp16-pair node images (gaudi_hip.hip: NodeScale)
  {
    NodeScale ns;
    for (int l = 0; l < L; ++l) {
      const std::string q = p + "gcl_" + std::to_string(l) + ".";
      ns.see(T.peek(q + "edge_mlp.0.weight", (int64_t)H * (2 * H + 2)), H, 2 * H + 2, 0, 2 * H);
      ns.see(T.peek(q + "node_mlp.0.weight", (int64_t)H * 2 * H), H, 2 * H, 0, 2 * H);
      ns.see(T.peek(q + "node_mlp.2.weight", (int64_t)H * H), H, H, 0, H);
      ns.see(T.peek(q + "edge_mlp.2.weight", (int64_t)H * H), H, H, 0, H, true);
      ns.see(T.peek(q + "coord_mlp.0.weight", (int64_t)H * H), H, H, 0, H, true);
    }
    hscale = ns.scale();
    if (!(hscale > 0.f) && h->variant == 8 && h->split)
      h->warn = std::string("predictor weights: the fp16-pair images cannot carry this weight set (") + ns.why() +
                "): guided calls run the fp32-instruction kernels (about 0.55 x the speed, same results at fp32 accuracy)";
  }
  auto pack = [&](bool lane_linear, std::vector<float>& w, std::vector<float>* ws) {
  w.assign((size_t)lay.total(), 0.f);
  if (ws) ws->assign(2 * (size_t)lay.total(), 0.f);
  // only the matrices of the edge-level GEMMs (W2, Wc1 and their transposes) carry the K tail: pe packs those, pn the rest
  PackMode pe;
  pe.lane_linear = lane_linear;
  pe.ktail = lane_linear && has_ktail(H, HP);
  pe.wbase = w.data();
  pe.ws = ws;
  pe.hscale = ws ? hscale : 0.f;
  pe.hktail = has_ktail(H, HP);
  const PackMode pn = pe.with_ktail(false);
  {
    const float* ew = T.get(p + "embedding.weight", (int64_t)H * F1);
    const float* eb = T.get(p + "embedding.bias", H);
    const float* ow = T.get(p + "embedding_out.weight", (int64_t)K * H);
    const float* ob = T.get(p + "embedding_out.bias", K);
    if (ew && eb && ow && ob) {
      for (int f = 0; f < H; ++f)
        for (int k = 0; k < F1; ++k) w[lay.emb_w() + f * F1 + k] = ew[f * F1 + k];
      pack_vec(&w[lay.emb_b()], eb, H);
      for (int o = 0; o < K; ++o)
        for (int k = 0; k < H; ++k) w[lay.out_w() + o * HP + k] = ow[o * H + k];
      pack_vec(&w[lay.out_b()], ob, K);
    }
  }
  const int ld1 = 2 * H + 2;
  for (int l = 0; l < L; ++l) {
    const std::string q = p + "gcl_" + std::to_string(l) + ".";
    float* G = &w[lay.layer(l)];
    float* V = G + 14 * PK;
    const float* W1 = T.get(q + "edge_mlp.0.weight", (int64_t)H * ld1);
    const float* b1 = T.get(q + "edge_mlp.0.bias", H);
    const float* W2 = T.get(q + "edge_mlp.2.weight", (int64_t)H * H);
    const float* b2 = T.get(q + "edge_mlp.2.bias", H);
    const float* Wn1 = T.get(q + "node_mlp.0.weight", (int64_t)H * 2 * H);
    const float* bn1 = T.get(q + "node_mlp.0.bias", H);
    const float* Wn2 = T.get(q + "node_mlp.2.weight", (int64_t)H * H);
    const float* bn2 = T.get(q + "node_mlp.2.bias", H);
    const float* Wc1 = T.get(q + "coord_mlp.0.weight", (int64_t)H * H);
    const float* bc1 = T.get(q + "coord_mlp.0.bias", H);
    const float* wc2 = T.get(q + "coord_mlp.2.weight", H);
    const float *wa = nullptr, *ba = nullptr;
    if (cfg->attention) {
      wa = T.get(q + "att_mlp.0.weight", H);
      ba = T.get(q + "att_mlp.0.bias", 1);
    }
    if (!(W1 && b1 && W2 && b2 && Wn1 && bn1 && Wn2 && bn2 && Wc1 && bc1 && wc2) || (cfg->attention && !(wa && ba)))
      continue;
    for (int tr = 0; tr < 2; ++tr) {
      float* M = G + tr * 7 * PK;
      pack_node_matrix(pn, M, W1, H, ld1, 0, HP, tr);
      pack_node_matrix(pn, M + PK, W1, H, ld1, H, HP, tr);
      pack_edge_matrix(pe, M + 2 * PK, W2, H, H, 0, HP, tr);
      pack_edge_matrix(pe, M + 3 * PK, Wc1, H, H, 0, HP, tr);
      pack_node_matrix(pn, M + 4 * PK, Wn1, H, 2 * H, 0, HP, tr);
      pack_node_matrix(pn, M + 5 * PK, Wn1, H, 2 * H, H, HP, tr);
      pack_node_matrix(pn, M + 6 * PK, Wn2, H, H, 0, HP, tr);
    }
    pack_col(V, W1, H, ld1, 2 * H);
    pack_col(V + HP, W1, H, ld1, 2 * H + 1);
    pack_vec(V + 2 * HP, b1, H);
    pack_vec(V + 3 * HP, b2, H);
    if (wa) pack_vec(V + 4 * HP, wa, H);
    pack_vec(V + 5 * HP, bc1, H);
    pack_vec(V + 6 * HP, wc2, H);
    pack_vec(V + 7 * HP, bn1, H);
    pack_vec(V + 8 * HP, bn2, H);
    if (ba) V[9 * HP] = ba[0];
    V[9 * HP + 1] = col_absmax(W1, H, ld1, 2 * H);      // max |c_r|, max |c_d| (gaudi_hip.hip: load_edm)
    V[9 * HP + 2] = col_absmax(W1, H, ld1, 2 * H + 1);
  }
  };
  std::vector<float> w, ws;
  const bool want_split = h->variant == 8 && h->split;
  pack(h->variant == 8, w, want_split ? &ws : nullptr);
  if (!T.missing.empty()) return fail(h, GAUDI_E_MISSING, "predictor checkpoint tensor missing or mis-shaped: " + T.missing);
  HIPCHECK(h, h->pred_w.reserve(sizeof(float) * w.size()));
  HIPCHECK(h, hipMemcpy(h->pred_w.p, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice));
  h->pred_w_bytes = sizeof(float) * w.size();
  h->pred_ws_bytes = 0;
  if (want_split) {
    HIPCHECK(h, h->pred_ws.reserve(sizeof(float) * ws.size()));
    HIPCHECK(h, hipMemcpy(h->pred_ws.p, ws.data(), sizeof(float) * ws.size(), hipMemcpyHostToDevice));
    h->pred_ws_bytes = sizeof(float) * ws.size();
  }
  h->pred_hinv = want_split && hscale > 0.f ? 1.0f / hscale : 0.f;
  if (h->variant == 8) {
    pack(false, w, nullptr);
    HIPCHECK(h, h->pred_w4.reserve(sizeof(float) * w.size()));
    HIPCHECK(h, hipMemcpy(h->pred_w4.p, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice));
  }
  {
    const int rc = pt_load(h, cfg, n, names, tensors, numel);
    if (rc) return rc;
  }
  h->pcfg = *cfg;
  h->HPP = HP;
  h->has_pred = true;
  return GAUDI_OK;
}

int gaudi_predictor_fwd(gaudi_handle* h, int B, int N, const float* z, const float* t, const float* node_mask,
                        const float* edge_mask, float* pred_out) {
  if (!h || !z || !t || !node_mask || !edge_mask || !pred_out) return GAUDI_E_INVALID;
  return run_predictor(h, B, N, z, t, node_mask, edge_mask, nullptr, pred_out, nullptr);
}

int gaudi_predictor_grad(gaudi_handle* h, int B, int N, const float* z, const float* t, const float* node_mask,
                         const float* edge_mask, const float* dpred, float* pred_out, float* grad_out) {
  if (!h || !z || !t || !node_mask || !edge_mask || !dpred || !grad_out) return GAUDI_E_INVALID;
  return run_predictor(h, B, N, z, t, node_mask, edge_mask, dpred, pred_out, grad_out);
}

int gaudi_set_readout_nodes(gaudi_handle* h, int n_pad) {
  if (!h || n_pad < 0) return GAUDI_E_INVALID;
  h->readout_n = n_pad;
  return GAUDI_OK;
}

}  // extern "C"
