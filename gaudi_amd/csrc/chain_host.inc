// chain_host.inc -- everything that drives a reverse chain (included at the end of gaudi_hip.hip, after pred_host.inc): the
// single steps (gaudi_step*, gaudi_decode), the whole chains (gaudi_sample*, gaudi_sample_chain) and the callback chains
// (gaudi_sample_cb*).  An entry point names what it wants in a ChainCall; chain_begin stages it (graph, KParams, workspaces,
// noise, time grid, seeded start, value target) and chain_finish copies the results out -- run_chain and sample_cb_impl differ
// only in the launches between the two.

// diagnostics replacing assert_correctly_masked and the masked mean-zero assertion next to it (utils.py:52-65) and the
// CoG re-projection of en_diffusion.py:1000-1006 (batch-wide condition -> host side)
static void finish_sample(int B, int N, const float* node_mask, float* x_out, int nanc, gaudi_diag* diag) {
  float leak = 0.f, cog = 0.f, big = 0.f;
  for (int b = 0; b < B; ++b) {
    float s[3] = {0, 0, 0};
    for (int n = 0; n < N; ++n)
      for (int d = 0; d < 3; ++d) {
        const float v = x_out[((size_t)b * N + n) * 3 + d];
        s[d] += v;
        big = std::max(big, std::fabs(v));
        leak = std::max(leak, std::fabs(v * (1.f - node_mask[b * N + n])));
      }
    for (int d = 0; d < 3; ++d) cog = std::max(cog, std::fabs(s[d]));
  }
  int reproj = 0;
  if (cog > 5e-2f) {
    reproj = 1;
    for (int b = 0; b < B; ++b) {
      float cnt = 0.f;
      for (int n = 0; n < N; ++n) cnt += node_mask[b * N + n];
      cnt = std::max(cnt, 1.f);
      for (int d = 0; d < 3; ++d) {
        float s = 0.f;
        for (int n = 0; n < N; ++n) s += x_out[((size_t)b * N + n) * 3 + d];
        const float mean = s / cnt;
        for (int n = 0; n < N; ++n) x_out[((size_t)b * N + n) * 3 + d] -= mean * node_mask[b * N + n];
      }
    }
  }
  if (diag) {
    diag->max_masked_leak = leak;
    diag->max_cog_abs = cog;
    diag->max_cog_rel = cog / (big + 1e-10f);
    diag->nan_count = nanc;
    diag->reprojected = reproj;
  }
}

// ---- value targets (gaudi_sample_target): one molecule's parameter row w | q | c | side | scale (device_common.h: target_seed)
static void vt_pack_row(const gaudi_target_spec& sp, int K, int b, float* row) {
  for (int k = 0; k < K; ++k) {
    row[k] = sp.w ? sp.w[(sp.w_per_mol ? (size_t)b * K : 0) + k] : 0.f;
    row[K + k] = sp.q ? sp.q[(sp.q_per_mol ? (size_t)b * K : 0) + k] : 0.f;
    row[2 * K + k] = sp.c ? sp.c[(sp.c_per_mol ? (size_t)b * K : 0) + k] : 0.f;
    row[3 * K + k] = sp.side ? (float)sp.side[(sp.side_per_mol ? (size_t)b * K : 0) + k] : 0.f;
  }
  row[4 * K] = sp.scale ? sp.scale[sp.scale_per_mol ? b : 0] : 1.f;
}
// refusals that need no device: K, sides, finiteness, the window against T (T <= 0: not checked)
static const char* vt_check(const gaudi_target_spec* sp, int B, int K, int T) {
  if (!sp) return "no target spec";
#ifdef GAUDI_STAMPS
  if (T > 0) return "value targets are not available in the GAUDI_STAMPS diagnostic build (it times the affine fused step only)";
#endif
  if (B <= 0) return "B must be positive";
  if (sp->K != K) return "the target spec's K differs from the predictor's number of outputs";
  if (K <= 0 || K > 16) return "a target spec takes 1 to 16 predictor outputs";
  auto finite = [&](const float* a, int per_mol, size_t per) {
    if (!a) return true;
    const size_t n = per_mol ? (size_t)B * per : per;
    for (size_t i = 0; i < n; ++i)
      if (!std::isfinite(a[i])) return false;
    return true;
  };
  if (!finite(sp->w, sp->w_per_mol, K) || !finite(sp->q, sp->q_per_mol, K) || !finite(sp->c, sp->c_per_mol, K) ||
      !finite(sp->scale, sp->scale_per_mol, 1))
    return "a target parameter (w, q, c or scale) is not finite";
  if (sp->side) {
    const size_t n = sp->side_per_mol ? (size_t)B * K : (size_t)K;
    for (size_t i = 0; i < n; ++i)
      if (sp->side[i] < -1 || sp->side[i] > 1) return "side must be -1 (lower bound), 0 (value) or +1 (upper bound)";
  }
  const bool dflt = sp->t_lo == 0 && sp->t_hi == 0;
  if (!dflt && T > 0) {
    if (sp->t_lo < 1 || sp->t_hi > T) return "the guidance window must lie inside 1..T";
    if (sp->t_lo > sp->t_hi) return "the guidance window is empty (t_lo > t_hi)";
  }
  return nullptr;
}

// One reverse chain, or a piece of one.  The defaults are what most callers pass; an entry point names only what it sets (designated
// initializers, in the order of the fields).
struct ChainCall {
  int B = 0, N = 0;  // graph
  const float *node_mask = nullptr, *edge_mask = nullptr;
  // start: z_in = z at the top of the range; do_init: drawn from the prior instead; seeded: z_in holds the un-normalised
  // [x | onehot] of given molecules, which the first launch noises to time index gp->t0 with raw draw 0 (the forward-noising
  // prologue of gaudi_predict_noised) -> zt_out
  const float* z_in = nullptr;
  bool do_init = false, seeded = false;
  int s_hi = 0, s_lo = 0;  // range: steps s_hi down to s_lo (rows of gp's table, or of the handle's), then the decode pass
  bool do_decode = false;
  const GridPlan* gp = nullptr;
  const float* noise = nullptr;  // noise: n_draws host-supplied raw draws from draw_base on, or Philox(seed, sample_offset + molecule)
  int draw_base = 0, n_draws = 1;
  uint64_t seed = 0;
  int64_t sample_offset = 0;
  float std0 = 1.0f;
  bool guided = false;  // guidance: without a target_w where the kernels take the target elsewhere (a value target's rows, a callback's dT/dpred)
  const float* target_w = nullptr;
  float scale = 0.f;
  // outputs (each optional; x_out / onehot_out are read with do_decode, zt_out with seeded, chain_out holds keep_frames frames)
  float *z_out = nullptr, *x_out = nullptr, *onehot_out = nullptr, *zt_out = nullptr;
  int* nan_count = nullptr;
  float* chain_out = nullptr;
  int keep_frames = 0;
  CallHints hints;  // (may_pack is run_chain's to decide)
};

// the refusals every chain starts with, in this order
static int chain_refuse(gaudi_handle* h, bool guided, bool check_stale = true) {
  if (!h->has_edm) return fail(h, GAUDI_E_STATE, "EDM weights not loaded");
  if (check_stale && h->edm_stale) return fail(h, GAUDI_E_STATE, kEdmStale);
  if (guided && !h->has_pred) return fail(h, GAUDI_E_STATE, "guided sampling needs predictor weights");
  return GAUDI_OK;
}

// host state of a chain between chain_begin and chain_finish
struct ChainStage {
  std::vector<float> as_start;  // a seeded start's [B][2] alpha | sigma
  std::vector<int32_t> vt_on;   // value target: which rows of the step table lie in the guidance window (empty: no value target)
  size_t vt_trace_bytes = 0;
};

// Stages the graph, fills P, reserves the workspaces and uploads noise, the time-grid table, the seeded start and the value target.
static int chain_begin(gaudi_handle* h, const ChainCall& c, const CallHints& hints, KParams& P, ChainStage& vs) {
  if (int rc = chain_refuse(h, c.guided)) return rc;
  HIPCHECK(h, hipSetDevice(h->device));
  const int B = c.B, N = c.N;
  const GridPlan* const gp = c.gp;
  int rc = stage_graph(h, B, N, c.node_mask, c.edge_mask, P, h->HPE, c.guided ? h->HPP : 0, hints);
  if (rc) return rc;
  fill_edm(h, P);
  const int D = 3 + P.F, T = P.T;
  if (c.s_hi >= (gp ? gp->rows : T) || c.s_lo < 0) return fail(h, GAUDI_E_INVALID, "step index out of range");
  const size_t zb = sizeof(float) * B * N * D;
  if (gp) {
    HIPCHECK(h, h->d_gcoef.reserve(sizeof(float) * gp->coef.size()));
    HIPCHECK(h, h->d_gidx.reserve(sizeof(int32_t) * gp->idx.size()));
    HIPCHECK(h, hipMemcpyAsync(h->d_gcoef.p, gp->coef.data(), sizeof(float) * gp->coef.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHECK(h, hipMemcpyAsync(h->d_gidx.p, gp->idx.data(), sizeof(int32_t) * gp->idx.size(), hipMemcpyHostToDevice, h->stream));
    P.coef = h->d_gcoef.as<float>();
    P.step_idx = h->d_gidx.as<int>();
  }
  if (c.seeded) {
    const float g = h->gamma[gp->t0];  // as gaudi_predict_noised: alpha (en_diffusion.py:375-377), sigma (:370-373)
    std::vector<float>& as_start = vs.as_start;  // (read by the copy below: lives until chain_finish has synchronised)
    as_start.resize((size_t)B * 2);
    for (int b = 0; b < B; ++b) {
      as_start[2 * b] = sqrtf(sigmoid_host(-g));
      as_start[2 * b + 1] = sqrtf(sigmoid_host(g));
    }
    HIPCHECK(h, h->d_as.reserve(sizeof(float) * 2 * B));
    HIPCHECK(h, hipMemcpyAsync(h->d_as.p, as_start.data(), sizeof(float) * 2 * B, hipMemcpyHostToDevice, h->stream));
    P.alpha_sigma = h->d_as.as<float>();
    if (c.zt_out) {
      HIPCHECK(h, h->d_zt.reserve(zb));
      HIPCHECK(h, hipMemsetAsync(h->d_zt.p, 0, zb, h->stream));
      P.zt_out = h->d_zt.as<float>();
    }
  }
  HIPCHECK(h, h->d_zin.reserve(zb));
  HIPCHECK(h, h->d_zout.reserve(zb));
  HIPCHECK(h, h->d_x.reserve(sizeof(float) * B * N * 3));
  HIPCHECK(h, h->d_h.reserve(sizeof(float) * B * N * P.F));
  HIPCHECK(h, h->d_nan.reserve(sizeof(int)));
  HIPCHECK(h, hipMemsetAsync(h->d_nan.p, 0, sizeof(int), h->stream));
  if (P.rowmap != nullptr) {  // packed: masked nodes have no slot in any workgroup -- their rows stay zero
    HIPCHECK(h, hipMemsetAsync(h->d_zin.p, 0, zb, h->stream));
    HIPCHECK(h, hipMemsetAsync(h->d_zout.p, 0, zb, h->stream));
    HIPCHECK(h, hipMemsetAsync(h->d_x.p, 0, sizeof(float) * B * N * 3, h->stream));
    HIPCHECK(h, hipMemsetAsync(h->d_h.p, 0, sizeof(float) * B * N * P.F, h->stream));
  }
  if (c.z_in) HIPCHECK(h, hipMemcpyAsync(h->d_zin.p, c.z_in, zb, hipMemcpyHostToDevice, h->stream));
  const bool fixn = h->fix_noise && c.do_init;  // whole-chain calls only (gaudi_step / gaudi_decode inject per-molecule draws)
  const size_t nzb = fixn ? sizeof(float) * N * D : zb;  // bytes of one raw draw
  if (c.noise) {
    HIPCHECK(h, h->d_noise.reserve(nzb * (size_t)c.n_draws));
    HIPCHECK(h, hipMemcpyAsync(h->d_noise.p, c.noise, nzb * (size_t)c.n_draws, hipMemcpyHostToDevice, h->stream));
    P.noise = h->d_noise.as<float>();
  }
  P.draw_base = c.draw_base;
  P.draw_stride = fixn ? (long long)N * D : (long long)B * N * D;
  P.fix_noise = fixn ? 1 : 0;
  P.fix_key = h->fix_key;
  P.seed = c.seed;
  P.sample_offset = c.sample_offset;
  P.std0 = c.std0;
  P.mode = MODE_SAMPLE;
  P.x_out = h->d_x.as<float>();
  P.h_out = h->d_h.as<float>();
  P.nan_count = h->d_nan.as<int>();
  P.guided = c.guided;
  P.scale = c.scale;
  if (c.chain_out) {
    HIPCHECK(h, h->d_chain.reserve(zb * (size_t)c.keep_frames));
    HIPCHECK(h, hipMemsetAsync(h->d_chain.p, 0, zb * (size_t)c.keep_frames, h->stream));
    P.chain_out = h->d_chain.as<float>();
    P.keep_frames = c.keep_frames;
  }
  if (c.guided) {
    static const float no_w[16] = {};  // (the kernels read the parameter rows or the caller's dT/dpred instead)
    rc = fill_pred(h, P, c.target_w ? c.target_w : no_w, B, N);
    if (rc) return rc;
  }
  if (hints.vt && c.guided) {
    const VtCall& v = *hints.vt;
    if (P.rowmap != nullptr || P.NR != P.N || P.B != B) return fail(h, GAUDI_E_STATE, "a value-target launch must hold one molecule per workgroup");
    const int K = v.K, RW = target_row_floats(K), rows = gp ? gp->rows : T;
    std::vector<float> par((size_t)B * RW);
    for (int b = 0; b < B; ++b) vt_pack_row(*v.spec, K, v.b0 + b, &par[(size_t)b * RW]);
    HIPCHECK(h, h->d_vtpar.reserve(sizeof(float) * par.size()));
    HIPCHECK(h, hipMemcpyAsync(h->d_vtpar.p, par.data(), sizeof(float) * par.size(), hipMemcpyHostToDevice, h->stream));
    VtDev vd{};
    vd.par = h->d_vtpar.as<float>();
    vd.B = B;
    const int t_lo = v.spec->t_lo > 0 ? v.spec->t_lo : 1, t_hi = v.spec->t_hi > 0 ? v.spec->t_hi : T;
    vs.vt_on.resize(rows);
    for (int r = 0; r < rows; ++r) {
      const int t_from = gp ? (r == gp->rows - 1 ? gp->t0 : gp->idx[r + 1]) : r + 1;  // the step of row r starts at this time index
      vs.vt_on[r] = t_lo <= t_from && t_from <= t_hi;
    }
    if (v.trace) {
      vs.vt_trace_bytes = sizeof(float) * (size_t)(c.s_hi - c.s_lo + 1) * B * (K + 2);
      HIPCHECK(h, h->d_vttrace.reserve(vs.vt_trace_bytes));
      HIPCHECK(h, hipMemsetAsync(h->d_vttrace.p, 0, vs.vt_trace_bytes, h->stream));
      vd.trace = h->d_vttrace.as<float>();
      vd.top = c.s_hi;
    }
    HIPCHECK(h, h->d_vtdev.reserve(sizeof(VtDev)));
    HIPCHECK(h, hipMemcpyAsync(h->d_vtdev.p, &vd, sizeof(VtDev), hipMemcpyHostToDevice, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));  // (par and vd are locals of this block)
    P.vt = h->d_vtdev.as<VtDev>();
  }
  return GAUDI_OK;
}

// The copies out, the NaN count and the sync.  z_latest: the device buffer that holds the chain's last z.
static int chain_finish(gaudi_handle* h, const ChainCall& c, const CallHints& hints, const ChainStage& vs, const float* z_latest) {
  const int B = c.B, N = c.N, F = h->ecfg.in_node_nf;
  const size_t zb = sizeof(float) * B * N * (3 + F);
  if (c.z_out) HIPCHECK(h, hipMemcpyAsync(c.z_out, z_latest, zb, hipMemcpyDeviceToHost, h->stream));
  if (c.seeded && c.zt_out) HIPCHECK(h, hipMemcpyAsync(c.zt_out, h->d_zt.p, zb, hipMemcpyDeviceToHost, h->stream));
  if (c.do_decode) {
    HIPCHECK(h, hipMemcpyAsync(c.x_out, h->d_x.p, sizeof(float) * B * N * 3, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipMemcpyAsync(c.onehot_out, h->d_h.p, sizeof(float) * B * N * F, hipMemcpyDeviceToHost, h->stream));
  }
  if (c.chain_out)
    HIPCHECK(h, hipMemcpyAsync(c.chain_out, h->d_chain.p, zb * (size_t)c.keep_frames, hipMemcpyDeviceToHost, h->stream));
  std::vector<float> vt_tr(vs.vt_trace_bytes / sizeof(float));
  if (vs.vt_trace_bytes) HIPCHECK(h, hipMemcpyAsync(vt_tr.data(), h->d_vttrace.p, vs.vt_trace_bytes, hipMemcpyDeviceToHost, h->stream));
  int nanc = 0;
  HIPCHECK(h, hipMemcpyAsync(&nanc, h->d_nan.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  if (vs.vt_trace_bytes) {  // this call's molecules are rows b0 .. b0 + B of the request's [steps][Btot][K + 2]
    const VtCall& v = *hints.vt;
    const size_t row = (size_t)v.K + 2;
    for (int st = 0; st <= c.s_hi - c.s_lo; ++st)
      std::memcpy(v.trace + ((size_t)st * v.Btot + v.b0) * row, &vt_tr[(size_t)st * B * row], sizeof(float) * B * row);
  }
  if (c.nan_count) *c.nan_count = nanc;
  return GAUDI_OK;
}

// shared by the single steps, gaudi_decode and the whole chains without a callback
static int run_chain(gaudi_handle* h, const ChainCall& c) {
  // sampling calls may pack small molecules into one workgroup (stage_graph8); a value target's seed and trace are per
  // molecule while a shared workgroup has ONE readout: those calls keep one molecule per workgroup
  CallHints hints = c.hints;
  hints.may_pack = c.chain_out == nullptr && hints.vt == nullptr;
  KParams P{};
  ChainStage vs;
  int rc = chain_begin(h, c, hints, P, vs);
  if (rc) return rc;
  const int s_hi = c.s_hi, s_lo = c.s_lo, hpp = c.guided ? h->HPP : 0;
  const bool do_init = c.do_init, do_decode = c.do_decode;
  const std::vector<int32_t>& vt_on = vs.vt_on;
  float* zin = h->d_zin.as<float>();
  float* zout = h->d_zout.as<float>();
  if (h->plan.two && c.guided) {
    // Large molecules (V4G kernels) and sin_embedding denoisers without a fused kernel, guided: every reverse step is two launches -- the EDM-only kernel runs the step up to
    // z_s before guidance (split = 1: denoise, update with noise), the predictor-only kernel the guidance update, the
    // projection and the NaN scrub (MODE_GUIDE) -- then one decode pass.
    for (int s = s_hi; s >= s_lo; --s) {
      P.mode = MODE_SAMPLE;
      P.s_hi = P.s_lo = s;
      P.do_init = (s == s_hi) && do_init;
      P.do_decode = 0;
      const bool off_window = !vt_on.empty() && !vt_on[s];  // zero gradient: the denoiser-only kernel finishes the step itself
      P.split = off_window ? 0 : 1;
      P.z_in = zin;
      P.z_out = zout;
      rc = launch(h, P, h->HPE, 0, 1);
      if (rc) return rc;
      P.alpha_sigma = nullptr;  // (a seeded start: the first launch has noised the given molecules)
      P.zt_out = nullptr;
      if (off_window) {
        std::swap(zin, zout);
        continue;
      }
      P.mode = MODE_GUIDE;
      P.do_init = 0;
      P.split = 0;
      P.z_in = zout;
      P.z_out = zin;
      rc = launch(h, P, 0, hpp, 0);
      if (rc) return rc;
    }
    if (do_decode) {
      P.mode = MODE_SAMPLE;
      P.split = 0;
      P.s_hi = -1;
      P.s_lo = 0;
      P.do_init = (s_hi < s_lo) && do_init;
      P.do_decode = 1;
      P.z_in = zin;
      P.z_out = zout;
      rc = launch(h, P, h->HPE, 0, 0);
      if (rc) return rc;
      std::swap(zin, zout);
    }
  } else {
  // chunk the chain into launches of steps_per_launch steps; z ping-pongs zout -> zin
  bool first = true;
  int s = s_hi;
  const bool any_steps = s_hi >= s_lo;
  do {
    int lo = any_steps ? std::max(s_lo, s - h->steps_per_launch + 1) : s + 1;
    if (!vt_on.empty() && any_steps) {
      // a guidance window is launch-uniform: the launch ends where the next step falls on the other side of it, and a launch
      // outside the window takes the guided step with a zero gradient (guided = 2: no predictor pass)
      int cut = s;
      while (cut > lo && vt_on[cut - 1] == vt_on[s]) --cut;
      lo = cut;
      P.guided = vt_on[s] ? 1 : 2;
    }
    P.s_hi = s;
    P.s_lo = lo;
    P.do_init = first && do_init;
    P.do_decode = do_decode && lo <= s_lo;
    P.z_in = zin;
    P.z_out = zout;
    rc = launch(h, P, h->HPE, hpp, any_steps ? (s - lo + 1) : 0);
    if (rc) return rc;
    P.alpha_sigma = nullptr;  // (a seeded start: the first launch has noised the given molecules)
    P.zt_out = nullptr;
    std::swap(zin, zout);
    first = false;
    s = lo - 1;
  } while (any_steps && s >= s_lo);
  }
  return chain_finish(h, c, hints, vs, zin);  // (after the swap, `zin` holds the latest z)
}

// Largest sub-batch one chain may run at once.  The guided path keeps an activation stash of 2.9 MB per molecule (default
// sizes) for the whole call; very large requests are cut into sub-batches of whole multiples of 256 molecules (one per
// CU) that fit `budget` bytes.  Noise is keyed by the global sample index, so the result does not depend on the cut.
static int max_sub_batch(gaudi_handle* h, int B, int N, bool guided) {
  if (!guided) return B;
  const long long per_mol = 4LL * pred_stash_floats(N, h->HPP, h->pcfg.n_layers, dense_ew4(N));
  long long budget = 0;
  if (const char* e = getenv("GAUDI_MAX_WORKSPACE_MB")) budget = atoll(e) * (1LL << 20);
  const bool forced = budget > 0;
  if (!forced) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return B;
    budget = (long long)((free_b + h->d_stash.cap) * 0.8);
  }
  long long bmax = std::max(1LL, budget / std::max(1LL, per_mol));
  if (bmax >= 256) bmax = bmax / 256 * 256;
  else if (!forced) bmax = std::min<long long>(B, 256);  // let the allocation itself report a too-small device
  return (int)std::min<long long>(B, bmax);
}

// Node slots of the widest packed group the RESIDENT split kernels take at these widths (one round of eight edge tiles), below N;
// 0: none (no split images, no such kernel).  A function of the widths only.
static int resident_node_limit(gaudi_handle* h, int N, bool guided) {
  const int hpe = h->HPE, hpp = guided ? h->HPP : 0;
  if (h->variant != 8 || !h->split || !h->edm_ws_bytes || (hpp && !h->pred_ws_bytes)) return 0;
  if (GAUDI_NODE_F16 && (!(h->edm_hinv > 0.f) || (hpp && !(h->pred_hinv > 0.f)))) return 0;
  const int Dz = 3 + h->ecfg.in_node_nf;
  for (int ng = std::min(N - 1, 32); ng >= 8; --ng)
    for (int mode = 1; mode <= 2; ++mode) {
      int pubx = 0, pub_ch = 0;
      if (have_kernel8(hpe, hpp, mode, false) && plan_pub8(hpe, hpp, ng, Dz, 16 * w8::kWaves, mode, pubx, pub_ch)) return ng;
    }
  return 0;
}


// What a time grid adds to a chain (gaudi_sample_grid, gaudi_sample_target and the callback form), checked: the step table and,
// for a start from given molecules, their [x | onehot] rows as the forward-noising prologue reads them.  A seeded start refuses
// fix_noise: that option shares the PRIOR draw between molecules, and given molecules have no prior draw.
struct GridStart {
  GridPlan gp;
  std::vector<float> xh0;  // empty: the chain starts from the prior
  const float* xh() const { return xh0.empty() ? nullptr : xh0.data(); }
};
static int grid_start(gaudi_handle* h, int B, int N, int n_grid, const int32_t* grid, const float* x0, const float* onehot0,
                      GridStart& g) {
  if (int rc = chain_refuse(h, false, false)) return rc;
  const int T = h->ecfg.diffusion_steps, F = h->ecfg.in_node_nf, D = 3 + F;
  if (const char* why = grid_check(T, n_grid, grid)) return fail(h, GAUDI_E_INVALID, why);
  if ((x0 != nullptr) != (onehot0 != nullptr)) return fail(h, GAUDI_E_INVALID, "a start from given molecules needs both x0 and onehot0");
  if (!x0 && grid[0] != T) return fail(h, GAUDI_E_INVALID, "a chain from the prior must start at time index T (grid[0] == T)");
  if (x0 && h->fix_noise) return fail(h, GAUDI_E_INVALID, "fix_noise applies to chains from the prior, not to a start from given molecules");
  make_grid_plan(h->gamma, T, n_grid, grid, g.gp);
  if (x0) {
    g.xh0.resize((size_t)B * N * D);
    for (size_t r = 0; r < (size_t)B * N; ++r) {
      for (int d = 0; d < 3; ++d) g.xh0[r * D + d] = x0[r * 3 + d];
      for (int k = 0; k < F; ++k) g.xh0[r * D + 3 + k] = onehot0[r * F + k];
    }
  }
  return GAUDI_OK;
}

// the one-row table of the step t_idx -> s_idx (gaudi_step_pair, gaudi_step_target)
static GridPlan pair_plan(gaudi_handle* h, int s_idx, int t_idx) {
  GridPlan gp;
  gp.rows = 1;
  gp.t0 = t_idx;
  gp.coef.resize(4);
  coef_row(h->gamma, h->ecfg.diffusion_steps, s_idx, t_idx, gp.coef.data());
  gp.idx.assign(1, s_idx);
  return gp;
}

// A whole chain and its decode pass for a request of any size.  req names the graph, the noise, the guidance, the outputs and,
// where there is one, the time grid with its start (z_in = the given molecules' [x | onehot]) and the value target (hints.vt);
// the range, the buckets and the sub-batches are made here.
static int sample_impl(gaudi_handle* h, const ChainCall& req, gaudi_diag* diag) {
  const int B = req.B, N = req.N;
  const float *node_mask = req.node_mask, *edge_mask = req.edge_mask, *noise = req.noise, *xh0 = req.z_in;
  float *x_out = req.x_out, *onehot_out = req.onehot_out, *z0_out = req.z_out, *zt_out = req.zt_out;
  const GridPlan* const gp = req.gp;
  if (!h || !node_mask || !edge_mask || !x_out || !onehot_out) return GAUDI_E_INVALID;
  if (int rc = chain_refuse(h, req.guided)) return rc;
  if (B <= 0 || N <= 0) return fail(h, GAUDI_E_INVALID, "B and N must be positive");
  HIPCHECK(h, hipSetDevice(h->device));
  const int T = h->ecfg.diffusion_steps, F = h->ecfg.in_node_nf, D = 3 + F;
  const int s_top = gp ? gp->rows - 1 : T - 1;  // first row of the step table the chain walks down from
  VtCall vt = req.hints.vt ? *req.hints.vt : VtCall{};  // this request's value target, with b0 = where the sub-batch in flight starts
  h->last_split_resident = 0;
  // ---- per-molecule kernel family (round 6).  A request whose padded N is beyond the resident kernels' LDS limit used to run
  // EVERY molecule on the V8G kernels (node buffers in a global scratch: 20 % slower on a molecule that would fit, DESIGN section 2).
  // Now the molecules that fit the resident kernels on their own -- at most `lim` live nodes and one round of eight edge tiles: a
  // function of the molecule's own graph and the widths, so a molecule's kernel (and its rounding) does not depend on which
  // other molecules share the call or the shard -- form a first bucket that runs packed on the resident kernels; the rest
  // run on V8G as before.  Noise is keyed by the molecule's index in the request either way.
  std::vector<int32_t> small, large;
  int lim = 0;
  if (h->variant == 8 && h->family_split && h->pack && h->gn8 && h->gn8_pack && !h->force_gn && !h->force_gn8 && !h->fix_noise &&
      !h->plan_force_waves && (int64_t)B * N < (1 << 28) && !req.hints.vt) {  // (the first bucket runs PACKED: not for a value target)
    Meta8 M;
    std::string err;
    const int hpp = req.guided ? h->HPP : 0;
    if (build_meta8(B, N, node_mask, edge_mask, M, err, h->plan_min_slots) == GAUDI_OK) {
      int pubx = 0, pub_ch = 0;
      bool fits = false;  // the unpacked resident plan of the whole call, any split mode
      for (int mode = 1; mode <= 2 && !fits; ++mode)
        fits = have_kernel8(h->HPE, hpp, mode, hpp && M.S > 16 * w8::kWaves) && plan_pub8(h->HPE, hpp, N, D, M.S, mode, pubx, pub_ch);
      if (!fits && (lim = resident_node_limit(h, N, req.guided)) > 0) {
        const std::vector<std::vector<int>> used = used_nodes(B, N, node_mask, edge_mask);
        for (int b = 0; b < B; ++b) ((int)used[b].size() <= lim && M.ntiles[b] <= w8::kWaves ? small : large).push_back(b);
      }
    }
  }
  struct Bucket {
    const std::vector<int32_t>* idx;  // nullptr: the whole request in place
    int narrow;
  };
  std::vector<Bucket> buckets;
  if (small.empty()) buckets.push_back({nullptr, 0});
  else {
    buckets.push_back({&small, lim});
    if (!large.empty()) buckets.push_back({&large, 0});
    h->last_split_resident = (int)small.size();
  }
  int nanc = 0;
  std::vector<float> nz, gm, ge, gx, gh, gz, gs, gt;
  for (const Bucket& bk : buckets) {
    const int Bb = bk.idx ? (int)bk.idx->size() : B;
    const float *nmb = node_mask, *emb = edge_mask, *nsb = noise;
    float *xo = x_out, *ho = onehot_out, *zo = z0_out, *zto = xh0 ? zt_out : nullptr;
    const float* xhb = xh0;
    if (bk.idx) {  // gather the bucket's molecules
      gm.resize((size_t)Bb * N);
      ge.resize((size_t)Bb * N * N);
      gx.assign((size_t)Bb * N * 3, 0.f);
      gh.assign((size_t)Bb * N * F, 0.f);
      for (int k = 0; k < Bb; ++k) {
        const int b = (*bk.idx)[k];
        std::memcpy(&gm[(size_t)k * N], node_mask + (size_t)b * N, sizeof(float) * N);
        std::memcpy(&ge[(size_t)k * N * N], edge_mask + (size_t)b * N * N, sizeof(float) * N * N);
      }
      nmb = gm.data();
      emb = ge.data();
      xo = gx.data();
      ho = gh.data();
      if (z0_out) {
        gz.assign((size_t)Bb * N * D, 0.f);
        zo = gz.data();
      }
      if (xh0) {
        gs.resize((size_t)Bb * N * D);
        for (int k = 0; k < Bb; ++k)
          std::memcpy(&gs[(size_t)k * N * D], xh0 + (size_t)(*bk.idx)[k] * N * D, sizeof(float) * (size_t)N * D);
        xhb = gs.data();
        if (zto) {
          gt.assign((size_t)Bb * N * D, 0.f);
          zto = gt.data();
        }
      }
    }
    ChainCall c = req;  // one sub-batch of this bucket: the whole chain from the top row, then the decode pass
    c.s_hi = s_top;
    c.do_decode = true;
    c.n_draws = T + 2;
    c.do_init = xhb == nullptr;
    c.seeded = xhb != nullptr;
    c.hints = {.narrow = bk.narrow, .vt = req.hints.vt ? &vt : nullptr};
    const int bmax = max_sub_batch(h, Bb, N, req.guided);
    // sub-batches plan with the whole batch's graph figures (same kernel family and edge-GEMM arithmetic for every cut)
    c.hints.cut = bmax < Bb;
    if (bmax < Bb && h->variant == 8 && !bk.narrow) {
      Meta8 M;
      std::string err;
      const int rc = build_meta8(Bb, N, nmb, emb, M, err);
      if (rc == GAUDI_E_CAPACITY) c.hints.force_waves = 4;
      else if (rc) return fail(h, rc, err);
      else c.hints.min_slots = M.S;
    }
    for (int b0 = 0; b0 < Bb; b0 += bmax) {
      const int nb = std::min(bmax, Bb - b0);
      const float* nzp = nsb;
      if (noise && !h->fix_noise && (nb != B || bk.idx)) {  // gather this sub-batch's draws out of [T+2][B][N][D]
        nz.resize((size_t)(T + 2) * nb * N * D);
        for (int d = 0; d < T + 2; ++d)
          for (int k = 0; k < nb; ++k) {
            const int b = bk.idx ? (*bk.idx)[b0 + k] : b0 + k;
            std::memcpy(&nz[((size_t)d * nb + k) * N * D], noise + ((size_t)d * B + b) * N * D, sizeof(float) * (size_t)N * D);
          }
        nzp = nz.data();
      }
      c.hints.molmap = bk.idx ? bk.idx->data() + b0 : nullptr;
      vt.b0 = b0;
      int nan_sub = 0;
      c.B = nb;
      c.node_mask = nmb + (size_t)b0 * N;
      c.edge_mask = emb + (size_t)b0 * N * N;
      c.z_in = xhb ? xhb + (size_t)b0 * N * D : nullptr;
      c.noise = nzp;
      c.sample_offset = bk.idx ? req.sample_offset : req.sample_offset + b0;
      c.z_out = zo ? zo + (size_t)b0 * N * D : nullptr;
      c.x_out = xo + (size_t)b0 * N * 3;
      c.onehot_out = ho + (size_t)b0 * N * F;
      c.zt_out = zto ? zto + (size_t)b0 * N * D : nullptr;
      c.nan_count = &nan_sub;
      int rc = run_chain(h, c);
      if (rc) return rc;
      nanc += nan_sub;
    }
    if (bk.idx)  // scatter the bucket's results
      for (int k = 0; k < Bb; ++k) {
        const int b = (*bk.idx)[k];
        std::memcpy(x_out + (size_t)b * N * 3, &gx[(size_t)k * N * 3], sizeof(float) * N * 3);
        std::memcpy(onehot_out + (size_t)b * N * F, &gh[(size_t)k * N * F], sizeof(float) * N * F);
        if (z0_out) std::memcpy(z0_out + (size_t)b * N * D, &gz[(size_t)k * N * D], sizeof(float) * N * D);
        if (zto) std::memcpy(zt_out + (size_t)b * N * D, &gt[(size_t)k * N * D], sizeof(float) * N * D);
      }
  }
  finish_sample(B, N, node_mask, x_out, nanc, diag);
  return GAUDI_OK;
}

// gaudi_sample_cb / gaudi_sample_cbz / gaudi_sample_cb_grid: exactly one of the two callbacks is set.  req as for sample_impl
// (no value target); the request runs as ONE chain -- no buckets, no sub-batches, no packing.
static int sample_cb_impl(gaudi_handle* h, const ChainCall& req, gaudi_target_cb target_grad, gaudi_target_cbz target_grad_z,
                          void* user, gaudi_diag* diag) {
  if (!h || !req.node_mask || !req.edge_mask || !req.x_out || !req.onehot_out || (!target_grad && !target_grad_z)) return GAUDI_E_INVALID;
  if (int rc = chain_refuse(h, true)) return rc;
#ifdef GAUDI_STAMPS
  // the stamped diagnostic build times the fused step only: its 8-wave guide phase drops the direct dT/dz term (sampler_kernel.h)
  if (target_grad_z) return fail(h, GAUDI_E_INVALID, "gaudi_sample_cbz is not available in the GAUDI_STAMPS diagnostic build");
#endif
  const GridPlan* const gp = req.gp;
  int nanc = 0;
  ChainCall c = req;  // the whole chain from the top row (one launch pair per step, below), then the decode pass
  c.s_hi = gp ? gp->rows - 1 : h->ecfg.diffusion_steps - 1;
  c.do_decode = true;
  c.n_draws = h->ecfg.diffusion_steps + 2;
  c.do_init = req.z_in == nullptr;
  c.seeded = req.z_in != nullptr;
  c.guided = true;
  c.nan_count = &nanc;
  const CallHints hints;
  KParams P{};
  ChainStage vs;
  int rc = chain_begin(h, c, hints, P, vs);
  if (rc) return rc;
  const int B = c.B, N = c.N, D = 3 + P.F, T = P.T, K = h->pcfg.out_nf, s_top = c.s_hi;
  const size_t zb = sizeof(float) * B * N * D, pb = sizeof(float) * B * K;
  const float* coef_h = gp ? gp->coef.data() : h->coef.data();
  HIPCHECK(h, h->d_pred.reserve(pb));
  HIPCHECK(h, h->d_dpred.reserve(pb));
  HIPCHECK(h, h->p_pred.reserve(pb));
  HIPCHECK(h, h->p_dpred.reserve(pb));
  if (target_grad_z) {  // the target also depends on z directly: z_s goes to the host, scale * mask * dT/dz comes back
    HIPCHECK(h, h->d_dz.reserve(zb));
    HIPCHECK(h, h->p_z.reserve(zb));
    HIPCHECK(h, h->p_dz.reserve(zb));
  }
  if (!h->cb_event) HIPCHECK(h, hipEventCreateWithFlags(&h->cb_event, hipEventDisableTiming));
  P.pred_out = h->d_pred.as<float>();
  P.dpred_in = h->d_dpred.as<float>();
  float* pred = h->p_pred.as<float>();
  float* dT = h->p_dpred.as<float>();
  float* zin = h->d_zin.as<float>();
  float* zout = h->d_zout.as<float>();
  // Large molecules (V4G kernels: node buffers in global memory) have no fused EDM + predictor instantiation (DESIGN.md
  // 7.12): phase A is the EDM-only kernel (split = 1: z_t -> z_s before guidance) followed by the predictor-only kernel's
  // forward half (MODE_GUIDE, split = 1), phase B the predictor-only kernel's second half (MODE_GUIDE, split = 2).
  const bool gn = h->plan.two;
  // GAUDI_DEBUG_CB: where a callback step's host time goes (enqueue / wait for pred / the caller's function)
  const bool dbg_cb = getenv("GAUDI_DEBUG_CB") != nullptr;
  double t_enq = 0, t_wait = 0, t_user = 0;
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  for (int s = s_top; s >= 0; --s) {
    const double t0 = dbg_cb ? now() : 0;
    const float t_step = gp ? coef_h[4 * s + 3] : (float)(s + 1) / (float)T;  // (the same float either way: coef_row)
    // phase A: z_t -> z_s (before guidance) and pred = predictor(z_s, t); the activation stash stays on the device
    P.mode = MODE_SAMPLE;
    P.s_hi = P.s_lo = s;
    P.do_init = s == s_top && c.do_init;
    P.do_decode = 0;
    P.split = 1;
    P.z_in = zin;
    P.z_out = zout;
    rc = launch(h, P, h->HPE, gn ? 0 : h->HPP, 1);
    if (rc) return rc;
    P.alpha_sigma = nullptr;
    P.zt_out = nullptr;
    if (gn) {
      P.mode = MODE_GUIDE;
      P.do_init = 0;
      P.z_in = zout;
      P.z_out = zin;
      rc = launch(h, P, 0, h->HPP, 0);
      if (rc) return rc;
    }
    HIPCHECK(h, hipMemcpyAsync(pred, h->d_pred.p, pb, hipMemcpyDeviceToHost, h->stream));
    if (target_grad_z) HIPCHECK(h, hipMemcpyAsync(h->p_z.p, zout, zb, hipMemcpyDeviceToHost, h->stream));  // z_s before guidance
    HIPCHECK(h, hipEventRecord(h->cb_event, h->stream));
    const double t1 = dbg_cb ? now() : 0;
    HIPCHECK(h, hipEventSynchronize(h->cb_event));
    const double t2 = dbg_cb ? now() : 0;
    std::memset(dT, 0, pb);
    if (target_grad_z) {
      float* dz = h->p_dz.as<float>();
      std::memset(dz, 0, zb);
      target_grad_z(user, B, N, D, K, h->p_z.as<float>(), pred, t_step, dT, dz);
      // energy = scale * sum_b T (en_diffusion.py:899-903); the reference asserts that the x part of the gradient is zero on
      // masked nodes (remove_mean_with_mask, utils.py:33-44): the direct term is masked here
      for (int b = 0; b < B; ++b)
        for (int n = 0; n < N; ++n) {
          const float m = c.scale * c.node_mask[(size_t)b * N + n];
          for (int d = 0; d < D; ++d) dz[((size_t)b * N + n) * D + d] *= m;
        }
      HIPCHECK(h, hipMemcpyAsync(h->d_dz.p, dz, zb, hipMemcpyHostToDevice, h->stream));
      P.dz_in = h->d_dz.as<float>();
    } else {
      target_grad(user, B, K, pred, t_step, dT);
    }
    const double t3 = dbg_cb ? now() : 0;
    HIPCHECK(h, hipMemcpyAsync(h->d_dpred.p, dT, pb, hipMemcpyHostToDevice, h->stream));
    // phase B: reverse pass with the caller's dT/dpred, clip / project / apply, CoG removal
    P.mode = gn ? MODE_GUIDE : MODE_SAMPLE;
    P.do_init = 0;
    P.split = 2;
    P.z_in = zout;
    P.z_out = zin;
    rc = launch(h, P, gn ? 0 : h->HPE, h->HPP, 0);
    if (rc) return rc;
    if (dbg_cb) {
      t_enq += (t1 - t0) + (now() - t3);
      t_wait += t2 - t1;
      t_user += t3 - t2;
    }
  }
  if (dbg_cb)
    fprintf(stderr, "[callback] per step: enqueue %.1f us, wait for pred %.1f us, caller's function %.1f us (%d steps)\n",
            1e6 * t_enq / (s_top + 1), 1e6 * t_wait / (s_top + 1), 1e6 * t_user / (s_top + 1), s_top + 1);
  // decode pass
  P.mode = MODE_SAMPLE;
  P.split = 0;
  P.s_hi = -1;
  P.s_lo = 0;
  P.do_init = 0;
  P.do_decode = 1;
  P.z_in = zin;
  P.z_out = zout;
  rc = launch(h, P, h->HPE, gn ? 0 : h->HPP, 0);
  if (rc) return rc;
  if (int rc2 = chain_finish(h, c, hints, vs, zout)) return rc2;
  finish_sample(B, N, c.node_mask, c.x_out, nanc, diag);
  return GAUDI_OK;
}

// Zero-fills the caller's trace ([rows][B][K + 2] or nullptr) and names it with the spec: the value-target part of a request.
static VtCall vt_request(const gaudi_target_spec* spec, int K, int B, int rows, float* trace) {
  if (trace) std::memset(trace, 0, sizeof(float) * (size_t)rows * B * (K + 2));
  return VtCall{spec, K, B, 0, trace};
}

extern "C" {

// (the single steps: eps_raw stands for one raw draw of a whole chain -- T - s_idx for the step that lands on s_idx, T + 1 for the decode pass)
int gaudi_step(gaudi_handle* h, int B, int N, int s_idx, const float* z_t, const float* node_mask,
               const float* edge_mask, const float* eps_raw, const float* target_w, float scale, float* zs_out) {
  if (!h || !z_t || !node_mask || !edge_mask || !eps_raw || !zs_out) return GAUDI_E_INVALID;
  return run_chain(h, {.B = B, .N = N, .node_mask = node_mask, .edge_mask = edge_mask, .z_in = z_t, .s_hi = s_idx, .s_lo = s_idx,
                       .noise = eps_raw, .draw_base = h->ecfg.diffusion_steps - s_idx, .guided = target_w != nullptr,
                       .target_w = target_w, .scale = scale, .z_out = zs_out});
}

int gaudi_step_pair(gaudi_handle* h, int B, int N, int s_idx, int t_idx, const float* z_t, const float* node_mask,
                    const float* edge_mask, const float* eps_raw, const float* target_w, float scale, float* zs_out) {
  if (!h || !z_t || !node_mask || !edge_mask || !eps_raw || !zs_out) return GAUDI_E_INVALID;
  if (int rc = chain_refuse(h, false)) return rc;
  const int T = h->ecfg.diffusion_steps;
  if (s_idx < 0 || t_idx <= s_idx || t_idx > T) return fail(h, GAUDI_E_INVALID, "a step needs 0 <= s_idx < t_idx <= T");
  const GridPlan gp = pair_plan(h, s_idx, t_idx);
  return run_chain(h, {.B = B, .N = N, .node_mask = node_mask, .edge_mask = edge_mask, .z_in = z_t, .gp = &gp, .noise = eps_raw,
                       .draw_base = T - s_idx, .guided = target_w != nullptr, .target_w = target_w, .scale = scale, .z_out = zs_out});
}

int gaudi_decode(gaudi_handle* h, int B, int N, const float* z0, const float* node_mask, const float* edge_mask,
                 const float* eps_raw, float* x_out, float* onehot_out) {
  if (!h || !z0 || !node_mask || !edge_mask || !eps_raw || !x_out || !onehot_out) return GAUDI_E_INVALID;
  return run_chain(h, {.B = B, .N = N, .node_mask = node_mask, .edge_mask = edge_mask, .z_in = z0, .s_hi = -1, .do_decode = true,
                       .noise = eps_raw, .draw_base = h->ecfg.diffusion_steps + 1, .x_out = x_out, .onehot_out = onehot_out});
}

int gaudi_sample(gaudi_handle* h, int B, int N, const float* node_mask, const float* edge_mask, uint64_t seed,
                 int64_t sample_offset, const float* noise, float std, const float* target_w, float scale,
                 float* x_out, float* onehot_out, float* z0_out, gaudi_diag* diag) {
  return sample_impl(h, {.B = B, .N = N, .node_mask = node_mask, .edge_mask = edge_mask, .noise = noise, .seed = seed,
                         .sample_offset = sample_offset, .std0 = std, .guided = target_w != nullptr, .target_w = target_w,
                         .scale = scale, .z_out = z0_out, .x_out = x_out, .onehot_out = onehot_out}, diag);
}

int gaudi_sample_grid(gaudi_handle* h, int B, int N, const float* node_mask, const float* edge_mask, uint64_t seed,
                      int64_t sample_offset, const float* noise, float std, const float* target_w, float scale, int n_grid,
                      const int32_t* grid, const float* x0, const float* onehot0, float* x_out, float* onehot_out, float* z0_out,
                      float* zt_out, gaudi_diag* diag) {
  if (!h || !node_mask || !edge_mask || !x_out || !onehot_out) return GAUDI_E_INVALID;
  if (B <= 0 || N <= 0) return fail(h, GAUDI_E_INVALID, "B and N must be positive");
  GridStart g;
  if (int rc = grid_start(h, B, N, n_grid, grid, x0, onehot0, g)) return rc;
  return sample_impl(h, {.B = B, .N = N, .node_mask = node_mask, .edge_mask = edge_mask, .z_in = g.xh(), .gp = &g.gp, .noise = noise,
                         .seed = seed, .sample_offset = sample_offset, .std0 = std, .guided = target_w != nullptr, .target_w = target_w,
                         .scale = scale, .z_out = z0_out, .x_out = x_out, .onehot_out = onehot_out, .zt_out = zt_out}, diag);
}

int gaudi_host_target_seed(const gaudi_target_spec* spec, int B, int K, const float* pred, float* out) {
  if (!spec || !pred || !out || vt_check(spec, B, K, 0)) return GAUDI_E_INVALID;
  std::vector<float> row(target_row_floats(K));
  for (int b = 0; b < B; ++b) {
    vt_pack_row(*spec, K, b, row.data());
    for (int k = 0; k < K; ++k) out[(size_t)b * K + k] = target_seed(row.data(), K, k, pred[(size_t)b * K + k]);
  }
  return GAUDI_OK;
}

int gaudi_sample_target(gaudi_handle* h, int B, int N, const float* node_mask, const float* edge_mask, uint64_t seed,
                        int64_t sample_offset, const float* noise, float std, const gaudi_target_spec* spec, int n_grid,
                        const int32_t* grid, const float* x0, const float* onehot0, float* x_out, float* onehot_out,
                        float* z0_out, float* zt_out, float* trace_out, gaudi_diag* diag) {
  if (!h || !node_mask || !edge_mask || !x_out || !onehot_out) return GAUDI_E_INVALID;
  if (B <= 0 || N <= 0) return fail(h, GAUDI_E_INVALID, "B and N must be positive");
  if (int rc = chain_refuse(h, true, false)) return rc;  // (stale weights are refused after the spec and the grid: sample_impl)
  const int T = h->ecfg.diffusion_steps, K = h->pcfg.out_nf;
  if (const char* why = vt_check(spec, B, K, T)) return fail(h, GAUDI_E_INVALID, why);
  std::vector<int32_t> unit;
  if (!grid) {  // the unit grid T, T - 1, ..., 0: gaudi_sample's chain
    unit.resize(T + 1);
    for (int k = 0; k <= T; ++k) unit[k] = T - k;
    grid = unit.data();
    n_grid = T + 1;
  }
  GridStart g;
  if (int rc = grid_start(h, B, N, n_grid, grid, x0, onehot0, g)) return rc;
  const VtCall vt = vt_request(spec, K, B, g.gp.rows, trace_out);
  return sample_impl(h, {.B = B, .N = N, .node_mask = node_mask, .edge_mask = edge_mask, .z_in = g.xh(), .gp = &g.gp, .noise = noise,
                         .seed = seed, .sample_offset = sample_offset, .std0 = std, .guided = true, .scale = 1.0f, .z_out = z0_out,
                         .x_out = x_out, .onehot_out = onehot_out, .zt_out = zt_out, .hints = {.vt = &vt}}, diag);
}

int gaudi_step_target(gaudi_handle* h, int B, int N, int s_idx, int t_idx, const float* z_t, const float* node_mask,
                      const float* edge_mask, const float* eps_raw, const gaudi_target_spec* spec, float* zs_out,
                      float* trace_out) {
  if (!h || !z_t || !node_mask || !edge_mask || !eps_raw || !zs_out) return GAUDI_E_INVALID;
  if (int rc = chain_refuse(h, true)) return rc;
  const int T = h->ecfg.diffusion_steps, K = h->pcfg.out_nf;
  if (s_idx < 0 || t_idx <= s_idx || t_idx > T) return fail(h, GAUDI_E_INVALID, "a step needs 0 <= s_idx < t_idx <= T");
  if (const char* why = vt_check(spec, B, K, T)) return fail(h, GAUDI_E_INVALID, why);
  const GridPlan gp = pair_plan(h, s_idx, t_idx);
  const VtCall vt = vt_request(spec, K, B, 1, trace_out);
  return run_chain(h, {.B = B, .N = N, .node_mask = node_mask, .edge_mask = edge_mask, .z_in = z_t, .gp = &gp, .noise = eps_raw,
                       .draw_base = T - s_idx, .guided = true, .scale = 1.0f, .z_out = zs_out, .hints = {.vt = &vt}});
}

int gaudi_sample_cb(gaudi_handle* h, int B, int N, const float* node_mask, const float* edge_mask, uint64_t seed,
                    int64_t sample_offset, const float* noise, float std, gaudi_target_cb target_grad, void* user,
                    float scale, float* x_out, float* onehot_out, float* z0_out, gaudi_diag* diag) {
  if (!target_grad) return GAUDI_E_INVALID;
  return sample_cb_impl(h, {.B = B, .N = N, .node_mask = node_mask, .edge_mask = edge_mask, .noise = noise, .seed = seed,
                            .sample_offset = sample_offset, .std0 = std, .scale = scale, .z_out = z0_out, .x_out = x_out,
                            .onehot_out = onehot_out}, target_grad, nullptr, user, diag);
}

int gaudi_sample_cbz(gaudi_handle* h, int B, int N, const float* node_mask, const float* edge_mask, uint64_t seed,
                     int64_t sample_offset, const float* noise, float std, gaudi_target_cbz target_grad, void* user,
                     float scale, float* x_out, float* onehot_out, float* z0_out, gaudi_diag* diag) {
  if (!target_grad) return GAUDI_E_INVALID;
  return sample_cb_impl(h, {.B = B, .N = N, .node_mask = node_mask, .edge_mask = edge_mask, .noise = noise, .seed = seed,
                            .sample_offset = sample_offset, .std0 = std, .scale = scale, .z_out = z0_out, .x_out = x_out,
                            .onehot_out = onehot_out}, nullptr, target_grad, user, diag);
}

int gaudi_sample_cb_grid(gaudi_handle* h, int B, int N, const float* node_mask, const float* edge_mask, uint64_t seed,
                         int64_t sample_offset, const float* noise, float std, gaudi_target_cb target_grad,
                         gaudi_target_cbz target_grad_z, void* user, float scale, int n_grid, const int32_t* grid, const float* x0,
                         const float* onehot0, float* x_out, float* onehot_out, float* z0_out, float* zt_out, gaudi_diag* diag) {
  if (!h || !node_mask || !edge_mask || !x_out || !onehot_out) return GAUDI_E_INVALID;
  if ((target_grad != nullptr) == (target_grad_z != nullptr)) return fail(h, GAUDI_E_INVALID, "exactly one of the two callbacks must be set");
  if (B <= 0 || N <= 0) return fail(h, GAUDI_E_INVALID, "B and N must be positive");
  GridStart g;
  if (int rc = grid_start(h, B, N, n_grid, grid, x0, onehot0, g)) return rc;
  return sample_cb_impl(h, {.B = B, .N = N, .node_mask = node_mask, .edge_mask = edge_mask, .z_in = g.xh(), .gp = &g.gp, .noise = noise,
                            .seed = seed, .sample_offset = sample_offset, .std0 = std, .scale = scale, .z_out = z0_out, .x_out = x_out,
                            .onehot_out = onehot_out, .zt_out = zt_out}, target_grad, target_grad_z, user, diag);
}

int gaudi_sample_chain(gaudi_handle* h, int B, int N, const float* node_mask, const float* edge_mask, uint64_t seed,
                       int64_t sample_offset, const float* noise, float std, int keep_frames, float* chain_out) {
  if (!h || !node_mask || !edge_mask || !chain_out) return GAUDI_E_INVALID;
  if (int rc = chain_refuse(h, false)) return rc;
  const int T = h->ecfg.diffusion_steps, F = h->ecfg.in_node_nf, D = 3 + F;
  if (keep_frames < 1 || keep_frames > T) return fail(h, GAUDI_E_INVALID, "keep_frames must be in 1..T");
  std::vector<float> x((size_t)B * N * 3), oh((size_t)B * N * F);
  int rc = run_chain(h, {.B = B, .N = N, .node_mask = node_mask, .edge_mask = edge_mask, .do_init = true, .s_hi = T - 1,
                         .do_decode = true, .noise = noise, .n_draws = T + 2, .seed = seed, .sample_offset = sample_offset, .std0 = std,
                         .x_out = x.data(), .onehot_out = oh.data(), .chain_out = chain_out, .keep_frames = keep_frames});
  if (rc) return rc;
  // chain[0] = cat[x, h_categorical] (en_diffusion.py:1168-1169)
  for (int b = 0; b < B; ++b)
    for (int n = 0; n < N; ++n) {
      float* dst = chain_out + ((size_t)b * N + n) * D;
      for (int d = 0; d < 3; ++d) dst[d] = x[((size_t)b * N + n) * 3 + d];
      for (int k = 0; k < F; ++k) dst[3 + k] = oh[((size_t)b * N + n) * F + k];
    }
  return GAUDI_OK;
}

}  // extern "C"
