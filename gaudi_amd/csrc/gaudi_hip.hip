// gaudi_hip.hip -- host side of libgaudi_hip.so: the C ABI declared in include/gaudi_hip.h.
// Builds the noise-schedule tables, packs reference-format checkpoints into the kernels' tile
// layout, turns (node_mask, edge_mask) into per-wave edge lists and launches the per-molecule
// persistent kernel (sampler_kernel.h) on the handle's own HIP stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <queue>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gaudi_hip.h"
#include "kernel_table.h"

using namespace gaudi;

// -------------------------------------------------------------------------------------------------
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return (T*)p; }
};

// pinned host memory (the per-step [B,K] exchange of gaudi_sample_cb: a pageable hipMemcpyAsync is staged and blocks)
struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return (T*)p; }
};

// Where a launch keeps its node buffers ([node slots][HP + 4] floats each); the values are what gaudi_node_buffers reports
enum NodeBuf : int {
  kResident = 0,         // all in LDS
  kAllGlobal = 1,        // all in the workgroup's global scratch (4 waves: V4G; 8 waves: V8G, round 4)
  kPqLds = 2,            // V8G with P and Q in LDS (round 6, kern8gp_*.hip)
  kPredFifthGlobal = 3,  // resident but the predictor's fifth buffer: wide groups on the FULL ring (round 6, kern8mp_*.hip)
};
// What the CURRENT call runs on: decided by stage_graph, read by launch, the fill_* functions, run_chain and the getters
struct LaunchPlan {
  int waves = 4;             // kernel family (an 8-wave handle falls back to 4 waves for graphs that do not fit)
  int ring = 0;              // 8 waves: 1 = split operands on the full weight ring, 2 = on the half ring, 0 = fp32 instructions
  bool mr = false;           // 8 waves: the predictor takes several rounds of edge tiles
  NodeBuf nodes = kResident;
  bool two = false;          // guided steps are two launches (denoiser-only kernel, then predictor-only kernel): no fused instantiation
  bool fr = false;           // 8 waves: launches on the resident full-ring kernel take its FR instantiation where one exists
  bool n1 = false;           // 8 waves: ... their N1 instantiation (at most 16 node slots, one tail k-step) where one exists
  int ef = 2;                // edge features of the denoiser's first Linears (24: a sin_embedding denoiser, 4-wave family only)
  int groups = 0;            // workgroups (= molecules unless packed)
  int nslots = 0;            // node slots per workgroup (= N unless the call runs wide groups)
  int hk = 0;                // floats of the kept split copy of h behind the LDS plan (0: none)
  int pubx = 0, pub_ch = 0;  // reverse pass: extra floats of the du publish buffer, feature tiles published per chunk (plan_pub8)
};

// A value-target request (gaudi_sample_target / gaudi_step_target): the chain stages the parameter rows of ITS molecules
// (request index = b0 + k), the window flags and the trace, and keeps every molecule alone in its workgroup.
struct VtCall {
  const gaudi_target_spec* spec = nullptr;
  int K = 0, Btot = 0, b0 = 0;
  float* trace = nullptr;  // host [rows][Btot][K + 2], zero-filled by the entry point, or nullptr
};

// What ONE call tells the planner beyond its graph (stage_graph / stage_graph8): filled in chain_host.inc, the defaults elsewhere.
struct CallHints {
  int min_slots = 0, force_waves = 0;  // gaudi_sample's sub-batches plan with their whole bucket's figures (cf. plan_min_slots)
  bool cut = false;  // gaudi_sample cut this request into sub-batches
  // Per-molecule kernel family (round 6): gaudi_sample sorts a request whose padded N is beyond the resident kernels' LDS limit into
  // molecules that fit those kernels on their OWN (few enough live nodes and edge tiles) and the rest (V8G), and runs the two
  // buckets one after the other.  narrow = node slots per workgroup of the first bucket's packed launch (< N); molmap =
  // the bucket's molecule -> index in the request (the Philox key is the molecule's global sample index).
  int narrow = 0;
  const int32_t* molmap = nullptr;
  bool may_pack = false;       // small molecules may share a workgroup (sampling chains only: run_chain)
  const VtCall* vt = nullptr;  // the value-target request this call is part of
};

struct gaudi_handle {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  std::string warn;  // the last non-fatal condition a caller should know about (gaudi_last_warning)
  bool has_edm = false, has_pred = false;
  gaudi_edm_config ecfg{};
  gaudi_pred_config pcfg{};
  int HPE = 0, HPP = 0;
  DevBuf edm_w, pred_w, coef_d, edm_w4, pred_w4;  // *_w4: row-major tiles for the 4-wave fallback of an 8-wave handle
  DevBuf edm_ws, pred_ws;                         // fp16-pair images of the edge-GEMM matrices (w8_split.h)
  size_t edm_w_bytes = 0, pred_w_bytes = 0, edm_ws_bytes = 0, pred_ws_bytes = 0;
  float edm_hinv = 0.f, pred_hinv = 0.f;  // 2^-s of the fp16-pair node images inside *_ws (w8_nodes_f16.h); 0: the weight set
                                          // was refused (node_scale) -- its calls run the fp32-instruction kernels
  std::vector<float> gamma, coef;
  // per-call workspaces
  DevBuf d_mask, d_order, d_edges, d_emask, d_npairs, d_seg, d_zin, d_zout, d_t, d_x, d_h, d_noise, d_nan, d_dpred,
      d_pred, d_tw, d_stash, d_chain, d_sx, d_stype, d_sn, d_sflags, d_sdist, d_sadj, d_saux, d_stab, d_as, d_ncols, d_soff,
      d_sidx, d_gnode, d_rowmap, d_compmol, d_ncomp, d_clock, d_gcoef, d_gidx, d_zt;  // d_gcoef / d_gidx / d_zt: time-grid chains
  DevBuf d_atoms[9];  // gaudi_rings_to_atoms (atoms.inc): its outputs and its tables
  DevBuf d_rings[13];  // gaudi_atoms_to_rings (rings.inc): its three inputs, its tables and its nine outputs
  DevBuf d_bonds[9];   // gaudi_bond_orders (bonds.inc): its four inputs, its tables and its four outputs
  DevBuf d_canon[11];  // gaudi_canonical_order (canon.inc): its four inputs and its seven outputs
  DevBuf d_fp[16];     // fingerprints and their similarity (fp.inc: FpBuf names the slots)
  int fp_lib_rows = 0, fp_lib_bins = 0;  // the resident fingerprint library (gaudi_fp_library_set); 0 rows: none
  DevBuf d_fps[16];    // neighbour lists, clusters and diverse picks of fingerprint batches (fp_select.inc: FsBuf names the slots)
  double fs_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // ... and the stage times of their most recent profiled call (FsStage)
  DevBuf d_sub[10];    // gaudi_substructure_search (sub.inc): its four inputs, the pattern plans and its five outputs
  DevBuf d_huckel[22];  // gaudi_huckel (huckel.inc): its five inputs, the tier lists, the table and its fifteen outputs
  DevBuf d_ppp[38];     // gaudi_ppp (ppp.inc): its six inputs, the tier lists, the table, its eighteen outputs and the density scratch;
                        // gaudi_ppp_cis (ppp_cis.inc): the hand-over rows and its ten outputs
  DevBuf d_ppp_open[33];  // gaudi_ppp_open (ppp_open.inc): gaudi_ppp's inputs and the multiplicity, its twenty-three outputs, the density scratch
  DevBuf d_ppp_scf[35];   // gaudi_ppp_scf (ppp_scf.inc): gaudi_ppp_open's inputs, its twenty-five outputs, the scratch of one launch
  DevBuf d_kekule[14];  // gaudi_kekule (kekule.inc): its four inputs, the tables and its nine outputs
  DevBuf d_ring[23];    // gaudi_ring_currents (ring_current.inc): its six inputs, the tier lists, the table and its fifteen outputs
  DevBuf d_react[21];   // gaudi_reactivity (reactivity.inc): its five inputs, the tier lists, the table, its thirteen outputs and the job words
  DevBuf d_vtpar, d_vttrace, d_vtdev;  // value targets: per-molecule parameter rows, the guidance trace, the VtDev that names them
  PinBuf p_pred, p_dpred;     // gaudi_sample_cb: pred [B,K] device -> host, dT/dpred [B,K] host -> device, once per step
  PinBuf p_z, p_dz;           // gaudi_sample_cbz: z_s [B,N,D] device -> host, scale * dT/dz host -> device
  DevBuf d_dz;
  hipEvent_t cb_event = nullptr;
  int steps_per_launch = 25;
  int variant = 8;            // 8 = two waves per SIMD (sampler_kernel8, default), 4 = one wave per SIMD (GAUDI_WAVES=4)
  LaunchPlan plan;            // what the CURRENT call runs on
  bool split = true;          // 8-wave kernels: GEMMs on the fp16 matrix pipe with operands split into fp16 pairs (GAUDI_EDGE_MATH=fp32: off)
  bool no_fr = false;         // GAUDI_NO_FR=1: never the FR instantiation of the resident full-ring kernel (kern8s2_*.hip)
  bool no_n1 = false;         // GAUDI_NO_N1=1: never the N1 instantiation of the resident full-ring kernel (kern8s1_*.hip)
  bool no_side = false;       // GAUDI_NO_SIDE=1: the N1 fused kernel never runs its side job (w8_pred.h: pred_forward, SD)
  std::string last_key;       // key_name of the kernel the most recent launch ran (gaudi_last_kernel_key)
  std::vector<std::string> key_log;  // the distinct key_names launched since gaudi_create, in first-launch order (gaudi_kernel_key_log)
  bool wide_full = true;      // GAUDI_WIDE_FULL=0: wide groups that do not fit the full ring run on the half ring (round 5)
  bool gn8_pq = true;         // GAUDI_GN8_PQ=0: never the P / Q-in-LDS form (kern8gp_*.hip)
  bool gn8 = true;            // GAUDI_GN8=0: molecules beyond the LDS limit go to the 4-wave V4G kernels, as in round 3
  bool force_gn8 = false;     // GAUDI_FORCE_GN8=1: V8G whenever it can run (test knob)
  bool pack = true;           // several small molecules per workgroup in sampling calls (GAUDI_PACK=0: off)
  int pairs_cap = -1;         // GAUDI_PAIRS_CAP: two-molecule groups of a wide launch (-1: chosen by wide_plan below; experiments)
  int pairs = 1;              // wide groups (more node slots than a molecule has, two rounds of edge tiles: e.g. two 11-ring cata
                              // molecules per workgroup): 0 = never, 1 = when the batch holds at least two molecules per CU and the
                              // classic packing shares next to nothing (default since round 5: the fp16-pair node GEMMs made the
                              // shared weight stream worth the second round), 2 = always (GAUDI_PAIRS)
  int num_cus = 256;
  bool pred_rounds = true;    // GAUDI_PRED_ROUNDS=0: guided calls with more than 128 edge slots go to the 4-wave kernels
  bool force_mr = false;      // GAUDI_FORCE_MR
  bool force_gn = false;      // GAUDI_FORCE_GN=1 at gaudi_create: use them whenever they exist (test knob)
  bool fix_noise = false;     // en_diffusion.py:562-566: one raw draw per call, broadcast over the batch
  long long fix_key = 0;      // global sample index whose Philox stream is shared
  int readout_n = 0;  // padded N the predictor readout divides by (0 = the call's N)
  struct PredTrainState* pt = nullptr;  // the predictor in torch layout for gaudi_predictor_loss_grad (pred_train_host.inc)
  struct EdmTrainState* et = nullptr;   // the denoiser in torch layout for gaudi_edm_loss_grad (edm_train_host.inc)
  bool edm_stale = false;  // gaudi_edm_set_train_weights changed the weights after the sampler images were packed
  // Plan hint (gaudi_set_plan_hint): the kernel family and the edge-GEMM arithmetic of a call follow from batch-wide maxima
  // (edge slots, a node's live edges).  A shard of a larger logical batch plans with the WHOLE batch's figures, so that a
  // molecule's rounding does not depend on where the batch was cut.  gaudi_sample passes the same for its own sub-batches as
  // an argument (CallHints above).
  int plan_min_slots = 0, plan_force_waves = 0;
  bool keep_h = true;         // GAUDI_KEEP_H=0: every node GEMM that reads h splits it again (round 5)
  bool gn8_pack = true;       // GAUDI_GN8_PACK=0: V8G launches keep a molecule's nodes where the masks have them (round 5)
  bool family_split = false;  // GAUDI_FAMILY_SPLIT=1: per-molecule kernel family (below).  Off by default: the two buckets run as two launches
                              // per 25 steps on one stream, each with its own tail -- c4x 76.8 against 84.3 mol/s in one family
  int last_split_resident = 0;  // molecules of the last gaudi_sample call that ran on the resident kernels beside a V8G bucket
  // profiling: launches are bracketed by HIP events on the handle's stream.  A small window of pending pairs is kept;
  // older pairs are folded into running sums and their events recycled (a T = 1000 callback chain makes 2001 launches).
  bool prof = false;
  struct EventLog {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending, spare;
    double ms = 0.0;
    long long n = 0;
    static constexpr size_t kWindow = 32;
    hipError_t fold(size_t keep) {
      while (pending.size() > keep) {
        float t = 0.f;
        hipError_t e = hipEventSynchronize(pending.front().second);
        if (e == hipSuccess) e = hipEventElapsedTime(&t, pending.front().first, pending.front().second);
        if (e != hipSuccess) return e;
        ms += t;
        ++n;
        spare.push_back(pending.front());
        pending.erase(pending.begin());
      }
      return hipSuccess;
    }
    hipError_t begin(hipStream_t st, std::pair<hipEvent_t, hipEvent_t>& ev) {
      hipError_t e = fold(kWindow - 1);
      if (e != hipSuccess) return e;
      if (!spare.empty()) {
        ev = spare.back();
        spare.pop_back();
      } else {
        if ((e = hipEventCreate(&ev.first)) != hipSuccess) return e;
        if ((e = hipEventCreate(&ev.second)) != hipSuccess) return e;
      }
      return hipEventRecord(ev.first, st);
    }
    hipError_t end(hipStream_t st, const std::pair<hipEvent_t, hipEvent_t>& ev) {
      pending.push_back(ev);
      return hipEventRecord(ev.second, st);
    }
    void reset(bool destroy) {
      for (auto& p : pending) spare.push_back(p);
      pending.clear();
      if (destroy) {
        for (auto& p : spare) {
          (void)hipEventDestroy(p.first);
          (void)hipEventDestroy(p.second);
        }
        spare.clear();
      }
      ms = 0.0;
      n = 0;
    }
  } prof_log, stab_log, atoms_log, rings_log, bonds_log, canon_log, fp_log, sub_log, huckel_log, ppp_log, ppp_cis_log, ppp_open_log, ppp_scf_log, kekule_log, ring_log, react_log;
  long long prof_steps = 0;
#ifdef GAUDI_STAMPS
  DevBuf d_stamps;
  unsigned long long stamp_acc[32] = {0};
#endif
};

#define HIPCHECK(h, call)                                                                         \
  do {                                                                                            \
    hipError_t e__ = (call);                                                                      \
    if (e__ != hipSuccess) {                                                                      \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e__);                              \
      return GAUDI_E_HIP;                                                                         \
    }                                                                                             \
  } while (0)

static int fail(gaudi_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}

// pred_train_host.inc (train_host.inc holds what it shares with edm_train_host.inc)
static void pt_release(gaudi_handle* h);
// edm_train_host.inc
static void et_release(gaudi_handle* h);
static int et_upload(gaudi_handle* h, const gaudi_edm_config* cfg, int n, const char* const* names, const float* const* tensors,
                     const int64_t* numel);
static const char* et_check(const gaudi_edm_config* cfg, int n, const char* const* names, const int64_t* numel);
extern const char* const kEdmStale;
static int pt_load(gaudi_handle* h, const gaudi_pred_config* cfg, int n, const char* const* names, const float* const* tensors,
                   const int64_t* numel);

// -------------------------------------------------------------------------------------------------
// noise schedule: PredefinedNoiseSchedule / polynomial_schedule / clip_noise_schedule
// (edm/equivariant_diffusion/en_diffusion.py:32-61, 191-218), float64 like the reference's numpy.
static std::vector<float> make_gamma(int T, double power, double precision) {
  const int steps = T + 1;
  if (power <= 0.0) {
    // the 'cosine' schedule (cosine_beta_schedule, en_diffusion.py:64-81; encoded as noise_power = 0): alphas_cumprod of
    // T + 2 points of cos^2, betas clipped to [0, 0.999]; no precision blend
    const int n = T + 2;
    const double s_ = 0.008, pi = 3.14159265358979323846;
    std::vector<double> ac(n);
    for (int i = 0; i < n; ++i) {
      const double x = (i == n - 1) ? (double)n : i * ((double)n / (double)(n - 1));  // np.linspace(0, n, n)
      const double c = std::cos(((x / n) + s_) / (1.0 + s_) * pi * 0.5);
      ac[i] = c * c;
    }
    const double a0 = ac[0];
    for (double& v : ac) v /= a0;
    std::vector<float> g(steps);
    double cum = 1.0;
    for (int i = 0; i < steps; ++i) {
      double beta = 1.0 - ac[i + 1] / ac[i];
      beta = std::min(std::max(beta, 0.0), 0.999);
      cum *= 1.0 - beta;
      g[i] = (float)(-(std::log(cum) - std::log(1.0 - cum)));
    }
    return g;
  }
  std::vector<double> a2(steps);
  const double step = (double)steps / (double)(steps - 1);  // np.linspace(0, steps, steps)
  for (int i = 0; i < steps; ++i) {
    double x = (i == steps - 1) ? (double)steps : i * step;
    double v = 1.0 - std::pow(x / steps, power);
    a2[i] = v * v;
  }
  // clip_noise_schedule: ratios alpha2[i]/alpha2[i-1] clipped to [1e-3, 1], cumulative product
  std::vector<double> out(steps);
  double prev = 1.0, cum = 1.0;
  for (int i = 0; i < steps; ++i) {
    double r = a2[i] / prev;
    r = std::min(std::max(r, 0.001), 1.0);
    cum *= r;
    out[i] = cum;
    prev = a2[i];
  }
  std::vector<float> g(steps);
  const double pr = 1.0 - 2.0 * precision;
  for (int i = 0; i < steps; ++i) {
    double a = pr * out[i] + precision;
    g[i] = (float)(-(std::log(a) - std::log(1.0 - a)));
  }
  return g;
}

static inline float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }
static inline float logsigmoid_f(float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }
static inline float sigmoid_host(float x) { return 1.0f / (1.0f + expf(-x)); }

// en_diffusion.py:433-457 (sigma_and_alpha_t_given_s), :365-373 (sigma), :843-849 (mu / sigma of p(z_s|z_t))
// one row for the step from time index t_idx down to s_idx (any pair s_idx < t_idx, as the reference's functions take)
static void coef_row(const std::vector<float>& g, int T, int s_idx, int t_idx, float* row) {
  const float gs = g[s_idx], gt = g[t_idx];
  const float sigma2 = -expm1f(softplus_f(gs) - softplus_f(gt));
  const float alpha_ts = expf(0.5f * (logsigmoid_f(-gt) - logsigmoid_f(-gs)));
  const float sigma_ts = sqrtf(sigma2);
  const float sigma_s = sqrtf(sigmoid_host(gs)), sigma_t = sqrtf(sigmoid_host(gt));
  row[0] = alpha_ts;
  row[1] = sigma2 / alpha_ts / sigma_t;
  row[2] = sigma_ts * sigma_s / sigma_t;
  row[3] = (float)t_idx / (float)T;
}
static void make_coef(const std::vector<float>& g, int T, std::vector<float>& coef) {
  coef.resize((size_t)T * 4);
  for (int s = 0; s < T; ++s) coef_row(g, T, s, s + 1, &coef[4 * s]);
}

// A chain on a time grid g[0] > g[1] > ... > g[n] = 0 (gaudi_sample_grid): the per-call step table.  Row r belongs to the step
// that LANDS on idx[r], rows ascending in time like the unit-stride table (row s lands on s), so the kernels walk it downwards
// exactly as they walk that one; the unit grid gives that table bit for bit.
struct GridPlan {
  int rows = 0;
  int t0 = 0;  // g[0]: the time index the chain starts at
  std::vector<float> coef;     // [rows][4]
  std::vector<int32_t> idx;    // [rows]
};
static const char* grid_check(int T, int n_grid, const int32_t* grid) {
  if (n_grid < 2 || !grid) return "a time grid needs at least two entries";
  if (grid[0] > T) return "the time grid exceeds T";
  if (grid[n_grid - 1] != 0) return "the time grid must end in 0";
  for (int k = 0; k + 1 < n_grid; ++k)
    if (grid[k + 1] >= grid[k]) return "the time grid must be strictly descending";
  return nullptr;
}
static void make_grid_plan(const std::vector<float>& g, int T, int n_grid, const int32_t* grid, GridPlan& gp) {
  gp.rows = n_grid - 1;
  gp.t0 = grid[0];
  gp.coef.resize((size_t)gp.rows * 4);
  gp.idx.resize(gp.rows);
  for (int r = 0; r < gp.rows; ++r) {
    const int k = gp.rows - 1 - r;  // step k of the chain: g[k] -> g[k + 1]
    coef_row(g, T, grid[k + 1], grid[k], &gp.coef[4 * r]);
    gp.idx[r] = grid[k + 1];
  }
}

// -------------------------------------------------------------------------------------------------
// checkpoint packing
struct Tensors {
  std::map<std::string, std::pair<const float*, int64_t>> m;
  std::string missing;
  const float* get(const std::string& k, int64_t numel) {
    auto it = m.find(k);
    if (it == m.end() || it->second.second != numel) {
      if (missing.empty())
        missing = k + (it == m.end() ? " (absent)" : " (numel " + std::to_string(it->second.second) + " != " +
                                                         std::to_string(numel) + ")");
      return nullptr;
    }
    return it->second.first;
  }
  // the tensor if it is there with that size (no complaint: get() of the same tensor reports what is wrong)
  const float* peek(const std::string& k, int64_t numel) const {
    auto it = m.find(k);
    return it == m.end() || it->second.second != numel ? nullptr : it->second.first;
  }
};

// Packing context of one checkpoint load (a value passed down -- no file-scope state: two handles may load concurrently).
//   lane_linear (8-wave kernels): inside a 16x16 tile float4 index L = (k%16/4)*16 + o%16 holds W[o][k .. k+3], i.e. lane L
//     of a wave reads the 16 bytes at offset 16 L whether the tile comes from L2 or from the LDS weight ring; otherwise the
//     tile is row-major (4-wave kernels)
//   ktail (8-wave kernels, H % 16 == 4): the last K chunk carries its 4 valid inputs on element 0 of the four lane groups
//   wbase / ws: when a split buffer is being filled, the fp32 buffer's base and the split image (w8_split.h) whose float
//     offsets are twice the fp32 ones
struct PackMode {
  bool lane_linear = false;
  bool ktail = false;
  float* wbase = nullptr;
  std::vector<float>* ws = nullptr;
  float hscale = 0.f;   // 2^s of the network's fp16-pair node images (w8_nodes_f16.h); 0: no such images
  bool hktail = false;  // ... their K tail (H % 16 == 4)
  PackMode with_ktail(bool kt) const {
    PackMode m = *this;
    m.ktail = kt;
    return m;
  }
};
static bool has_ktail(int H, int HP) { return HP - H == 12; }
// W[o][col0 + k] (row stride ldw), o,k < H  ->  tile-packed [HP/16][HP/16][16][16]: dst[((k/16*T + o/16)*16 + o%16)*16 + k%16]
static void pack_matrix(const PackMode& pm, float* dst, const float* W, int H, int ldw, int col0, int HP, bool transpose = false) {
  const int T = HP / 16;
  for (int o = 0; o < H; ++o)
    for (int k = 0; k < H; ++k) {
      const float v = transpose ? W[(size_t)k * ldw + col0 + o] : W[(size_t)o * ldw + col0 + k];
      const size_t tile = ((size_t)(k / 16) * T + o / 16) * 256;
      size_t in = pm.lane_linear ? (size_t)(((k % 16) / 4) * 16 + o % 16) * 4 + k % 4 : (size_t)(o % 16) * 16 + k % 16;
      if (pm.lane_linear && pm.ktail && k / 16 == T - 1) in = (size_t)((k % 16) * 16 + o % 16) * 4;  // k % 16 < 4 here
      dst[tile + in] = v;
    }
}
// fp16 helpers of the weight images (round to nearest even; NaN stays NaN)
static uint16_t f16_bits(float x) {
  const _Float16 hv = (_Float16)x;
  uint16_t u;
  std::memcpy(&u, &hv, 2);
  return u;
}
static float f16_value(uint16_t b) {
  _Float16 hv;
  std::memcpy(&hv, &b, 2);
  return (float)hv;
}
// Split image of an edge-GEMM matrix (w8_split.h, round 5: fp16 pairs): units of 1 KiB ordered [K chunk m][output tile t][piece p];
// lane L = (row L & 15, group g = L >> 4) holds 8 fp16: slots 0-3 = inputs 16(2m) + 4g .. +3, slots 4-7 = inputs 16(2m+1) + 4g .. +3.
// Pieces of w s (s = the network's power-of-two scale, NodeScale below): hi = fp16(w s), lo = fp16(w s - hi), both round-to-
// nearest-even; a NaN weight gives NaN pieces (the product is NaN like the fp32 product), infinite weights are refused by
// NodeScale.  K tail (pm.ktail, odd tile count >= 3 = SplitGeo::kTailOK): the last chunk holds only the tail tile; it is stored
// as T fp32 tiles in pack_matrix's K-tail form, scaled by s (the accumulators run in scaled units), and issued as one fp32
// k-step per tile.
static void pack_matrix_split(const PackMode& pm, float* dst, const float* W, int H, int ldw, int col0, int HP, bool transpose) {
  const int T = HP / 16;
  const bool tail = pm.ktail && (T & 1) && T >= 3;
  const float sc = pm.hscale > 0.f ? pm.hscale : 1.0f;
  uint16_t* d = (uint16_t*)dst;
  for (int o = 0; o < H; ++o)
    for (int k = 0; k < H; ++k) {
      const float v = (transpose ? W[(size_t)k * ldw + col0 + o] : W[(size_t)o * ldw + col0 + k]) * sc;
      const int tile = k / 16, m = tile / 2, g = (k % 16) / 4, e = 4 * (tile & 1) + (k & 3), t = o / 16, L = g * 16 + o % 16;
      if (tail && tile == T - 1) {  // k % 16 < 4 here
        dst[(size_t)(m * T * w8::kPieces + t) * 256 + (size_t)((k % 16) * 16 + o % 16) * 4] = v;
        continue;
      }
      const uint16_t hi = f16_bits(v);
      d[((size_t)((m * T + t) * w8::kPieces + 0) * 64 + L) * 8 + e] = hi;
      d[((size_t)((m * T + t) * w8::kPieces + 1) * 64 + L) * 8 + e] = f16_bits(v - f16_value(hi));
    }
}
// An edge-GEMM matrix: the fp32 tiles (K tail included where the width has one) and, when a split buffer is being filled,
// its split image at twice the float offset
static void pack_edge_matrix(const PackMode& pm, float* dst, const float* W, int H, int ldw, int col0, int HP, bool transpose = false) {
  pack_matrix(pm, dst, W, H, ldw, col0, HP, transpose);
  if (pm.ws != nullptr) pack_matrix_split(pm, pm.ws->data() + 2 * (size_t)(dst - pm.wbase), W, H, ldw, col0, HP, transpose);
}
// fp16-pair image of a node-GEMM matrix (w8_nodes_f16.h): w 2^s = hi + lo 2^-11 with hi = fp16(w 2^s), lo = fp16((w 2^s - hi) 2^11), both
// round-to-nearest-even (NaN stays NaN; the host refuses infinite weights, node_scale below).  Units of 1 KiB ordered
// [K chunk m of 32 inputs][output tile t][piece]; lane L = (row L & 15, group g = L >> 4) holds inputs 32 m + 8 g .. +7.
// An odd tile count leaves a last half chunk of 16 inputs: a trailing block of T x 256 floats, UNSCALED fp32, [tile][k-step q]
// [lane (row, g)] = W[row][16 (T-1) + 4 q + g]: v_mfma_f32_16x16x4_f32 steps (one of them when H % 16 == 4).
static void pack_matrix_f16(float* dst, const float* W, int H, int ldw, int col0, int HP, bool transpose, float scale) {
  const int T = HP / 16;
  uint16_t* d = (uint16_t*)dst;
  for (int o = 0; o < H; ++o)
    for (int k = 0; k < H; ++k) {
      const float v = transpose ? W[(size_t)k * ldw + col0 + o] : W[(size_t)o * ldw + col0 + k];
      const int t = o / 16, i = o % 16;
      if (w8::nh_odd(HP) && k >= 16 * (T - 1)) {  // the last half chunk: fp32, unscaled, [tile][k-step q][lane (row, g)]
        const int kk = k - 16 * (T - 1);
        dst[(size_t)w8::nh_tail_off(HP) + t * 256 + (kk / 4) * 64 + (kk % 4) * 16 + i] = v;
        continue;
      }
      const int m = k / 32, L = ((k % 32) / 8) * 16 + i, e = k % 8;
      const float vs = v * scale;
      const uint16_t hi = f16_bits(vs);
      const uint16_t lo = f16_bits((vs - f16_value(hi)) * 2048.f);
      d[(((size_t)(m * T + t) * 2 + 0) * 64 + L) * 8 + e] = hi;
      d[(((size_t)(m * T + t) * 2 + 1) * 64 + L) * 8 + e] = lo;
    }
}
// One power of two for all matrices of a network (node-level AND edge-level: w8_nodes_f16.h, w8_split.h): the largest finite
// |w| lands in [2^13, 2^14).  An entry keeps 22 significant bits down to 2^-17 of the largest one in the edge images (lo shares
// hi's exponent range: one accumulator) and down to 2^-25 in the node images (lo carries its own exponent), with fp16's
// absolute floor below that.  The form is refused -- the call then runs the fp32-instruction kernels, and the load says so
// (gaudi_last_warning) -- when a matrix holds an infinity (fp16 pieces would turn inf x 0 and inf - inf into NaN where the fp32
// product keeps inf) or when a whole matrix lies below those floors.
struct NodeScale {
  // node-level and edge-level matrices apart: the node images carry an entry with 22 bits down to 2^-25 of the scale's top (lo has
  // its own exponent), the edge images down to 2^-17 (lo shares hi's range)
  float gmax = 0.f, min_node = INFINITY, min_edge = INFINITY;
  bool inf = false;
  void see(const float* W, int rows, int ldw, int col0, int cols, bool edge = false) {
    if (!W) return;
    float m = 0.f;
    for (int o = 0; o < rows; ++o)
      for (int k = 0; k < cols; ++k) {
        const float a = std::fabs(W[(size_t)o * ldw + col0 + k]);
        if (std::isinf(a)) inf = true;
        else if (a == a) m = std::max(m, a);
      }
    gmax = std::max(gmax, m);
    if (m > 0.f) (edge ? min_edge : min_node) = std::min(edge ? min_edge : min_node, m);
  }
  // Round 6: the rule is as narrow as the images allow.  Through round 5 ANY matrix 2^12 below the network's
  // largest entry refused the set (one small matrix: the whole network at 0.55 x the speed, silently).  Now: an edge matrix may lie
  // 2^17 below (its largest entries then still carry 21-22 bits, its error stays at 2^-22 of ITS largest entry -- the norm a GEMM's
  // error is measured in), a node matrix 2^25; and the refusal is loud (gaudi_last_warning).  One exponent per MATRIX instead was
  // built and measured: parity-green, 1.0-1.5 % slower on the headline in three forms (profiles/r06c_per_matrix_scale_ab.txt,
  // tools/experiments/per_matrix_scale.patch).
  bool too_small() const { return min_edge < gmax * 7.62939453125e-6f /* 2^-17 */ || min_node < gmax * 2.98023223876953125e-8f /* 2^-25 */; }
  // -> 2^s (0: refused; why() says which rule)
  float scale() const {
    if (inf || !(gmax > 0.f) || too_small()) return 0.f;
    int ex;
    std::frexp(gmax, &ex);  // gmax = f 2^ex, f in [0.5, 1)
    if (14 - ex > 126 || 14 - ex < -126) return 0.f;  // (the scale and its inverse must be normal numbers: |w| around 2^-112 .. 2^140)
    return std::ldexp(1.f, 14 - ex);
  }
  const char* why() const {
    if (inf) return "a weight matrix holds an infinity";
    if (!(gmax > 0.f)) return "every weight matrix is zero or NaN";
    if (too_small())
      return "the largest entry of some weight matrix lies more than 2^17 (edge-level matrices; 2^25: node-level) below the largest entry of the network";
    return "the largest weight is outside 2^-112 .. 2^140";
  }
};
// A node-GEMM matrix: the fp32 tiles and, when the split buffer is being filled and the network's scale is known, its fp16-pair
// image at twice the float offset (the split buffer's slots of the node matrices)
static void pack_node_matrix(const PackMode& pm, float* dst, const float* W, int H, int ldw, int col0, int HP, bool transpose = false) {
  pack_matrix(pm, dst, W, H, ldw, col0, HP, transpose);
  if (pm.ws != nullptr && pm.hscale > 0.f)
    pack_matrix_f16(pm.ws->data() + 2 * (size_t)(dst - pm.wbase), W, H, ldw, col0, HP, transpose, pm.hscale);
}
static void pack_vec(float* dst, const float* v, int n) { std::memcpy(dst, v, sizeof(float) * n); }
static void pack_col(float* dst, const float* W, int H, int ldw, int col) {
  for (int o = 0; o < H; ++o) dst[o] = W[(size_t)o * ldw + col];
}
// max |W[o][col]| over the rows (NaN if any entry is: the bound it enters must not hide one)
static float col_absmax(const float* W, int H, int ldw, int col) {
  float m = 0.f;
  bool nan = false;
  for (int o = 0; o < H; ++o) {
    const float a = std::fabs(W[(size_t)o * ldw + col]);
    nan |= a != a;
    m = std::max(m, a);
  }
  return nan ? NAN : m;
}

// -------------------------------------------------------------------------------------------------
// graph metadata: live edges of each molecule, receiving nodes dealt to the 4 waves (LPT), each
// wave's edge list sorted by receiving node and padded to 32 ("bucketed by degree").
struct Meta {
  int EW = 32;
  std::vector<int> order, npairs, ncols;
  std::vector<uint32_t> edges, seg;
  std::vector<float> emask;
};

static int build_meta(int B, int N, const float* node_mask, const float* edge_mask, Meta& M, std::string& err) {
  if (N > 255) {
    err = "N > 255 unsupported";
    return GAUDI_E_CAPACITY;
  }
  struct Mol {
    std::vector<std::vector<std::pair<int, float>>> nbr;  // per receiving node: (j, mask)
    int owner[256];
    int total = 0;
  };
  std::vector<Mol> mols(B);
  M.ncols.assign(B, 1);
  int maxlen = 0;
  std::vector<std::vector<int>> wl(B * kWaves);
  for (int b = 0; b < B; ++b) {
    Mol& m = mols[b];
    m.nbr.resize(N);
    // Edges between two MASKED nodes are dropped: the reference leaves the identity block "padded ring <-> its
    // orientation node" unmasked (sampling_edm.py:147-159), but a masked node's features are multiplied by node_mask = 0
    // after every layer and its outputs are masked, and no live node has an edge to it, so those messages reach nothing.
    // ncols = 1 + the last node that is live or has a live edge: node-level GEMMs stop there (hetero batches padded to
    // 20 nodes: molecules of up to 6 rings need one 16-node column tile instead of two).
    int last = 0;
    for (int i = 0; i < N; ++i) {
      const bool li = node_mask == nullptr || node_mask[(size_t)b * N + i] != 0.f;
      if (li) last = i;
      for (int j = 0; j < N; ++j) {
        const float v = edge_mask[((size_t)b * N + i) * N + j];
        const bool lj = node_mask == nullptr || node_mask[(size_t)b * N + j] != 0.f;
        if (v != 0.f && (li || lj)) {
          m.nbr[i].push_back({j, v});
          ++m.total;
          last = std::max(last, std::max(i, j));
        }
      }
    }
    M.ncols[b] = last + 1;
    // longest-processing-time assignment of receiving nodes to waves
    std::vector<int> idx(N);
    for (int i = 0; i < N; ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int c) { return m.nbr[a].size() > m.nbr[c].size(); });
    int load[kWaves] = {0, 0, 0, 0};
    for (int i : idx) {
      int w = 0;
      for (int k = 1; k < kWaves; ++k)
        if (load[k] < load[w]) w = k;
      m.owner[i] = w;
      load[w] += (int)m.nbr[i].size();
    }
    for (int w = 0; w < kWaves; ++w) maxlen = std::max(maxlen, load[w]);
  }
  M.EW = std::max(32, (maxlen + 31) / 32 * 32);
  if (M.EW > 0x7fff) {
    err = "too many edges per wave";
    return GAUDI_E_CAPACITY;
  }
  const int EW = M.EW;
  M.edges.assign((size_t)B * kWaves * EW, 0);
  M.emask.assign((size_t)B * kWaves * EW, 0.f);
  M.npairs.assign((size_t)B * kWaves, 0);
  M.seg.assign((size_t)B * N, 0);
  for (int b = 0; b < B; ++b) {
    Mol& m = mols[b];
    int fill[kWaves] = {0, 0, 0, 0};
    int last_i[kWaves] = {0, 0, 0, 0};
    for (int i = 0; i < N; ++i) {
      const int w = m.owner[i];
      const int st = fill[w];
      for (auto& e : m.nbr[i]) {
        const size_t s = ((size_t)b * kWaves + w) * EW + fill[w]++;
        M.edges[s] = (uint32_t)i | ((uint32_t)e.first << 8);
        M.emask[s] = e.second;
      }
      if (!m.nbr[i].empty()) last_i[w] = i;
      M.seg[(size_t)b * N + i] = ((uint32_t)w << 30) | ((uint32_t)st << 15) | (uint32_t)m.nbr[i].size();
    }
    for (int w = 0; w < kWaves; ++w) {
      const int padded = (fill[w] + 31) / 32 * 32;
      for (int s = fill[w]; s < padded; ++s)  // padding slots: same receiving node, mask 0
        M.edges[((size_t)b * kWaves + w) * EW + s] = (uint32_t)last_i[w] | ((uint32_t)last_i[w] << 8);
      M.npairs[(size_t)b * kWaves + w] = padded / 32;
    }
  }
  M.order.resize(B);
  for (int b = 0; b < B; ++b) M.order[b] = b;
  std::stable_sort(M.order.begin(), M.order.end(), [&](int a, int c) { return mols[a].total > mols[c].total; });
  (void)node_mask;
  return GAUDI_OK;
}

// -------------------------------------------------------------------------------------------------
// graph metadata of the 8-wave kernels: ONE flat slot list per molecule -- live edges sorted by receiving node (then by
// sending node), cut into 16-slot tiles (tile tau -> wave tau & 7, round tau >> 3).  A node's run may straddle two tiles but
// never three (a run that would is moved to the next tile boundary), so its edge -> node sum has at most two partials.
struct Meta8 {
  int S = 16;
  std::vector<int> order, ntiles, ncols;
  std::vector<uint32_t> edges, seg;
  std::vector<float> emask;
  std::vector<uint16_t> soff, sidx;
};

// align: [B][N] flags or nullptr -- a node whose flag is set starts its edge run at a tile boundary (packed launches: the
// first node of every component, so that a molecule's tiles are the ones it has on its own)
static int build_meta8(int B, int N, const float* node_mask, const float* edge_mask, Meta8& M, std::string& err,
                       int min_slots = 0, const uint8_t* align = nullptr) {
  if (N > 255) {
    err = "N > 255 unsupported";
    return GAUDI_E_CAPACITY;
  }
  struct Slot {
    int i, j;
    float m;
    bool live;
  };
  std::vector<std::vector<Slot>> slots(B);
  std::vector<std::vector<std::pair<int, int>>> runs(B);  // per node: (first slot, length)
  M.ncols.assign(B, 1);
  M.ntiles.assign(B, 0);
  std::vector<int> total(B, 0);
  int max_tiles = 1;
  for (int b = 0; b < B; ++b) {
    std::vector<Slot>& sl = slots[b];
    runs[b].assign(N, {0, 0});
    int last = 0;
    bool want_align = false;
    for (int i = 0; i < N; ++i) {
      const bool li = node_mask == nullptr || node_mask[(size_t)b * N + i] != 0.f;
      if (li) last = i;
      std::vector<Slot> run;
      for (int j = 0; j < N; ++j) {
        const float v = edge_mask[((size_t)b * N + i) * N + j];
        const bool lj = node_mask == nullptr || node_mask[(size_t)b * N + j] != 0.f;
        if (v != 0.f && (li || lj)) {  // edges between two masked nodes reach nothing (see build_meta)
          run.push_back({i, j, v, true});
          last = std::max(last, std::max(i, j));
        }
      }
      const int L = (int)run.size();
      if (align != nullptr && align[(size_t)b * N + i]) want_align = true;  // (kept pending over nodes without a run)
      if (L == 0) {
        runs[b][i] = {(int)sl.size(), 0};
        continue;
      }
      if (L > 32) {
        err = "a node with more than 32 live edges is not supported by the 8-wave kernels";
        return GAUDI_E_CAPACITY;
      }
      if (want_align && !sl.empty()) {  // first run of a component: start a new tile
        const int prev_i = sl.back().i;
        while (sl.size() % 16) sl.push_back({prev_i, prev_i, 0.f, false});
      }
      want_align = false;
      const int o = (int)sl.size() % 16;
      if ((o + L + 15) / 16 > 2) {  // would straddle three tiles: start at the next tile boundary
        const int prev_i = sl.empty() ? i : sl.back().i;
        while (sl.size() % 16) sl.push_back({prev_i, prev_i, 0.f, false});
      }
      runs[b][i] = {(int)sl.size(), L};
      sl.insert(sl.end(), run.begin(), run.end());
      total[b] += L;
    }
    if (!sl.empty()) {
      const int prev_i = sl.back().i;
      while (sl.size() % 16) sl.push_back({prev_i, prev_i, 0.f, false});
    }
    M.ncols[b] = last + 1;
    M.ntiles[b] = (int)sl.size() / 16;
    max_tiles = std::max(max_tiles, M.ntiles[b]);
  }
  M.S = std::max(16 * max_tiles, (min_slots + 15) / 16 * 16);  // min_slots: plan hint (slot capacity of the whole logical batch)
  if (M.S > 0xffff) {
    err = "too many edge slots";
    return GAUDI_E_CAPACITY;
  }
  const int S = M.S;
  M.edges.assign((size_t)B * S, 0);
  M.emask.assign((size_t)B * S, 0.f);
  M.seg.assign((size_t)B * N, 0);
  M.soff.assign((size_t)B * (N + 1), 0);
  M.sidx.assign((size_t)B * S, 0);
  for (int b = 0; b < B; ++b) {
    const std::vector<Slot>& sl = slots[b];
    const int ns = (int)sl.size();
    for (int t0 = 0; t0 < ns; t0 += 16) {
      int c = 0;
      while (c < 16) {  // segments of equal receiving node inside the tile (padding extends the segment before it)
        int e = c;
        while (e + 1 < 16 && sl[t0 + e + 1].i == sl[t0 + c].i) ++e;
        const int i = sl[t0 + c].i;
        const int part = runs[b][i].second > 0 && runs[b][i].first < t0 ? 1 : 0;  // the node's run began in an earlier tile
        for (int k = c; k <= e; ++k) {
          const Slot& q = sl[t0 + k];
          M.edges[(size_t)b * S + t0 + k] = (uint32_t)q.i | ((uint32_t)q.j << 8) | ((uint32_t)c << 16) |
                                            ((uint32_t)(k == e) << 20) | ((uint32_t)part << 21);
          M.emask[(size_t)b * S + t0 + k] = q.m;
        }
        c = e + 1;
      }
    }
    for (int i = 0; i < N; ++i)
      M.seg[(size_t)b * N + i] = ((uint32_t)runs[b][i].first << 16) | (uint32_t)runs[b][i].second;
    // slots by SENDING node, ascending slot (= ascending receiving node): the transposed sums of the reverse pass
    uint16_t* off = &M.soff[(size_t)b * (N + 1)];
    uint16_t* idx = &M.sidx[(size_t)b * S];
    int n_out = 0;
    for (int j = 0; j < N; ++j) {
      off[j] = (uint16_t)n_out;
      for (int k = 0; k < ns; ++k)
        if (sl[k].live && sl[k].j == j) idx[n_out++] = (uint16_t)k;
    }
    off[N] = (uint16_t)n_out;
  }
  M.order.resize(B);
  for (int b = 0; b < B; ++b) M.order[b] = b;
  std::stable_sort(M.order.begin(), M.order.end(), [&](int a, int c) {
    return M.ntiles[a] != M.ntiles[c] ? M.ntiles[a] > M.ntiles[c] : total[a] > total[c];
  });
  return GAUDI_OK;
}

// -------------------------------------------------------------------------------------------------
// kernel table: the instantiations live in kern*_*.hip (compiled in parallel); each registers its entries here at load time
// (kernel_table.h).  A build that links fewer of them (tools/build_stamped.sh, tools/build_variant.sh) finds fewer kernels.
KernelTable* gaudi::g_kernel_tables;

static const KernelEntry* find_entry(const KernelKey& k) {
  for (const KernelTable* t = g_kernel_tables; t; t = t->next)
    for (int i = 0; i < t->n; ++i)
      if (t->entries[i].key == k) return &t->entries[i];
  return nullptr;
}
static kernel_fn find_kernel(const KernelKey& k) {
  const KernelEntry* e = find_entry(k);
  return e ? e->fn : nullptr;
}
static std::string key_name(const KernelKey& k) {
  char buf[160];
  snprintf(buf, sizeof buf, "waves=%d SP=%d MR=%d GN=%d FR=%d PG=%d N1=%d EF=%d HPE=%d HPP=%d VT=%d", k.waves, k.sp, (int)k.mr, k.gn,
           (int)k.fr, (int)k.pg, (int)k.n1, k.ef, k.hpe, k.hpp, (int)k.vt);
  return buf;
}
// two translation units registering one key is a build mistake: the first such key by name, or "" (gaudi_create)
static std::string duplicate_kernel_key() {
  std::vector<KernelKey> seen;
  for (const KernelTable* t = g_kernel_tables; t; t = t->next)
    for (int i = 0; i < t->n; ++i) {
      if (std::find(seen.begin(), seen.end(), t->entries[i].key) != seen.end()) return key_name(t->entries[i].key);
      seen.push_back(t->entries[i].key);
    }
  return "";
}
// the template argument GN of a residency (sampler_kernel.h: V4T / V8T)
static int gn_of(NodeBuf nodes) { return nodes == kAllGlobal ? 1 : nodes == kPqLds ? 2 : 0; }
// 4-wave kernels: node buffers resident or in global memory (V4G: molecules beyond the LDS limit), ef = 24 for a sin_embedding
// denoiser.  There is no fused (EDM + predictor) V4G instantiation: at the default widths it sits on the register cliff (512
// registers, 1120 spilled scalars) and faulted; a guided step of a large molecule is two launches, EDM-only then predictor-only
static KernelKey key4(int hpe, int hpp, bool gn = false, int ef = 2) {
  KernelKey k{};  // (fields by name: a reordered KernelKey must not change what is looked up)
  k.waves = 4;
  k.gn = gn ? 1 : 0;
  k.ef = ef;
  k.hpe = hpe;
  k.hpp = hpp;
  return k;
}
// 8-wave kernels: ring = 0 fp32 instructions, 1 / 2 split operands (fp16 pairs) on the full / half weight ring; mr: the call holds a
// graph of more than one round of edge tiles AND runs the predictor; V8G (kAllGlobal, kPqLds) and the wide-group kernel on the full
// ring (kPredFifthGlobal) exist as ring = 1, mr = true only
static KernelKey key8(int hpe, int hpp, int ring, bool mr, NodeBuf nodes = kResident) {
  KernelKey k{};
  k.waves = 8;
  k.sp = ring;
  k.mr = mr;
  k.gn = gn_of(nodes);
  k.pg = nodes == kPredFifthGlobal;
  k.ef = 2;
  k.hpe = hpe;
  k.hpp = hpp;
  return k;
}
static bool have_kernel8(int hpe, int hpp, int ring, bool mr, NodeBuf nodes = kResident) {
  return find_kernel(key8(hpe, hpp, ring, mr, nodes)) != nullptr;
}
// node buffers of ONE launch of a call: the wide-group form is the fused kernel's; the call's other launches are resident
static NodeBuf launch_nodes(const LaunchPlan& p, int hpe, int hpp) {
  return p.nodes == kPredFifthGlobal && !(hpe && hpp) ? kResident : p.nodes;
}
// The kernel of a launch of the networks (hpe, hpp) under a plan.  MR applies to launches that run the predictor; a value-target
// launch (vt) runs the VT instantiation of its kernel, which exists for launches with a predictor; the predictor-only launches of
// a sin_embedding handle (no sin_embedding there) take the ordinary kernels.
// key: the key of the kernel returned (what gaudi_last_kernel_key names).
static kernel_fn plan_kernel(const LaunchPlan& p, int hpe, int hpp, bool vt, KernelKey* key = nullptr) {
  KernelKey unused;
  KernelKey& k = key ? *key : unused;
  if (p.waves != 8) {
    k = key4(hpe, hpp, p.nodes == kAllGlobal, hpe ? p.ef : 2);
    k.vt = vt && hpp;
    return find_kernel(k);
  }
  const NodeBuf nodes = launch_nodes(p, hpe, hpp);
  const bool mr = p.mr && hpp;
  k = nodes == kResident ? key8(hpe, hpp, p.ring, mr) : key8(hpe, hpp, 1, true, nodes);
  k.vt = vt && hpp;
  // two column tiles per node GEMM on the resident full-ring kernel: its FR instantiation (same arithmetic, same results).
  // (a kPredFifthGlobal plan is an mr plan: its fused launch never comes here)
  if (p.fr && nodes == kResident && !mr) {
    k.fr = true;
    if (kernel_fn f = find_kernel(k)) return f;
    k.fr = false;
  }
  // at most 16 node slots there: its N1 instantiation (one column tile per node GEMM compiled in; same arithmetic, same results)
  if (p.n1 && nodes == kResident && !mr) {
    k.n1 = true;
    if (kernel_fn f = find_kernel(k)) return f;
    k.n1 = false;
  }
  return find_kernel(k);
}

// smallest instantiated padded hidden size >= H (0 if none)
static int round_hidden(int H) {
  static const int sizes[] = {32, 48, 64, 128, 192, 208, 256};
  for (int s : sizes)
    if (s >= H) return s;
  return 0;
}

// gn: node buffers in global memory (V4G kernels)
// edge slots per wave of the 4-wave kernels for the fully connected graph of N nodes (build_meta: whole receiving nodes are
// dealt to the waves, the longest list rounded up to 32)
static int dense_ew4(int N) { return std::max(32, ((N + kWaves - 1) / kWaves * (N - 1) + 31) / 32 * 32); }

// ef: edge features of the denoiser's first Linears (2, or 24 for sin_embedding: edm_device.h, NetSmem)
static size_t lds_bytes(int hpe, int hpp, int N, int D, int EW, bool gn = false, int ef = 2) {
  size_t net = 0;
  if (hpe)
    net = std::max(net, (size_t)((gn ? 0 : 4 * N * (hpe + 4)) + kWaves * 16 * (hpe + 4) + 8 * N + kWaves * EW * 9 + (6 + ef) * hpe +
                                 (ef > 2 ? kWaves * EW * ef : 0)));
  if (hpp) net = std::max(net, (size_t)((gn ? 0 : 5 * N * (hpp + 4)) + kWaves * 16 * (hpp + 4) + 12 * N + kWaves * EW * 10 + 32 + 10 * hpp));
  return sizeof(float) * (common_floats(N, D, EW) + net);
}
static size_t gnode_floats(int hpe, int hpp, int N) {
  return std::max((size_t)(hpe ? 4 * N * (hpe + 4) : 0), (size_t)(hpp ? 5 * N * (hpp + 4) : 0));
}

// nodes: kAllGlobal / kPqLds keep w8_edm.h: gn_lds_buffers node buffers in LDS; kPredFifthGlobal is the resident plan with four
// predictor buffers (w8_pred.h: PredSmem, PG)
static size_t lds_floats8_base(int hpe, int hpp, int N, int D, int S, int split, NodeBuf nodes = kResident) {
  size_t net = 0;
  const int pbuf = nodes == kPredFifthGlobal ? 4 : 5;
  const int gn = gn_of(nodes);
  if (hpe) net = std::max(net, (size_t)((gn ? w8::gn_lds_buffers(gn) : 5) * N * (hpe + 4) + w8::edge_ring_floats(hpe, split) + 8 * N + 2 * align4(N) + 96 + S * 9 + 8 * hpe));
  if (hpp) net = std::max(net, (size_t)(w8::edge_ring_floats(hpp, split) + (gn ? w8::gn_lds_buffers(gn) : pbuf) * N * (hpp + 4) + 12 * N + 2 * align4(N) + 96 + S * 10 + 32 + 10 * hpp));
  return common_floats8(N, D, S) + net;
}
static size_t gnode_floats8(int hpe, int hpp, int N) {
  return std::max((size_t)(hpe ? 5 * N * (hpe + 4) : 0), (size_t)(hpp ? 5 * N * (hpp + 4) : 0));
}
// V8G stages up to two node buffers in the idle weight ring before each node GEMM (w8_common.h: stage_rows)
static bool gn8_stage_fits(int hpe, int hpp, int N) {
  for (int hp : {hpe, hpp})
    if (hp && 2 * (size_t)w8::stage_stride(N * (hp + 4)) > w8::edge_ring_floats(hp, 1)) return false;
  return true;
}
// The reverse pass publishes du of every slot pub_ch feature tiles at a time into [b0 | b1 | pubx extra floats]: pick the
// largest pub_ch that fits 160 KiB, then the extra floats that choice needs.  false: the molecule does not fit.
// fp16-pair node GEMMs (every split-operand kernel): the split copy of ONE GEMM input must fit the region the kernels use -- the
// ring's free slot (full ring), the whole ring where it idles across node phases (half ring, gn) -- for N node columns
static bool node_f16_fits(int hp, int N, int split, NodeBuf nodes) {
  const bool gn = gn_of(nodes) != 0;
  if (!hp || !split || !GAUDI_NODE_F16) return true;
  if (N > (gn ? 48 : 32)) return false;  // column tiles of one pass: three in the gn kernels, two in the resident ones
  const int nct = N <= 16 ? 1 : N <= 32 ? 2 : 3;
  const int ring = w8::edge_ring_floats(hp, split);
  return w8::nh_split_floats(hp, nct) <= (w8::node_ring_idle(hp, split, gn) ? ring : ring / 2);
}
static bool plan_pub8(int hpe, int hpp, int N, int D, int S, int split, int& pubx, int& pub_ch, NodeBuf nodes = kResident) {
  pubx = 0;
  pub_ch = 0;
  const int gn = gn_of(nodes);  // (kPredFifthGlobal: the resident kernels' planning with four predictor buffers in LDS)
  if (!node_f16_fits(hpe, N, split, nodes) || !node_f16_fits(hpp, N, split, nodes)) return false;
  const long long cap = 160 * 1024 / 4 - 64;  // floats (a little headroom for the runtime's own static LDS)
  const long long base = (long long)lds_floats8_base(hpe, hpp, N, D, S, split, nodes);
  if (base > cap) return false;
  if (!hpp) return true;
  const int T = hpp / 16;
  // b0 + b1 double as the head of the publish buffer; with the split edge GEMMs the (then idle) weight ring follows them
  // (V8G: b0 / b1 are in global memory, the buffer is the ring and what follows it)
  const long long own = (gn ? 0LL : 2LL * N * (hpp + 4)) + (split ? w8::edge_ring_floats(hpp, split) : 0);
  pub_ch = w8::pub_chunk_tiles(S, own + (cap - base), T);
  if (pub_ch < 1) return false;
  // prefer the smallest chunk that gives the same number of chunks (less LDS, same barriers)
  const int nch = (T + pub_ch - 1) / pub_ch;
  pub_ch = (T + nch - 1) / nch;
  pubx = (int)std::max(0LL, (long long)S * (16 * pub_ch + 4) - own);
  return true;
}
static size_t lds_bytes8(int hpe, int hpp, int N, int D, int S, int pubx, int split, NodeBuf nodes = kResident) {
  return sizeof(float) * (lds_floats8_base(hpe, hpp, N, D, S, split, nodes) + (hpp ? pubx : 0));
}

static int launch(gaudi_handle* h, const KParams& P, int hpe, int hpp, long long steps) {
  const LaunchPlan& plan = h->plan;
  const bool v8 = plan.waves == 8;
  const bool se = hpe && plan.ef > 2;  // stage_graph keeps such a call on the 4-wave family
  KernelKey key{};
  const kernel_fn fn = plan_kernel(plan, hpe, hpp, P.vt != nullptr, &key);
  if (!fn)
    return fail(h, GAUDI_E_INVALID,
                "no kernel instantiated for padded hidden sizes (" + std::to_string(hpe) + "," + std::to_string(hpp) + ")" +
                    (v8 ? " in the 8-wave family" : se ? " among the sin_embedding kernels" : ""));
  size_t lds = v8 ? lds_bytes8(hpe, hpp, P.N, 3 + P.F, P.EW, P.pubx, plan.ring, launch_nodes(plan, hpe, hpp))
                  : lds_bytes(hpe, hpp, P.N, 3 + P.F, P.EW, plan.nodes == kAllGlobal, se ? 24 : 2);
  if (v8 && P.hk_off) lds = sizeof(float) * ((size_t)P.hk_off + (size_t)plan.hk);  // the kept split copy of h sits behind the FUSED plan
  if (lds > 160 * 1024)
    return fail(h, GAUDI_E_CAPACITY, "molecule needs " + std::to_string(lds) + " B of LDS (>160 KiB): N too large");
  {
    // hipFuncAttributeMaxDynamicSharedMemorySize belongs to the function, not to a handle: one process-wide record per
    // (device, kernel), only ever raised, so that no handle launches with more dynamic LDS than the attribute allows
    static std::mutex attr_mu;
    static std::map<std::pair<int, const void*>, int> granted_by_fn;
    std::lock_guard<std::mutex> lock(attr_mu);
    int& granted = granted_by_fn[{h->device, (const void*)fn}];
    if ((int)lds > granted) {
      HIPCHECK(h, hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      granted = (int)lds;
    }
  }
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (h->prof) HIPCHECK(h, h->prof_log.begin(h->stream, ev));
#ifdef GAUDI_STAMPS
  KParams PS = P;
  HIPCHECK(h, h->d_stamps.reserve(sizeof(unsigned long long) * 32));
  HIPCHECK(h, hipMemsetAsync(h->d_stamps.p, 0, sizeof(unsigned long long) * 32, h->stream));
  PS.stamps = h->d_stamps.as<unsigned long long>();
  hipLaunchKernelGGL(fn, dim3(P.B), dim3(v8 ? w8::kThreads : kThreads), lds, h->stream, PS);
  {
    unsigned long long tmp[32];
    HIPCHECK(h, hipMemcpyAsync(tmp, h->d_stamps.p, sizeof(tmp), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 32; ++i) h->stamp_acc[i] += tmp[i];
    if (getenv("GAUDI_PRINT_STAMPS")) {
      static const char* nm[] = {"node_gemm", "edge_gemm", "edge_epilogue", "barrier", "misc", "bwd_node", "bwd_stash_reload",
                                 "bwd_colsum_tail", "pub_wait", "stash", "pub_write", "colsum_loop", "colsum_barrier", "b_dcp",
                                 "b_gemm_de", "b_dv", "b_gemm_dt1", "b_du", "stage_vectors", "geo", "edm_embed_head", "noise_update",
                                 "bwd_reload_loads", "bwd_vec_commit", "pred_readout", "bwd_prologue", "x2", "x3", "b_dx_sum", "f_coord_update"};
      static_assert(sizeof(nm) / sizeof(nm[0]) == ST_N, "one name per stamp id");
      unsigned long long tot = 0;
      for (int i = 0; i < ST_N; ++i) tot += h->stamp_acc[i];
      fprintf(stderr, "[stamps] cumulative shares (block 0, wave 0):");
      for (int i = 0; i < ST_N; ++i) fprintf(stderr, " %s=%.1f%%", nm[i], 100.0 * h->stamp_acc[i] / (tot ? tot : 1));
      fprintf(stderr, " total=%llu ticks\n", tot);
      if (tmp[31])
        fprintf(stderr, "[stamps] shader clock during this launch: %.0f MHz (%llu cycles / %llu ticks of 100 MHz)\n",
                100.0 * (double)tmp[30] / (double)tmp[31], tmp[30], tmp[31]);
    }
  }
#else
  if (h->prof) {  // profiled launches also leave their clock counters (sampler_kernel.h: KParams::clock_out)
    KParams PC = P;
    HIPCHECK(h, h->d_clock.reserve(sizeof(unsigned long long) * 4));
    PC.clock_out = h->d_clock.as<unsigned long long>();
    hipLaunchKernelGGL(fn, dim3(P.B), dim3(v8 ? w8::kThreads : kThreads), lds, h->stream, PC);
  } else {
    hipLaunchKernelGGL(fn, dim3(P.B), dim3(v8 ? w8::kThreads : kThreads), lds, h->stream, P);
  }
#endif
  HIPCHECK(h, hipGetLastError());
  h->last_key = key_name(key);
  if (std::find(h->key_log.begin(), h->key_log.end(), h->last_key) == h->key_log.end()) h->key_log.push_back(h->last_key);
  // A launch that runs the side job -- the plan placed its rows AND the kernel launched has the job compiled in -- says so behind
  // its key (the log keeps the table's keys: the job is a launch parameter, not an instantiation)
  if (const KernelEntry* e = find_entry(key); e && (e->side & 1) && P.side_off != 0) h->last_key += " SD=" + std::to_string(e->side);
  if (getenv("GAUDI_DEBUG_PLAN")) fprintf(stderr, "[launch] %s\n", h->last_key.c_str());
  if (h->prof) {
    HIPCHECK(h, h->prof_log.end(h->stream, ev));
    h->prof_steps += steps;
  }
  return GAUDI_OK;
}

// Packed launches: groups of molecules, each group one graph of N node slots
struct Pack {
  int G = 0;
  int NG = 0;                         // node slots per group (= N, or more: wide groups)
  std::vector<float> umask, uemask;   // [G][NG], [G][NG][NG]: the union graphs
  std::vector<uint8_t> align;         // [G][NG]: first slot of every component (tile alignment in build_meta8)
  std::vector<int32_t> rowmap;        // [G][NG]: slot -> molecule * N + node | component << 28, or -1
  std::vector<int32_t> compmol;       // [G][kMaxComp]
  std::vector<int32_t> ncomp;         // [G]
};
// NG node slots and TG edge tiles per group (N and 8: the classic packing; more: wide groups, whose edge phases run in rounds)
// nodes a molecule needs slots for in a packed launch: live ones and any node that touches a live edge, in their own order
static std::vector<std::vector<int>> used_nodes(int B, int N, const float* node_mask, const float* edge_mask) {
  std::vector<std::vector<int>> used(B);
  for (int b = 0; b < B; ++b) {
    std::vector<char> keep(N, 0);
    for (int i = 0; i < N; ++i) {
      const bool li = node_mask[(size_t)b * N + i] != 0.f;
      if (li) keep[i] = 1;
      for (int j = 0; j < N; ++j) {
        const bool lj = node_mask[(size_t)b * N + j] != 0.f;
        if (edge_mask[((size_t)b * N + i) * N + j] != 0.f && (li || lj)) keep[i] = keep[j] = 1;
      }
    }
    for (int i = 0; i < N; ++i)
      if (keep[i]) used[b].push_back(i);
  }
  return used;
}
// narrow: NG may be SMALLER than N (every molecule must then fit NG slots on its own: the caller checks) -- rows of the global
// arrays keep the stride N.  maxcomp: molecules per group (1: every molecule alone, its nodes compacted to the front slots).
// molmap: molecule -> index the noise is keyed with (a bucket of a larger request), or nullptr.
// max_multi: groups that may hold more than one molecule (a MIXED wide launch: pairs first, the rest alone in the same kernel).
static void pack_groups(int B, int N, const float* node_mask, const float* edge_mask, const Meta8& M, Pack& pk, int NG = 0,
                        int TG = w8::kWaves, bool narrow = false, int maxcomp = kMaxComp, const int32_t* molmap = nullptr,
                        int max_multi = INT_MAX) {
  if (NG < N && !narrow) NG = N;
  const std::vector<std::vector<int>> used = used_nodes(B, N, node_mask, edge_mask);
  struct Group {
    std::vector<int> mols;
    int nodes = 0, tiles = 0;
  };
  std::vector<Group> groups;
  int multi = 0;
  for (int b : M.order) {  // heaviest first
    const int nn = (int)used[b].size(), nt = M.ntiles[b];
    Group* fit = nullptr;
    for (Group& g : groups)
      if ((int)g.mols.size() < maxcomp && g.nodes + nn <= NG && g.tiles + nt <= TG && (g.mols.size() > 1 || multi < max_multi)) {
        fit = &g;
        if (g.mols.size() == 1) ++multi;
        break;
      }
    if (!fit) {
      groups.emplace_back();
      fit = &groups.back();
    }
    fit->mols.push_back(b);
    fit->nodes += nn;
    fit->tiles += nt;
  }
  const int G = (int)groups.size();
  pk.G = G;
  pk.NG = NG;
  pk.umask.assign((size_t)G * NG, 0.f);
  pk.uemask.assign((size_t)G * NG * NG, 0.f);
  pk.align.assign((size_t)G * NG, 0);
  pk.rowmap.assign((size_t)G * NG, -1);
  pk.compmol.assign((size_t)G * kMaxComp, 0);
  pk.ncomp.assign(G, 0);
  std::vector<int> slot_of(N);
  for (int g = 0; g < G; ++g) {
    int base = 0;
    for (size_t k = 0; k < groups[g].mols.size(); ++k) {
      const int b = groups[g].mols[k];
      pk.compmol[(size_t)g * kMaxComp + k] = molmap ? molmap[b] : b;
      std::fill(slot_of.begin(), slot_of.end(), -1);
      for (size_t r = 0; r < used[b].size(); ++r) slot_of[used[b][r]] = base + (int)r;
      if (!used[b].empty()) pk.align[(size_t)g * NG + base] = 1;
      for (int i : used[b]) {
        const int si = slot_of[i];
        pk.umask[(size_t)g * NG + si] = node_mask[(size_t)b * N + i];
        pk.rowmap[(size_t)g * NG + si] = (b * N + i) | ((int32_t)k << 28);
        for (int j : used[b])
          pk.uemask[((size_t)g * NG + si) * NG + slot_of[j]] = edge_mask[((size_t)b * N + i) * N + j];
      }
      base += (int)used[b].size();
    }
    pk.ncomp[g] = (int)groups[g].mols.size();
  }
}

// upload masks + metadata, fill the graph part of KParams
// -> GAUDI_OK, or a positive value = "run this call on the 4-wave kernels" (graph outside the 8-wave kernels' limits)
// plan: written once, at the end (a fall-back or an error leaves it as it came)
static int stage_graph8(gaudi_handle* h, int B, int N, const float* node_mask, const float* edge_mask, KParams& P, int hpe,
                        int hpp, const CallHints& hints, LaunchPlan& plan) {
  if (std::max(h->plan_force_waves, hints.force_waves) == 4) return 1;  // the whole logical batch runs on 4 waves
  Meta8 M;
  std::string err;
  int rc = build_meta8(B, N, node_mask, edge_mask, M, err, std::max(h->plan_min_slots, hints.min_slots));
  if (rc == GAUDI_E_CAPACITY) return 1;
  if (rc) return fail(h, rc, err);
  // more than one round of eight edge tiles (a graph of more than 128 live-edge slots, e.g. a fully connected molecule of
  // 12+ nodes): the 8-wave kernels run the rounds one after the other (GAUDI_PRED_ROUNDS=0: the round-2 behaviour, such calls
  // go to the 4-wave kernels); the LDS plan below decides whether the larger per-slot arrays and publish buffer still fit
  const bool mr = hpp && (M.S > 16 * w8::kWaves || h->force_mr);
  if (mr && !h->pred_rounds) return 1;
  // ---- packing: small molecules share a workgroup as the components of one graph (sampling calls only).  First-fit in
  // the heaviest-first order; a group holds at most kMaxComp molecules, N node slots and 8 edge tiles (one round on 8
  // waves).  A molecule keeps its own tiles (component starts are tile-aligned), its nodes keep their relative order, its
  // noise is keyed by its own sample and node indices, and every per-molecule reduction runs per component in the order
  // the molecule's own workgroup would use: the result does not depend on the packing, bit for bit.
  if (!have_kernel8(hpe, hpp, 0, mr) && !have_kernel8(hpe, hpp, 1, mr) && !have_kernel8(hpe, hpp, 2, mr)) return 1;
  const int Dz = 3 + (hpe ? h->ecfg.in_node_nf : h->pcfg.in_nf);
  // the arithmetic of the edge GEMMs for S edge slots on NS node slots: split operands when the kernel exists and its larger weight
  // ring fits (1 = full ring, 2 = half ring); else fp32 MFMAs (0); else -1 = this call runs on 4 waves
  // the split-operand kernels run their node GEMMs on fp16 pairs: a weight set whose images were refused (NodeScale) keeps the
  // fp32-instruction kernels
  const bool node_f16_ok = !GAUDI_NODE_F16 || ((!hpe || h->edm_hinv > 0.f) && (!hpp || h->pred_hinv > 0.f));
  struct RingPlan {
    int mode = -1, pubx = 0, pub_ch = 0;
  };
  auto plan_for = [&](int NS, int S, bool mrk) -> RingPlan {
    RingPlan r;
    if (h->split && (!hpe || h->edm_ws_bytes) && (!hpp || h->pred_ws_bytes) && node_f16_ok)
      for (int mode = 1; mode <= 2; ++mode)
        if (have_kernel8(hpe, hpp, mode, mrk) && plan_pub8(hpe, hpp, NS, Dz, S, mode, r.pubx, r.pub_ch)) return RingPlan{mode, r.pubx, r.pub_ch};
    return have_kernel8(hpe, hpp, 0, mrk) && plan_pub8(hpe, hpp, NS, Dz, S, 0, r.pubx, r.pub_ch) ? RingPlan{0, r.pubx, r.pub_ch} : RingPlan{};
  };
  RingPlan acc = plan_for(N, M.S, mr);  // the accepted plan: the unpacked resident one until a later stage replaces it
  int mode_u = acc.mode;
  Pack pk;
  const int B0 = B;
  const float* nm_used = node_mask;
  int n_slots = N;
  bool mr_run = mr;
  bool narrow_taken = false, use_pack = false, pg_run = false;
  // Round 6: a bucket of molecules that fit the resident kernels on their own (gaudi_sample: per-molecule kernel family) while the
  // call's padded N does not -- packed groups of hints.narrow (< N) node slots, one round of eight edge tiles.
  if (hints.narrow > 0 && hints.narrow < N && hints.may_pack && (int64_t)B * N < (1 << 28)) {
    pack_groups(B, N, node_mask, edge_mask, M, pk, hints.narrow, w8::kWaves, true, kMaxComp, hints.molmap);
    Meta8 M2;
    rc = build_meta8(pk.G, hints.narrow, pk.umask.data(), pk.uemask.data(), M2, err, 0, pk.align.data());
    if (rc != GAUDI_OK) return fail(h, rc, "per-molecule kernel family: " + err);
    const bool mr2 = hpp && M2.S > 16 * w8::kWaves;
    const RingPlan p2 = plan_for(hints.narrow, M2.S, mr2);
    if (p2.mode < 1 || mr2) return fail(h, GAUDI_E_CAPACITY, "per-molecule kernel family: the resident plan of the small bucket does not fit");
    M = std::move(M2);
    B = pk.G;
    nm_used = pk.umask.data();
    n_slots = hints.narrow;
    acc = p2;
    mode_u = p2.mode;
    mr_run = mr2;
    narrow_taken = use_pack = true;
  }
  // V8G (round 4): a molecule whose node buffers do not fit LDS beside the ring runs on the 8-wave kernels with those five
  // buffers in a per-workgroup global scratch (split edge GEMMs, full ring, several rounds of edge tiles) -- before round 4
  // such calls fell to the 4-wave V4G kernels (fp32 matrix instructions, two launches per guided step)
  // Round 6: of the five, P and Q stay in LDS where that plan fits (kern8gp_*.hip; +3.6 % on 40-node molecules) -- a function of
  // the widths, N and the edge slots the plan is made with (the whole batch's: hints.min_slots / plan_min_slots), like the rest
  NodeBuf gn8 = kResident;
  RingPlan gplan{1, 0, 0};
  if (!narrow_taken && (mode_u < 0 || h->force_gn8) && h->gn8 && h->split && (!hpe || h->edm_ws_bytes) && (!hpp || h->pred_ws_bytes) && node_f16_ok &&
      (GAUDI_NODE_F16 || gn8_stage_fits(hpe, hpp, N))) {
    if (h->gn8_pq && GAUDI_NODE_F16 && have_kernel8(hpe, hpp, 1, true, kPqLds) && plan_pub8(hpe, hpp, N, Dz, M.S, 1, gplan.pubx, gplan.pub_ch, kPqLds)) gn8 = kPqLds;
    else if (have_kernel8(hpe, hpp, 1, true, kAllGlobal) && plan_pub8(hpe, hpp, N, Dz, M.S, 1, gplan.pubx, gplan.pub_ch, kAllGlobal)) gn8 = kAllGlobal;
  }
  if (gn8) {
    acc = gplan;
    mode_u = 1;
  }
  if (mode_u < 0) return 1;
  // V8G sampling calls (round 6): every molecule alone in its workgroup as before, but its nodes COMPACTED to the front slots
  // (a hetero molecule's rings and orientation nodes are two blocks of the padded index range: n rings occupy columns up to
  // N / 2 + n) -- fewer node-GEMM column tiles; the packed form also carries the molecule's index in the request (hints.molmap).
  if (gn8 && hints.may_pack && h->pack && h->gn8_pack && (int64_t)B * N < (1 << 28)) {
    pack_groups(B, N, node_mask, edge_mask, M, pk, N, 1 << 20, false, 1, hints.molmap);
    Meta8 M2;
    int pubx2 = 0, pub_ch2 = 0;
    if (build_meta8(pk.G, N, pk.umask.data(), pk.uemask.data(), M2, err, M.S, pk.align.data()) == GAUDI_OK && M2.S == M.S &&
        plan_pub8(hpe, hpp, N, Dz, M2.S, 1, pubx2, pub_ch2, gn8)) {
      M = std::move(M2);
      B = pk.G;
      nm_used = pk.umask.data();
      acc.pubx = pubx2;
      acc.pub_ch = pub_ch2;
      use_pack = true;
    } else {
      if (hints.molmap) return fail(h, GAUDI_E_CAPACITY, "per-molecule kernel family: the packed V8G plan does not fit");
      pk = Pack();
    }
  }
  // (a row of the map holds molecule * N + node in 28 bits)
  if (!gn8 && !narrow_taken && hints.may_pack && h->pack && B > 1 && (int64_t)B * N < (1 << 28)) {
    // Candidate group shapes, widest first.  WIDE groups (opt-in: GAUDI_PAIRS=1 for batches of at least two molecules per CU, 2
    // always): up to 2 N node slots and two rounds of eight edge tiles -- e.g. two 11-ring cata molecules, or three to four small
    // hetero ones, per workgroup.  Every node-level matrix is then streamed from L2 once for all of them and the per-GEMM fixed
    // costs are shared; the edge phases run their rounds one after the other on the half ring (the predictor on the MR
    // kernels).  Bit-identical to the narrow launch.  Then the classic shape: N node slots, one round.
    struct Cand {
      int NG, TG;
    };
    std::vector<Cand> cands;
    // (pairs == 1, the default: when the batch holds at least two molecules per CU AND the classic shape packs next to nothing --
    // cata molecules fill their N slots; a hetero batch whose small molecules already share workgroups gains nothing from the
    // second round: C4 -0.9 %, C3 at 1 024 molecules +2.6 %, C2 at 1 024 +6.7 % with the fp16-pair node GEMMs, profiles/r05c_*)
    // Round 6: "pays" is decided by ROUNDS of workgroups on the chip -- a workgroup of two molecules takes 1.81 x one molecule's time
    // (111.5 against 2 x 30.8 ms per launch, profiles/r06h_wide_pairs*), so pairs win where they save enough rounds: 257-512 and
    // 769-1024 molecules on 256 CUs (2 -> 1.8 and 4 -> 3.6 round-times), not 513-768 (3 -> 3.6).  Same bits either way.
    // MIXED launches: with p two-molecule groups and B - 2 p single ones in the same wide kernel (heaviest first: the pairs), the
    // makespan on the chip's CUs is what a list schedule gives -- wide_plan tries p = every multiple of the CU count and "all pairs",
    // and takes the wide kernel where its best beats ceil(B / CUs) rounds of the one-molecule kernel: 640 molecules run as 256 pairs +
    // 128 single ones (2.84 round-times against 3), 1 024 as 512 pairs, 256 one per workgroup.
    bool want_wide = h->pairs == 2;
    int max_multi = INT_MAX;
    if (h->pairs == 1 && B > h->num_cus) {
      const int cus = std::max(1, h->num_cus);
      const double solo = (double)((B + cus - 1) / cus);
      auto makespan = [&](int p) {  // list schedule of p jobs of kPair and B - 2 p jobs of kAlone on `cus` machines, longest first
        // (measured at the default widths, profiles/r06k_wide_group_rule.txt: a pair 2 228 ms, a molecule alone in the wide kernel 1 325 ms,
        // the one-molecule kernel 1 236 ms per 1 000 steps)
        const double kPair = 1.81, kAlone = 1.07;
        std::priority_queue<double, std::vector<double>, std::greater<double>> free_at;
        for (int c = 0; c < cus; ++c) free_at.push(0.0);
        double end = 0.0;
        auto run = [&](int n, double cost) {
          for (int k = 0; k < n; ++k) {
            const double t = free_at.top() + cost;
            free_at.pop();
            free_at.push(t);
            end = std::max(end, t);
          }
        };
        run(p, kPair);
        run(B - 2 * p, kAlone);
        return end;
      };
      double best = solo * 0.995;  // (the one-molecule kernel unless the wide one is clearly ahead)
      int best_p = -1;
      for (int p = cus; p <= B / 2 + cus - 1; p += cus) {
        const int pp = std::min(p, B / 2);
        const double m = makespan(pp);
        if (m < best) { best = m; best_p = pp; }
      }
      if (h->pairs_cap >= 0) best_p = std::min(h->pairs_cap, B / 2);
      if (best_p >= 0) {
        pack_groups(B, N, node_mask, edge_mask, M, pk, N, w8::kWaves);
        want_wide = (long long)pk.G * 10 >= (long long)B * 9;
        max_multi = best_p;
      }
    }
    if (want_wide && h->pairs_cap >= 0) max_multi = h->pairs_cap;  // (experiments)
    if (want_wide)
      for (int ng = std::min(2 * N, 32); ng > N; --ng) {
        const long long cap = 160 * 1024 / 4 - 64;
        if ((long long)lds_floats8_base(hpe, hpp, ng, Dz, 16 * (w8::kWaves + 1), h->split ? 2 : 0) > cap) continue;  // cannot fit whatever the slots
        cands.push_back({ng, 2 * w8::kWaves});
      }
    cands.push_back({N, w8::kWaves});
    for (const Cand& cd : cands) {
      const bool wide = cd.NG > N;
      pack_groups(B, N, node_mask, edge_mask, M, pk, cd.NG, cd.TG, false, kMaxComp, nullptr, wide ? max_multi : INT_MAX);
      if (pk.G >= B && !(wide && h->pairs_cap == 0)) continue;  // (GAUDI_PAIRS_CAP=0: every molecule alone in the wide kernel -- diagnostic)
      Meta8 M2;
      rc = build_meta8(pk.G, cd.NG, pk.umask.data(), pk.uemask.data(), M2, err, wide ? 0 : M.S, pk.align.data());
      if (rc != GAUDI_OK) continue;
      const bool mr2 = hpp && M2.S > 16 * w8::kWaves;
      if (!wide && M2.S > std::max(M.S, 16 * w8::kWaves)) continue;  // (a classic group holds <= 8 tiles)
      if (mr2 && !mr && !h->pred_rounds) continue;
      // a packed launch has more edge slots per workgroup; it must keep the ARITHMETIC the unpacked plan has -- split operands
      // (full or half ring: the same sums in the same order) or fp32 instructions -- because the plan of a sharded batch is the
      // same on every rank (gaudi_set_plan_hint) and packing must not move a rank off it
      RingPlan p2 = plan_for(cd.NG, M2.S, mr2);
      if (p2.mode < 0 || (p2.mode != 0) != (mode_u != 0)) continue;
      // Round 6: a wide group that fits the HALF ring only (two cata-11 molecules at the default widths: five predictor buffers of 22
      // node slots + the 52 KiB ring are 171 KB) runs on the FULL ring with the predictor's fifth node buffer in the workgroup's global
      // scratch (kern8mp_fused.hip) -- the same sums in the same order, one trip per K chunk instead of two
      RingPlan full{1, 0, 0};
      if (wide && p2.mode == 2 && mr2 && h->wide_full && hpe && hpp && have_kernel8(hpe, hpp, 1, true, kPredFifthGlobal) &&
          plan_pub8(hpe, hpp, cd.NG, Dz, M2.S, 1, full.pubx, full.pub_ch, kPredFifthGlobal)) {
        p2 = full;
        pg_run = true;
      }
      M = std::move(M2);
      B = pk.G;
      nm_used = pk.umask.data();
      n_slots = cd.NG;
      acc = p2;
      mr_run = mr2;
      use_pack = true;
      break;
    }
  }
  const bool packed = use_pack;
  const NodeBuf nodes = pg_run ? kPredFifthGlobal : gn8;
  P.pubx = acc.pubx;
  P.pub_ch = acc.pub_ch;
  // The N1 instantiation of the resident full-ring kernel (plan_kernel): one column tile per node GEMM, i.e. at most 16 node slots
  // per workgroup, packed or not; and its tail blocks hold ONE k-step (w8_nodes_f16.h: kTailOne), so a network whose padded width
  // has a tail block must be one of H % 16 == 4 (196 -> 208; a predictor of 200 or 208 features keeps the plain kernel)
  auto one_step_tail = [](int H, int HP) { return !HP || !w8::nh_odd(HP) || has_ktail(H, HP); };
  const bool n1_run = !h->no_n1 && nodes == kResident && acc.mode == 1 && n_slots <= 16 &&  // (mr: plan_kernel, per launch)
                      one_step_tail(h->ecfg.hidden_nf, hpe) && one_step_tail(h->pcfg.hidden_nf, hpp);
  if (getenv("GAUDI_DEBUG_PLAN"))
    fprintf(stderr, "[plan] molecules=%d workgroups=%d N=%d node slots=%d S=%d split=%d mr=%d nodes=%d n1=%d pub_ch=%d pubx=%d lds=%zu\n", B0, B,
            N, n_slots, M.S, acc.mode, (int)mr_run, (int)nodes, (int)n1_run, acc.pub_ch, acc.pubx,
            lds_bytes8(hpe, hpp, n_slots, Dz, M.S, acc.pubx, acc.mode, nodes));
  auto up = [&](DevBuf& d, const void* src, size_t bytes) -> hipError_t {
    hipError_t e = d.reserve(bytes);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, h->stream);
  };
  HIPCHECK(h, up(h->d_ncols, M.ncols.data(), sizeof(int) * B));
  HIPCHECK(h, up(h->d_mask, nm_used, sizeof(float) * B * n_slots));
  if (packed) {
    HIPCHECK(h, up(h->d_rowmap, pk.rowmap.data(), sizeof(int32_t) * pk.rowmap.size()));
    HIPCHECK(h, up(h->d_compmol, pk.compmol.data(), sizeof(int32_t) * pk.compmol.size()));
    HIPCHECK(h, up(h->d_ncomp, pk.ncomp.data(), sizeof(int32_t) * pk.ncomp.size()));
  }
  HIPCHECK(h, up(h->d_order, M.order.data(), sizeof(int) * B));
  HIPCHECK(h, up(h->d_edges, M.edges.data(), sizeof(uint32_t) * M.edges.size()));
  HIPCHECK(h, up(h->d_emask, M.emask.data(), sizeof(float) * M.emask.size()));
  HIPCHECK(h, up(h->d_npairs, M.ntiles.data(), sizeof(int) * B));
  HIPCHECK(h, up(h->d_seg, M.seg.data(), sizeof(uint32_t) * M.seg.size()));
  HIPCHECK(h, up(h->d_soff, M.soff.data(), sizeof(uint16_t) * M.soff.size()));
  HIPCHECK(h, up(h->d_sidx, M.sidx.data(), sizeof(uint16_t) * M.sidx.size()));
  HIPCHECK(h, hipStreamSynchronize(h->stream));  // M goes out of scope
  P.B = B;
  P.N = n_slots;
  P.NR = N;
  P.EW = M.S;
  P.node_mask = h->d_mask.as<float>();
  P.order = h->d_order.as<int>();
  P.edges = h->d_edges.as<uint32_t>();
  P.emask = h->d_emask.as<float>();
  P.npairs = h->d_npairs.as<int>();
  P.seginfo = h->d_seg.as<uint32_t>();
  P.ncols = h->d_ncols.as<int>();
  P.soff = h->d_soff.as<uint16_t>();
  P.sidx = h->d_sidx.as<uint16_t>();
  P.rowmap = packed ? h->d_rowmap.as<int32_t>() : nullptr;
  P.compmol = packed ? h->d_compmol.as<int32_t>() : nullptr;
  P.ncomp = packed ? h->d_ncomp.as<int32_t>() : nullptr;
  // Kept split copy of h (w8_nodes_f16.h: node_ctx_keep): behind everything the plan of BOTH networks needs, when 160 KiB leave the
  // room -- C2 / C3 do (46 KB free), 20-22 node slots do not.  Same results either way (the copy is a function of h alone).
  // The side job of the N1 fused kernel (w8_pred.h: pred_forward, SD; asked for through P.side_off): the last wave of EVERY workgroup is without an
  // edge tile (at most 7 tiles each: 11 fully connected nodes), h's copy is kept, and the job's rows -- [node slots][hpp + 4], in
  // front of that copy -- fit too.  Same results as the N1 kernel.
  P.hk_off = 0;
  P.side_off = 0;
  int hk = 0;
  bool side_run = false;
  if (h->keep_h && GAUDI_NODE_F16 && acc.mode >= 1 && nodes == kResident) {
    const size_t floats = lds_bytes8(hpe, hpp, n_slots, Dz, M.S, acc.pubx, acc.mode) / sizeof(float);
    const size_t at = (floats + 3) & ~(size_t)3;
    const size_t need = (size_t)w8::nh_keep_floats(std::max(hpe, hpp), n_slots);
    KernelKey kn = key8(hpe, hpp, 1, false);  // (the fused N1 kernel this plan's guided launches take, if it has the job)
    kn.n1 = true;
    const KernelEntry* const en = find_entry(kn);
    const bool side_want = !h->no_side && n1_run && hpe && hpp && !mr_run && en != nullptr && (en->side & 1) &&
                           *std::max_element(M.ntiles.begin(), M.ntiles.begin() + B) <= w8::kWaves - 1;
    const size_t side = (size_t)n_slots * (hpp + 4);  // (a multiple of 4 floats)
    if (side_want && (at + side + need) * sizeof(float) + 1024 <= 160 * 1024) {
      P.side_off = (int)at;
      P.hk_off = (int)(at + side);
      hk = (int)need;
      side_run = true;
    } else if ((at + need) * sizeof(float) + 1024 <= 160 * 1024) {
      P.hk_off = (int)at;
      hk = (int)need;
    }
  }
  if (getenv("GAUDI_DEBUG_PLAN")) fprintf(stderr, "[plan] side=%d side_off=%d hk_off=%d hk=%d\n", (int)side_run, P.side_off, P.hk_off, hk);
  if (pg_run) {  // one [node slots][hpp + 4] buffer per workgroup
    const size_t stride = ((size_t)n_slots * (hpp + 4) + 63) / 64 * 64;
    HIPCHECK(h, h->d_gnode.reserve(sizeof(float) * (stride * (size_t)B + 256)));
    P.gnode = h->d_gnode.as<float>();
    P.gnode_stride = (long long)stride;
  }
  if (gn8) {
    const size_t stride = (gnode_floats8(hpe, hpp, N) + 63) / 64 * 64;
    HIPCHECK(h, h->d_gnode.reserve(sizeof(float) * (stride * (size_t)B + 256)));  // (+ the staging copies' 1 KiB read granule)
    P.gnode = h->d_gnode.as<float>();
    P.gnode_stride = (long long)stride;
  }
  plan.waves = 8;
  plan.ring = acc.mode;
  plan.mr = mr_run;
  plan.nodes = nodes;
  // (the FR instantiation: launches on the resident full-ring kernel with two column tiles per node GEMM, launch / plan_kernel)
  plan.fr = !h->no_fr && gn8 == kResident && acc.mode == 1 && n_slots > 16;
  plan.n1 = n1_run;
  plan.groups = B;
  plan.nslots = n_slots;
  plan.hk = hk;
  plan.pubx = acc.pubx;
  plan.pub_ch = acc.pub_ch;
  return GAUDI_OK;
}

// hpe / hpp: padded hidden sizes of the networks this call runs (0 = not used)
static int stage_graph(gaudi_handle* h, int B, int N, const float* node_mask, const float* edge_mask, KParams& P, int hpe,
                       int hpp, const CallHints& hints) {
  if (B <= 0 || N <= 0) return fail(h, GAUDI_E_INVALID, "B and N must be positive");
  // a node slot's row word holds molecule * N + node in 28 bits (sampler_kernel.h: row_of / comp_of)
  if ((int64_t)B * N >= (1 << 28)) return fail(h, GAUDI_E_CAPACITY, "B * N must stay below 2^28 per call: cut the request into several calls");
  LaunchPlan plan;  // (assigned to the handle where this function succeeds: a failed call leaves the last call's plan)
  // a sin_embedding denoiser (24 edge features per first Linear, egnn_new.py:269-273) exists in the 4-wave family only
  const bool se = hpe && h->ecfg.sin_embedding;
  if (h->variant == 8 && !h->force_gn && !se) {
    const int rc8 = stage_graph8(h, B, N, node_mask, edge_mask, P, hpe, hpp, hints, plan);
    if (rc8 == GAUDI_OK) h->plan = plan;
    if (rc8 <= 0) return rc8;
    P.pubx = P.pub_ch = 0;  // fall back to the 4-wave kernels for this call
  }
  plan.groups = B;
  plan.nslots = N;
  // the 4-wave reverse pass parks [4 waves][N * 3] partial coordinate gradients in its 4 x 16 x (HP + 4) transposition scratch
  if (hpp && 4 * N * 3 > 4 * 16 * (hpp + 4))
    return fail(h, GAUDI_E_CAPACITY, "N too large for the 4-wave predictor kernels at this hidden size");
  Meta M;
  std::string err;
  int rc = build_meta(B, N, node_mask, edge_mask, M, err);
  if (rc) return fail(h, rc, err);
  HIPCHECK(h, h->d_mask.reserve(sizeof(float) * B * N));
  HIPCHECK(h, h->d_order.reserve(sizeof(int) * B));
  HIPCHECK(h, h->d_edges.reserve(sizeof(uint32_t) * M.edges.size()));
  HIPCHECK(h, h->d_emask.reserve(sizeof(float) * M.emask.size()));
  HIPCHECK(h, h->d_npairs.reserve(sizeof(int) * M.npairs.size()));
  HIPCHECK(h, h->d_seg.reserve(sizeof(uint32_t) * M.seg.size()));
  HIPCHECK(h, h->d_ncols.reserve(sizeof(int) * B));
  HIPCHECK(h, hipMemcpyAsync(h->d_ncols.p, M.ncols.data(), sizeof(int) * B, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(h->d_mask.p, node_mask, sizeof(float) * B * N, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(h->d_order.p, M.order.data(), sizeof(int) * B, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(h->d_edges.p, M.edges.data(), sizeof(uint32_t) * M.edges.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(h->d_emask.p, M.emask.data(), sizeof(float) * M.emask.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(h->d_npairs.p, M.npairs.data(), sizeof(int) * M.npairs.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(h->d_seg.p, M.seg.data(), sizeof(uint32_t) * M.seg.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));  // M goes out of scope
  P.B = B;
  P.N = N;
  P.NR = N;
  P.EW = M.EW;
  P.node_mask = h->d_mask.as<float>();
  P.order = h->d_order.as<int>();
  P.edges = h->d_edges.as<uint32_t>();
  P.emask = h->d_emask.as<float>();
  P.npairs = h->d_npairs.as<int>();
  P.seginfo = h->d_seg.as<uint32_t>();
  P.ncols = h->d_ncols.as<int>();
  // Molecules whose node buffers do not fit 160 KiB of LDS (beyond ~22 graph nodes at the default widths) run on the V4G
  // kernels: same code, node buffers in a per-workgroup global scratch (L2-resident).  The reference has no size cap
  // (sampling_edm.py:172-209); this one is N <= 255 (node indices are bytes in the edge words).
  // While the call is a shard of a larger logical batch (plan hint) or one of gaudi_sample's sub-batches, the choice is made
  // for the DENSE graph of N nodes, not for this batch's edges: the cuts of one logical batch must not land on different
  // kernels because one of them happens to be sparser.  A call that stands alone decides from its own edge lists (a sparse
  // hetero batch of 18-20 nodes fits the resident kernels where the dense graph would not).
  const int Dz = 3 + (hpe ? h->ecfg.in_node_nf : h->pcfg.in_nf);
  const bool part_of_batch = h->plan_min_slots || h->plan_force_waves || hints.min_slots || hints.force_waves || hints.cut;
  const int ef = plan.ef = se ? 24 : 2;
  // (the V4G predictor-only kernel is the ordinary one for a sin_embedding handle too)
  const bool have_g = (!hpe || find_kernel(key4(hpe, 0, true, ef))) && (!hpp || find_kernel(key4(0, hpp, true)));
  if (h->force_gn || lds_bytes(hpe, hpp, N, Dz, part_of_batch ? std::max(M.EW, dense_ew4(N)) : M.EW, false, ef) > 160 * 1024) {
    if (have_g && lds_bytes(hpe, hpp, N, Dz, M.EW, true, ef) <= 160 * 1024) {
      plan.nodes = kAllGlobal;
      const size_t stride = (gnode_floats(hpe, hpp, N) + 63) / 64 * 64;
      HIPCHECK(h, h->d_gnode.reserve(sizeof(float) * stride * (size_t)B));
      P.gnode = h->d_gnode.as<float>();
      P.gnode_stride = (long long)stride;
    }
  }
  // Guided steps as two launches: the V4G kernels have no fused instantiation, and a sin_embedding denoiser has one at the tiny and the
  // default width pairs only -- every other width runs its denoiser-only kernel followed by the ordinary predictor-only kernel
  plan.two = plan.nodes == kAllGlobal || (se && hpp && !find_kernel(key4(hpe, hpp, false, ef)));
  h->plan = plan;
  return GAUDI_OK;
}

static void fill_edm(gaudi_handle* h, KParams& P) {
  const gaudi_edm_config& c = h->ecfg;
  P.F = c.in_node_nf;
  P.T = c.diffusion_steps;
  P.edm.w = (h->variant == 8 && h->plan.waves == 4) ? h->edm_w4.as<float>() : h->edm_w.as<float>();
  P.edm.w_bytes = (unsigned)h->edm_w_bytes;
  P.edm.F = c.in_node_nf;
  P.edm.L = c.n_layers;
  P.edm.S = c.inv_sublayers;
  P.edm.attention = c.attention;
  P.edm.use_tanh = c.tanh;
  P.edm.coords_range = c.coords_range;
  P.edm.norm_constant = c.norm_constant;
  // aggregation_method 'mean' (normalization_factor = 0 in the config): unsorted_segment_sum divides by the number of edges of
  // the dense list that share the row, masked ones included (egnn_new.py:416-420) = the call's padded node count
  P.edm.normf = c.normalization_factor > 0.f ? c.normalization_factor : (float)P.NR;
  P.edm.ktail = h->plan.waves == 8 && has_ktail(c.hidden_nf, h->HPE);
  P.edm.ws = h->edm_ws.as<float>();
  P.edm.ws_bytes = (unsigned)h->edm_ws_bytes;
  P.edm.hinv = h->edm_hinv;
  P.coef = h->coef_d.as<float>();
  const float g0 = h->gamma[0];
  P.alpha0 = sqrtf(sigmoid_host(-g0));
  P.sigma0 = sqrtf(sigmoid_host(g0));
  P.sigma_x = expf(0.5f * g0);  // SNR(-0.5*gamma_0), en_diffusion.py:538
  P.nv0 = c.norm_values[0];
  P.nv1 = c.norm_values[1];
}

// -------------------------------------------------------------------------------------------------
extern "C" {

int gaudi_create(int device, gaudi_handle** out) {
  if (!out) return GAUDI_E_INVALID;
  *out = nullptr;
  static const std::string dup = duplicate_kernel_key();
  if (!dup.empty()) {
    fprintf(stderr, "libgaudi_hip: two translation units register the kernel %s\n", dup.c_str());
    return GAUDI_E_INVALID;
  }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return GAUDI_E_HIP;
  gaudi_handle* h = new gaudi_handle();
  h->device = device;
  if (const char* v = getenv("GAUDI_WAVES")) h->variant = atoi(v) == 4 ? 4 : 8;
  if (const char* v = getenv("GAUDI_EDGE_MATH")) h->split = std::string(v) != "fp32";
  if (const char* v = getenv("GAUDI_FORCE_GN")) h->force_gn = atoi(v) != 0;
  if (const char* v = getenv("GAUDI_GN8")) h->gn8 = atoi(v) != 0;
  if (const char* v = getenv("GAUDI_FORCE_GN8")) h->force_gn8 = atoi(v) != 0;
  if (const char* v = getenv("GAUDI_FORCE_MR")) h->force_mr = atoi(v) != 0;  // diagnostic: one-round graphs on the MR kernels
  if (const char* v = getenv("GAUDI_PACK")) h->pack = atoi(v) != 0;
  if (const char* v = getenv("GAUDI_GN8_PACK")) h->gn8_pack = atoi(v) != 0;
  if (const char* v = getenv("GAUDI_GN8_PQ")) h->gn8_pq = atoi(v) != 0;
  if (const char* v = getenv("GAUDI_WIDE_FULL")) h->wide_full = atoi(v) != 0;
  if (const char* v = getenv("GAUDI_KEEP_H")) h->keep_h = atoi(v) != 0;
  if (const char* v = getenv("GAUDI_FAMILY_SPLIT")) h->family_split = atoi(v) != 0;
  if (const char* v = getenv("GAUDI_PAIRS")) h->pairs = atoi(v);
  if (const char* v = getenv("GAUDI_PAIRS_CAP")) h->pairs_cap = atoi(v);
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) h->num_cus = cus;
  }
  if (const char* v = getenv("GAUDI_PRED_ROUNDS")) h->pred_rounds = atoi(v) != 0;
  h->no_fr = getenv("GAUDI_NO_FR") != nullptr;
  h->no_n1 = getenv("GAUDI_NO_N1") != nullptr;
  h->no_side = getenv("GAUDI_NO_SIDE") != nullptr;
  h->plan.waves = h->variant;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return GAUDI_E_HIP;
  }
  *out = h;
  return GAUDI_OK;
}

void gaudi_destroy(gaudi_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->prof_log.reset(true);
  h->stab_log.reset(true);
  h->atoms_log.reset(true);
  h->rings_log.reset(true);
  h->bonds_log.reset(true);
  h->canon_log.reset(true);
  h->fp_log.reset(true);
  h->sub_log.reset(true);
  h->huckel_log.reset(true);
  h->ppp_log.reset(true);
  h->ppp_cis_log.reset(true);
  h->ppp_open_log.reset(true);
  h->ppp_scf_log.reset(true);
  h->kekule_log.reset(true);
  h->ring_log.reset(true);
  h->react_log.reset(true);
  DevBuf* bufs[] = {&h->edm_w, &h->pred_w, &h->coef_d, &h->edm_w4, &h->pred_w4, &h->edm_ws, &h->pred_ws, &h->d_mask, &h->d_order, &h->d_edges, &h->d_emask, &h->d_npairs,
                    &h->d_seg, &h->d_zin, &h->d_zout, &h->d_t, &h->d_x, &h->d_h, &h->d_noise, &h->d_nan, &h->d_dpred,
                    &h->d_pred, &h->d_tw, &h->d_stash, &h->d_chain, &h->d_sx, &h->d_stype, &h->d_sn,
                    &h->d_sflags, &h->d_sdist, &h->d_sadj, &h->d_saux, &h->d_stab, &h->d_as, &h->d_ncols, &h->d_soff, &h->d_sidx,
                    &h->d_gnode, &h->d_rowmap, &h->d_compmol, &h->d_ncomp, &h->d_gcoef, &h->d_gidx, &h->d_zt, &h->d_vtpar, &h->d_vttrace, &h->d_vtdev};
  for (DevBuf* b : bufs) b->release();
  for (DevBuf& b : h->d_atoms) b.release();
  for (DevBuf& b : h->d_rings) b.release();
  for (DevBuf& b : h->d_bonds) b.release();
  for (DevBuf& b : h->d_canon) b.release();
  for (DevBuf& b : h->d_fp) b.release();
  for (DevBuf& b : h->d_fps) b.release();
  for (DevBuf& b : h->d_sub) b.release();
  for (DevBuf& b : h->d_huckel) b.release();
  for (DevBuf& b : h->d_ppp) b.release();
  for (DevBuf& b : h->d_ppp_open) b.release();
  for (DevBuf& b : h->d_ppp_scf) b.release();
  for (DevBuf& b : h->d_kekule) b.release();
  for (DevBuf& b : h->d_ring) b.release();
  for (DevBuf& b : h->d_react) b.release();
  pt_release(h);
  et_release(h);
  h->p_pred.release();
  h->p_dpred.release();
  h->p_z.release();
  h->p_dz.release();
  h->d_dz.release();
  if (h->cb_event) (void)hipEventDestroy(h->cb_event);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

const char* gaudi_last_error(const gaudi_handle* h) { return h ? h->err.c_str() : "null handle"; }
const char* gaudi_last_warning(const gaudi_handle* h) { return h ? h->warn.c_str() : ""; }
int gaudi_last_kernel_key(const gaudi_handle* h, char* buf, int n) {
  if (!h || !buf || n <= 0) return GAUDI_E_INVALID;
  snprintf(buf, (size_t)n, "%s", h->last_key.c_str());
  return GAUDI_OK;
}
// names, one per line, cut to n bytes (NUL-terminated); returns the bytes the whole text needs, its NUL included
static int copy_lines(const std::vector<std::string>& names, char* buf, int n) {
  std::string all;
  for (const std::string& s : names) all += s + "\n";
  if (buf && n > 0) snprintf(buf, (size_t)n, "%s", all.c_str());
  return (int)all.size() + 1;
}
int gaudi_host_kernel_keys(char* buf, int n) {
  if (n < 0) return GAUDI_E_INVALID;
  std::vector<std::string> names;
  for (const KernelTable* t = g_kernel_tables; t; t = t->next)
    for (int i = 0; i < t->n; ++i) names.push_back(key_name(t->entries[i].key));
  std::sort(names.begin(), names.end());  // (the tables link in load order, which means nothing)
  return copy_lines(names, buf, n);
}
int gaudi_kernel_key_log(const gaudi_handle* h, char* buf, int n) {
  if (!h || n < 0) return GAUDI_E_INVALID;
  return copy_lines(h->key_log, buf, n);
}
int gaudi_abi_version(void) { return GAUDI_ABI_VERSION; }
int gaudi_profile_clock(gaudi_handle* h, double* shader_mhz) {
  if (!h || !shader_mhz) return GAUDI_E_INVALID;
  *shader_mhz = 0.0;
  if (!h->d_clock.p) return GAUDI_OK;  // no profiled launch yet
  HIPCHECK(h, hipSetDevice(h->device));
  unsigned long long c[4] = {0, 0, 0, 0};
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, hipMemcpy(c, h->d_clock.p, sizeof(c), hipMemcpyDeviceToHost));
  if (c[3] > c[1] && c[2] > c[0]) *shader_mhz = 100.0 * (double)(c[2] - c[0]) / (double)(c[3] - c[1]);
  return GAUDI_OK;
}
int gaudi_last_keep_h(const gaudi_handle* h, int32_t* lds_floats) {
  if (!h || !lds_floats) return GAUDI_E_INVALID;
  *lds_floats = h->plan.hk;
  return GAUDI_OK;
}
int gaudi_last_family_split(const gaudi_handle* h, int32_t* resident_molecules) {
  if (!h || !resident_molecules) return GAUDI_E_INVALID;
  *resident_molecules = h->last_split_resident;
  return GAUDI_OK;
}

int gaudi_load_edm(gaudi_handle* h, const gaudi_edm_config* cfg, int n, const char* const* names,
                   const float* const* tensors, const int64_t* numel) {
  if (!h || !cfg) return GAUDI_E_INVALID;
  HIPCHECK(h, hipSetDevice(h->device));
  const int H = cfg->hidden_nf, F = cfg->in_node_nf, F1 = F + 1, L = cfg->n_layers, S = cfg->inv_sublayers;
  if (H <= 0 || H > 256) return fail(h, GAUDI_E_INVALID, "hidden_nf must be in 1..256");
  if (F < 1 || F > 15) return fail(h, GAUDI_E_INVALID, "in_node_nf must be in 1..15");
  if (L < 1 || S < 1 || cfg->diffusion_steps < 1) return fail(h, GAUDI_E_INVALID, "bad n_layers/inv_sublayers/diffusion_steps");
  if (!(cfg->normalization_factor >= 0.f)) return fail(h, GAUDI_E_INVALID, "normalization_factor must be > 0 (or 0: 'mean' aggregation)");
  const int HP = round_hidden(H);
  if (!HP) return fail(h, GAUDI_E_INVALID, "no kernel instantiated for this hidden size");
  Tensors T;
  for (int i = 0; i < n; ++i) T.m[names[i]] = {tensors[i], numel[i]};
  const int EF = cfg->sin_embedding ? 24 : 2;  // edge_feat_nf (egnn_new.py:269-273): 2 x 12 sinusoids of (r, d0), or the two scalars
  EdmLayout lay{HP, F1, L, S, EF};
  const std::string p = "dynamics.egnn.";
  const int PK = HP * HP;
  // tile layout: lane-linear for the 8-wave kernels, row-major for the 4-wave ones (kept as the fallback of the 8-wave
  // variant for graphs that do not fit it)
  // the exponent of the fp16-pair node images: every node-GEMM matrix of the network (the A | B column blocks of W1, Wn1, Wn2)
  float hscale = 0.f;
  {
    NodeScale ns;
    for (int l = 0; l < L; ++l) {
      for (int s = 0; s <= S; ++s) {
        const std::string q = p + "e_block_" + std::to_string(l) + (s < S ? ".gcl_" + std::to_string(s) + "." : ".gcl_equiv.");
        ns.see(T.peek(q + (s < S ? "edge_mlp.0.weight" : "coord_mlp.0.weight"), (int64_t)H * (2 * H + EF)), H, 2 * H + EF, 0, 2 * H);
        ns.see(T.peek(q + (s < S ? "edge_mlp.2.weight" : "coord_mlp.2.weight"), (int64_t)H * H), H, H, 0, H, true);
        if (s < S) {
          ns.see(T.peek(q + "node_mlp.0.weight", (int64_t)H * 2 * H), H, 2 * H, 0, 2 * H);
          ns.see(T.peek(q + "node_mlp.2.weight", (int64_t)H * H), H, H, 0, H);
        }
      }
    }
    hscale = ns.scale();
    if (!(hscale > 0.f) && h->variant == 8 && h->split && EF == 2)
      h->warn = std::string("EDM weights: the fp16-pair images cannot carry this weight set (") + ns.why() +
                "): its calls run the fp32-instruction kernels (about 0.55 x the speed, same results at fp32 accuracy)";
  }
  auto pack = [&](bool lane_linear, std::vector<float>& w, std::vector<float>* ws) {
  w.assign((size_t)lay.total(), 0.f);
  if (ws) ws->assign(2 * (size_t)lay.total(), 0.f);
  // only the matrices of the edge-level GEMMs carry the K tail: pe packs those, pn the node-level ones
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
    const float* ow = T.get(p + "embedding_out.weight", (int64_t)F1 * H);
    const float* ob = T.get(p + "embedding_out.bias", F1);
    if (ew && eb && ow && ob) {
      for (int f = 0; f < H; ++f)
        for (int k = 0; k < F1; ++k) w[lay.emb_w() + f * F1 + k] = ew[f * F1 + k];
      pack_vec(&w[lay.emb_b()], eb, H);
      for (int o = 0; o < F1; ++o)
        for (int k = 0; k < H; ++k) w[lay.out_w() + o * HP + k] = ow[o * H + k];
      pack_vec(&w[lay.out_b()], ob, F1);
    }
  }
  const int ld1 = 2 * H + EF;
  for (int l = 0; l < L; ++l) {
    for (int s = 0; s < S; ++s) {
      const std::string q = p + "e_block_" + std::to_string(l) + ".gcl_" + std::to_string(s) + ".";
      float* G = &w[lay.gcl(l, s)];
      float* V = G + 6 * PK;
      const float* W1 = T.get(q + "edge_mlp.0.weight", (int64_t)H * ld1);
      const float* b1 = T.get(q + "edge_mlp.0.bias", H);
      const float* W2 = T.get(q + "edge_mlp.2.weight", (int64_t)H * H);
      const float* b2 = T.get(q + "edge_mlp.2.bias", H);
      const float* Wn1 = T.get(q + "node_mlp.0.weight", (int64_t)H * 2 * H);
      const float* bn1 = T.get(q + "node_mlp.0.bias", H);
      const float* Wn2 = T.get(q + "node_mlp.2.weight", (int64_t)H * H);
      const float* bn2 = T.get(q + "node_mlp.2.bias", H);
      const float *wa = nullptr, *ba = nullptr;
      if (cfg->attention) {
        wa = T.get(q + "att_mlp.0.weight", H);
        ba = T.get(q + "att_mlp.0.bias", 1);
      }
      if (!(W1 && b1 && W2 && b2 && Wn1 && bn1 && Wn2 && bn2) || (cfg->attention && !(wa && ba))) continue;
      pack_node_matrix(pn, G, W1, H, ld1, 0, HP);
      pack_node_matrix(pn, G + PK, W1, H, ld1, H, HP);
      pack_edge_matrix(pe, G + 2 * PK, W2, H, H, 0, HP);
      pack_node_matrix(pn, G + 3 * PK, Wn1, H, 2 * H, 0, HP);
      pack_node_matrix(pn, G + 4 * PK, Wn1, H, 2 * H, H, HP);
      pack_node_matrix(pn, G + 5 * PK, Wn2, H, H, 0, HP);
      for (int k = 0; k < EF; ++k) pack_col(V + k * HP, W1, H, ld1, 2 * H + k);  // c_r, c_d (or the 24 sinusoid columns)
      pack_vec(V + EF * HP, b1, H);
      pack_vec(V + (EF + 1) * HP, b2, H);
      if (wa) pack_vec(V + (EF + 2) * HP, wa, H);
      pack_vec(V + (EF + 3) * HP, bn1, H);
      pack_vec(V + (EF + 4) * HP, bn2, H);
      if (ba) V[(EF + 5) * HP] = ba[0];
      V[(EF + 5) * HP + 1] = col_absmax(W1, H, ld1, 2 * H);      // max |c_r|, max |c_d|: the split edge GEMMs' column scales are
      V[(EF + 5) * HP + 2] = col_absmax(W1, H, ld1, 2 * H + 1);  // bounded with them (w8_split.h; EF = 2 only)
    }
    const std::string q = p + "e_block_" + std::to_string(l) + ".gcl_equiv.";
    float* E = &w[lay.equ(l)];
    float* V = E + 3 * PK;
    const float* W1 = T.get(q + "coord_mlp.0.weight", (int64_t)H * ld1);
    const float* b1 = T.get(q + "coord_mlp.0.bias", H);
    const float* W2 = T.get(q + "coord_mlp.2.weight", (int64_t)H * H);
    const float* b2 = T.get(q + "coord_mlp.2.bias", H);
    const float* w3 = T.get(q + "coord_mlp.4.weight", H);
    if (!(W1 && b1 && W2 && b2 && w3)) continue;
    pack_node_matrix(pn, E, W1, H, ld1, 0, HP);
    pack_node_matrix(pn, E + PK, W1, H, ld1, H, HP);
    pack_edge_matrix(pe, E + 2 * PK, W2, H, H, 0, HP);
    for (int k = 0; k < EF; ++k) pack_col(V + k * HP, W1, H, ld1, 2 * H + k);
    pack_vec(V + EF * HP, b1, H);
    pack_vec(V + (EF + 1) * HP, b2, H);
    pack_vec(V + (EF + 2) * HP, w3, H);
    V[(EF + 3) * HP] = col_absmax(W1, H, ld1, 2 * H);
    V[(EF + 3) * HP + 1] = col_absmax(W1, H, ld1, 2 * H + 1);
  }
  };
  std::vector<float> w, ws;
  // a sin_embedding denoiser only ever runs on the 4-wave kernels (stage_graph): no fp16-pair images, and the row-major pack twice
  const bool want_split = h->variant == 8 && h->split && EF == 2;
  pack(h->variant == 8 && EF == 2, w, want_split ? &ws : nullptr);
  if (!T.missing.empty()) return fail(h, GAUDI_E_MISSING, "EDM checkpoint tensor missing or mis-shaped: " + T.missing);
  if (const char* bad = et_check(cfg, n, names, numel))  // the training copy's table, before anything is replaced
    return fail(h, GAUDI_E_MISSING, std::string("EDM tensor mis-shaped: ") + bad);
  HIPCHECK(h, h->edm_w.reserve(sizeof(float) * w.size()));
  HIPCHECK(h, hipMemcpy(h->edm_w.p, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice));
  h->edm_w_bytes = sizeof(float) * w.size();
  h->edm_ws_bytes = 0;
  if (want_split) {
    HIPCHECK(h, h->edm_ws.reserve(sizeof(float) * ws.size()));
    HIPCHECK(h, hipMemcpy(h->edm_ws.p, ws.data(), sizeof(float) * ws.size(), hipMemcpyHostToDevice));
    h->edm_ws_bytes = sizeof(float) * ws.size();
  }
  h->edm_hinv = want_split && hscale > 0.f ? 1.0f / hscale : 0.f;
  if (h->variant == 8) {
    pack(false, w, nullptr);
    HIPCHECK(h, h->edm_w4.reserve(sizeof(float) * w.size()));
    HIPCHECK(h, hipMemcpy(h->edm_w4.p, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice));
  }
  h->gamma = make_gamma(cfg->diffusion_steps, cfg->noise_power, cfg->noise_precision);
  make_coef(h->gamma, cfg->diffusion_steps, h->coef);
  HIPCHECK(h, h->coef_d.reserve(sizeof(float) * h->coef.size()));
  HIPCHECK(h, hipMemcpy(h->coef_d.p, h->coef.data(), sizeof(float) * h->coef.size(), hipMemcpyHostToDevice));
  h->ecfg = *cfg;
  h->HPE = HP;
  h->has_edm = true;
  h->edm_stale = false;
  // the torch-layout copy of the training kernels (edm_train_host.inc): both copies now hold these weights
  const int rc_train = et_upload(h, cfg, n, names, tensors, numel);
  if (rc_train) {  // (an upload error: no half-loaded handle)
    h->has_edm = false;
    return rc_train;
  }
  return GAUDI_OK;
}

int gaudi_get_gamma(gaudi_handle* h, float* gamma_out) {
  if (!h || !gamma_out) return GAUDI_E_INVALID;
  if (!h->has_edm) return fail(h, GAUDI_E_STATE, "EDM weights not loaded");
  std::memcpy(gamma_out, h->gamma.data(), sizeof(float) * h->gamma.size());
  return GAUDI_OK;
}

int gaudi_get_step_coefficients(gaudi_handle* h, float* coef_out) {
  if (!h || !coef_out) return GAUDI_E_INVALID;
  if (!h->has_edm) return fail(h, GAUDI_E_STATE, "EDM weights not loaded");
  std::memcpy(coef_out, h->coef.data(), sizeof(float) * h->coef.size());
  return GAUDI_OK;
}

int gaudi_phi(gaudi_handle* h, int B, int N, const float* z, const float* t, const float* node_mask,
              const float* edge_mask, float* eps_out) {
  if (!h || !z || !t || !node_mask || !edge_mask || !eps_out) return GAUDI_E_INVALID;
  if (!h->has_edm) return fail(h, GAUDI_E_STATE, "EDM weights not loaded");
  if (h->edm_stale) return fail(h, GAUDI_E_STATE, kEdmStale);
  HIPCHECK(h, hipSetDevice(h->device));
  KParams P{};
  int rc = stage_graph(h, B, N, node_mask, edge_mask, P, h->HPE, 0, CallHints{});
  if (rc) return rc;
  fill_edm(h, P);
  const size_t zb = sizeof(float) * B * N * (3 + P.F);
  HIPCHECK(h, h->d_zin.reserve(zb));
  HIPCHECK(h, h->d_zout.reserve(zb));
  HIPCHECK(h, h->d_t.reserve(sizeof(float) * B));
  HIPCHECK(h, hipMemcpyAsync(h->d_zin.p, z, zb, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(h->d_t.p, t, sizeof(float) * B, hipMemcpyHostToDevice, h->stream));
  P.mode = MODE_PHI;
  P.z_in = h->d_zin.as<float>();
  P.z_out = h->d_zout.as<float>();
  P.t_in = h->d_t.as<float>();
  rc = launch(h, P, h->HPE, 0, 0);
  if (rc) return rc;
  HIPCHECK(h, hipMemcpyAsync(eps_out, h->d_zout.p, zb, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  return GAUDI_OK;
}

__global__ void philox_kernel(unsigned long long seed, long long sample_offset, int B, int n_elem, int draw0, int n_draws,
                              float* out) {
  const long long total = (long long)n_draws * B * n_elem;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int e = (int)(i % n_elem);
    const int b = (int)((i / n_elem) % B);
    const int dr = (int)(i / ((long long)n_elem * B));
    const f4 v = philox_normal4(seed, (uint64_t)(sample_offset + b), (uint32_t)(draw0 + dr), (uint32_t)(e >> 2));
    out[i] = v[e & 3];
  }
}

int gaudi_philox_normal(gaudi_handle* h, uint64_t seed, int64_t sample_offset, int B, int n_elem, int draw0, int n_draws,
                        float* out) {
  if (!h || !out || B <= 0 || n_elem <= 0 || n_draws <= 0) return GAUDI_E_INVALID;
  HIPCHECK(h, hipSetDevice(h->device));
  const size_t bytes = sizeof(float) * (size_t)B * n_elem * n_draws;
  HIPCHECK(h, h->d_noise.reserve(bytes));
  hipLaunchKernelGGL(philox_kernel, dim3(256), dim3(256), 0, h->stream, seed, sample_offset, B, n_elem, draw0, n_draws,
                     h->d_noise.as<float>());
  HIPCHECK(h, hipGetLastError());
  HIPCHECK(h, hipMemcpyAsync(out, h->d_noise.p, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  return GAUDI_OK;
}

// ---- device-free entry points: the host logic of the library, callable (and tested) without a GPU
int gaudi_host_schedule(int T, float noise_power, float noise_precision, float* gamma_out, float* coef_out) {
  if (T < 1 || !gamma_out || !(noise_power >= 0.f)) return GAUDI_E_INVALID;
  const std::vector<float> g = make_gamma(T, noise_power, noise_precision);
  std::memcpy(gamma_out, g.data(), sizeof(float) * g.size());
  if (coef_out) {
    std::vector<float> c;
    make_coef(g, T, c);
    std::memcpy(coef_out, c.data(), sizeof(float) * c.size());
  }
  return GAUDI_OK;
}

int gaudi_host_grid_coefficients(int T, float noise_power, float noise_precision, int n_grid, const int32_t* grid, float* coef_out,
                                 int32_t* land_out) {
  if (T < 1 || !coef_out || grid_check(T, n_grid, grid)) return GAUDI_E_INVALID;
  GridPlan gp;
  make_grid_plan(make_gamma(T, noise_power, noise_precision), T, n_grid, grid, gp);
  for (int k = 0; k < gp.rows; ++k) {  // step order: row k = the step g[k] -> g[k + 1]
    std::memcpy(coef_out + 4 * k, &gp.coef[4 * (size_t)(gp.rows - 1 - k)], sizeof(float) * 4);
    if (land_out) land_out[k] = gp.idx[gp.rows - 1 - k];
  }
  return GAUDI_OK;
}

int gaudi_host_graph_meta(int B, int N, const float* node_mask, const float* edge_mask, int32_t* ew_out,
                          int32_t* order_out, int32_t* npairs_out, uint32_t* seg_out, uint32_t* edges_out,
                          float* emask_out, int32_t edges_capacity, int32_t* ncols_out) {
  if (B <= 0 || N <= 0 || !edge_mask || !ew_out) return GAUDI_E_INVALID;
  Meta M;
  std::string err;
  const int rc = build_meta(B, N, node_mask, edge_mask, M, err);
  if (rc) return rc;
  *ew_out = M.EW;
  if (order_out) std::memcpy(order_out, M.order.data(), sizeof(int) * B);
  if (npairs_out) std::memcpy(npairs_out, M.npairs.data(), sizeof(int) * B * kWaves);
  if (seg_out) std::memcpy(seg_out, M.seg.data(), sizeof(uint32_t) * B * N);
  if (ncols_out) std::memcpy(ncols_out, M.ncols.data(), sizeof(int) * B);
  if (edges_out || emask_out) {
    if ((size_t)edges_capacity < M.edges.size()) return GAUDI_E_CAPACITY;
    if (edges_out) std::memcpy(edges_out, M.edges.data(), sizeof(uint32_t) * M.edges.size());
    if (emask_out) std::memcpy(emask_out, M.emask.data(), sizeof(float) * M.emask.size());
  }
  return GAUDI_OK;
}

int gaudi_host_graph_meta8(int B, int N, const float* node_mask, const float* edge_mask, int32_t* slots_out,
                           int32_t* order_out, int32_t* ntiles_out, uint32_t* seg_out, uint32_t* edges_out, float* emask_out,
                           uint16_t* soff_out, uint16_t* sidx_out, int32_t edges_capacity, int32_t* ncols_out) {
  if (B <= 0 || N <= 0 || !edge_mask || !slots_out) return GAUDI_E_INVALID;
  Meta8 M;
  std::string err;
  const int rc = build_meta8(B, N, node_mask, edge_mask, M, err);
  if (rc) return rc;
  *slots_out = M.S;
  if (order_out) std::memcpy(order_out, M.order.data(), sizeof(int) * B);
  if (ntiles_out) std::memcpy(ntiles_out, M.ntiles.data(), sizeof(int) * B);
  if (seg_out) std::memcpy(seg_out, M.seg.data(), sizeof(uint32_t) * B * N);
  if (ncols_out) std::memcpy(ncols_out, M.ncols.data(), sizeof(int) * B);
  if (soff_out) std::memcpy(soff_out, M.soff.data(), sizeof(uint16_t) * M.soff.size());
  if (edges_out || emask_out || sidx_out) {
    if ((size_t)edges_capacity < M.edges.size()) return GAUDI_E_CAPACITY;
    if (edges_out) std::memcpy(edges_out, M.edges.data(), sizeof(uint32_t) * M.edges.size());
    if (emask_out) std::memcpy(emask_out, M.emask.data(), sizeof(float) * M.emask.size());
    if (sidx_out) std::memcpy(sidx_out, M.sidx.data(), sizeof(uint16_t) * M.sidx.size());
  }
  return GAUDI_OK;
}

int gaudi_host_pack_plan(int B, int N, const float* node_mask, const float* edge_mask, int32_t* groups_out, int32_t* group_of_out,
                         int32_t* ntiles_out, int32_t* ncols_out) {
  if (B <= 0 || N <= 0 || !node_mask || !edge_mask || !groups_out) return GAUDI_E_INVALID;
  Meta8 M;
  std::string err;
  int rc = build_meta8(B, N, node_mask, edge_mask, M, err);
  if (rc) return rc;
  Pack pk;
  pack_groups(B, N, node_mask, edge_mask, M, pk);
  Meta8 M2;
  rc = build_meta8(pk.G, N, pk.umask.data(), pk.uemask.data(), M2, err, M.S, pk.align.data());
  if (rc) return rc;
  *groups_out = pk.G;
  for (int g = 0; g < pk.G; ++g) {
    if (ntiles_out) ntiles_out[g] = M2.ntiles[g];
    if (ncols_out) ncols_out[g] = M2.ncols[g];
    if (group_of_out)
      for (int k = 0; k < pk.ncomp[g]; ++k) group_of_out[pk.compmol[(size_t)g * kMaxComp + k]] = g;
  }
  return GAUDI_OK;
}

int gaudi_host_pack_plan_wide(int B, int N, int node_slots, int tiles, const float* node_mask, const float* edge_mask,
                              int32_t* groups_out, int32_t* group_of_out, int32_t* ntiles_out, int32_t* ncols_out) {
  if (B <= 0 || N <= 0 || node_slots < N || node_slots > 255 || tiles < 1 || !node_mask || !edge_mask || !groups_out) return GAUDI_E_INVALID;
  Meta8 M;
  std::string err;
  int rc = build_meta8(B, N, node_mask, edge_mask, M, err);
  if (rc) return rc;
  Pack pk;
  pack_groups(B, N, node_mask, edge_mask, M, pk, node_slots, tiles);
  Meta8 M2;
  rc = build_meta8(pk.G, node_slots, pk.umask.data(), pk.uemask.data(), M2, err, 0, pk.align.data());
  if (rc) return rc;
  *groups_out = pk.G;
  for (int g = 0; g < pk.G; ++g) {
    if (ntiles_out) ntiles_out[g] = M2.ntiles[g];
    if (ncols_out) ncols_out[g] = M2.ncols[g];
    if (group_of_out)
      for (int k = 0; k < pk.ncomp[g]; ++k) group_of_out[pk.compmol[(size_t)g * kMaxComp + k]] = g;
  }
  return GAUDI_OK;
}

int gaudi_kernel_variant(const gaudi_handle* h, int32_t* configured, int32_t* last_call) {
  if (!h) return GAUDI_E_INVALID;
  if (configured) *configured = h->variant;
  if (last_call) *last_call = h->plan.waves;
  return GAUDI_OK;
}

int gaudi_last_workgroups(const gaudi_handle* h, int32_t* workgroups, int32_t* node_slots) {
  if (!h || !workgroups) return GAUDI_E_INVALID;
  *workgroups = h->plan.groups;
  if (node_slots) *node_slots = h->plan.nslots;
  return GAUDI_OK;
}

int gaudi_node_buffers(const gaudi_handle* h, int32_t* last_call) {
  if (!h || !last_call) return GAUDI_E_INVALID;
  *last_call = (int32_t)h->plan.nodes;
  return GAUDI_OK;
}

int gaudi_edge_math(const gaudi_handle* h, int32_t* configured, int32_t* last_call) {
  if (!h) return GAUDI_E_INVALID;
  if (configured) *configured = (h->variant == 8 && h->split) ? 1 : 0;
  if (last_call) *last_call = h->plan.ring;
  return GAUDI_OK;
}

int gaudi_set_plan_hint(gaudi_handle* h, int32_t min_slots, int32_t force_waves) {
  if (!h || min_slots < 0 || (force_waves != 0 && force_waves != 4)) return GAUDI_E_INVALID;
  h->plan_min_slots = min_slots;
  h->plan_force_waves = force_waves;
  return GAUDI_OK;
}

int gaudi_host_pack_matrix(int H, int ldw, int col0, int HP, int transpose, const float* W, float* packed_out) {
  if (H < 1 || HP < H || HP % 16 || !W || !packed_out) return GAUDI_E_INVALID;
  std::memset(packed_out, 0, sizeof(float) * (size_t)HP * HP);
  pack_matrix(PackMode{}, packed_out, W, H, ldw, col0, HP, transpose != 0);
  return GAUDI_OK;
}

int gaudi_host_pack_matrix_split(int H, int ldw, int col0, int HP, int transpose, int ktail, float scale, const float* W,
                                 float* packed_out) {
  if (H < 1 || HP < H || HP % 16 || !W || !packed_out || !(scale > 0.f)) return GAUDI_E_INVALID;
  const int T = HP / 16;
  std::memset(packed_out, 0, sizeof(float) * (size_t)((T + 1) / 2) * T * w8::kPieces * 256);
  PackMode pm;
  pm.lane_linear = true;
  pm.ktail = ktail != 0 && has_ktail(H, HP);
  pm.hscale = scale;
  pack_matrix_split(pm, packed_out, W, H, ldw, col0, HP, transpose != 0);
  return GAUDI_OK;
}

int gaudi_host_pack_matrix_f16(int H, int ldw, int col0, int HP, int transpose, float scale, const float* W, float* packed_out) {
  if (H < 1 || HP < H || HP % 16 || !W || !packed_out || !(scale > 0.f)) return GAUDI_E_INVALID;
  std::memset(packed_out, 0, sizeof(float) * (size_t)HP * HP);
  pack_matrix_f16(packed_out, W, H, ldw, col0, HP, transpose != 0, scale);
  return GAUDI_OK;
}

int gaudi_host_weight_scale(int n, const float* const* blocks, const int32_t* rows, const int32_t* cols, const int32_t* ldw,
                            float* scale_out) {
  if (n < 1 || !blocks || !rows || !cols || !ldw || !scale_out) return GAUDI_E_INVALID;
  NodeScale ns;
  for (int i = 0; i < n; ++i) ns.see(blocks[i], rows[i], ldw[i], 0, cols[i], true);  // (as edge-level matrices: the stricter floor)
  *scale_out = ns.scale();
  return GAUDI_OK;
}

int gaudi_host_node_operand_offset(int column_tiles, int chunk, int tile, int c, int g, int32_t* float_offset_out) {
  if (column_tiles < 1 || column_tiles > 3 || chunk < 0 || tile < 0 || tile >= column_tiles || c < 0 || c > 15 || g < 0 || g > 3 || !float_offset_out)
    return GAUDI_E_INVALID;
  *float_offset_out = chunk * w8::nh_chunk_stride(column_tiles) + tile * 512 + w8::nh_bpos(c, g);
  return GAUDI_OK;
}

int gaudi_profile_reset(gaudi_handle* h, int enable) {
  if (!h) return GAUDI_E_INVALID;
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->prof_log.reset(false);
  h->stab_log.reset(false);
  h->atoms_log.reset(false);
  h->rings_log.reset(false);
  h->bonds_log.reset(false);
  h->canon_log.reset(false);
  h->fp_log.reset(false);
  h->sub_log.reset(false);
  h->huckel_log.reset(false);
  h->ppp_log.reset(false);
  h->ppp_cis_log.reset(false);
  h->ppp_open_log.reset(false);
  h->ppp_scf_log.reset(false);
  h->kekule_log.reset(false);
  h->ring_log.reset(false);
  h->react_log.reset(false);
  h->prof_steps = 0;
  h->prof = enable != 0;
  return GAUDI_OK;
}

int gaudi_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms, int64_t* steps_done) {
  if (!h) return GAUDI_E_INVALID;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, h->prof_log.fold(0));
  if (n_launches) *n_launches = (int32_t)h->prof_log.n;
  if (total_ms) *total_ms = h->prof_log.ms;
  if (steps_done) *steps_done = h->prof_steps;
  return GAUDI_OK;
}

int gaudi_set_fix_noise(gaudi_handle* h, int enable, int64_t key_sample) {
  if (!h) return GAUDI_E_INVALID;
  h->fix_noise = enable != 0;
  h->fix_key = key_sample;
  return GAUDI_OK;
}

int gaudi_set_steps_per_launch(gaudi_handle* h, int steps) {
  if (!h || steps < 1) return GAUDI_E_INVALID;
  h->steps_per_launch = steps;
  return GAUDI_OK;
}

}  // extern "C"

#include "pred_host.inc"
#include "chain_host.inc"
#include "train_host.inc"
#include "pred_train_host.inc"
#include "stability.inc"
#include "atoms.inc"
#include "rings.inc"
#include "bonds.inc"
#include "canon.inc"
#include "fp.inc"
#include "fp_select.inc"
#include "sub.inc"
#include "huckel.inc"
#include "ppp.inc"
#include "ppp_open.inc"
#include "ppp_scf.inc"
#include "ppp_cis.inc"
#include "kekule.inc"
#include "ring_current.inc"
#include "reactivity.inc"
#include "nll_host.inc"
#include "edm_train_host.inc"
