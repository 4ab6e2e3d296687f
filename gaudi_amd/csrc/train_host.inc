// train_host.inc -- what the two training halves of the C ABI share (included in gaudi_hip.hip before pred_train_host.inc and
// edm_train_host.inc): the weights in torch layout and their upload, the role-table layout, the chunk scratch carver, the plan
// of weight-gradient products and the copy-out of the gradient.  train_device.h describes the buffers and the kernels' pieces.
#include "train_device.h"

// the network in torch layout for the training kernels, and the buffers every gradient call reuses
struct TrainState {
  std::vector<std::string> names;     // the names passed to the loader, in order
  std::vector<int64_t> numel, start;  // per tensor
  std::vector<int32_t> has_grad;
  std::vector<int> off;               // float offset per role (-1 absent)
  int64_t total = 0;
  DevBuf w, wt, doff, grad, scratch, jobs, tiles;
  void release() {
    DevBuf* bufs[] = {&w, &wt, &doff, &grad, &scratch, &jobs, &tiles};
    for (DevBuf* b : bufs) b->release();
  }
};

// one row of a network's name -> role table: the tensor `name` is a [rows][cols] matrix (cols 1: a vector) at `slot`
struct TrainRole {
  int slot;
  std::string name;
  int rows, cols;
  bool grad;  // has a gradient path
};

// Host only: start / off / has_grad per tensor from a role table, and wt = the flat buffer with every matrix transposed
// (NULL: skip).  Returns 0, or the name of a tensor whose size does not match its role.
static const char* tr_layout(const std::vector<TrainRole>& roles, int n_slots, int n, const char* const* names,
                             const float* const* tensors, const int64_t* numel, std::vector<int64_t>& start, std::vector<int>& off,
                             std::vector<int32_t>& has_grad, float* wt) {
  start.resize(n);
  has_grad.assign(n, 0);
  off.assign(n_slots, -1);
  int64_t total = 0;
  std::map<std::string, int> idx;
  for (int i = 0; i < n; ++i) {
    start[i] = total;
    total += numel[i];
    idx[names[i]] = i;
    if (wt && tensors) std::copy(tensors[i], tensors[i] + numel[i], wt + start[i]);
  }
  const char* bad = nullptr;
  for (const TrainRole& r : roles) {
    auto it = idx.find(r.name);
    if (it == idx.end()) continue;
    const int i = it->second;
    if (numel[i] != (int64_t)r.rows * r.cols) {
      if (!bad) bad = names[i];
      continue;
    }
    off[r.slot] = (int)start[i];
    has_grad[i] = r.grad;
    if (wt && tensors && r.rows > 1 && r.cols > 1)
      for (int a = 0; a < r.rows; ++a)
        for (int c = 0; c < r.cols; ++c) wt[start[i] + (int64_t)c * r.rows + a] = tensors[i][(int64_t)a * r.cols + c];
  }
  return bad;
}

// The roles of the GCL `q` that both networks have under the same names, in both enums at consecutive slots: edge_mlp and (with
// attention) att_mlp from slot e0 (E0W, E0B, E2W, E2B, AW, AB), node_mlp from slot n0 (N0W, N0B, N2W, N2B).
static void tr_edge_roles(std::vector<TrainRole>& t, const std::string& q, int H, int ld1, bool attention, int e0) {
  t.push_back({e0, q + "edge_mlp.0.weight", H, ld1, true});
  t.push_back({e0 + 1, q + "edge_mlp.0.bias", H, 1, true});
  t.push_back({e0 + 2, q + "edge_mlp.2.weight", H, H, true});
  t.push_back({e0 + 3, q + "edge_mlp.2.bias", H, 1, true});
  if (attention) {
    t.push_back({e0 + 4, q + "att_mlp.0.weight", 1, H, true});
    t.push_back({e0 + 5, q + "att_mlp.0.bias", 1, 1, true});
  }
}
static void tr_node_roles(std::vector<TrainRole>& t, const std::string& q, int H, int n0) {
  t.push_back({n0, q + "node_mlp.0.weight", H, 2 * H, true});
  t.push_back({n0 + 1, q + "node_mlp.0.bias", H, 1, true});
  t.push_back({n0 + 2, q + "node_mlp.2.weight", H, H, true});
  t.push_back({n0 + 3, q + "node_mlp.2.bias", H, 1, true});
}

// the torch-layout copy (and its transposes) the training kernels read; layout(start, off, has_grad, wt) is the network's
// pt_layout / et_layout.  Nothing of `s` changes when a tensor is mis-shaped.
template <class Layout>
static int tr_upload(gaudi_handle* h, TrainState& s, const char* what, int n, const char* const* names,
                     const float* const* tensors, const int64_t* numel, Layout layout) {
  std::vector<int64_t> start;
  std::vector<int> off;
  std::vector<int32_t> has;
  int64_t total = 0;
  for (int i = 0; i < n; ++i) total += numel[i];
  std::vector<float> w((size_t)total), wt((size_t)total);
  const char* bad = layout(start, off, has, wt.data());
  if (bad) return fail(h, GAUDI_E_MISSING, std::string(what) + " tensor mis-shaped: " + bad);
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

// The chunk scratch, carved array by array ([Bc][...] each).  Every list of arrays runs twice per call: with a null base it only
// counts the floats one molecule takes (which sizes the chunk), with the real base and Bc it hands out the pointers -- the count
// and the pointers cannot disagree.
struct Carver {
  float* base;
  int64_t bc;
  int64_t per = 0;  // floats per molecule taken so far
  float* take(int64_t n) {
    float* r = base ? base + per * bc : nullptr;
    per += n;
    return r;
  }
};

// the arrays both networks have (train_device.h: TrainBufs), from b's N, H, L: n_stash h stashes, an input of F1 columns, a
// readout gradient of Kout columns
static void tr_carve(gaudi_train::TrainBufs& b, Carver& c, int64_t n_stash, int F1, int Kout) {
  const int64_t N = b.N, H = b.H, E = N * N;
  b.hs = c.take(n_stash * N * H);
  b.xs = c.take((int64_t)(b.L + 1) * N * 4);
  b.hin = c.take(N * F1);
  float** node[] = {&b.P, &b.Q, &b.agg, &b.qp, &b.q, &b.dr, &b.dP, &b.dQ, &b.dh};
  for (float** q : node) *q = c.take(N * H);
  b.dx = c.take(4 * N);
  b.dhout = c.take(N * Kout);
  float** edge[] = {&b.U, &b.Su, &b.V, &b.M, &b.EF, &b.DE};
  for (float** q : edge) *q = c.take(E * H);
  b.diff = c.take(4 * E);
  b.dcd = c.take(4 * E);
  float** sc[] = {&b.rad, &b.gate, &b.dap, &b.phi, &b.ppre, &b.dp};
  for (float** q : sc) *q = c.take(E);
}

// chunk size: the largest batch slice whose scratch fits in 1 GiB, or in the KiB the knob `env` names (tests of the chunked
// path); the knob is read on every call
static int tr_chunk(int B, int64_t floats_per_mol, const char* env) {
  int64_t bytes = 1LL << 30;
  if (const char* e = getenv(env)) {
    const long long kb = atoll(e);
    if (kb > 0) bytes = kb * 1024LL;
  }
  return (int)std::max<int64_t>(1, std::min<int64_t>(B, bytes / (int64_t)sizeof(float) / floats_per_mol));
}

// The weight-gradient products (gaudi_train::OuterJob, 32 x 32 output tiles) of one call, grouped into the launches that
// follow each reverse kernel: once for a full chunk of Bc molecules and, when B % Bc, once more for the short last chunk.
struct OuterPlan {
  using Bufs = gaudi_train::TrainBufs;
  float* G = nullptr;  // the flat gradient on the device
  std::vector<gaudi_train::OuterJob> jobs;
  std::vector<int4> tiles;
  std::vector<std::pair<int, int>> launches;  // (first tile, tiles)
  size_t per_chunk = 0, base = 0;             // launches of one chunk; the first launch of the selected chunk size
  int full = 0, first = 0;
  const gaudi_train::OuterJob* djobs = nullptr;
  const int4* dtiles = nullptr;

  // G[off ...][ldg] += sum over R rows of Y[r][0..M) (x) X[r][0..Kc)   (X == nullptr: ones, Kc = 1)
  void job(const float* Yp, int ldy, int M, const float* Xp, int ldx, int Kc, int off, int ldg, int R) {
    jobs.push_back(gaudi_train::OuterJob{Yp, Xp, G + off, ldy, ldx, ldg, M, Kc, R});
    for (int m0 = 0; m0 < M; m0 += 32)
      for (int k0 = 0; k0 < Kc; k0 += 32) tiles.push_back(make_int4((int)jobs.size() - 1, m0, k0, 0));
  }
  void begin() { first = (int)tiles.size(); }                                // the jobs of one launch lie between
  void end() { launches.push_back({first, (int)tiles.size() - first}); }   // begin() and end()
  // list(bc) lists the launches of a chunk of bc molecules
  template <class List>
  void build(int B, int Bc, List list) {
    full = Bc;
    list(Bc);
    per_chunk = launches.size();
    if (B % Bc) list(B % Bc);
  }
  int upload(gaudi_handle* h, TrainState& s) {
    HIPCHECK(h, s.jobs.reserve(sizeof(gaudi_train::OuterJob) * jobs.size()));
    HIPCHECK(h, s.tiles.reserve(sizeof(int4) * tiles.size()));
    HIPCHECK(h, hipMemcpyAsync(s.jobs.p, jobs.data(), sizeof(gaudi_train::OuterJob) * jobs.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHECK(h, hipMemcpyAsync(s.tiles.p, tiles.data(), sizeof(int4) * tiles.size(), hipMemcpyHostToDevice, h->stream));
    djobs = s.jobs.as<gaudi_train::OuterJob>();
    dtiles = s.tiles.as<int4>();
    return GAUDI_OK;
  }
  void select(int bc) { base = bc == full ? 0 : per_chunk; }  // the plan of a full chunk, or of the short last one
  hipError_t launch(size_t i, hipStream_t stream) const {      // launch i of the selected chunk size
    const auto& ln = launches[base + i];
    return (hipError_t)gaudi_pt_outer(djobs, dtiles + ln.first, ln.second, stream);
  }

  // the first two layers of an edge MLP: W1 = [A | B | C] over [h_i | h_j | attributes], b1, W2, b2.  attr: the column groups
  // (array, width) of the attribute block, `A` columns in all
  void edge_jobs(const Bufs& b, const float* hl, int w1, int b1, int w2, int b2, int A, int Rn, int Re,
                 std::initializer_list<std::pair<const float*, int>> attr) {
    const int H = b.H, ld1 = 2 * H + A;
    job(b.dP, H, H, hl, H, H, w1, ld1, Rn);
    job(b.dQ, H, H, hl, H, H, w1 + H, ld1, Rn);
    int col = w1 + 2 * H;
    for (const auto& a : attr) {
      job(b.U, H, H, a.first, a.second, a.second, col, ld1, Re);
      col += a.second;
    }
    job(b.dP, H, H, nullptr, 0, 1, b1, 1, Rn);
    job(b.V, H, H, b.Su, H, H, w2, H, Re);
    job(b.V, H, H, nullptr, 0, 1, b2, 1, Re);
  }
  void att_jobs(const Bufs& b, int aw, int ab, int Re) {
    job(b.dap, 1, 1, b.M, b.H, b.H, aw, b.H, Re);
    job(b.dap, 1, 1, nullptr, 0, 1, ab, 1, Re);
  }
  void node_jobs(const Bufs& b, const float* hl, int n0w, int n0b, int n2w, int n2b, int Rn) {
    const int H = b.H;
    job(b.qp, H, H, hl, H, H, n0w, 2 * H, Rn);
    job(b.qp, H, H, b.agg, H, H, n0w + H, 2 * H, Rn);
    job(b.qp, H, H, nullptr, 0, 1, n0b, 1, Rn);
    job(b.dr, H, H, b.q, H, H, n2w, H, Rn);
    job(b.dr, H, H, nullptr, 0, 1, n2b, 1, Rn);
  }
  // embedding_out over the final h (hL, Kout outputs) and embedding over the input of F1 columns; o0: the head's offsets
  void head_jobs(const Bufs& b, const float* hL, int Kout, int F1, const int* o0, int Rn) {
    using namespace gaudi_train;
    job(b.dhout, Kout, Kout, hL, b.H, b.H, o0[OUT_W], b.H, Rn);
    job(b.dhout, Kout, Kout, nullptr, 0, 1, o0[OUT_B], 1, Rn);
    job(b.dh, b.H, b.H, b.hin, F1, F1, o0[EMB_W], F1, Rn);
    job(b.dh, b.H, b.H, nullptr, 0, 1, o0[EMB_B], 1, Rn);
  }
};

// gradients out: torch layout, names order; tensors without a gradient path are left untouched.  Waits for the stream.
static int tr_grads_out(gaudi_handle* h, const TrainState& s, float* grad_out, int32_t* has_grad_out) {
  std::vector<float> g((size_t)s.total);
  HIPCHECK(h, hipMemcpyAsync(g.data(), s.grad.p, sizeof(float) * (size_t)s.total, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < s.numel.size(); ++i) {
    has_grad_out[i] = s.has_grad[i];
    if (s.has_grad[i]) std::copy(g.begin() + s.start[i], g.begin() + s.start[i] + s.numel[i], grad_out + s.start[i]);
  }
  return GAUDI_OK;
}
