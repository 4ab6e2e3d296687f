// sub.inc -- substructure search over graphs of atoms: does a molecule contain a pattern, where, and how often (included after
// fp.inc at the end of gaudi_hip.hip; DESIGN.md section 8k).
//
// Graphs on both sides are canon.inc's (canon_graph reads and checks them): vertices = the non-hydrogen atoms, label = element * 8
// + H count, edges = the bonds between non-hydrogen atoms, unlabelled.  An embedding is an injective map of the pattern's vertices
// to the molecule's with equal elements, every pattern edge on a molecule edge (a monomorphism, not an induced subgraph), and per
// pattern flag: H_EXACT -- equal H counts; CLOSED -- equal heavy degrees.
//
// The match order of a pattern is fixed by host code (sub_plan): position 0 is the vertex whose element is rarest in the pattern
// (ties: the larger heavy degree, then the smaller index); every next position takes the unplaced vertex with the most neighbours
// already placed (ties: the smaller index), its parent is the neighbour placed earliest, and its other placed neighbours are the
// back edges, a 32-bit mask of positions.  count, first and covered do not depend on the order when the status is OK.
//
// ONE text, two builds, as canon.inc and fp.inc.  A 64-lane wave per molecule: it builds the graph once, sorts every neighbour row
// ascending, derives a 192 x 192 adjacency bit matrix (a back-edge test = one LDS read and a bit test), then loops over the
// patterns, whose plans come from a small global table into LDS.  Lanes are ROOTS: lane l owns the target vertices l, l + 64,
// l + 128 as images of position 0 and runs its own depth-first search as a lock-step state machine -- one iteration of the wave's
// loop tests one candidate (the next neighbour of the parent's image, ascending) and descends, or backtracks when the neighbours
// are exhausted.  The wave iterates while any lane is active; there is no fence inside the loop, so no lane waits where others
// skip.  A lane's state (map, cursors, best embedding, used set) lives in LDS with the lane as the fastest-varying index: the lanes
// of one step touch consecutive banks.  The budget is GAUDI_SUB_MAX_STEPS candidate tests PER ROOT, so where a search is cut
// does not depend on which lane ran the root, and both builds agree bit for bit even when they give up.  count is a wave sum,
// covered an OR, first a lexicographic minimum over the lanes' bests: all order-free.  Integer arithmetic only, no global memory
// traffic inside the search loop, no atomics on global memory; nothing depends on the molecule's place in the batch.

namespace gaudi {

constexpr int kSubWaves = 2;
constexpr int kSubMaxQuery = GAUDI_SUB_MAX_QUERY;
constexpr int kSubMaxPatterns = GAUDI_SUB_MAX_PATTERNS;
constexpr int kSubMaxSteps = GAUDI_SUB_MAX_STEPS;
static_assert(kSubMaxQuery == 32, "a position fits a bit of the back-edge mask; a map is eight dwords");
static_assert(kSubMaxSteps >= 1 && kSubMaxSteps <= (1 << 22), "192 roots * the cap fits an int");
static_assert(GAUDI_SUB_OK == GAUDI_CANON_OK && GAUDI_SUB_BAD_INPUT == GAUDI_CANON_BAD_INPUT && GAUDI_SUB_OVERFLOW == GAUDI_CANON_OVERFLOW &&
                  GAUDI_SUB_EMPTY == GAUDI_CANON_EMPTY && GAUDI_SUB_GAVE_UP == GAUDI_CANON_GAVE_UP,
              "a molecule's refusal is canon_graph's status");

// One pattern as the kernel reads it: unsigned words only, bytes packed four to a word (sub_byte)
struct SubPlan {
  unsigned int status, n, flags, reserved;  // GAUDI_SUB_OK or GAUDI_SUB_BAD_PATTERN; vertices; GAUDI_SUB_H_EXACT | GAUDI_SUB_CLOSED
  unsigned int back[kSubMaxQuery];          // position k: the earlier positions adjacent to it, the parent's left out
  unsigned int parent[kSubMaxQuery / 4];    // position k >= 1: the position of its parent
  unsigned int label[kSubMaxQuery / 4];     // position k: element * 8 + H count
  unsigned int deg[kSubMaxQuery / 4];       // position k: heavy degree
  unsigned int pos[kSubMaxQuery / 4];       // vertex v (ascending atom index): its position
  unsigned int atom[kSubMaxQuery / 2];      // vertex v: its atom index in the pattern's arrays (two to a word)
};

__host__ __device__ __forceinline__ int sub_byte(const unsigned int* a, int k) { return (int)((a[k >> 2] >> ((k & 3) * 8)) & 0xffu); }
__host__ __device__ __forceinline__ int sub_half(const unsigned int* a, int k) { return (int)((a[k >> 1] >> ((k & 1) * 16)) & 0xffffu); }

struct SubSmem {
  CanonSmem g;
  unsigned int abit[kCanonMaxHeavy][6];        // bit u of row v: u and v are bonded
  unsigned char tdeg[kCanonMaxHeavy];          // heavy degree
  // per lane (the host build has one): byte k of a map at [k >> 2][lane][k & 3], so one position of all lanes is 64 consecutive dwords
  unsigned int used[6][kRwLanes];              // the target vertices of the positions placed
  unsigned char map[kSubMaxQuery / 4][kRwLanes][4];   // position -> target vertex
  unsigned char cur[kSubMaxQuery / 4][kRwLanes][4];   // position -> the next entry of its parent's image's neighbour row
  unsigned char best[kSubMaxQuery / 4][kRwLanes][4];  // the smallest embedding this lane found, by position
  unsigned int cov[6];                         // the target vertices some embedding found uses
  SubPlan plan;
};

struct SubParams {
  CanonParams in;  // the input fields only
  int P, QA;
  const SubPlan* plans;    // [P]
  int* count;              // [B][P]
  int* first;              // [B][P][QA], or nullptr
  unsigned char* covered;  // [B][P][A], or nullptr
  int* steps;              // [B][P]
  int* status;             // [B][P]
};

static int g_sub_root_steps = 0;  // host build: the largest per-root step count since the last reset (gaudi_host_substructure_root_steps)

__host__ __device__ __forceinline__ void sub_cover(unsigned int* word, unsigned int bit) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(word, bit);  // an LDS integer OR: the result does not depend on the order
#else
  *word |= bit;
#endif
}

// the lane's search state outside LDS
struct SubLane {
  int root, d, steps_root, steps, count;
  bool gave, active;
};

__host__ __device__ __forceinline__ void sub_next_root(SubLane& L, int H) {
#if !defined(__HIP_DEVICE_COMPILE__)
  if (L.steps_root > g_sub_root_steps) g_sub_root_steps = L.steps_root;
#endif
  L.steps += L.steps_root;
  L.steps_root = 0;
  L.d = 0;
  L.root += kRwLanes;
  L.active = L.root < H;
}

// pattern position k may sit on target vertex t: element, and what the flags ask
__host__ __device__ __forceinline__ bool sub_fits(const SubSmem& s, int k, int t, int flags) {
  const int tl = s.g.label[t], pl = sub_byte(s.plan.label, k);
  bool ok = (tl >> 3) == (pl >> 3);
  if (flags & GAUDI_SUB_H_EXACT) ok = ok && tl == pl;
  if (flags & GAUDI_SUB_CLOSED) ok = ok && (int)s.tdeg[t] == sub_byte(s.plan.deg, k);
  return ok;
}

// the map of positions 0..n-1 is an embedding: counted, its vertices covered, kept if it is the lane's smallest in vertex order
__host__ __device__ __forceinline__ void sub_found(SubSmem& s, SubLane& L, int lane, int n) {
  bool better = L.count == 0;
  if (!better)
    for (int v = 0; v < n; ++v) {
      const int p = sub_byte(s.plan.pos, v);
      const int a = s.map[p >> 2][lane][p & 3], o = s.best[p >> 2][lane][p & 3];
      if (a != o) {
        better = a < o;
        break;
      }
    }
  for (int k = 0; k < n; ++k) {
    const int t = s.map[k >> 2][lane][k & 3];
    sub_cover(&s.cov[t >> 5], 1u << (t & 31));
    if (better) s.best[k >> 2][lane][k & 3] = (unsigned char)t;
  }
  ++L.count;
}

// ONE step of a lane's search: the root tested, one candidate tested (and the search a level deeper if it fits), or one level back
__host__ __device__ __forceinline__ void sub_step(SubSmem& s, SubLane& L, int lane, int H, int n, int flags) {
  if (L.d == 0) {
    const int t = L.root;
    L.steps_root = 1;
    if (!sub_fits(s, 0, t, flags)) {
      sub_next_root(L, H);
      return;
    }
    s.map[0][lane][0] = (unsigned char)t;
    if (n == 1) {
      sub_found(s, L, lane, n);
      sub_next_root(L, H);
      return;
    }
    s.used[t >> 5][lane] |= 1u << (t & 31);
    s.cur[0][lane][1] = 0;
    L.d = 1;
    return;
  }
  const int k = L.d;
  const int c = s.cur[k >> 2][lane][k & 3];
  const int pp = sub_byte(s.plan.parent, k);
  const int pv = s.map[pp >> 2][lane][pp & 3];
  const int cand = c < kCanonDeg ? (int)s.g.adj[pv][c < kCanonDeg ? c : 0] : kCanonNone;
  if (cand == kCanonNone) {  // the neighbours are exhausted: the position before comes off the map
    const int j = k - 1;
    const int t = s.map[j >> 2][lane][j & 3];
    s.used[t >> 5][lane] &= ~(1u << (t & 31));
    L.d = j;
    if (j == 0) sub_next_root(L, H);
    return;
  }
  if (L.steps_root >= kSubMaxSteps) {  // the budget of this root is spent: what it found so far stays
    L.gave = true;
    for (int q = 0; q < 6; ++q) s.used[q][lane] = 0u;
    sub_next_root(L, H);
    return;
  }
  s.cur[k >> 2][lane][k & 3] = (unsigned char)(c + 1);
  ++L.steps_root;
  bool ok = !((s.used[cand >> 5][lane] >> (cand & 31)) & 1u) && sub_fits(s, k, cand, flags);
  unsigned int back = ok ? s.plan.back[k] : 0u;
  while (back) {
    const int j = __builtin_ctz(back);
    back &= back - 1u;
    const int t = s.map[j >> 2][lane][j & 3];
    if (!((s.abit[cand][t >> 5] >> (t & 31)) & 1u)) {
      ok = false;
      break;
    }
  }
  if (!ok) return;
  s.map[k >> 2][lane][k & 3] = (unsigned char)cand;
  if (k + 1 == n) {  // complete: the last position stays open for its next candidate
    sub_found(s, L, lane, n);
    return;
  }
  s.used[cand >> 5][lane] |= 1u << (cand & 31);
  const int d = k + 1;
  s.cur[d >> 2][lane][d & 3] = 0;
  L.d = d;
}

// One molecule against every pattern.  Every branch around a fence or a reduction is lane-uniform.
__host__ __device__ inline void substructure_search(const SubParams& P, SubSmem& s, int b, int lane) {
  int H = 0, E = 0;
  const int mstatus = canon_graph(P.in, s.g, b, lane, H, E);
  if (mstatus == GAUDI_CANON_OK) {
    for (int v = lane; v < H; v += kRwLanes) {
      int c[8];
      for (int k = 0; k < 8; ++k) c[k] = s.g.adj[v][k];
      canon_sort8(c);  // none (0xff) is above every vertex: the neighbours ascending, then the padding
      unsigned int row[6] = {0u, 0u, 0u, 0u, 0u, 0u};
      int deg = 0;
      for (int k = 0; k < 8; ++k) {
        const int o = c[k];
        const bool there = o != kCanonNone;
        s.g.adj[v][k] = (unsigned char)o;
        deg += there;
        for (int q = 0; q < 6; ++q) row[q] |= there && (o >> 5) == q ? 1u << (o & 31) : 0u;
      }
      for (int q = 0; q < 6; ++q) s.abit[v][q] = row[q];
      s.tdeg[v] = (unsigned char)deg;
    }
    for (int q = 0; q < 6; ++q) s.used[q][lane] = 0u;
  }
  for (int p = 0; p < P.P; ++p) {
    rw_fence();  // the pattern before is done with the plan and the cover
    const SubPlan& src = P.plans[p];
    for (int i = lane; i < kSubMaxQuery; i += kRwLanes) s.plan.back[i] = src.back[i];
    for (int i = lane; i < kSubMaxQuery / 4; i += kRwLanes) {
      s.plan.parent[i] = src.parent[i];
      s.plan.label[i] = src.label[i];
      s.plan.deg[i] = src.deg[i];
      s.plan.pos[i] = src.pos[i];
    }
    for (int i = lane; i < kSubMaxQuery / 2; i += kRwLanes) s.plan.atom[i] = src.atom[i];
    for (int i = lane; i < 6; i += kRwLanes) s.cov[i] = 0u;
    rw_fence();
    const size_t cell = (size_t)b * P.P + p;
    const int pstatus = (int)src.status, n = (int)src.n, flags = (int)src.flags;  // (the same words in every lane)
    if (pstatus != GAUDI_SUB_OK || mstatus != GAUDI_CANON_OK) {
      if (lane == 0) P.status[cell] = pstatus != GAUDI_SUB_OK ? pstatus : mstatus;
      continue;
    }
    SubLane L;
    L.root = lane;
    L.d = 0;
    L.steps_root = 0;
    L.steps = 0;
    L.count = 0;
    L.gave = false;
    L.active = lane < H;
    while (rw_any(L.active))
      if (L.active) sub_step(s, L, lane, H, n, flags);
    rw_fence();  // every lane's cover
    int count, lo, hi;
    (void)rw_scan(L.count, lane, count);
    (void)rw_scan(L.steps & 0xffff, lane, lo);
    (void)rw_scan(L.steps >> 16, lane, hi);
    const long long steps = ((long long)hi << 16) + lo;
    const bool gave = rw_any(L.gave);
    if (P.covered)
      for (int v = lane; v < H; v += kRwLanes)
        if ((s.cov[v >> 5] >> (v & 31)) & 1u) P.covered[cell * P.in.A + s.g.hv[v]] = 1;
    if (P.first && count > 0) {
      // the lexicographic minimum in the pattern's own atom order: vertex by vertex, the lanes whose best is not the minimum drop
      // out.  Vertices are numbered in ascending atom index on both sides, so vertex order is atom order.
      bool alive = L.count > 0;
      for (int v = 0; v < n; ++v) {
        const int pq = sub_byte(s.plan.pos, v);
        const int key = alive ? (int)s.best[pq >> 2][lane][pq & 3] : kCanonFar;
        const int m = rw_min(key);
        alive = alive && key == m;
        if (lane == 0) P.first[cell * P.QA + sub_half(s.plan.atom, v)] = (int)s.g.hv[m];
      }
    }
    if (lane == 0) {
      P.count[cell] = count;
      P.steps[cell] = steps > 0x7fffffffll ? 0x7fffffff : (int)steps;
      P.status[cell] = gave ? GAUDI_SUB_GAVE_UP : GAUDI_SUB_OK;
    }
  }
}

__global__ __launch_bounds__(64 * kSubWaves) void sub_kernel(const SubParams P) {
  __shared__ SubSmem smem[kSubWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * kSubWaves + w;
  if (b >= P.in.B) return;
  substructure_search(P, smem[w], b, lane);
}

static void sub_set_byte(unsigned int* a, int k, int v) { a[k >> 2] |= (unsigned int)(v & 0xff) << ((k & 3) * 8); }

// The plan of pattern p (host code; `g` is scratch).  Refused -- empty, no non-hydrogen atom, more than kSubMaxQuery vertices, not
// connected, an unknown flag, or anything canon_graph refuses (a bad index or element, a self bond, a duplicate bond, more than 8
// bonds at an atom) -- the plan says GAUDI_SUB_BAD_PATTERN and nothing else.
static void sub_plan(const CanonParams& in, int p, int flags, CanonSmem& g, SubPlan& out) {
  memset(&out, 0, sizeof(out));
  out.status = GAUDI_SUB_BAD_PATTERN;
  if (flags & ~(GAUDI_SUB_H_EXACT | GAUDI_SUB_CLOSED)) return;
  int n = 0, E = 0;
  if (canon_graph(in, g, p, 0, n, E) != GAUDI_CANON_OK || n < 1 || n > kSubMaxQuery) return;
  int deg[kSubMaxQuery], per_elem[kCanonMaxElems] = {0}, pos[kSubMaxQuery], order[kSubMaxQuery];
  for (int v = 0; v < n; ++v) {
    deg[v] = 0;
    for (int k = 0; k < kCanonDeg; ++k) deg[v] += g.adj[v][k] != kCanonNone;
    ++per_elem[g.label[v] >> 3];
    pos[v] = -1;
  }
  int first = 0;
  for (int v = 1; v < n; ++v) {
    const int cv = per_elem[g.label[v] >> 3], cf = per_elem[g.label[first] >> 3];
    if (cv < cf || (cv == cf && deg[v] > deg[first])) first = v;
  }
  order[0] = first;
  pos[first] = 0;
  for (int k = 1; k < n; ++k) {
    int pick = -1, most = 0;
    for (int v = 0; v < n; ++v) {
      if (pos[v] >= 0) continue;
      int placed = 0;
      for (int q = 0; q < kCanonDeg; ++q) placed += g.adj[v][q] != kCanonNone && pos[g.adj[v][q]] >= 0;
      if (placed > most) {
        most = placed;
        pick = v;
      }
    }
    if (pick < 0) return;  // nothing left touches what is placed: not connected
    int parent = kSubMaxQuery;
    for (int q = 0; q < kCanonDeg; ++q)
      if (g.adj[pick][q] != kCanonNone && pos[g.adj[pick][q]] >= 0 && pos[g.adj[pick][q]] < parent) parent = pos[g.adj[pick][q]];
    for (int q = 0; q < kCanonDeg; ++q)
      if (g.adj[pick][q] != kCanonNone && pos[g.adj[pick][q]] >= 0 && pos[g.adj[pick][q]] != parent) out.back[k] |= 1u << pos[g.adj[pick][q]];
    sub_set_byte(out.parent, k, parent);
    order[k] = pick;
    pos[pick] = k;
  }
  for (int k = 0; k < n; ++k) {
    sub_set_byte(out.label, k, g.label[order[k]]);
    sub_set_byte(out.deg, k, deg[order[k]]);
  }
  for (int v = 0; v < n; ++v) {
    sub_set_byte(out.pos, v, pos[v]);
    out.atom[v >> 1] |= (unsigned int)g.hv[v] << ((v & 1) * 16);
  }
  out.n = (unsigned int)n;
  out.flags = (unsigned int)flags;
  out.status = GAUDI_SUB_OK;
}

// the arguments both entry points share, checked; the plans of the P patterns
static int sub_prepare(int n_elems, int h_elem, int c_elem, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                       const int32_t* bonds, const int32_t* n_bonds, int P, int QA, int QM, const int32_t* p_elem,
                       const int32_t* p_n_atoms, const int32_t* p_bonds, const int32_t* p_n_bonds, const int32_t* p_flags,
                       std::vector<SubPlan>& plans, const char** why) {
  if (int rc = canon_prepare(n_elems, h_elem, c_elem, B, A, M, elem, n_atoms, bonds, n_bonds, why)) return rc;
  *why = "invalid argument";
  if (!p_elem || !p_n_atoms || !p_bonds || !p_n_bonds || !p_flags || P < 0 || QA < 1 || QM < 1) return GAUDI_E_INVALID;
  if (P > kSubMaxPatterns) { *why = "more than GAUDI_SUB_MAX_PATTERNS patterns in one call"; return GAUDI_E_CAPACITY; }
  if ((long long)B * P * (A > QA ? A : QA) > (1ll << 31)) { *why = "B * P * max(A, QA) beyond 2^31"; return GAUDI_E_CAPACITY; }
  CanonParams in{};
  in.B = P;
  in.A = QA;
  in.M = QM;
  in.n_elems = n_elems;
  in.h_elem = h_elem;
  in.c_elem = c_elem;
  in.elem = p_elem;
  in.n_atoms = p_n_atoms;
  in.bonds = p_bonds;
  in.n_bonds = p_n_bonds;
  std::vector<CanonSmem> g(1);
  plans.resize(P);
  for (int p = 0; p < P; ++p) sub_plan(in, p, p_flags[p], g[0], plans[p]);
  return GAUDI_OK;
}

}  // namespace gaudi

#define GAUDI_SUB_ARGS                                                                                                          \
  int n_elems, int h_elem, int c_elem, int B, int A, int M, const int32_t *elem, const int32_t *n_atoms, const int32_t *bonds,  \
      const int32_t *n_bonds, int P, int QA, int QM, const int32_t *p_elem, const int32_t *p_n_atoms, const int32_t *p_bonds,   \
      const int32_t *p_n_bonds, const int32_t *p_flags, int32_t *count_out, int32_t *first_out, uint8_t *covered_out,           \
      int32_t *steps_out, int32_t *status_out
#define GAUDI_SUB_PASS                                                                                                        \
  n_elems, h_elem, c_elem, B, A, M, elem, n_atoms, bonds, n_bonds, P, QA, QM, p_elem, p_n_atoms, p_bonds, p_n_bonds, p_flags

extern "C" int gaudi_substructure_search(gaudi_handle* h, GAUDI_SUB_ARGS) {
  if (!h || !count_out || !steps_out || !status_out) return GAUDI_E_INVALID;
  const char* why = "";
  std::vector<gaudi::SubPlan> plans;
  if (int rc = gaudi::sub_prepare(GAUDI_SUB_PASS, plans, &why)) return fail(h, rc, why);
  if (B == 0 || P == 0) return GAUDI_OK;
  HIPCHECK(h, hipSetDevice(h->device));
  const size_t nB = (size_t)B, cells = nB * P;
  const size_t isz[5] = {sizeof(int) * nB * A, sizeof(int) * nB, sizeof(int) * nB * M * 2, sizeof(int) * nB, sizeof(gaudi::SubPlan) * P};
  const void* ins[5] = {elem, n_atoms, bonds, n_bonds, plans.data()};
  for (int i = 0; i < 5; ++i) {
    HIPCHECK(h, h->d_sub[i].reserve(isz[i]));
    HIPCHECK(h, hipMemcpyAsync(h->d_sub[i].p, ins[i], isz[i], hipMemcpyHostToDevice, h->stream));
  }
  // a refused cell writes its status only: zero everywhere else, -1 in first
  const size_t osz[5] = {sizeof(int) * cells, first_out ? sizeof(int) * cells * QA : 0, covered_out ? cells * A : 0, sizeof(int) * cells,
                         sizeof(int) * cells};
  void* outs[5] = {count_out, first_out, covered_out, steps_out, status_out};
  for (int i = 0; i < 5; ++i) {
    if (!outs[i]) continue;
    HIPCHECK(h, h->d_sub[5 + i].reserve(osz[i]));
    HIPCHECK(h, hipMemsetAsync(h->d_sub[5 + i].p, i == 1 ? 0xff : 0, osz[i], h->stream));
  }
  gaudi::SubParams S{};
  S.in.B = B;
  S.in.A = A;
  S.in.M = M;
  S.in.n_elems = n_elems;
  S.in.h_elem = h_elem;
  S.in.c_elem = c_elem;
  S.in.elem = h->d_sub[0].as<int>();
  S.in.n_atoms = h->d_sub[1].as<int>();
  S.in.bonds = h->d_sub[2].as<int>();
  S.in.n_bonds = h->d_sub[3].as<int>();
  S.P = P;
  S.QA = QA;
  S.plans = h->d_sub[4].as<gaudi::SubPlan>();
  S.count = h->d_sub[5].as<int>();
  S.first = first_out ? h->d_sub[6].as<int>() : nullptr;
  S.covered = covered_out ? h->d_sub[7].as<unsigned char>() : nullptr;
  S.steps = h->d_sub[8].as<int>();
  S.status = h->d_sub[9].as<int>();
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (h->prof) HIPCHECK(h, h->sub_log.begin(h->stream, ev));
  hipLaunchKernelGGL(gaudi::sub_kernel, dim3((B + gaudi::kSubWaves - 1) / gaudi::kSubWaves), dim3(64 * gaudi::kSubWaves), 0, h->stream, S);
  HIPCHECK(h, hipGetLastError());
  if (h->prof) HIPCHECK(h, h->sub_log.end(h->stream, ev));
  for (int i = 0; i < 5; ++i)
    if (outs[i]) HIPCHECK(h, hipMemcpyAsync(outs[i], h->d_sub[5 + i].p, osz[i], hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  return GAUDI_OK;
}

extern "C" int gaudi_host_substructure_search(GAUDI_SUB_ARGS) {
  if (!count_out || !steps_out || !status_out) return GAUDI_E_INVALID;
  const char* why = "";
  std::vector<gaudi::SubPlan> plans;
  if (int rc = gaudi::sub_prepare(GAUDI_SUB_PASS, plans, &why)) return rc;
  if (B == 0 || P == 0) return GAUDI_OK;
  const size_t cells = (size_t)B * P;
  memset(count_out, 0, sizeof(int) * cells);
  if (first_out) memset(first_out, 0xff, sizeof(int) * cells * QA);
  if (covered_out) memset(covered_out, 0, cells * A);
  memset(steps_out, 0, sizeof(int) * cells);
  memset(status_out, 0, sizeof(int) * cells);
  gaudi::SubParams S{};
  S.in.B = B;
  S.in.A = A;
  S.in.M = M;
  S.in.n_elems = n_elems;
  S.in.h_elem = h_elem;
  S.in.c_elem = c_elem;
  S.in.elem = elem;
  S.in.n_atoms = n_atoms;
  S.in.bonds = bonds;
  S.in.n_bonds = n_bonds;
  S.P = P;
  S.QA = QA;
  S.plans = plans.data();
  S.count = count_out;
  S.first = first_out;
  S.covered = covered_out;
  S.steps = steps_out;
  S.status = status_out;
  std::vector<gaudi::SubSmem> W(1);
  for (int b = 0; b < B; ++b) gaudi::substructure_search(S, W[0], b, 0);
  return GAUDI_OK;
}
#undef GAUDI_SUB_ARGS
#undef GAUDI_SUB_PASS

extern "C" int gaudi_host_substructure_root_steps(int reset) {
  const int was = gaudi::g_sub_root_steps;
  if (reset) gaudi::g_sub_root_steps = 0;
  return was;
}

extern "C" int gaudi_substructure_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms) {
  if (!h || !n_launches || !total_ms) return GAUDI_E_INVALID;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, h->sub_log.fold(0));
  *n_launches = (int32_t)h->sub_log.n;
  *total_ms = h->sub_log.ms;
  return GAUDI_OK;
}
