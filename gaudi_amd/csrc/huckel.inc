// huckel.inc -- Hueckel molecular-orbital levels, frontier gap, pi charges and pi bond orders of a graph of atoms (included after
// sub.inc at the end of gaudi_hip.hip; DESIGN.md section 8l).
//
// The graph is canon.inc's (canon_graph reads and checks it): vertices = the non-hydrogen atoms with their element, H count and
// heavy degree.  coordination = heavy degree + H count; the table maps (element, coordination 0..4) to a site class or to "not a
// pi centre"; a class has a Coulomb term h, an electron count n_e and a bond factor k.  In units of |beta| with alpha = 0 the
// matrix over the pi centres (numbered in ascending atom index) is M_rr = h_r, M_rs = k_r * k_s for bonded centres (or the pair
// value the table lists).  An orbital's energy is alpha + x beta, beta < 0: the larger x, the lower the level.
//
// ONE text, two builds, as canon.inc / fp.inc / sub.inc: a 64-lane wave per molecule on the device, one lane that walks every index
// on the host (kRwLanes).  Per molecule:
//   1. canon_graph; sites classified and compacted; A = M and V = I as fp32 in LDS, rows padded to P + 1 floats so that lanes
//      sweeping a row and lanes sweeping a column both touch distinct banks;
//   2. cyclic two-sided Jacobi on a round-robin (tournament) schedule that is a function of n_pi ALONE: with m = n_pi rounded up to
//      even, a sweep is m - 1 rounds of m / 2 disjoint pairs, round r pairing m - 1 with r and (r + j) with (r - j) mod (m - 1);
//      pairs with the dummy index idle.  Per round one lane per pair computes the rotation from a_pp, a_qq, a_pq; all lanes apply
//      the row updates; after a fence the column updates of A and V.  Every element is written by exactly one lane from values the
//      phase before completed.  A sweep starts while max |off-diagonal| > 2^-24 (a maximum has no order); kHuckelSweeps sweeps
//      without getting there is NOT_CONVERGED (jacobi_sweeps below: ppp.inc runs the same routine inside its SCF loop);
//   3. levels are NOT read off the Jacobi diagonal (it drifts with every rotation): lane i takes the Rayleigh quotient of column i
//      of V with the sparse matrix the molecule started from, rows ascending, a row's bonds in adjacency order, and normalises
//      the column;
//   4. levels ranked by counting (ties: the smaller index first), filled two to a level from the lowest energy; HOMO, LUMO, gap,
//      the pi energy, and with one lane per atom / bond the pi charges and pi bond orders.
// Every fp32 operation is individually rounded (contraction off, correctly rounded / and sqrtf: the stability.inc idiom) and
// every sum runs in one fixed order, so the device gives the host build's bits, and a molecule's result does not depend on the
// capacity tier P, on the batch or on its place in it.  No atomics; plain LDS and rw_fence.

namespace gaudi {

constexpr int kHuckelMaxPi = GAUDI_HUCKEL_MAX_PI;
constexpr int kHuckelMaxClasses = GAUDI_HUCKEL_MAX_CLASSES;
constexpr int kHuckelSweeps = GAUDI_HUCKEL_MAX_SWEEPS;
constexpr int kHuckelNbr = 4;             // a pi centre's coordination is at most 4, so it has at most 4 neighbours
constexpr int kHuckelCoords = 5;          // coordination 0..4
constexpr float kHuckelOff = 5.9604645e-8f;   // 2^-24: half an ulp of a diagonal element of order one
constexpr float kHuckelDegenerate = 1e-3f;
static_assert(kHuckelMaxPi == 128 && kHuckelMaxPi < kCanonNone, "a pi index fits a byte; the largest tier is 128");
static_assert(GAUDI_HUCKEL_OK == GAUDI_CANON_OK && GAUDI_HUCKEL_BAD_INPUT == GAUDI_CANON_BAD_INPUT &&
                  GAUDI_HUCKEL_OVERFLOW == GAUDI_CANON_OVERFLOW && GAUDI_HUCKEL_EMPTY == GAUDI_CANON_EMPTY,
              "a molecule's refusal is canon_graph's status");

// the table as the kernel reads it (huckel_table builds it from gaudi_huckel_tables)
struct HuckelTab {
  int site_class[kCanonMaxElems][kHuckelCoords];  // -1: not a pi centre
  int n_e[kHuckelMaxClasses];
  float h[kHuckelMaxClasses];
  float kk[kHuckelMaxClasses][kHuckelMaxClasses];  // the off-diagonal element of a bonded pair of classes
};

template <int P>
struct HuckelSmem {
  CanonSmem g;
  float a[P][P + 1], v[P][P + 1];
  float hd[P], kn[P][kHuckelNbr];  // the sparse matrix: diagonal; the elements of a centre's bonds
  float x[P], lev[P];              // levels by column; by rank
  float rc[P / 2], rs[P / 2], rpp[P / 2], rqq[P / 2];  // a round's rotations: cosine, sine, the new diagonal pair
  unsigned char rp[P / 2], rq[P / 2];                  // ... and their index pairs, p < q; q = none for an idle pair
  unsigned char nb[P][kHuckelNbr];   // a centre's bonded centres, none-padded
  unsigned char vert[P];             // pi centre -> vertex
  unsigned char ord[P], occ[P];      // rank -> column; rank -> occupation
  signed char cls[P];
  unsigned char pidx[kCanonMaxHeavy];  // vertex -> pi centre, none for an excluded atom
  signed char vcls[kCanonMaxHeavy];    // vertex -> site class, -1 for an excluded atom
};
static_assert(sizeof(HuckelSmem<128>) <= 160 * 1024, "the largest tier fits the LDS of a CU");

struct HuckelParams {
  CanonParams in;  // the input fields only
  const int* mol;  // the molecules of this launch (one capacity tier)
  const int* charge;
  const HuckelTab* tab;
  float* levels;              // [B][kHuckelMaxPi]
  unsigned char* occupation;  // [B][kHuckelMaxPi]
  int *n_pi, *n_electrons, *n_excluded, *sweeps, *flags, *status;  // [B]
  float *homo, *lumo, *gap, *e_pi;                                 // [B]
  float* pi_charge;         // [B][A]
  float* pi_bond_order;     // [B][M]
  signed char* site_class;  // [B][A]
};

__host__ __device__ __forceinline__ int huckel_bits(float f) { return __builtin_bit_cast(int, f); }

// Cyclic two-sided Jacobi on the symmetric n x n matrix in s.a, the rotations accumulated into s.v (the caller sets it to I),
// on the round-robin schedule of the header; S is any work space with a, v and the rotation arrays of HuckelSmem (ppp.inc has
// one).  A sweep starts while max |off-diagonal| > threshold; true: it got there within kHuckelSweeps sweeps.  `sweeps` gains
// the sweeps run.  Every lane of the wave calls it with the same n and threshold.
template <int P, class S>
__host__ __device__ inline bool jacobi_sweeps(S& s, int n, int lane, float threshold, int& sweeps) {
#pragma clang fp contract(off)
  static_assert((P & (P - 1)) == 0 && P <= kHuckelMaxPi, "a work item splits into (pair, index) by a shift");
  const int m = n + (n & 1), half = m >> 1, rounds = m - 1;
  constexpr int kShift = P == 128 ? 7 : P == 64 ? 6 : P == 32 ? 5 : P == 16 ? 4 : -1;
  static_assert(kShift > 0, "capacity tiers are 16, 32, 64, 128");
  int done = 0;
  bool converged = false;
  for (;;) {
    float off = 0.0f;
    for (int r = lane; r < n; r += kRwLanes)
      for (int c = 0; c < r; ++c) {
        const float t = fabsf(s.a[r][c]);
        off = t > off ? t : off;
      }
    const int worst = -rw_min(-huckel_bits(off));  // non-negative floats order as their bits
    if (worst <= huckel_bits(threshold)) {
      converged = true;
      break;
    }
    if (done == kHuckelSweeps) break;
    for (int rd = 0; rd < rounds; ++rd) {
      for (int j = lane; j < half; j += kRwLanes) {
        const int pa = j == 0 ? m - 1 : (rd + j) % rounds, pb = j == 0 ? rd : (rd - j + rounds) % rounds;
        const int p = pa < pb ? pa : pb, q = pa < pb ? pb : pa;
        float c = 1.0f, sn = 0.0f, npp = 0.0f, nqq = 0.0f;
        if (q < n) {
          const float app = s.a[p][p], aqq = s.a[q][q], apq = s.a[p][q];
          npp = app;
          nqq = aqq;
          if (apq != 0.0f) {
            const float theta = (aqq - app) / (2.0f * apq);
            float t = 1.0f / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
            t = theta < 0.0f ? -t : t;
            c = 1.0f / sqrtf(t * t + 1.0f);
            sn = t * c;
            const float d = t * apq;
            npp = app - d;
            nqq = aqq + d;
          }
        }
        s.rp[j] = (unsigned char)p;
        s.rq[j] = (unsigned char)(q < n ? q : kCanonNone);
        s.rc[j] = c;
        s.rs[j] = sn;
        s.rpp[j] = npp;
        s.rqq[j] = nqq;
      }
      rw_fence();
      for (int it = lane; it < half * P; it += kRwLanes) {  // rows p and q of J^T A
        const int j = it >> kShift, k = it & (P - 1), q = s.rq[j];
        if (k >= n || q == kCanonNone) continue;
        const int p = s.rp[j];
        const float c = s.rc[j], sn = s.rs[j], x = s.a[p][k], y = s.a[q][k];
        s.a[p][k] = c * x - sn * y;
        s.a[q][k] = sn * x + c * y;
      }
      rw_fence();
      for (int it = lane; it < half * P; it += kRwLanes) {  // columns p and q of (J^T A) J and of V J
        const int j = it >> kShift, k = it & (P - 1), q = s.rq[j];
        if (k >= n || q == kCanonNone) continue;
        const int p = s.rp[j];
        const float c = s.rc[j], sn = s.rs[j], x = s.a[k][p], y = s.a[k][q];
        float nx = c * x - sn * y, ny = sn * x + c * y;
        if (k == p) {  // the pair's own 2 x 2 block in closed form: the element rotated away is zero, not rounding noise
          nx = s.rpp[j];
          ny = 0.0f;
        }
        if (k == q) {
          nx = 0.0f;
          ny = s.rqq[j];
        }
        s.a[k][p] = nx;
        s.a[k][q] = ny;
        const float vx = s.v[k][p], vy = s.v[k][q];
        s.v[k][p] = c * vx - sn * vy;
        s.v[k][q] = sn * vx + c * vy;
      }
      rw_fence();
    }
    ++done;
  }
  sweeps += done;
  return converged;
}

// Step 1 for molecule b whose graph is in s.g (H vertices): site classes, the pi centres numbered in ascending atom index
// (vertices are) into s.vcls, s.pidx, s.vert, s.cls.  -> n centres, n_el electrons and GAUDI_HUCKEL_OK, or the status that refuses
// the molecule.  S is any work space with these arrays (ring_current.inc has one); every exit is lane-uniform.
template <int P, class S>
__host__ __device__ inline int huckel_sites(const HuckelTab& T, S& s, int H, int charge, int lane, int& n, int& n_el) {
  const int per = (H + kRwLanes - 1) / kRwLanes, lo = lane * per, hi = lo + per < H ? lo + per : H;
  int cnt = 0, el = 0;
  for (int v = lo; v < hi; ++v) {
    const int label = s.g.label[v];
    int coord = label & 7;
    for (int k = 0; k < kCanonDeg; ++k) coord += s.g.adj[v][k] != kCanonNone;
    const int c = coord < kHuckelCoords ? T.site_class[label >> 3][coord] : -1;
    s.vcls[v] = (signed char)c;
    cnt += c >= 0;
    el += c >= 0 ? T.n_e[c] : 0;
  }
  int pos = rw_scan(cnt, lane, n);
  (void)rw_scan(el, lane, n_el);
  n_el -= charge;
  for (int v = lo; v < hi; ++v) {
    const int c = s.vcls[v];
    s.pidx[v] = (unsigned char)(c >= 0 && pos < P ? pos : kCanonNone);
    if (c >= 0) {
      if (pos < P) {
        s.vert[pos] = (unsigned char)v;
        s.cls[pos] = (signed char)c;
      }
      ++pos;
    }
  }
  if (n == 0) return GAUDI_HUCKEL_NO_PI;
  if (n > P) return GAUDI_HUCKEL_OVERFLOW;  // (the host sends a molecule to a tier that holds its heavy atoms: P is 128 here)
  if (n_el < 0 || n_el > 2 * n) return GAUDI_HUCKEL_BAD_INPUT;  // a charge the pi system cannot carry
  rw_fence();
  return GAUDI_HUCKEL_OK;
}

// A = M, V = I; the sparse matrix (s.hd, s.nb, s.kn) kept for the Rayleigh pass
template <class S>
__host__ __device__ inline void huckel_matrix(const HuckelTab& T, S& s, int n, int lane) {
  for (int r = 0; r < n; ++r)
    for (int c = lane; c < n; c += kRwLanes) {
      s.a[r][c] = 0.0f;
      s.v[r][c] = r == c ? 1.0f : 0.0f;
    }
  rw_fence();
  for (int r = lane; r < n; r += kRwLanes) {
    const int v = s.vert[r], cr = s.cls[r];
    const float hr = T.h[cr];
    s.a[r][r] = hr;
    s.hd[r] = hr;
    int d = 0;
    for (int k = 0; k < kCanonDeg; ++k) {
      const int o = s.g.adj[v][k];
      if (o == kCanonNone) continue;
      const int ps = s.pidx[o];
      if (ps == kCanonNone) continue;
      const float kk = T.kk[cr][s.cls[ps]];
      s.a[r][ps] = kk;
      if (d < kHuckelNbr) {
        s.nb[r][d] = (unsigned char)ps;
        s.kn[r][d] = kk;
      }
      ++d;
    }
    for (; d < kHuckelNbr; ++d) {
      s.nb[r][d] = (unsigned char)kCanonNone;
      s.kn[r][d] = 0.0f;
    }
  }
  rw_fence();
}

// Step 3: s.x[i] = the Rayleigh quotient of column i of V with the sparse matrix, rows ascending, a row's bonds in adjacency
// order; the column normalised.
template <class S>
__host__ __device__ inline void huckel_rayleigh(S& s, int n, int lane) {
#pragma clang fp contract(off)
  for (int i = lane; i < n; i += kRwLanes) {
    float num = 0.0f, den = 0.0f;
    for (int r = 0; r < n; ++r) {
      const float vr = s.v[r][i], vv = vr * vr;
      den = den + vv;
      num = num + s.hd[r] * vv;
      for (int d = 0; d < kHuckelNbr; ++d) {
        const int o = s.nb[r][d];
        if (o == kCanonNone || o <= r) continue;  // every bond once, from its smaller end
        num = num + 2.0f * (s.kn[r][d] * (vr * s.v[o][i]));
      }
    }
    s.x[i] = num / den;
    const float norm = sqrtf(den);
    for (int r = 0; r < n; ++r) s.v[r][i] = s.v[r][i] / norm;
  }
  rw_fence();
}

// One molecule.  Every branch around a fence or a reduction is lane-uniform.
template <int P>
__host__ __device__ inline void huckel_molecule(const HuckelParams& Q, HuckelSmem<P>& s, int b, int lane) {
#pragma clang fp contract(off)
  const int A = Q.in.A, M = Q.in.M;
  int H = 0, E = 0;
  const int gstatus = canon_graph(Q.in, s.g, b, lane, H, E);
  if (gstatus != GAUDI_CANON_OK) {
    if (lane == 0) Q.status[b] = gstatus;
    return;
  }
  const HuckelTab& T = *Q.tab;
  // ---- 1. site classes; the pi centres numbered in ascending atom index (vertices are)
  int n, n_el;
  const int refused = huckel_sites<P>(T, s, H, Q.charge[b], lane, n, n_el);
  if (refused != GAUDI_HUCKEL_OK) {
    if (lane == 0) Q.status[b] = refused;
    return;
  }
  // ---- A = M, V = I; the sparse matrix kept for step 3
  huckel_matrix(T, s, n, lane);
  // ---- 2. Jacobi sweeps
  int sweeps = 0;
  const bool converged = jacobi_sweeps<P>(s, n, lane, kHuckelOff, sweeps);
  // ---- 3. Rayleigh quotients with the matrix the molecule started from; columns normalised
  huckel_rayleigh(s, n, lane);
  // ---- 4. ranks, occupations, the frontier
  const int n_occ = (n_el + 1) >> 1;  // levels holding an electron
  for (int i = lane; i < n; i += kRwLanes) {
    const float xi = s.x[i];
    int rk = 0;
    for (int j = 0; j < n; ++j) {
      const float xj = s.x[j];
      rk += xj > xi || (xj == xi && j < i);
    }
    const int oc = 2 * (rk + 1) <= n_el ? 2 : 2 * rk + 1 == n_el ? 1 : 0;
    s.ord[rk] = (unsigned char)i;
    s.lev[rk] = xi;
    s.occ[rk] = (unsigned char)oc;
    Q.levels[(size_t)b * kHuckelMaxPi + rk] = xi;
    Q.occupation[(size_t)b * kHuckelMaxPi + rk] = (unsigned char)oc;
  }
  rw_fence();
  if (lane == 0) {
    const bool open = n_el & 1;
    int ih = n_occ - 1, il = open ? n_occ - 1 : n_occ;
    if (ih < 0) ih = il;   // no electron: both names go to the lowest level
    if (il >= n) il = ih;  // no empty level: both to the highest
    int flags = open ? GAUDI_HUCKEL_OPEN_SHELL : 0;
    if (n_occ >= 1 && n_occ < n && s.lev[n_occ - 1] - s.lev[n_occ] < kHuckelDegenerate) flags |= GAUDI_HUCKEL_DEGENERATE;
    float e = 0.0f;
    for (int k = 0; k < n_occ; ++k) e = e + (float)s.occ[k] * s.lev[k];
    Q.homo[b] = s.lev[ih];
    Q.lumo[b] = s.lev[il];
    Q.gap[b] = s.lev[ih] - s.lev[il];
    Q.e_pi[b] = e;
    Q.n_pi[b] = n;
    Q.n_electrons[b] = n_el;
    Q.n_excluded[b] = H - n;
    Q.sweeps[b] = sweeps;
    Q.flags[b] = flags;
    Q.status[b] = converged ? GAUDI_HUCKEL_OK : GAUDI_HUCKEL_NOT_CONVERGED;
  }
  const int n_atoms = Q.in.n_atoms[b], n_bonds = Q.in.n_bonds[b];
  for (int a = lane; a < n_atoms; a += kRwLanes) {
    const int hv = s.g.hidx[a];
    Q.site_class[(size_t)b * A + a] = (signed char)(hv == kCanonNone ? -1 : (int)s.vcls[hv]);
  }
  for (int r = lane; r < n; r += kRwLanes) {
    float acc = 0.0f;
    for (int k = 0; k < n_occ; ++k) {
      const float vr = s.v[r][s.ord[k]];
      acc = acc + (float)s.occ[k] * (vr * vr);
    }
    Q.pi_charge[(size_t)b * A + s.g.hv[s.vert[r]]] = (float)T.n_e[s.cls[r]] - acc;
  }
  for (int k = lane; k < n_bonds; k += kRwLanes) {
    const int hi_ = s.g.hidx[s.g.bl[k][0]], hj = s.g.hidx[s.g.bl[k][1]];
    if (hi_ == kCanonNone || hj == kCanonNone) continue;
    const int pr = s.pidx[hi_], ps = s.pidx[hj];
    if (pr == kCanonNone || ps == kCanonNone) continue;
    float acc = 0.0f;
    for (int q = 0; q < n_occ; ++q) {
      const int i = s.ord[q];
      acc = acc + (float)s.occ[q] * (s.v[pr][i] * s.v[ps][i]);
    }
    Q.pi_bond_order[(size_t)b * M + k] = acc;
  }
}

template <int P>
__global__ __launch_bounds__(64) void huckel_kernel(const HuckelParams Q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char huckel_lds[];
  huckel_molecule<P>(Q, *reinterpret_cast<HuckelSmem<P>*>(huckel_lds), Q.mol[blockIdx.x], (int)threadIdx.x);
}

// The table checked and turned into what the kernel reads.  false: GAUDI_HUCKEL_BAD_TABLE.
static bool huckel_table(const gaudi_huckel_tables* t, HuckelTab& out) {
  memset(&out, 0, sizeof(out));
  if (t->n_classes < 1 || t->n_classes > kHuckelMaxClasses) return false;
  for (int c = 0; c < t->n_classes; ++c) {
    if (t->n_e[c] < 0 || t->n_e[c] > 2 || !std::isfinite(t->h[c]) || !std::isfinite(t->k[c])) return false;
    out.n_e[c] = t->n_e[c];
    out.h[c] = t->h[c];
  }
  for (int e = 0; e < kCanonMaxElems; ++e)
    for (int d = 0; d < kHuckelCoords; ++d) {
      const int c = e < t->n_elems ? t->site_class[e][d] : -1;
      if (c < -1 || c >= t->n_classes) return false;
      out.site_class[e][d] = c;
    }
  for (int i = 0; i < t->n_classes; ++i)
    for (int j = 0; j < t->n_classes; ++j) {
#pragma clang fp contract(off)
      const float ij = t->k_pair[i][j], ji = t->k_pair[j][i];
      const bool hij = !std::isnan(ij), hji = !std::isnan(ji);
      if ((hij && std::isinf(ij)) || (hij && hji && ij != ji)) return false;  // a listed pair is finite and the same both ways
      out.kk[i][j] = hij ? ij : hji ? ji : t->k[i] * t->k[j];
    }
  return true;
}

// the smallest tier that holds the molecule's heavy atoms: 0, 1, 2 = 32, 64, 128 (what is larger goes to 128, which decides)
static int huckel_tier(int h_elem, int A, const int32_t* elem, int n) {
  int heavy = 0;
  for (int a = 0; a < n && a < A; ++a) heavy += elem[a] != h_elem;
  return heavy <= 32 ? 0 : heavy <= 64 ? 1 : 2;
}

// the arguments the entry points share, checked; the molecules of each tier, tier after tier in `mol` (ppp.inc routes the same way)
static int huckel_route(int n_elems, int h_elem, int c_elem, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                        const int32_t* bonds, const int32_t* n_bonds, std::vector<int>& mol, int (&tier_n)[3], const char** why) {
  if (int rc = canon_prepare(n_elems, h_elem, c_elem, B, A, M, elem, n_atoms, bonds, n_bonds, why)) return rc;
  if ((long long)B * (A > M ? A : M) > (1ll << 31) || (long long)B * kHuckelMaxPi > (1ll << 31)) {
    *why = "B * max(A, M, 128) beyond 2^31";
    return GAUDI_E_CAPACITY;
  }
  std::vector<int> tier(B);
  tier_n[0] = tier_n[1] = tier_n[2] = 0;
  for (int b = 0; b < B; ++b) ++tier_n[tier[b] = huckel_tier(h_elem, A, elem + (size_t)b * A, n_atoms[b])];
  int at[3] = {0, tier_n[0], tier_n[0] + tier_n[1]};
  mol.resize(B);
  for (int b = 0; b < B; ++b) mol[at[tier[b]]++] = b;
  return GAUDI_OK;
}

// ... and the table
static int huckel_prepare(const gaudi_huckel_tables* t, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                          const int32_t* bonds, const int32_t* n_bonds, HuckelTab& tab, bool& table_ok, std::vector<int>& mol,
                          int (&tier_n)[3], const char** why) {
  *why = "invalid argument";
  if (!t) return GAUDI_E_INVALID;
  if (int rc = huckel_route(t->n_elems, t->h_elem, t->c_elem, B, A, M, elem, n_atoms, bonds, n_bonds, mol, tier_n, why)) return rc;
  table_ok = huckel_table(t, tab);
  return GAUDI_OK;
}

struct HuckelOut {
  float* levels;
  uint8_t* occupation;
  int32_t *n_pi, *n_electrons, *n_excluded, *sweeps, *flags, *status;
  float *homo, *lumo, *gap, *e_pi, *pi_charge, *pi_bond_order;
  int8_t* site_class;
};
constexpr int kHuckelOuts = 15;

static void huckel_out_list(const HuckelOut& o, int B, int A, int M, void* (&p)[kHuckelOuts], size_t (&sz)[kHuckelOuts]) {
  const size_t nB = (size_t)B;
  void* ptrs[kHuckelOuts] = {o.levels, o.occupation, o.n_pi, o.n_electrons, o.n_excluded, o.sweeps, o.flags, o.status,
                             o.homo, o.lumo, o.gap, o.e_pi, o.pi_charge, o.pi_bond_order, o.site_class};
  const size_t sizes[kHuckelOuts] = {4 * nB * kHuckelMaxPi, nB * kHuckelMaxPi, 4 * nB, 4 * nB, 4 * nB, 4 * nB, 4 * nB, 4 * nB,
                                     4 * nB, 4 * nB, 4 * nB, 4 * nB, 4 * nB * A, 4 * nB * M, nB * A};
  for (int i = 0; i < kHuckelOuts; ++i) {
    p[i] = ptrs[i];
    sz[i] = sizes[i];
  }
}

static void huckel_params(HuckelParams& Q, const gaudi_huckel_tables* t, int B, int A, int M, void* (&outs)[kHuckelOuts]) {
  Q.in.B = B;
  Q.in.A = A;
  Q.in.M = M;
  Q.in.n_elems = t->n_elems;
  Q.in.h_elem = t->h_elem;
  Q.in.c_elem = t->c_elem;
  Q.levels = (float*)outs[0];
  Q.occupation = (unsigned char*)outs[1];
  Q.n_pi = (int*)outs[2];
  Q.n_electrons = (int*)outs[3];
  Q.n_excluded = (int*)outs[4];
  Q.sweeps = (int*)outs[5];
  Q.flags = (int*)outs[6];
  Q.status = (int*)outs[7];
  Q.homo = (float*)outs[8];
  Q.lumo = (float*)outs[9];
  Q.gap = (float*)outs[10];
  Q.e_pi = (float*)outs[11];
  Q.pi_charge = (float*)outs[12];
  Q.pi_bond_order = (float*)outs[13];
  Q.site_class = (signed char*)outs[14];
}

template <int P>
static int huckel_launch(gaudi_handle* h, HuckelParams Q, const int* mol, int count) {
  if (count == 0) return GAUDI_OK;
  Q.mol = mol;
  constexpr int lds = (int)sizeof(HuckelSmem<P>);
  {
    // the attribute belongs to the function: one process-wide record per device (see the sampler's launch)
    static std::mutex mu;
    static std::map<int, bool> raised;
    std::lock_guard<std::mutex> lock(mu);
    if (!raised[h->device]) {
      HIPCHECK(h, hipFuncSetAttribute((const void*)huckel_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      raised[h->device] = true;
    }
  }
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (h->prof) HIPCHECK(h, h->huckel_log.begin(h->stream, ev));
  hipLaunchKernelGGL(huckel_kernel<P>, dim3(count), dim3(64), lds, h->stream, Q);
  HIPCHECK(h, hipGetLastError());
  if (h->prof) HIPCHECK(h, h->huckel_log.end(h->stream, ev));
  return GAUDI_OK;
}

template <int P>
static void huckel_host_tier(const HuckelParams& Q, const int* mol, int count) {
  if (count == 0) return;
  std::vector<HuckelSmem<P>> W(1);
  for (int i = 0; i < count; ++i) huckel_molecule<P>(Q, W[0], mol[i], 0);
}

}  // namespace gaudi

#define GAUDI_HUCKEL_ARGS                                                                                                        \
  const gaudi_huckel_tables *tables, int B, int A, int M, const int32_t *elem, const int32_t *n_atoms, const int32_t *bonds,     \
      const int32_t *n_bonds, const int32_t *charge, float *levels_out, uint8_t *occupation_out, int32_t *n_pi_out,              \
      int32_t *n_electrons_out, int32_t *n_excluded_out, int32_t *sweeps_out, int32_t *flags_out, int32_t *status_out,           \
      float *homo_out, float *lumo_out, float *gap_out, float *e_pi_out, float *pi_charge_out, float *pi_bond_order_out,         \
      int8_t *site_class_out
#define GAUDI_HUCKEL_OUT                                                                                                         \
  gaudi::HuckelOut {                                                                                                             \
    levels_out, occupation_out, n_pi_out, n_electrons_out, n_excluded_out, sweeps_out, flags_out, status_out, homo_out,          \
        lumo_out, gap_out, e_pi_out, pi_charge_out, pi_bond_order_out, site_class_out                                            \
  }

extern "C" int gaudi_huckel(gaudi_handle* h, GAUDI_HUCKEL_ARGS) {
  if (!h) return GAUDI_E_INVALID;
  void* outs[gaudi::kHuckelOuts];
  size_t osz[gaudi::kHuckelOuts];
  gaudi::huckel_out_list(GAUDI_HUCKEL_OUT, B > 0 ? B : 0, A, M, outs, osz);
  for (void* p : outs)
    if (!p) return fail(h, GAUDI_E_INVALID, "every output array is required");
  const char* why = "";
  std::vector<gaudi::HuckelTab> tab(1);
  std::vector<int> mol;
  int tier_n[3];
  bool table_ok = false;
  if (int rc = gaudi::huckel_prepare(tables, B, A, M, elem, n_atoms, bonds, n_bonds, tab[0], table_ok, mol, tier_n, &why))
    return fail(h, rc, why);
  if (B == 0) return GAUDI_OK;
  if (!table_ok) {  // nothing runs on a table that cannot be read: every row zero
    for (int i = 0; i < gaudi::kHuckelOuts; ++i) memset(outs[i], 0, osz[i]);
    for (int b = 0; b < B; ++b) status_out[b] = GAUDI_HUCKEL_BAD_TABLE;
    return GAUDI_OK;
  }
  HIPCHECK(h, hipSetDevice(h->device));
  const size_t nB = (size_t)B;
  std::vector<int32_t> zero;
  if (!charge) zero.assign(nB, 0);
  constexpr int kIn = 7;
  const size_t isz[kIn] = {sizeof(int) * nB * A, sizeof(int) * nB, sizeof(int) * nB * M * 2, sizeof(int) * nB, sizeof(int) * nB,
                           sizeof(int) * nB,     sizeof(gaudi::HuckelTab)};
  const void* ins[kIn] = {elem, n_atoms, bonds, n_bonds, charge ? charge : zero.data(), mol.data(), tab.data()};
  for (int i = 0; i < kIn; ++i) {
    HIPCHECK(h, h->d_huckel[i].reserve(isz[i]));
    HIPCHECK(h, hipMemcpyAsync(h->d_huckel[i].p, ins[i], isz[i], hipMemcpyHostToDevice, h->stream));
  }
  void* douts[gaudi::kHuckelOuts];
  for (int i = 0; i < gaudi::kHuckelOuts; ++i) {  // a refused molecule writes its status only: zero everywhere else
    HIPCHECK(h, h->d_huckel[kIn + i].reserve(osz[i]));
    HIPCHECK(h, hipMemsetAsync(h->d_huckel[kIn + i].p, 0, osz[i], h->stream));
    douts[i] = h->d_huckel[kIn + i].p;
  }
  gaudi::HuckelParams Q{};
  gaudi::huckel_params(Q, tables, B, A, M, douts);
  Q.in.elem = h->d_huckel[0].as<int>();
  Q.in.n_atoms = h->d_huckel[1].as<int>();
  Q.in.bonds = h->d_huckel[2].as<int>();
  Q.in.n_bonds = h->d_huckel[3].as<int>();
  Q.charge = h->d_huckel[4].as<int>();
  Q.tab = h->d_huckel[6].as<gaudi::HuckelTab>();
  const int* dmol = h->d_huckel[5].as<int>();
  if (int rc = gaudi::huckel_launch<32>(h, Q, dmol, tier_n[0])) return rc;
  if (int rc = gaudi::huckel_launch<64>(h, Q, dmol + tier_n[0], tier_n[1])) return rc;
  if (int rc = gaudi::huckel_launch<128>(h, Q, dmol + tier_n[0] + tier_n[1], tier_n[2])) return rc;
  for (int i = 0; i < gaudi::kHuckelOuts; ++i)
    HIPCHECK(h, hipMemcpyAsync(outs[i], douts[i], osz[i], hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  return GAUDI_OK;
}

extern "C" int gaudi_host_huckel(GAUDI_HUCKEL_ARGS) {
  void* outs[gaudi::kHuckelOuts];
  size_t osz[gaudi::kHuckelOuts];
  gaudi::huckel_out_list(GAUDI_HUCKEL_OUT, B > 0 ? B : 0, A, M, outs, osz);
  for (void* p : outs)
    if (!p) return GAUDI_E_INVALID;
  const char* why = "";
  std::vector<gaudi::HuckelTab> tab(1);
  std::vector<int> mol;
  int tier_n[3];
  bool table_ok = false;
  if (int rc = gaudi::huckel_prepare(tables, B, A, M, elem, n_atoms, bonds, n_bonds, tab[0], table_ok, mol, tier_n, &why)) return rc;
  if (B == 0) return GAUDI_OK;
  for (int i = 0; i < gaudi::kHuckelOuts; ++i) memset(outs[i], 0, osz[i]);
  if (!table_ok) {
    for (int b = 0; b < B; ++b) status_out[b] = GAUDI_HUCKEL_BAD_TABLE;
    return GAUDI_OK;
  }
  std::vector<int32_t> zero;
  if (!charge) zero.assign((size_t)B, 0);
  gaudi::HuckelParams Q{};
  gaudi::huckel_params(Q, tables, B, A, M, outs);
  Q.in.elem = elem;
  Q.in.n_atoms = n_atoms;
  Q.in.bonds = bonds;
  Q.in.n_bonds = n_bonds;
  Q.charge = charge ? charge : zero.data();
  Q.tab = tab.data();
  gaudi::huckel_host_tier<32>(Q, mol.data(), tier_n[0]);
  gaudi::huckel_host_tier<64>(Q, mol.data() + tier_n[0], tier_n[1]);
  gaudi::huckel_host_tier<128>(Q, mol.data() + tier_n[0] + tier_n[1], tier_n[2]);
  return GAUDI_OK;
}
#undef GAUDI_HUCKEL_ARGS
#undef GAUDI_HUCKEL_OUT

extern "C" int gaudi_huckel_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms) {
  if (!h || !n_launches || !total_ms) return GAUDI_E_INVALID;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, h->huckel_log.fold(0));
  *n_launches = (int32_t)h->huckel_log.n;
  *total_ms = h->huckel_log.ms;
  return GAUDI_OK;
}
