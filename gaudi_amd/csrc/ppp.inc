// ppp.inc -- Pariser-Parr-Pople self-consistent pi levels, gap, charges and bond orders in eV of a graph of atoms with coordinates
// (included after huckel.inc at the end of gaudi_hip.hip; DESIGN.md section 8m; the model is spelled out in include/gaudi_hip.h).
//
// The pi centres are huckel.inc's: canon_graph, coordination = heavy degree + H count, the table's site classes, the centres
// numbered in ascending atom index.  ONE text, two builds, as huckel.inc: a 64-lane wave per molecule on the device, one lane that
// walks every index on the host (kRwLanes).  Per molecule:
//   1. canon_graph; sites classified and compacted; per centre its coordinates, I, gamma, z and its (at most four) bonds with
//      their beta in LDS; the geometry checked; H_rr and the core repulsion (both functions of the geometry alone);
//   2. the SCF loop.  a = F(P), v = I; jacobi_sweeps (huckel.inc) diagonalises; the columns are normalised and ranked by the
//      rotated diagonal; P_new = 2 sum over the occupied columns, delta_p = max |P_new - P|, P = (1 - damping) P_new + damping P;
//   3. after the loop P = P_new of the last eigenvectors, a = F(P); the levels are the dense Rayleigh quotients v^T F v, ranked
//      again; occupations, frontier, energies, charges and bond orders from these ranks.
// gamma_rs is recomputed from the coordinates wherever it is needed (a sqrt and a division: n^2 per iteration against the solver's
// n^3), and it is the same bits for (r, s) and (s, r): every operand pair enters a commutative operation.
// WHERE P LIVES: a and v are 132 KB of the CU's 160 KB in the 128 tier, so P is a row of global scratch per workgroup, P * P floats.
// Every loop that writes P_rc and every loop that reads it runs c over the lane's own columns (c = lane, lane + 64, ...), so a lane
// only ever reads what it wrote itself and global memory needs no cross-lane ordering.  What every lane needs of P, its diagonal,
// is kept in LDS (s.pd) behind rw_fence.  On the host the scratch is a vector.
// THE CIS STAGE (ppp_cis.inc, gaudi_ppp_cis) is a second kernel: with Q.cis set, a molecule that solved leaves what that stage
// needs in a row of global scratch (ppp_cis_handover); with Q.cis null (gaudi_ppp) nothing is written and nothing changes.
// Every fp32 operation is individually rounded (contraction off, correctly rounded / and sqrtf) and every sum runs in one fixed
// order; delta_p and the diagonal maximum are reduced through their bits.  No atomics.  Every branch around a fence or a reduction
// is lane-uniform.
// OPEN SHELLS (ppp_open.inc, gaudi_ppp_open; DESIGN.md section 8s): ppp_molecule<P, true> is the same text with Dewar's half-electron
// occupations 2 / 1 / 0 -- a row is (molecule, charge, multiplicity) -- and, after the eighteen outputs, the state energy in fp64,
// the spin density and the singly occupied ranks.  Every addition stands behind `if constexpr (Open)`: ppp_molecule<P, false> is
// operation for operation what it was.
// PULAY'S DIIS (ppp_scf.inc, gaudi_ppp_scf; DESIGN.md section 8t): ppp_molecule<P, true, true> is the same text again with a ring of
// Fock matrices and commutators behind the density in the scratch row ([1 + 2 * diis_size][P * P] floats, every matrix under the
// density's own rule: a lane reads only the columns it wrote).  Every addition stands behind `if constexpr (Diis)`:
// ppp_molecule<P, *, false> is operation for operation what it was.

namespace gaudi {

constexpr int kPppIterations = GAUDI_PPP_MAX_ITERATIONS;
constexpr float kPppCoulomb = 14.397f;         // e^2 / (4 pi eps0) in eV Angstrom
constexpr float kPppDeltaP = 1.52587890625e-5f;  // 2^-16
constexpr float kPppTooClose2 = 0.25f;         // (0.5 Angstrom)^2
constexpr float kPppDegenerate = 1e-3f;        // eV
constexpr int kPppDiisMax = GAUDI_PPP_DIIS_MAX;  // the longest history of ppp_molecule<P, Open, true>
constexpr float kPppDiisError = GAUDI_PPP_DIIS_ERROR;  // eV: the commutator a converged row may be left with (section 8t)
static_assert(GAUDI_PPP_OPEN_TIE == 2 * GAUDI_PPP_CIS_TRIPLET_UNSTABLE, "the next free bit of flags");
// The hand-over to the CIS stage (ppp_cis.inc): a row of global scratch per molecule, in floats.  n and n_occ as their bits, the
// separation of the window's edge level from the level just outside it on either side (-1: no level outside), the centres'
// coordinates and gamma, the active levels (0..7 occupied in ascending rank, 8..15 empty) and their eigenvector columns; behind
// them the CIS stage's own stash of its two matrices.
constexpr int kCisMaxWindow = GAUDI_PPP_CIS_MAX_WINDOW, kCisAct = 2 * kCisMaxWindow;
constexpr int kCisXyz = 4, kCisGam = kCisXyz + 3 * kHuckelMaxPi, kCisEps = kCisGam + kHuckelMaxPi, kCisCoef = kCisEps + kCisAct;
constexpr int kCisMatS = kCisCoef + kCisAct * kHuckelMaxPi, kCisMatT = kCisMatS + GAUDI_PPP_CIS_MAX_STATES * GAUDI_PPP_CIS_MAX_STATES;
constexpr int kCisRow = kCisMatT + GAUDI_PPP_CIS_MAX_STATES * GAUDI_PPP_CIS_MAX_STATES;
static_assert(GAUDI_PPP_OPEN_SHELL > GAUDI_HUCKEL_BAD_TABLE && GAUDI_PPP_BAD_GEOMETRY > GAUDI_HUCKEL_BAD_TABLE &&
                  GAUDI_PPP_DEGENERATE == GAUDI_HUCKEL_DEGENERATE,
              "the shared statuses and flags keep gaudi_huckel's values");

// the table as the kernel reads it (ppp_table builds it from gaudi_ppp_tables)
struct PppTab {
  int site_class[kCanonMaxElems][kHuckelCoords];  // -1: not a pi centre
  int z[kHuckelMaxClasses];
  float ion[kHuckelMaxClasses], gam[kHuckelMaxClasses];
  float beta[kHuckelMaxClasses][kHuckelMaxClasses];  // the resonance integral of a bonded pair of classes
};

template <int P>
struct PppSmem {
  CanonSmem g;
  float a[P][P + 1], v[P][P + 1];
  float xyz[P][3], ion[P], gam[P], zc[P];  // per centre: coordinates, I, gamma, z
  float hd[P], pd[P];                      // H_rr; P_rr
  float bn[P][kHuckelNbr];                 // beta of a centre's bonds
  float x[P], lev[P];                      // levels by column (and per-column partial sums); by rank
  float rc[P / 2], rs[P / 2], rpp[P / 2], rqq[P / 2];  // jacobi_sweeps' rotations
  unsigned char rp[P / 2], rq[P / 2];
  unsigned char nb[P][kHuckelNbr];   // a centre's bonded centres, none-padded
  unsigned char vert[P];             // pi centre -> vertex
  unsigned char ord[P];              // rank -> column
  signed char cls[P];
  unsigned char pidx[kCanonMaxHeavy];  // vertex -> pi centre, none for an excluded atom
  signed char vcls[kCanonMaxHeavy];    // vertex -> site class, -1 for an excluded atom
  double xd[P];                        // per-column partial sums in fp64 (ppp_molecule<P, true> only; last, so that every other
                                       // member keeps the offset it had)
  double db[kPppDiisMax][kPppDiisMax];          // ppp_molecule<P, true, true> only (ppp_scf.inc): B by ring slot, and the bordered
  double dm[kPppDiisMax + 1][kPppDiisMax + 2];  // system with its right-hand side
};
static_assert(sizeof(PppSmem<128>) <= 160 * 1024, "the largest tier fits the LDS of a CU");

struct PppParams {
  CanonParams in;  // the input fields only
  const int* mol;  // the molecules of this launch (one capacity tier)
  const int* charge;
  const float* xyz;  // [B][A][3]
  const PppTab* tab;
  float* scratch;    // [workgroups of the launch][P * P]: the density matrix
  float* cis;        // [B][kCisRow]: the hand-over to the CIS stage; null: none
  int window;        // ... and its active window
  int repulsion;
  float damping;
  float* levels;              // [B][kHuckelMaxPi]
  unsigned char* occupation;  // [B][kHuckelMaxPi]
  float* pi_charge;           // [B][A]
  float* pi_bond_order;       // [B][M]
  signed char* site_class;    // [B][A]
  int *n_pi, *n_electrons, *n_excluded, *iterations, *sweeps, *flags, *status;  // [B]
  float *homo, *lumo, *gap, *e_electronic, *e_core, *delta_p;                   // [B]
  // gaudi_ppp_open only (ppp_molecule<P, true>)
  const int* multiplicity;  // [B]
  float* spin_density;      // [B][A]
  double *e_state, *he_correction;  // [B]
  int *n_open, *somo;       // [B]; [B][2]
  // gaudi_ppp_scf only (ppp_molecule<P, true, true>); scratch is then [workgroups of the launch][1 + 2 * diis_size][P * P]
  int diis_size, diis_start;
  float* diis_error;    // [B]
  int* n_extrapolated;  // [B]
};

// gamma_rs, r != s: symmetric in its bits.  S is any work space with xyz and gam (ppp_cis.inc has one).
template <class S>
__host__ __device__ __forceinline__ float ppp_gamma(const S& s, int r, int c, int repulsion) {
#pragma clang fp contract(off)
  const float dx = s.xyz[r][0] - s.xyz[c][0], dy = s.xyz[r][1] - s.xyz[c][1], dz = s.xyz[r][2] - s.xyz[c][2];
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  const float a = (2.0f * kPppCoulomb) / (s.gam[r] + s.gam[c]);
  return repulsion == GAUDI_PPP_OHNO ? kPppCoulomb / sqrtf(d2 + a * a) : kPppCoulomb / (sqrtf(d2) + a);
}

// beta_rc: the bond list of centre c searched for r
template <int P>
__host__ __device__ __forceinline__ float ppp_beta(const PppSmem<P>& s, int r, int c) {
  float b = 0.0f;
  for (int d = 0; d < kHuckelNbr; ++d) b = s.nb[c][d] == r ? s.bn[c][d] : b;
  return b;
}

// a = F(P) from the scratch row and s.pd.  The lane's own columns; the column's diagonal element from the same trip.
template <int P>
__host__ __device__ inline void ppp_fock(PppSmem<P>& s, const float* pm, int n, int lane, int repulsion) {
#pragma clang fp contract(off)
  for (int c = lane; c < n; c += kRwLanes) {
    float coul = 0.0f;
    for (int r = 0; r < n; ++r) {
      if (r == c) continue;
      const float g = ppp_gamma(s, r, c, repulsion);
      coul = coul + (s.pd[r] - s.zc[r]) * g;
      s.a[r][c] = ppp_beta(s, r, c) - 0.5f * pm[r * P + c] * g;
    }
    s.a[c][c] = (0.5f * s.pd[c] * s.gam[c] - s.ion[c]) + coul;
  }
}

// P_rc of the ranked columns: twice the n_occ doubly occupied ones, and once the n_open singly occupied ones behind them.
template <int P, bool Open>
__host__ __device__ __forceinline__ float ppp_density(const PppSmem<P>& s, int r, int c, int n_occ, int n_open) {
#pragma clang fp contract(off)
  float acc = 0.0f;
  for (int k = 0; k < n_occ; ++k) {
    const int i = s.ord[k];
    acc = acc + s.v[r][i] * s.v[c][i];
  }
  float p = 2.0f * acc;
  if constexpr (Open) {
    if (n_open > 0) {
      float half = 0.0f;
      for (int k = n_occ; k < n_occ + n_open; ++k) {
        const int i = s.ord[k];
        half = half + s.v[r][i] * s.v[c][i];
      }
      p = p + half;
    }
  }
  return p;
}

// Whether the levels on either boundary of the open set (ranks n_occ - 1 | n_occ, n_occ + n_open - 1 | n_occ + n_open) are closer
// than kPppDegenerate; lev(rank) reads a ranked level.  Every lane computes the same answer from LDS.
template <class L>
__host__ __device__ __forceinline__ bool ppp_open_tie(const L& lev, int n, int n_occ, int n_open) {
#pragma clang fp contract(off)
  if (n_open == 0) return false;
  const int top = n_occ + n_open;
  bool tie = false;
  if (n_occ >= 1) tie = lev(n_occ) - lev(n_occ - 1) < kPppDegenerate;
  if (top < n) tie = tie || lev(top) - lev(top - 1) < kPppDegenerate;
  return tie;
}

// What the CIS stage needs of a solved molecule, written to its hand-over row (the layout above); s.ord and s.lev are the final ranks.
template <int P>
__host__ __device__ inline void ppp_cis_handover(const PppParams& Q, const PppSmem<P>& s, int b, int n, int n_occ, int lane) {
#pragma clang fp contract(off)
  float* row = Q.cis + (size_t)b * kCisRow;
  const int W = Q.window, n_virt = n - n_occ;
  const int n_o = n_occ < W ? n_occ : W, n_v = n_virt < W ? n_virt : W, first = n_occ - n_o, last = n_occ + n_v;
  if (lane == 0) {
    row[0] = __builtin_bit_cast(float, n);
    row[1] = __builtin_bit_cast(float, n_occ);
    row[2] = n_o > 0 && first > 0 ? s.lev[first] - s.lev[first - 1] : -1.0f;
    row[3] = n_v > 0 && last < n ? s.lev[last] - s.lev[last - 1] : -1.0f;
  }
  for (int r = lane; r < n; r += kRwLanes) {
    for (int k = 0; k < 3; ++k) row[kCisXyz + 3 * r + k] = s.xyz[r][k];
    row[kCisGam + r] = s.gam[r];
  }
  for (int q = lane; q < kCisAct; q += kRwLanes) {
    const int rank = q < kCisMaxWindow ? (q < n_o ? first + q : -1) : (q - kCisMaxWindow < n_v ? n_occ + q - kCisMaxWindow : -1);
    row[kCisEps + q] = rank < 0 ? 0.0f : s.lev[rank];
  }
  for (int q = 0; q < kCisAct; ++q) {
    const int rank = q < kCisMaxWindow ? (q < n_o ? first + q : -1) : (q - kCisMaxWindow < n_v ? n_occ + q - kCisMaxWindow : -1);
    const int col = rank < 0 ? 0 : s.ord[rank];
    for (int r = lane; r < n; r += kRwLanes) row[kCisCoef + q * kHuckelMaxPi + r] = rank < 0 ? 0.0f : s.v[r][col];
  }
}

// One molecule; `pm` is its scratch row.  Every branch around a fence or a reduction is lane-uniform.
template <int P>
__host__ __device__ inline float ppp_diis_error(PppSmem<P>& s, const float* pm, float* f_slot, float* e_slot, int n, int lane);
template <int P>
__host__ __device__ inline void ppp_diis_products(PppSmem<P>& s, const float* es, int size, int head, int len, int n, int lane);
template <int P>
__host__ __device__ inline int ppp_diis_solve(PppSmem<P>& s, int size, int& head, int& len, int lane);
template <int P>
__host__ __device__ inline void ppp_diis_combine(PppSmem<P>& s, const float* fs, int size, int head, int len, int n, int lane);

template <int P, bool Open = false, bool Diis = false>
__host__ __device__ inline void ppp_molecule(const PppParams& Q, PppSmem<P>& s, float* pm, int b, int lane) {
#pragma clang fp contract(off)
  const int A = Q.in.A, M = Q.in.M;
  int H = 0, E = 0;
  const int gstatus = canon_graph(Q.in, s.g, b, lane, H, E);
  if (gstatus != GAUDI_CANON_OK) {
    if (lane == 0) Q.status[b] = gstatus;
    return;
  }
  const PppTab& T = *Q.tab;
  // ---- 1. site classes; the pi centres numbered in ascending atom index (huckel.inc, step 1)
  const int per = (H + kRwLanes - 1) / kRwLanes, lo = lane * per, hi = lo + per < H ? lo + per : H;
  int cnt = 0, el = 0;
  for (int v = lo; v < hi; ++v) {
    const int label = s.g.label[v];
    int coord = label & 7;
    for (int k = 0; k < kCanonDeg; ++k) coord += s.g.adj[v][k] != kCanonNone;
    const int c = coord < kHuckelCoords ? T.site_class[label >> 3][coord] : -1;
    s.vcls[v] = (signed char)c;
    cnt += c >= 0;
    el += c >= 0 ? T.z[c] : 0;
  }
  int n, n_el;
  int pos = rw_scan(cnt, lane, n);
  (void)rw_scan(el, lane, n_el);
  n_el -= Q.charge[b];
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
  int refused = GAUDI_HUCKEL_OK;
  if (n == 0) refused = GAUDI_HUCKEL_NO_PI;
  else if (n > P) refused = GAUDI_HUCKEL_OVERFLOW;  // (the host sends a molecule to a tier that holds its heavy atoms: P is 128 here)
  else if (n_el < 0 || n_el > 2 * n) refused = GAUDI_HUCKEL_BAD_INPUT;  // a charge the pi system cannot carry
  else if (!Open && (n_el & 1)) refused = GAUDI_PPP_OPEN_SHELL;
  int n_open = 0;
  if constexpr (Open) {  // the multiplicity: 0 is the lowest the parity allows; n_open = multiplicity - 1 singly occupied levels
    const int asked = Q.multiplicity[b];
    if (asked >= 0 && asked <= 3) n_open = (asked == 0 ? 1 + (n_el & 1) : asked) - 1;  // (only then: no arithmetic on a wild value)
    if (refused == GAUDI_HUCKEL_OK &&
        (asked < 0 || asked > 3 || n_el < n_open || ((n_el - n_open) & 1) || ((n_el - n_open) >> 1) + n_open > n))
      refused = GAUDI_HUCKEL_BAD_INPUT;
  }
  if (refused != GAUDI_HUCKEL_OK) {
    if (lane == 0) Q.status[b] = refused;
    return;
  }
  rw_fence();
  // ---- per centre: coordinates, parameters, bonds
  bool bad = false;
  for (int r = lane; r < n; r += kRwLanes) {
    const int v = s.vert[r], cr = s.cls[r];
    const float* at = Q.xyz + ((size_t)b * A + s.g.hv[v]) * 3;
    for (int k = 0; k < 3; ++k) {
      const float t = at[k];
      bad = bad || (huckel_bits(t) & 0x7f800000) == 0x7f800000;  // infinite or not a number
      s.xyz[r][k] = t;
    }
    s.ion[r] = T.ion[cr];
    s.gam[r] = T.gam[cr];
    s.zc[r] = (float)T.z[cr];
    s.pd[r] = (float)T.z[cr];  // P starts as diag(z)
    int d = 0;
    for (int k = 0; k < kCanonDeg; ++k) {
      const int o = s.g.adj[v][k];
      if (o == kCanonNone) continue;
      const int ps = s.pidx[o];
      if (ps == kCanonNone) continue;
      if (d < kHuckelNbr) {
        s.nb[r][d] = (unsigned char)ps;
        s.bn[r][d] = T.beta[cr][s.cls[ps]];
      }
      ++d;
    }
    for (; d < kHuckelNbr; ++d) {
      s.nb[r][d] = (unsigned char)kCanonNone;
      s.bn[r][d] = 0.0f;
    }
  }
  rw_fence();
  if (!rw_any(bad)) {
    for (int c = lane; c < n; c += kRwLanes)
      for (int r = 0; r < c; ++r) {
        const float dx = s.xyz[r][0] - s.xyz[c][0], dy = s.xyz[r][1] - s.xyz[c][1], dz = s.xyz[r][2] - s.xyz[c][2];
        bad = bad || !((dx * dx + dy * dy) + dz * dz >= kPppTooClose2);  // (an overflow to infinity passes: gamma_rs is then 0)
      }
    bad = rw_any(bad);
  } else {
    bad = true;
  }
  if (bad) {
    if (lane == 0) Q.status[b] = GAUDI_PPP_BAD_GEOMETRY;
    return;
  }
  // ---- H_rr and the core repulsion; P = diag(z) in the scratch row
  const int repulsion = Q.repulsion;
  for (int c = lane; c < n; c += kRwLanes) {
    float att = 0.0f, rep = 0.0f;
    [[maybe_unused]] double rep64 = 0.0;
    for (int r = 0; r < n; ++r) {
      pm[r * P + c] = r == c ? s.zc[c] : 0.0f;
      if (r == c) continue;
      const float g = ppp_gamma(s, r, c, repulsion);
      att = att + s.zc[r] * g;
      if (r < c) rep = rep + (s.zc[r] * s.zc[c]) * g;
      if constexpr (Open)
        if (r < c) rep64 = rep64 + (double)((s.zc[r] * s.zc[c]) * g);
    }
    s.hd[c] = -s.ion[c] - att;
    s.x[c] = rep;
    if constexpr (Open) s.xd[c] = rep64;
  }
  rw_fence();
  float e_core = 0.0f;
  double e_core64 = 0.0;
  if (lane == 0) {
    for (int c = 0; c < n; ++c) e_core = e_core + s.x[c];
    if constexpr (Open)
      for (int c = 0; c < n; ++c) e_core64 = e_core64 + s.xd[c];
  }
  rw_fence();
  // ---- 2. the SCF loop
  const int n_occ = (n_el - n_open) >> 1;  // the doubly occupied levels
  bool tie = false;
  const float damping = Q.damping, fresh = 1.0f - damping;
  float threshold = 0.0f, delta = 0.0f;
  int iterations = 0, sweeps = 0;
  bool converged = false, jacobi_ok = true;
  [[maybe_unused]] int head = 0, len = 0, n_extrapolated = 0;  // the ring: its oldest slot and its length
  [[maybe_unused]] float diis_error = 0.0f;
  for (;;) {
    ppp_fock(s, pm, n, lane, repulsion);
    if constexpr (Diis) {
      static_assert(Open, "the DIIS path is built on the open-shell text");
      if (iterations + 1 >= Q.diis_start) {  // (lane-uniform: the iteration, the ring's length and the retries belong to the row)
        const int size = Q.diis_size;
        float* fs = pm + P * P;
        float* es = fs + (size_t)size * (P * P);
        rw_fence();
        if (len == size) {  // the oldest entry leaves
          head = head + 1 == size ? 0 : head + 1;
          --len;
        }
        const int slot = (head + len) % size;
        diis_error = ppp_diis_error(s, pm, fs + (size_t)slot * (P * P), es + (size_t)slot * (P * P), n, lane);
        ++len;
        ppp_diis_products(s, es, size, head, len, n, lane);
        const int used = ppp_diis_solve(s, size, head, len, lane);
        if (used >= 2) {
          ppp_diis_combine(s, fs, size, head, len, n, lane);
          ++n_extrapolated;
        }
      }
    }
    for (int r = 0; r < n; ++r)
      for (int c = lane; c < n; c += kRwLanes) s.v[r][c] = r == c ? 1.0f : 0.0f;
    rw_fence();
    if (iterations == 0) {  // the solver's threshold: 2^-24 of the largest |F_rr|, rounded up to a power of two
      float big = 0.0f;
      for (int r = lane; r < n; r += kRwLanes) {
        const float t = fabsf(s.a[r][r]);
        big = t > big ? t : big;
      }
      const int bits = -rw_min(-huckel_bits(big));
      int e = (bits >> 23) + ((bits & 0x7fffff) != 0) - 24;  // the biased exponent of 2^-24 times that power of two
      e = e < 1 ? 1 : e > 254 ? 254 : e;
      threshold = __builtin_bit_cast(float, e << 23);
    }
    jacobi_ok = jacobi_sweeps<P>(s, n, lane, threshold, sweeps) && jacobi_ok;
    ++iterations;
    for (int i = lane; i < n; i += kRwLanes) {  // columns normalised; the level of a column: the rotated diagonal
      float den = 0.0f;
      for (int r = 0; r < n; ++r) {
        const float vr = s.v[r][i];
        den = den + vr * vr;
      }
      const float norm = sqrtf(den);
      for (int r = 0; r < n; ++r) s.v[r][i] = s.v[r][i] / norm;
      s.x[i] = s.a[i][i];
    }
    rw_fence();
    for (int i = lane; i < n; i += kRwLanes) {
      const float xi = s.x[i];
      int rk = 0;
      for (int j = 0; j < n; ++j) {
        const float xj = s.x[j];
        rk += xj < xi || (xj == xi && j < i);
      }
      s.ord[rk] = (unsigned char)i;
    }
    rw_fence();
    if constexpr (Open) tie = tie || ppp_open_tie([&](int k) { return s.x[s.ord[k]]; }, n, n_occ, n_open);
    float worst = 0.0f;
    for (int c = lane; c < n; c += kRwLanes)
      for (int r = 0; r < n; ++r) {
        const float fresh_p = ppp_density<P, Open>(s, r, c, n_occ, n_open), old = pm[r * P + c], d = fabsf(fresh_p - old);
        worst = d > worst ? d : worst;
        float mixed = fresh * fresh_p + damping * old;
        if constexpr (Diis)
          if (iterations >= Q.diis_start) mixed = fresh_p;  // no damping once the history runs
        pm[r * P + c] = mixed;
        if (r == c) s.pd[c] = mixed;
      }
    delta = __builtin_bit_cast(float, -rw_min(-huckel_bits(worst)));
    rw_fence();
    converged = delta <= kPppDeltaP;
    if constexpr (Diis) converged = converged && diis_error <= kPppDiisError;  // (a stagnant history reads delta_p = 0)
    if (converged || iterations == kPppIterations) break;
  }
  // ---- 3. P = P_new of the last eigenvectors; a = F(P); levels = v^T F v
  for (int c = lane; c < n; c += kRwLanes)
    for (int r = 0; r < n; ++r) {
      const float p = ppp_density<P, Open>(s, r, c, n_occ, n_open);
      pm[r * P + c] = p;
      if (r == c) s.pd[c] = p;
    }
  rw_fence();
  ppp_fock(s, pm, n, lane, repulsion);
  rw_fence();
  for (int i = lane; i < n; i += kRwLanes) {
    float num = 0.0f;
    for (int r = 0; r < n; ++r) {
      float row = 0.0f;
      for (int c = 0; c < n; ++c) row = row + s.a[r][c] * s.v[c][i];
      num = num + s.v[r][i] * row;
    }
    s.x[i] = num;
  }
  rw_fence();
  for (int i = lane; i < n; i += kRwLanes) {
    const float xi = s.x[i];
    int rk = 0;
    for (int j = 0; j < n; ++j) {
      const float xj = s.x[j];
      rk += xj < xi || (xj == xi && j < i);
    }
    const int oc = rk < n_occ ? 2 : rk < n_occ + n_open ? 1 : 0;
    s.ord[rk] = (unsigned char)i;
    s.lev[rk] = xi;
    Q.levels[(size_t)b * kHuckelMaxPi + rk] = xi;
    Q.occupation[(size_t)b * kHuckelMaxPi + rk] = (unsigned char)oc;
  }
  rw_fence();
  if (Q.cis && converged && jacobi_ok) ppp_cis_handover(Q, s, b, n, n_occ, lane);
  // the density of these ranks: the energy by columns, the charges from its diagonal
  for (int c = lane; c < n; c += kRwLanes) {
    float e = 0.0f;
    [[maybe_unused]] double e64 = 0.0;
    for (int r = 0; r < n; ++r) {
      const float p = ppp_density<P, Open>(s, r, c, n_occ, n_open), f = s.a[r][c];
      const float hf = (r == c ? s.hd[c] : ppp_beta(s, r, c)) + f;
      e = e + p * hf;
      if constexpr (Open) e64 = e64 + (double)p * (double)hf;
      if (r == c) Q.pi_charge[(size_t)b * A + s.g.hv[s.vert[c]]] = s.zc[c] - p;
    }
    s.x[c] = e;
    if constexpr (Open) {
      s.xd[c] = e64;
      float spin = 0.0f;
      for (int k = n_occ; k < n_occ + n_open; ++k) {
        const float vc = s.v[c][s.ord[k]];
        spin = spin + vc * vc;
      }
      Q.spin_density[(size_t)b * A + s.g.hv[s.vert[c]]] = spin;
    }
  }
  rw_fence();
  if constexpr (Open) {
    // the state energy in fp64 from the fp32 elements: E_he = 1/2 sum P (H + F); the half-electron correction
    // -J_mm / 4 (doublet), -(J_mm + J_nn) / 4 - K_mn / 2 (triplet), by columns and then over the columns in ascending order
    double e_he = 0.0, corr = 0.0;
    if (lane == 0)
      for (int c = 0; c < n; ++c) e_he = e_he + s.xd[c];
    rw_fence();
    if (n_open > 0) {
      const int m = s.ord[n_occ], q = s.ord[n_occ + n_open - 1];  // the open columns (the same one for a doublet)
      for (int c = lane; c < n; c += kRwLanes) {
        const double cm = (double)s.v[c][m], cq = (double)s.v[c][q];
        double jm = 0.0, jq = 0.0, kx = 0.0;
        for (int r = 0; r < n; ++r) {
          const double g = (double)(r == c ? s.gam[c] : ppp_gamma(s, r, c, repulsion));
          const double rm = (double)s.v[r][m], rq = (double)s.v[r][q];
          jm = jm + ((rm * rm) * (cm * cm)) * g;
          jq = jq + ((rq * rq) * (cq * cq)) * g;
          kx = kx + ((rm * rq) * (cm * cq)) * g;
        }
        s.xd[c] = n_open == 1 ? 0.25 * jm : 0.25 * (jm + jq) + 0.5 * kx;
      }
      rw_fence();
      if (lane == 0)
        for (int c = 0; c < n; ++c) corr = corr + s.xd[c];
    }
    if (lane == 0) {
      Q.he_correction[b] = 0.0 - corr;
      Q.e_state[b] = (0.5 * e_he - corr) + e_core64;
      Q.n_open[b] = n_open;
      for (int k = 0; k < 2; ++k) Q.somo[(size_t)b * 2 + k] = k < n_open ? n_occ + k : -1;
    }
    tie = tie || ppp_open_tie([&](int k) { return s.lev[k]; }, n, n_occ, n_open);
  }
  if (lane == 0) {
    int ih = n_occ + n_open - 1, il = n_occ + n_open;
    if (ih < 0) ih = il;   // no electron: both names go to the lowest level
    if (il >= n) il = ih;  // no empty level: both to the highest
    int flags = 0;
    if (il > ih && s.lev[il] - s.lev[ih] < kPppDegenerate) flags |= GAUDI_PPP_DEGENERATE;
    if (tie) flags |= GAUDI_PPP_OPEN_TIE;
    if (!converged) flags |= GAUDI_PPP_SCF_CAP;
    if (!jacobi_ok) flags |= GAUDI_PPP_JACOBI_CAP;
    float e = 0.0f;
    for (int c = 0; c < n; ++c) e = e + s.x[c];
    Q.homo[b] = s.lev[ih];
    Q.lumo[b] = s.lev[il];
    Q.gap[b] = s.lev[il] - s.lev[ih];
    Q.e_electronic[b] = 0.5f * e;
    Q.e_core[b] = e_core;
    Q.delta_p[b] = delta;
    Q.n_pi[b] = n;
    Q.n_electrons[b] = n_el;
    Q.n_excluded[b] = H - n;
    Q.iterations[b] = iterations;
    Q.sweeps[b] = sweeps;
    Q.flags[b] = flags;
    Q.status[b] = converged && jacobi_ok ? GAUDI_HUCKEL_OK : GAUDI_HUCKEL_NOT_CONVERGED;
    if constexpr (Diis) {
      Q.diis_error[b] = diis_error;
      Q.n_extrapolated[b] = n_extrapolated;
    }
  }
  const int n_atoms = Q.in.n_atoms[b], n_bonds = Q.in.n_bonds[b];
  for (int a = lane; a < n_atoms; a += kRwLanes) {
    const int hv = s.g.hidx[a];
    Q.site_class[(size_t)b * A + a] = (signed char)(hv == kCanonNone ? -1 : (int)s.vcls[hv]);
  }
  for (int k = lane; k < n_bonds; k += kRwLanes) {
    const int hi_ = s.g.hidx[s.g.bl[k][0]], hj = s.g.hidx[s.g.bl[k][1]];
    if (hi_ == kCanonNone || hj == kCanonNone) continue;
    const int pr = s.pidx[hi_], ps = s.pidx[hj];
    if (pr == kCanonNone || ps == kCanonNone) continue;
    Q.pi_bond_order[(size_t)b * M + k] = ppp_density<P, Open>(s, pr, ps, n_occ, n_open);
  }
}

template <int P>
__global__ __launch_bounds__(64) void ppp_kernel(const PppParams Q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ppp_lds[];
  ppp_molecule<P>(Q, *reinterpret_cast<PppSmem<P>*>(ppp_lds), Q.scratch + (size_t)blockIdx.x * (P * P), Q.mol[blockIdx.x],
                  (int)threadIdx.x);
}

// The table and the call's two numbers checked and turned into what the kernel reads.  false: GAUDI_HUCKEL_BAD_TABLE.
static bool ppp_table(const gaudi_ppp_tables* t, int repulsion, float damping, PppTab& out) {
  memset(&out, 0, sizeof(out));
  if (repulsion != GAUDI_PPP_MATAGA_NISHIMOTO && repulsion != GAUDI_PPP_OHNO) return false;
  if (!(damping >= 0.0f && damping < 1.0f)) return false;
  if (t->n_classes < 1 || t->n_classes > kHuckelMaxClasses || !std::isfinite(t->beta0)) return false;
  for (int c = 0; c < t->n_classes; ++c) {
    if (t->z[c] < 0 || t->z[c] > 2 || !std::isfinite(t->I[c]) || !std::isfinite(t->k[c]) || !std::isfinite(t->gamma[c]) ||
        !(t->gamma[c] > 0.0f))
      return false;
    out.z[c] = t->z[c];
    out.ion[c] = t->I[c];
    out.gam[c] = t->gamma[c];
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
      const float ij = t->beta_pair[i][j], ji = t->beta_pair[j][i];
      const bool hij = !std::isnan(ij), hji = !std::isnan(ji);
      if ((hij && std::isinf(ij)) || (hij && hji && ij != ji)) return false;  // a listed pair is finite and the same both ways
      out.beta[i][j] = hij ? ij : hji ? ji : t->beta0 * (t->k[i] * t->k[j]);
    }
  return true;
}

struct PppOut {
  float* levels;
  uint8_t* occupation;
  float *pi_charge, *pi_bond_order;
  int8_t* site_class;
  int32_t *n_pi, *n_electrons, *n_excluded, *iterations, *sweeps, *flags, *status;
  float *homo, *lumo, *gap, *e_electronic, *e_core, *delta_p;
};
constexpr int kPppOuts = 18, kPppStatusOut = 11;

static void ppp_out_list(const PppOut& o, int B, int A, int M, void* (&p)[kPppOuts], size_t (&sz)[kPppOuts]) {
  const size_t nB = (size_t)B;
  void* ptrs[kPppOuts] = {o.levels, o.occupation, o.pi_charge, o.pi_bond_order, o.site_class, o.n_pi, o.n_electrons, o.n_excluded,
                          o.iterations, o.sweeps, o.flags, o.status, o.homo, o.lumo, o.gap, o.e_electronic, o.e_core, o.delta_p};
  const size_t sizes[kPppOuts] = {4 * nB * kHuckelMaxPi, nB * kHuckelMaxPi, 4 * nB * A, 4 * nB * M, nB * A, 4 * nB, 4 * nB, 4 * nB, 4 * nB,
                                  4 * nB, 4 * nB, 4 * nB, 4 * nB, 4 * nB, 4 * nB, 4 * nB, 4 * nB, 4 * nB};
  for (int i = 0; i < kPppOuts; ++i) {
    p[i] = ptrs[i];
    sz[i] = sizes[i];
  }
}

static void ppp_params(PppParams& Q, const gaudi_ppp_tables* t, int B, int A, int M, int repulsion, float damping,
                       void* (&outs)[kPppOuts]) {
  Q.in.B = B;
  Q.in.A = A;
  Q.in.M = M;
  Q.in.n_elems = t->n_elems;
  Q.in.h_elem = t->h_elem;
  Q.in.c_elem = t->c_elem;
  Q.repulsion = repulsion;
  Q.damping = damping;
  Q.levels = (float*)outs[0];
  Q.occupation = (unsigned char*)outs[1];
  Q.pi_charge = (float*)outs[2];
  Q.pi_bond_order = (float*)outs[3];
  Q.site_class = (signed char*)outs[4];
  Q.n_pi = (int*)outs[5];
  Q.n_electrons = (int*)outs[6];
  Q.n_excluded = (int*)outs[7];
  Q.iterations = (int*)outs[8];
  Q.sweeps = (int*)outs[9];
  Q.flags = (int*)outs[10];
  Q.status = (int*)outs[kPppStatusOut];
  Q.homo = (float*)outs[12];
  Q.lumo = (float*)outs[13];
  Q.gap = (float*)outs[14];
  Q.e_electronic = (float*)outs[15];
  Q.e_core = (float*)outs[16];
  Q.delta_p = (float*)outs[17];
}

template <int P>
static int ppp_launch(gaudi_handle* h, PppParams Q, const int* mol, int count) {
  if (count == 0) return GAUDI_OK;
  Q.mol = mol;
  constexpr int lds = (int)sizeof(PppSmem<P>);
  {
    // the attribute belongs to the function: one process-wide record per device (see the sampler's launch)
    static std::mutex mu;
    static std::map<int, bool> raised;
    std::lock_guard<std::mutex> lock(mu);
    if (!raised[h->device]) {
      HIPCHECK(h, hipFuncSetAttribute((const void*)ppp_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      raised[h->device] = true;
    }
  }
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (h->prof) HIPCHECK(h, h->ppp_log.begin(h->stream, ev));
  hipLaunchKernelGGL(ppp_kernel<P>, dim3(count), dim3(64), lds, h->stream, Q);
  HIPCHECK(h, hipGetLastError());
  if (h->prof) HIPCHECK(h, h->ppp_log.end(h->stream, ev));
  return GAUDI_OK;
}

template <int P>
static void ppp_host_tier(const PppParams& Q, const int* mol, int count) {
  if (count == 0) return;
  std::vector<PppSmem<P>> W(1);
  std::vector<float> pm((size_t)P * P);
  for (int i = 0; i < count; ++i) ppp_molecule<P>(Q, W[0], pm.data(), mol[i], 0);
}

// the ten outputs the CIS stage adds (ppp_cis.inc)
struct CisOut {
  float *singlet, *triplet, *osc, *dipole;
  uint8_t* lead;
  float* lead_weight;
  int32_t *n_states, *n_active_occ, *n_active_virt, *cis_sweeps;
};
constexpr int kCisOuts = 10;

static void cis_out_list(const CisOut& o, int B, void* (&p)[kCisOuts], size_t (&sz)[kCisOuts]) {
  const size_t nB = (size_t)B, row = GAUDI_PPP_CIS_MAX_STATES;
  void* ptrs[kCisOuts] = {o.singlet, o.triplet, o.osc, o.dipole, o.lead, o.lead_weight, o.n_states, o.n_active_occ, o.n_active_virt,
                          o.cis_sweeps};
  const size_t sizes[kCisOuts] = {4 * nB * row, 4 * nB * row, 4 * nB * row, 12 * nB * row, 2 * nB * row, 4 * nB * row, 4 * nB, 4 * nB,
                                  4 * nB, 4 * nB};
  for (int i = 0; i < kCisOuts; ++i) {
    p[i] = ptrs[i];
    sz[i] = sizes[i];
  }
}

static int cis_device(gaudi_handle* h, const PppParams& Q, int B, void* (&douts)[kCisOuts]);  // ppp_cis.inc
static void cis_host(const PppParams& Q, int B, void* (&outs)[kCisOuts]);

#define GAUDI_PPP_ARGS                                                                                                           \
  const gaudi_ppp_tables *tables, int B, int A, int M, const int32_t *elem, const int32_t *n_atoms, const int32_t *bonds,        \
      const int32_t *n_bonds, const float *xyz, const int32_t *charge, int repulsion, float damping, float *levels_out,          \
      uint8_t *occupation_out, float *pi_charge_out, float *pi_bond_order_out, int8_t *site_class_out, int32_t *n_pi_out,        \
      int32_t *n_electrons_out, int32_t *n_excluded_out, int32_t *iterations_out, int32_t *sweeps_out, int32_t *flags_out,       \
      int32_t *status_out, float *homo_out, float *lumo_out, float *gap_out, float *e_electronic_out, float *e_core_out,         \
      float *delta_p_out
#define GAUDI_PPP_PASS                                                                                                           \
  tables, B, A, M, elem, n_atoms, bonds, n_bonds, xyz, charge, repulsion, damping, levels_out, occupation_out, pi_charge_out,    \
      pi_bond_order_out, site_class_out, n_pi_out, n_electrons_out, n_excluded_out, iterations_out, sweeps_out, flags_out,       \
      status_out, homo_out, lumo_out, gap_out, e_electronic_out, e_core_out, delta_p_out
#define GAUDI_PPP_CIS_ARGS                                                                                                       \
  float *singlet_out, float *triplet_out, float *osc_out, float *dipole_out, uint8_t *lead_out, float *lead_weight_out,          \
      int32_t *n_states_out, int32_t *n_active_occ_out, int32_t *n_active_virt_out, int32_t *cis_sweeps_out
#define GAUDI_PPP_OUT                                                                                                            \
  gaudi::PppOut {                                                                                                                \
    levels_out, occupation_out, pi_charge_out, pi_bond_order_out, site_class_out, n_pi_out, n_electrons_out, n_excluded_out,     \
        iterations_out, sweeps_out, flags_out, status_out, homo_out, lumo_out, gap_out, e_electronic_out, e_core_out,            \
        delta_p_out                                                                                                              \
  }

// gaudi_ppp (cis null) and gaudi_ppp_cis: the SCF launches, then the CIS launch on the same stream
static int ppp_device(gaudi_handle* h, GAUDI_PPP_ARGS, const CisOut* cis, int window) {
  if (!h) return GAUDI_E_INVALID;
  void* outs[kPppOuts];
  size_t osz[kPppOuts];
  ppp_out_list(GAUDI_PPP_OUT, B > 0 ? B : 0, A, M, outs, osz);
  for (void* p : outs)
    if (!p) return fail(h, GAUDI_E_INVALID, "every output array is required");
  void* couts[kCisOuts] = {};
  size_t csz[kCisOuts] = {};
  if (cis) {
    cis_out_list(*cis, B > 0 ? B : 0, couts, csz);
    for (void* p : couts)
      if (!p) return fail(h, GAUDI_E_INVALID, "every output array is required");
  }
  if (!tables || !xyz) return fail(h, GAUDI_E_INVALID, "invalid argument");
  const char* why = "";
  std::vector<int> mol;
  int tier_n[3];
  if (int rc = huckel_route(tables->n_elems, tables->h_elem, tables->c_elem, B, A, M, elem, n_atoms, bonds, n_bonds, mol,
                            tier_n, &why))
    return fail(h, rc, why);
  if (B == 0) return GAUDI_OK;
  std::vector<PppTab> tab(1);
  // nothing runs on a table that cannot be read, or with a window outside 1..8: every row zero
  if (!ppp_table(tables, repulsion, damping, tab[0]) || (cis && (window < 1 || window > kCisMaxWindow))) {
    for (int i = 0; i < kPppOuts; ++i) memset(outs[i], 0, osz[i]);
    for (int i = 0; cis && i < kCisOuts; ++i) memset(couts[i], 0, csz[i]);
    for (int b = 0; b < B; ++b) status_out[b] = GAUDI_HUCKEL_BAD_TABLE;
    return GAUDI_OK;
  }
  HIPCHECK(h, hipSetDevice(h->device));
  const size_t nB = (size_t)B;
  std::vector<int32_t> zero;
  if (!charge) zero.assign(nB, 0);
  constexpr int kIn = 8;
  const size_t isz[kIn] = {sizeof(int) * nB * A, sizeof(int) * nB, sizeof(int) * nB * M * 2, sizeof(int) * nB, sizeof(int) * nB,
                           sizeof(int) * nB,     sizeof(PppTab), sizeof(float) * nB * A * 3};
  const void* ins[kIn] = {elem, n_atoms, bonds, n_bonds, charge ? charge : zero.data(), mol.data(), tab.data(), xyz};
  for (int i = 0; i < kIn; ++i) {
    HIPCHECK(h, h->d_ppp[i].reserve(isz[i]));
    HIPCHECK(h, hipMemcpyAsync(h->d_ppp[i].p, ins[i], isz[i], hipMemcpyHostToDevice, h->stream));
  }
  void* douts[kPppOuts];
  for (int i = 0; i < kPppOuts; ++i) {  // a refused molecule writes its status only: zero everywhere else
    HIPCHECK(h, h->d_ppp[kIn + i].reserve(osz[i]));
    HIPCHECK(h, hipMemsetAsync(h->d_ppp[kIn + i].p, 0, osz[i], h->stream));
    douts[i] = h->d_ppp[kIn + i].p;
  }
  // the density rows: the launches follow one another on the stream, so they share the largest tier's
  size_t rows = 0;
  const int cap[3] = {32, 64, 128};
  for (int k = 0; k < 3; ++k) rows = std::max(rows, (size_t)tier_n[k] * cap[k] * cap[k]);
  DevBuf& scratch = h->d_ppp[kIn + kPppOuts];
  HIPCHECK(h, scratch.reserve(sizeof(float) * rows));
  PppParams Q{};
  ppp_params(Q, tables, B, A, M, repulsion, damping, douts);
  Q.in.elem = h->d_ppp[0].as<int>();
  Q.in.n_atoms = h->d_ppp[1].as<int>();
  Q.in.bonds = h->d_ppp[2].as<int>();
  Q.in.n_bonds = h->d_ppp[3].as<int>();
  Q.charge = h->d_ppp[4].as<int>();
  Q.tab = h->d_ppp[6].as<PppTab>();
  Q.xyz = h->d_ppp[7].as<float>();
  Q.scratch = scratch.as<float>();
  constexpr int kCisBuf = kIn + kPppOuts + 1;  // the hand-over rows, then the ten CIS outputs
  void* dcis[kCisOuts] = {};
  if (cis) {
    HIPCHECK(h, h->d_ppp[kCisBuf].reserve(sizeof(float) * nB * kCisRow));
    Q.cis = h->d_ppp[kCisBuf].as<float>();
    Q.window = window;
    for (int i = 0; i < kCisOuts; ++i) {
      HIPCHECK(h, h->d_ppp[kCisBuf + 1 + i].reserve(csz[i]));
      HIPCHECK(h, hipMemsetAsync(h->d_ppp[kCisBuf + 1 + i].p, 0, csz[i], h->stream));
      dcis[i] = h->d_ppp[kCisBuf + 1 + i].p;
    }
  }
  const int* dmol = h->d_ppp[5].as<int>();
  if (int rc = ppp_launch<32>(h, Q, dmol, tier_n[0])) return rc;
  if (int rc = ppp_launch<64>(h, Q, dmol + tier_n[0], tier_n[1])) return rc;
  if (int rc = ppp_launch<128>(h, Q, dmol + tier_n[0] + tier_n[1], tier_n[2])) return rc;
  if (cis)
    if (int rc = cis_device(h, Q, B, dcis)) return rc;
  for (int i = 0; i < kPppOuts; ++i)
    HIPCHECK(h, hipMemcpyAsync(outs[i], douts[i], osz[i], hipMemcpyDeviceToHost, h->stream));
  for (int i = 0; cis && i < kCisOuts; ++i)
    HIPCHECK(h, hipMemcpyAsync(couts[i], dcis[i], csz[i], hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  return GAUDI_OK;
}

static int ppp_host(GAUDI_PPP_ARGS, const CisOut* cis, int window) {
  void* outs[kPppOuts];
  size_t osz[kPppOuts];
  ppp_out_list(GAUDI_PPP_OUT, B > 0 ? B : 0, A, M, outs, osz);
  for (void* p : outs)
    if (!p) return GAUDI_E_INVALID;
  void* couts[kCisOuts] = {};
  size_t csz[kCisOuts] = {};
  if (cis) {
    cis_out_list(*cis, B > 0 ? B : 0, couts, csz);
    for (void* p : couts)
      if (!p) return GAUDI_E_INVALID;
  }
  if (!tables || !xyz) return GAUDI_E_INVALID;
  const char* why = "";
  std::vector<int> mol;
  int tier_n[3];
  if (int rc = huckel_route(tables->n_elems, tables->h_elem, tables->c_elem, B, A, M, elem, n_atoms, bonds, n_bonds, mol,
                            tier_n, &why))
    return rc;
  if (B == 0) return GAUDI_OK;
  for (int i = 0; i < kPppOuts; ++i) memset(outs[i], 0, osz[i]);
  for (int i = 0; cis && i < kCisOuts; ++i) memset(couts[i], 0, csz[i]);
  std::vector<PppTab> tab(1);
  if (!ppp_table(tables, repulsion, damping, tab[0]) || (cis && (window < 1 || window > kCisMaxWindow))) {
    for (int b = 0; b < B; ++b) status_out[b] = GAUDI_HUCKEL_BAD_TABLE;
    return GAUDI_OK;
  }
  std::vector<int32_t> zero;
  if (!charge) zero.assign((size_t)B, 0);
  PppParams Q{};
  ppp_params(Q, tables, B, A, M, repulsion, damping, outs);
  Q.in.elem = elem;
  Q.in.n_atoms = n_atoms;
  Q.in.bonds = bonds;
  Q.in.n_bonds = n_bonds;
  Q.charge = charge ? charge : zero.data();
  Q.xyz = xyz;
  Q.tab = tab.data();
  std::vector<float> rows;
  if (cis) {
    rows.assign((size_t)B * kCisRow, 0.0f);
    Q.cis = rows.data();
    Q.window = window;
  }
  ppp_host_tier<32>(Q, mol.data(), tier_n[0]);
  ppp_host_tier<64>(Q, mol.data() + tier_n[0], tier_n[1]);
  ppp_host_tier<128>(Q, mol.data() + tier_n[0] + tier_n[1], tier_n[2]);
  if (cis) cis_host(Q, B, couts);
  return GAUDI_OK;
}

}  // namespace gaudi

extern "C" int gaudi_ppp(gaudi_handle* h, GAUDI_PPP_ARGS) { return gaudi::ppp_device(h, GAUDI_PPP_PASS, nullptr, 0); }

extern "C" int gaudi_host_ppp(GAUDI_PPP_ARGS) { return gaudi::ppp_host(GAUDI_PPP_PASS, nullptr, 0); }
// (the argument macros are ppp_cis.inc's too: it undefines them)

extern "C" int gaudi_ppp_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms) {
  if (!h || !n_launches || !total_ms) return GAUDI_E_INVALID;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, h->ppp_log.fold(0));
  *n_launches = (int32_t)h->ppp_log.n;
  *total_ms = h->ppp_log.ms;
  return GAUDI_OK;
}
