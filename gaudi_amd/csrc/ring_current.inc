// ring_current.inc -- Hueckel-London ring currents of a graph of atoms with coordinates: the pi current a perpendicular magnetic
// field induces in every bond and every ring (included after kekule.inc at the end of gaudi_hip.hip; DESIGN.md section 8p; the
// model is spelled out in include/gaudi_hip.h).
//
// The pi centres, the matrix and the levels are huckel.inc's, through its own routines: canon_graph, huckel_sites, huckel_matrix,
// jacobi_sweeps, huckel_rayleigh.  ONE text, two builds, as huckel.inc: a 64-lane wave per molecule on the device, one lane that
// walks every index on the host (kRwLanes).  Per molecule, after the levels are ranked:
//   1. the refusals that need no geometry (SMALL_GAP; a pi graph without a cycle leaves as OK with nothing but zeros);
//   2. coordinates of the pi centres, the geometry rule of ppp.inc; lane 0: centroid, scatter matrix, its 3 x 3 Jacobi
//      diagonalisation, the normal; all lanes: r - c and the area s_rs of every bond slot;
//   3. the response, all lanes, in the LDS the diagonalised matrix leaves free (s.a; k runs over occupied ranks, l over empty):
//        u_k = A v_k           into a[k][r]   (rows below n_occ; A is sparse: at most four terms)
//        W_lk = 2 v_l.u_k / (eps_k - eps_l)  into a[l][k]   (rows from n_occ on)
//        z_k = sum_l W_lk v_l  into a[k][r]   (over u, which is spent)
//      so that Q_sr = sum_k (z_k[s] v_k[r] - v_k[s] z_k[r]); one lane per listed bond then takes P_rs and Q_sr and writes the bond
//      current, and both directions of it into the bond's two slots.  W, u and z need no LDS of their own: a tier's LDS is
//      huckel.inc's plus the geometry, slot and ring arrays of RcSmem (7.0 / 8.4 / 11.2 KB);
//   4. rings: lane a walks the chordless paths from centre a through larger centres only and closes them on a after 4, 5 or 6
//      centres with second < last (kekule.inc's walk, for three lengths); counted, stored at the prefix of the counts, ranked by
//      sorted atom tuple, turned to positive area;
//   5. ring currents: C^T C (small integers) and C^T b by one lane per element, Gaussian elimination without pivoting (one lane
//      per row, a fence per column), back substitution on lane 0; the rings are then a basis of the cycle space, so a bond on none
//      of them lies on no cycle and its current is set to the exact zero Kirchhoff's law gives it; the residual, one lane per centre.
// Every fp32 operation is individually rounded (contraction off, correctly rounded / and sqrtf) and every sum runs in one fixed
// order; every element is computed by ONE lane from LDS state the phase before completed, so the device gives the host build's
// bits and a molecule's result does not depend on the tier P, on the batch or on its place in it.  No atomics; plain LDS, plain
// vector stores and rw_fence.  Every branch around a fence or a reduction is lane-uniform.

namespace gaudi {

constexpr int kRcMaxRings = GAUDI_RING_CURRENT_MAX_RINGS, kRcMaxSize = GAUDI_RING_CURRENT_MAX_SIZE;
constexpr int kRcPlaneSweeps = 12;        // 3 x 3 Jacobi converges quadratically: 12 sweeps are never reached
constexpr float kRcSmallGap = 1e-3f;      // |beta|
constexpr float kRcMinArea = 1e-3f;       // Angstrom^2
constexpr float kRcTooClose2 = 0.25f;     // (0.5 Angstrom)^2, as ppp.inc
constexpr float kRcUnit = 1.1316065276f;  // c0 = 2 A0 / 9, A0 = (3 sqrt(3) / 2) 1.40^2: the bond current of benzene
static_assert(kRcMaxRings == 32 && kRcMaxSize == 6, "ring rows are [32][6]; a row of the normal equations is a lane's");
static_assert(GAUDI_RING_CURRENT_SMALL_GAP > GAUDI_PPP_BAD_GEOMETRY, "the shared statuses keep their values");

template <int P>
struct RcSmem : HuckelSmem<P> {
  float xyz[P][3];                                    // a centre's coordinates; minus the centroid once the plane is known
  float sa[P][kHuckelNbr], jc[P][kHuckelNbr];         // per bond slot (huckel's nb): the area s_rs; the reported current r -> s
  float m3[3][3], v3[3][3], pl[8];                    // the scatter matrix and its eigenvectors; normal, centroid, rms
  float nm[kRcMaxRings][kRcMaxRings + 1], rhs[kRcMaxRings], cur[kRcMaxRings], area[kRcMaxRings];
  kek_u64 uam[kRcMaxRings][2];                        // a ring's centres as a mask, in the order found
  unsigned char cyc[kRcMaxRings][kRcMaxSize], scyc[kRcMaxRings][kRcMaxSize];  // rings in cycle order: as found, as reported
  unsigned char csz[kRcMaxRings], ssz[kRcMaxRings];
  unsigned char comp[P];                              // the centre's component: its lowest centre
};
static_assert(sizeof(RcSmem<128>) <= 160 * 1024, "the largest tier fits the LDS of a CU");

struct RcParams {
  CanonParams in;  // the input fields only
  const int* mol;  // the molecules of this launch (one capacity tier)
  const int* charge;
  const float* xyz;  // [B][A][3]
  const HuckelTab* tab;
  float* bond_current;  // [B][M]
  int* n_rings;         // [B]
  int* ring_atoms;      // [B][32][6]
  int* ring_size;       // [B][32]
  float *ring_current, *ring_area;                // [B][32]
  float* normal;                                  // [B][3]
  float *rms, *gap, *residual;                    // [B]
  int *n_pi, *n_electrons, *sweeps, *flags, *status;  // [B]
};

// the slot of centre y among the bonds of centre x; kHuckelNbr: not bonded
template <class S>
__host__ __device__ __forceinline__ int rc_slot(const S& s, int x, int y) {
  int d = kHuckelNbr;
  for (int q = kHuckelNbr - 1; q >= 0; --q) d = s.nb[x][q] == y ? q : d;
  return d;
}
template <class S>
__host__ __device__ __forceinline__ bool rc_adj(const S& s, int x, int y) {
  return rc_slot(s, x, y) < kHuckelNbr;
}

template <class S>
__host__ __device__ __forceinline__ void rc_emit(S& s, bool store, int at, int size, int a, int p1, int p2, int p3, int p4, int p5) {
  if (!store || at >= kRcMaxRings) return;
  unsigned char* c = s.cyc[at];
  c[0] = (unsigned char)a;
  c[1] = (unsigned char)p1;
  c[2] = (unsigned char)p2;
  c[3] = (unsigned char)p3;
  c[4] = (unsigned char)p4;
  c[5] = (unsigned char)p5;
  s.csz[at] = (unsigned char)size;
}

// Chordless cycles of 4, 5 or 6 pi centres whose smallest centre is a, each once (second centre < last centre).  Returns their
// number; with `store` they are written to s.cyc[base ...] while base + found stays below kRcMaxRings.
template <class S>
__host__ __device__ inline int rc_ring_enum(S& s, int a, bool store, int base) {
  int found = 0;
  for (int q1 = 0; q1 < kHuckelNbr; ++q1) {
    const int p1 = s.nb[a][q1];
    if (p1 == kCanonNone) break;
    if (p1 <= a) continue;
    for (int q2 = 0; q2 < kHuckelNbr; ++q2) {
      const int p2 = s.nb[p1][q2];
      if (p2 == kCanonNone) break;
      if (p2 <= a || rc_adj(s, p2, a)) continue;
      for (int q3 = 0; q3 < kHuckelNbr; ++q3) {
        const int p3 = s.nb[p2][q3];
        if (p3 == kCanonNone) break;
        if (p3 <= a || p3 == p1 || rc_adj(s, p3, p1)) continue;
        if (rc_adj(s, p3, a)) {  // a four-ring; no longer ring runs through this path (a - p3 would be its chord)
          if (p3 > p1) {
            rc_emit(s, store, base + found, 4, a, p1, p2, p3, kCanonNone, kCanonNone);
            ++found;
          }
          continue;
        }
        for (int q4 = 0; q4 < kHuckelNbr; ++q4) {
          const int p4 = s.nb[p3][q4];
          if (p4 == kCanonNone) break;
          if (p4 <= a || p4 == p2 || rc_adj(s, p4, p1) || rc_adj(s, p4, p2)) continue;
          if (rc_adj(s, p4, a)) {
            if (p4 > p1) {
              rc_emit(s, store, base + found, 5, a, p1, p2, p3, p4, kCanonNone);
              ++found;
            }
            continue;
          }
          for (int q5 = 0; q5 < kHuckelNbr; ++q5) {
            const int p5 = s.nb[p4][q5];
            if (p5 == kCanonNone) break;
            if (p5 <= a || p5 == p3 || p5 < p1 || !rc_adj(s, p5, a)) continue;
            if (rc_adj(s, p5, p1) || rc_adj(s, p5, p2) || rc_adj(s, p5, p3)) continue;
            rc_emit(s, store, base + found, 6, a, p1, p2, p3, p4, p5);
            ++found;
          }
        }
      }
    }
  }
  return found;
}

// Lane 0: the plane of the n centres in s.xyz.  s.pl[0..2] = the normal, s.pl[3..5] = the centroid.
template <class S>
__host__ __device__ inline void rc_plane(S& s, int n) {
#pragma clang fp contract(off)
  float cx = 0.0f, cy = 0.0f, cz = 0.0f;
  for (int r = 0; r < n; ++r) {
    cx = cx + s.xyz[r][0];
    cy = cy + s.xyz[r][1];
    cz = cz + s.xyz[r][2];
  }
  const float fn = (float)n;
  cx = cx / fn;
  cy = cy / fn;
  cz = cz / fn;
  float xx = 0.0f, xy = 0.0f, xz = 0.0f, yy = 0.0f, yz = 0.0f, zz = 0.0f;
  for (int r = 0; r < n; ++r) {
    const float dx = s.xyz[r][0] - cx, dy = s.xyz[r][1] - cy, dz = s.xyz[r][2] - cz;
    xx = xx + dx * dx;
    xy = xy + dx * dy;
    xz = xz + dx * dz;
    yy = yy + dy * dy;
    yz = yz + dy * dz;
    zz = zz + dz * dz;
  }
  s.m3[0][0] = xx;
  s.m3[1][1] = yy;
  s.m3[2][2] = zz;
  s.m3[0][1] = s.m3[1][0] = xy;
  s.m3[0][2] = s.m3[2][0] = xz;
  s.m3[1][2] = s.m3[2][1] = yz;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) s.v3[i][j] = i == j ? 1.0f : 0.0f;
  // cyclic Jacobi, the rotation of jacobi_sweeps; a sweep starts while an off-diagonal element is not zero
  for (int sweep = 0; sweep < kRcPlaneSweeps; ++sweep) {
    if (s.m3[0][1] == 0.0f && s.m3[0][2] == 0.0f && s.m3[1][2] == 0.0f) break;
    for (int pair = 0; pair < 3; ++pair) {
      const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2, o = 3 - p - q;
      const float app = s.m3[p][p], aqq = s.m3[q][q], apq = s.m3[p][q];
      if (apq == 0.0f) continue;
      const float theta = (aqq - app) / (2.0f * apq);
      float t = 1.0f / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
      t = theta < 0.0f ? -t : t;
      const float c = 1.0f / sqrtf(t * t + 1.0f), sn = t * c, d = t * apq;
      const float aop = s.m3[o][p], aoq = s.m3[o][q];
      s.m3[p][p] = app - d;
      s.m3[q][q] = aqq + d;
      s.m3[p][q] = s.m3[q][p] = 0.0f;
      s.m3[o][p] = s.m3[p][o] = c * aop - sn * aoq;
      s.m3[o][q] = s.m3[q][o] = sn * aop + c * aoq;
      for (int k = 0; k < 3; ++k) {
        const float vp = s.v3[k][p], vq = s.v3[k][q];
        s.v3[k][p] = c * vp - sn * vq;
        s.v3[k][q] = sn * vp + c * vq;
      }
    }
  }
  int low = 0;
  for (int k = 1; k < 3; ++k) low = s.m3[k][k] < s.m3[low][low] ? k : low;
  float nx = s.v3[0][low], ny = s.v3[1][low], nz = s.v3[2][low];
  const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
  nx = nx / len;
  ny = ny / len;
  nz = nz / len;
  float big = nx;  // the component of largest magnitude is positive; the lower index wins a tie
  big = fabsf(ny) > fabsf(big) ? ny : big;
  big = fabsf(nz) > fabsf(big) ? nz : big;
  if (big < 0.0f) {
    nx = -nx;
    ny = -ny;
    nz = -nz;
  }
  s.pl[0] = nx;
  s.pl[1] = ny;
  s.pl[2] = nz;
  s.pl[3] = cx;
  s.pl[4] = cy;
  s.pl[5] = cz;
}

// the status of a molecule that leaves without a result
#define GAUDI_RC_LEAVE(code)               \
  {                                        \
    if (lane == 0) Q.status[b] = (code);   \
    return;                                \
  }

// One molecule.  Every branch around a fence or a reduction is lane-uniform.
template <int P>
__host__ __device__ inline void ring_current_molecule(const RcParams& Q, RcSmem<P>& s, int b, int lane) {
#pragma clang fp contract(off)
  const int A = Q.in.A, M = Q.in.M;
  int H = 0, E = 0;
  const int gstatus = canon_graph(Q.in, s.g, b, lane, H, E);
  if (gstatus != GAUDI_CANON_OK) GAUDI_RC_LEAVE(gstatus);
  const HuckelTab& T = *Q.tab;
  // ---- the levels: huckel.inc's steps 1 to 3
  int n, n_el;
  const int refused = huckel_sites<P>(T, s, H, Q.charge[b], lane, n, n_el);
  if (refused != GAUDI_HUCKEL_OK) GAUDI_RC_LEAVE(refused);
  if (n_el & 1) GAUDI_RC_LEAVE(GAUDI_PPP_OPEN_SHELL);
  huckel_matrix(T, s, n, lane);
  int sweeps = 0;
  if (!jacobi_sweeps<P>(s, n, lane, kHuckelOff, sweeps)) GAUDI_RC_LEAVE(GAUDI_HUCKEL_NOT_CONVERGED);
  huckel_rayleigh(s, n, lane);
  for (int i = lane; i < n; i += kRwLanes) {  // ranks by counting, ties: the smaller index first (huckel.inc, step 4)
    const float xi = s.x[i];
    int rk = 0;
    for (int j = 0; j < n; ++j) {
      const float xj = s.x[j];
      rk += xj > xi || (xj == xi && j < i);
    }
    s.ord[rk] = (unsigned char)i;
    s.lev[rk] = xi;
  }
  rw_fence();
  // ---- 1. what needs no geometry
  const int n_occ = n_el >> 1;
  if (n_occ < 1 || n_occ >= n) GAUDI_RC_LEAVE(GAUDI_RING_CURRENT_SMALL_GAP);
  const float gap = s.lev[n_occ - 1] - s.lev[n_occ];
  if (gap < kRcSmallGap) GAUDI_RC_LEAVE(GAUDI_RING_CURRENT_SMALL_GAP);
  int ends = 0;
  for (int r = lane; r < n; r += kRwLanes) {
    for (int d = 0; d < kHuckelNbr; ++d) ends += s.nb[r][d] != kCanonNone;
    s.comp[r] = (unsigned char)r;
  }
  int ends_all;
  (void)rw_scan(ends, lane, ends_all);
  rw_fence();
  for (;;) {  // components by min-label propagation (labels only fall, so racing reads are harmless)
    bool changed = false;
    for (int r = lane; r < n; r += kRwLanes) {
      int lo = s.comp[r];
      for (int d = 0; d < kHuckelNbr; ++d) {
        const int o = s.nb[r][d];
        if (o == kCanonNone) break;
        const int l = s.comp[o];
        lo = l < lo ? l : lo;
      }
      if (lo < s.comp[r]) {
        s.comp[r] = (unsigned char)lo;
        changed = true;
      }
    }
    rw_fence();
    if (!rw_any(changed)) break;
  }
  int roots = 0;
  for (int r = lane; r < n; r += kRwLanes) roots += s.comp[r] == r;
  int comps;
  (void)rw_scan(roots, lane, comps);
  const int cyclo = (ends_all >> 1) - n + comps;
  int* ring_atoms = Q.ring_atoms + (size_t)b * kRcMaxRings * kRcMaxSize;
  if (cyclo == 0) {  // no cycle: no current, and no plane is needed
    for (int i = lane; i < kRcMaxRings * kRcMaxSize; i += kRwLanes) ring_atoms[i] = -1;
    if (lane == 0) {
      Q.gap[b] = gap;
      Q.n_pi[b] = n;
      Q.n_electrons[b] = n_el;
      Q.sweeps[b] = sweeps;
      Q.status[b] = GAUDI_HUCKEL_OK;
    }
    return;
  }
  // ---- 2. coordinates, the geometry rule of ppp.inc, the plane, the areas
  bool bad = false;
  for (int r = lane; r < n; r += kRwLanes) {
    const float* at = Q.xyz + ((size_t)b * A + s.g.hv[s.vert[r]]) * 3;
    for (int k = 0; k < 3; ++k) {
      const float t = at[k];
      bad = bad || (huckel_bits(t) & 0x7f800000) == 0x7f800000;  // infinite or not a number
      s.xyz[r][k] = t;
    }
  }
  rw_fence();
  if (!rw_any(bad)) {
    for (int c = lane; c < n; c += kRwLanes)
      for (int r = 0; r < c; ++r) {
        const float dx = s.xyz[r][0] - s.xyz[c][0], dy = s.xyz[r][1] - s.xyz[c][1], dz = s.xyz[r][2] - s.xyz[c][2];
        bad = bad || !((dx * dx + dy * dy) + dz * dz >= kRcTooClose2);
      }
    bad = rw_any(bad);
  } else {
    bad = true;
  }
  if (bad) GAUDI_RC_LEAVE(GAUDI_PPP_BAD_GEOMETRY);
  if (lane == 0) rc_plane(s, n);
  rw_fence();
  const float nx = s.pl[0], ny = s.pl[1], nz = s.pl[2];
  {
    const float cx = s.pl[3], cy = s.pl[4], cz = s.pl[5];
    for (int r = lane; r < n; r += kRwLanes) {
      s.xyz[r][0] = s.xyz[r][0] - cx;
      s.xyz[r][1] = s.xyz[r][1] - cy;
      s.xyz[r][2] = s.xyz[r][2] - cz;
    }
  }
  rw_fence();
  for (int it = lane; it < n * kHuckelNbr; it += kRwLanes) {
    const int r = it / kHuckelNbr, d = it % kHuckelNbr, o = s.nb[r][d];
    float area = 0.0f;
    if (o != kCanonNone) {
      const float ax = s.xyz[r][0], ay = s.xyz[r][1], az = s.xyz[r][2], bx = s.xyz[o][0], by = s.xyz[o][1], bz = s.xyz[o][2];
      const float kx = ay * bz - az * by, ky = az * bx - ax * bz, kz = ax * by - ay * bx;  // exactly antisymmetric in (r, o)
      area = 0.5f * ((nx * kx + ny * ky) + nz * kz);
    }
    s.sa[r][d] = area;
    s.jc[r][d] = 0.0f;
  }
  if (lane == 0) {  // the root mean square distance from the plane
    float sum = 0.0f;
    for (int r = 0; r < n; ++r) {
      const float d = (nx * s.xyz[r][0] + ny * s.xyz[r][1]) + nz * s.xyz[r][2];
      sum = sum + d * d;
    }
    s.pl[6] = sqrtf(sum / (float)n);
  }
  rw_fence();
  // ---- 3. the response.  u_k = A v_k, A_rs = E_rs s_rs = -M_rs s_rs
  const int n_virt = n - n_occ;
  for (int it = lane; it < n_occ * n; it += kRwLanes) {
    const int k = it / n, r = it - k * n, col = s.ord[k];
    float u = 0.0f;
    for (int d = 0; d < kHuckelNbr; ++d) {
      const int o = s.nb[r][d];
      if (o == kCanonNone) break;
      u = u + (-s.kn[r][d] * s.sa[r][d]) * s.v[o][col];
    }
    s.a[k][r] = u;
  }
  rw_fence();
  for (int it = lane; it < n_virt * n_occ; it += kRwLanes) {  // W_lk = 2 a_lk / (eps_k - eps_l), eps = -x
    const int li = it / n_occ, k = it - li * n_occ, l = n_occ + li, col = s.ord[l];
    float acc = 0.0f;
    for (int r = 0; r < n; ++r) acc = acc + s.v[r][col] * s.a[k][r];
    s.a[l][k] = (2.0f * acc) / (s.lev[l] - s.lev[k]);
  }
  rw_fence();
  for (int it = lane; it < n_occ * n; it += kRwLanes) {  // z_k = sum_l W_lk v_l
    const int k = it / n, r = it - k * n;
    float z = 0.0f;
    for (int l = n_occ; l < n; ++l) z = z + s.a[l][k] * s.v[r][s.ord[l]];
    s.a[k][r] = z;
  }
  rw_fence();
  const int n_bonds = Q.in.n_bonds[b];
  for (int e = lane; e < n_bonds; e += kRwLanes) {
    const int hi_ = s.g.hidx[s.g.bl[e][0]], hj = s.g.hidx[s.g.bl[e][1]];
    if (hi_ == kCanonNone || hj == kCanonNone) continue;
    const int pr = s.pidx[hi_], ps = s.pidx[hj];
    if (pr == kCanonNone || ps == kCanonNone) continue;
    const int d = rc_slot(s, pr, ps), back = rc_slot(s, ps, pr);
    if (d == kHuckelNbr || back == kHuckelNbr) continue;
    float p = 0.0f, q = 0.0f;
    for (int k = 0; k < n_occ; ++k) {
      const int col = s.ord[k];
      const float vr = s.v[pr][col], vs = s.v[ps][col];
      p = p + vr * vs;
      q = q + (s.a[k][ps] * vr - vs * s.a[k][pr]);
    }
    const float j = 2.0f * (-s.kn[pr][d] * (s.sa[pr][d] * (2.0f * p) + q));
    const float reported = -j / kRcUnit;
    Q.bond_current[(size_t)b * M + e] = reported;
    s.jc[pr][d] = reported;
    s.jc[ps][back] = -reported;
  }
  rw_fence();
  // ---- 4. the rings: counted, stored at the prefix of the counts, ranked by their sorted atom tuple, turned to positive area
  int mine = 0;
  for (int a = lane; a < n; a += kRwLanes) mine += rc_ring_enum(s, a, false, 0);
  int R;
  int base = rw_scan(mine, lane, R);
  bool defined = R == cyclo && R <= kRcMaxRings;
  if (defined) {
    for (int a = lane; a < n; a += kRwLanes) base += rc_ring_enum(s, a, true, base);
    rw_fence();
    for (int r = lane; r < R; r += kRwLanes) {
      kek_u64 a0 = 0, a1 = 0;
      for (int j = 0; j < kRcMaxSize; ++j) {
        const int x = j < s.csz[r] ? (int)s.cyc[r][j] : 128;
        a0 |= kek_lo(x);
        a1 |= kek_hi(x);
      }
      s.uam[r][0] = a0;
      s.uam[r][1] = a1;
    }
    rw_fence();
    bool flat = false;
    for (int r = lane; r < R; r += kRwLanes) {
      // of two chordless cycles (neither holds the other) the one with the lowest centre they differ in has the smaller sorted tuple
      const kek_u64 a0 = s.uam[r][0], a1 = s.uam[r][1];
      int rank = 0;
      for (int o = 0; o < R; ++o) {
        const kek_u64 d0 = a0 ^ s.uam[o][0], d1 = a1 ^ s.uam[o][1];
        rank += d0 ? ((d0 & (0 - d0)) & s.uam[o][0]) != 0 : d1 ? ((d1 & (0 - d1)) & s.uam[o][1]) != 0 : 0;
      }
      const int size = s.csz[r];
      float area = 0.0f;
      for (int j = 0; j < size; ++j) {
        const int x = s.cyc[r][j], y = s.cyc[r][j + 1 == size ? 0 : j + 1];
        area = area + s.sa[x][rc_slot(s, x, y) & (kHuckelNbr - 1)];
      }
      const bool turn = area < 0.0f;  // the other way round from the same centre, its area summed in the order it is reported in
      for (int j = 0; j < kRcMaxSize; ++j) {
        const int from = j >= size ? 0 : j == 0 || !turn ? j : size - j;
        s.scyc[rank][j] = j < size ? s.cyc[r][from] : (unsigned char)kCanonNone;
      }
      if (turn) {
        area = 0.0f;
        for (int j = 0; j < size; ++j) {
          const int x = s.scyc[rank][j], y = s.scyc[rank][j + 1 == size ? 0 : j + 1];
          area = area + s.sa[x][rc_slot(s, x, y) & (kHuckelNbr - 1)];
        }
      }
      s.ssz[rank] = (unsigned char)size;
      s.area[rank] = area;
      flat = flat || !(area > kRcMinArea);
    }
    rw_fence();
    defined = !rw_any(flat);
  }
  // ---- 5. the ring currents: (C^T C) I = C^T b
  float residual = 0.0f;
  if (defined) {
    for (int it = lane; it < R * R; it += kRwLanes) {
      const int r = it / R, q = it - r * R, nr = s.ssz[r], nq = s.ssz[q];
      int sum = 0;
      for (int i = 0; i < nr; ++i) {
        const int x = s.scyc[r][i], y = s.scyc[r][i + 1 == nr ? 0 : i + 1];
        for (int j = 0; j < nq; ++j) {
          const int u = s.scyc[q][j], w = s.scyc[q][j + 1 == nq ? 0 : j + 1];
          sum += (x == u && y == w) - (x == w && y == u);
        }
      }
      s.nm[r][q] = (float)sum;
    }
    for (int r = lane; r < R; r += kRwLanes) {
      const int nr = s.ssz[r];
      float sum = 0.0f;
      for (int i = 0; i < nr; ++i) {
        const int x = s.scyc[r][i], y = s.scyc[r][i + 1 == nr ? 0 : i + 1];
        sum = sum + s.jc[x][rc_slot(s, x, y) & (kHuckelNbr - 1)];
      }
      s.rhs[r] = sum;
    }
    rw_fence();
    for (int p = 0; p < R; ++p) {
      const float piv = s.nm[p][p];
      if (!(piv > 0.0f)) {
        defined = false;
        break;
      }
      for (int i = p + 1 + lane; i < R; i += kRwLanes) {
        const float f = s.nm[i][p] / piv;
        for (int c = p + 1; c < R; ++c) s.nm[i][c] = s.nm[i][c] - f * s.nm[p][c];
        s.rhs[i] = s.rhs[i] - f * s.rhs[p];
      }
      rw_fence();
    }
  }
  if (defined) {
    if (lane == 0)
      for (int p = R - 1; p >= 0; --p) {
        float acc = s.rhs[p];
        for (int c = p + 1; c < R; ++c) acc = acc - s.nm[p][c] * s.cur[c];
        s.cur[p] = acc / s.nm[p][p];
      }
    // the rings are a basis of the cycle space, so a bond on none of them lies on no cycle: Kirchhoff's law gives it exactly zero
    for (int e = lane; e < n_bonds; e += kRwLanes) {
      const int hi_ = s.g.hidx[s.g.bl[e][0]], hj = s.g.hidx[s.g.bl[e][1]];
      if (hi_ == kCanonNone || hj == kCanonNone) continue;
      const int pr = s.pidx[hi_], ps = s.pidx[hj];
      if (pr == kCanonNone || ps == kCanonNone) continue;
      const int d = rc_slot(s, pr, ps), back = rc_slot(s, ps, pr);
      if (d == kHuckelNbr || back == kHuckelNbr) continue;
      bool on = false;
      for (int q = 0; q < R; ++q) {
        const int nq = s.ssz[q];
        for (int j = 0; j < nq; ++j) {
          const int u = s.scyc[q][j], w = s.scyc[q][j + 1 == nq ? 0 : j + 1];
          on = on || (u == pr && w == ps) || (u == ps && w == pr);
        }
      }
      if (!on) {
        Q.bond_current[(size_t)b * M + e] = 0.0f;
        s.jc[pr][d] = 0.0f;
        s.jc[ps][back] = 0.0f;
      }
    }
    rw_fence();
    float worst = 0.0f;
    for (int r = lane; r < n; r += kRwLanes)
      for (int d = 0; d < kHuckelNbr; ++d) {
        const int o = s.nb[r][d];
        if (o == kCanonNone) break;
        if (o < r) continue;  // every bond once
        float ci = 0.0f;
        for (int q = 0; q < R; ++q) {
          const int nq = s.ssz[q];
          for (int j = 0; j < nq; ++j) {
            const int u = s.scyc[q][j], w = s.scyc[q][j + 1 == nq ? 0 : j + 1];
            if (u == r && w == o) ci = ci + s.cur[q];
            if (u == o && w == r) ci = ci - s.cur[q];
          }
        }
        const float t = fabsf(ci - s.jc[r][d]);
        worst = t > worst ? t : worst;
      }
    residual = __builtin_bit_cast(float, -rw_min(-huckel_bits(worst)));  // non-negative floats order as their bits
  }
  // ---- outputs
  if (defined) {
    for (int i = lane; i < kRcMaxRings * kRcMaxSize; i += kRwLanes) {
      const int r = i / kRcMaxSize, j = i - r * kRcMaxSize;
      ring_atoms[i] = r < R && j < s.ssz[r] ? (int)s.g.hv[s.vert[s.scyc[r][j]]] : -1;
    }
    for (int r = lane; r < R; r += kRwLanes) {
      Q.ring_size[(size_t)b * kRcMaxRings + r] = s.ssz[r];
      Q.ring_current[(size_t)b * kRcMaxRings + r] = s.cur[r];
      Q.ring_area[(size_t)b * kRcMaxRings + r] = s.area[r];
    }
  }
  if (lane == 0) {
    Q.n_rings[b] = defined ? R : 0;
    Q.normal[(size_t)b * 3 + 0] = nx;
    Q.normal[(size_t)b * 3 + 1] = ny;
    Q.normal[(size_t)b * 3 + 2] = nz;
    Q.rms[b] = s.pl[6];
    Q.gap[b] = gap;
    Q.residual[b] = residual;
    Q.n_pi[b] = n;
    Q.n_electrons[b] = n_el;
    Q.sweeps[b] = sweeps;
    Q.flags[b] = defined ? 0 : GAUDI_RING_CURRENT_RINGS_UNDEFINED;
    Q.status[b] = GAUDI_HUCKEL_OK;
  }
}
#undef GAUDI_RC_LEAVE

template <int P>
__global__ __launch_bounds__(64) void ring_current_kernel(const RcParams Q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ring_current_lds[];
  ring_current_molecule<P>(Q, *reinterpret_cast<RcSmem<P>*>(ring_current_lds), Q.mol[blockIdx.x], (int)threadIdx.x);
}

struct RcOut {
  float* bond_current;
  int32_t *n_rings, *ring_atoms, *ring_size;
  float *ring_current, *ring_area, *normal, *rms, *gap, *residual;
  int32_t *n_pi, *n_electrons, *sweeps, *flags, *status;
};
constexpr int kRcOuts = 15, kRcStatusOut = 14;

static void rc_out_list(const RcOut& o, int B, int M, void* (&p)[kRcOuts], size_t (&sz)[kRcOuts]) {
  const size_t nB = (size_t)B, rings = kRcMaxRings;
  void* ptrs[kRcOuts] = {o.bond_current, o.n_rings, o.ring_atoms, o.ring_size, o.ring_current, o.ring_area, o.normal, o.rms,
                         o.gap, o.residual, o.n_pi, o.n_electrons, o.sweeps, o.flags, o.status};
  const size_t sizes[kRcOuts] = {4 * nB * M, 4 * nB, 4 * nB * rings * kRcMaxSize, 4 * nB * rings, 4 * nB * rings, 4 * nB * rings,
                                 12 * nB, 4 * nB, 4 * nB, 4 * nB, 4 * nB, 4 * nB, 4 * nB, 4 * nB, 4 * nB};
  for (int i = 0; i < kRcOuts; ++i) {
    p[i] = ptrs[i];
    sz[i] = sizes[i];
  }
}

static void rc_params(RcParams& Q, const gaudi_huckel_tables* t, int B, int A, int M, void* (&outs)[kRcOuts]) {
  Q.in.B = B;
  Q.in.A = A;
  Q.in.M = M;
  Q.in.n_elems = t->n_elems;
  Q.in.h_elem = t->h_elem;
  Q.in.c_elem = t->c_elem;
  Q.bond_current = (float*)outs[0];
  Q.n_rings = (int*)outs[1];
  Q.ring_atoms = (int*)outs[2];
  Q.ring_size = (int*)outs[3];
  Q.ring_current = (float*)outs[4];
  Q.ring_area = (float*)outs[5];
  Q.normal = (float*)outs[6];
  Q.rms = (float*)outs[7];
  Q.gap = (float*)outs[8];
  Q.residual = (float*)outs[9];
  Q.n_pi = (int*)outs[10];
  Q.n_electrons = (int*)outs[11];
  Q.sweeps = (int*)outs[12];
  Q.flags = (int*)outs[13];
  Q.status = (int*)outs[kRcStatusOut];
}

// the arguments checked, the molecules routed and the table read, as gaudi_huckel does
static int rc_prepare(const gaudi_huckel_tables* t, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                      const int32_t* bonds, const int32_t* n_bonds, const float* xyz, HuckelTab& tab, bool& table_ok,
                      std::vector<int>& mol, int (&tier_n)[3], const char** why) {
  *why = "invalid argument";
  if (!xyz) return GAUDI_E_INVALID;
  if (int rc = huckel_prepare(t, B, A, M, elem, n_atoms, bonds, n_bonds, tab, table_ok, mol, tier_n, why)) return rc;
  if ((long long)B * (kRcMaxRings * kRcMaxSize) > (1ll << 31)) {
    *why = "B * 192 beyond 2^31";
    return GAUDI_E_CAPACITY;
  }
  return GAUDI_OK;
}

template <int P>
static int rc_launch(gaudi_handle* h, RcParams Q, const int* mol, int count) {
  if (count == 0) return GAUDI_OK;
  Q.mol = mol;
  constexpr int lds = (int)sizeof(RcSmem<P>);
  {
    // the attribute belongs to the function: one process-wide record per device (see the sampler's launch)
    static std::mutex mu;
    static std::map<int, bool> raised;
    std::lock_guard<std::mutex> lock(mu);
    if (!raised[h->device]) {
      HIPCHECK(h, hipFuncSetAttribute((const void*)ring_current_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      raised[h->device] = true;
    }
  }
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (h->prof) HIPCHECK(h, h->ring_log.begin(h->stream, ev));
  hipLaunchKernelGGL(ring_current_kernel<P>, dim3(count), dim3(64), lds, h->stream, Q);
  HIPCHECK(h, hipGetLastError());
  if (h->prof) HIPCHECK(h, h->ring_log.end(h->stream, ev));
  return GAUDI_OK;
}

template <int P>
static void rc_host_tier(const RcParams& Q, const int* mol, int count) {
  if (count == 0) return;
  std::vector<RcSmem<P>> W(1);
  for (int i = 0; i < count; ++i) ring_current_molecule<P>(Q, W[0], mol[i], 0);
}

}  // namespace gaudi

#define GAUDI_RC_ARGS                                                                                                            \
  const gaudi_huckel_tables *tables, int B, int A, int M, const int32_t *elem, const int32_t *n_atoms, const int32_t *bonds,     \
      const int32_t *n_bonds, const float *xyz, const int32_t *charge, float *bond_current_out, int32_t *n_rings_out,            \
      int32_t *ring_atoms_out, int32_t *ring_size_out, float *ring_current_out, float *ring_area_out, float *normal_out,         \
      float *rms_out_of_plane_out, float *gap_out, float *residual_out, int32_t *n_pi_out, int32_t *n_electrons_out,             \
      int32_t *sweeps_out, int32_t *flags_out, int32_t *status_out
#define GAUDI_RC_OUT                                                                                                             \
  gaudi::RcOut {                                                                                                                 \
    bond_current_out, n_rings_out, ring_atoms_out, ring_size_out, ring_current_out, ring_area_out, normal_out,                   \
        rms_out_of_plane_out, gap_out, residual_out, n_pi_out, n_electrons_out, sweeps_out, flags_out, status_out                \
  }

extern "C" int gaudi_ring_currents(gaudi_handle* h, GAUDI_RC_ARGS) {
  if (!h) return GAUDI_E_INVALID;
  void* outs[gaudi::kRcOuts];
  size_t osz[gaudi::kRcOuts];
  gaudi::rc_out_list(GAUDI_RC_OUT, B > 0 ? B : 0, M, outs, osz);
  for (void* p : outs)
    if (!p) return fail(h, GAUDI_E_INVALID, "every output array is required");
  const char* why = "";
  std::vector<gaudi::HuckelTab> tab(1);
  std::vector<int> mol;
  int tier_n[3];
  bool table_ok = false;
  if (int rc = gaudi::rc_prepare(tables, B, A, M, elem, n_atoms, bonds, n_bonds, xyz, tab[0], table_ok, mol, tier_n, &why))
    return fail(h, rc, why);
  if (B == 0) return GAUDI_OK;
  if (!table_ok) {  // nothing runs on a table that cannot be read: every row zero
    for (int i = 0; i < gaudi::kRcOuts; ++i) memset(outs[i], 0, osz[i]);
    for (int b = 0; b < B; ++b) status_out[b] = GAUDI_HUCKEL_BAD_TABLE;
    return GAUDI_OK;
  }
  HIPCHECK(h, hipSetDevice(h->device));
  const size_t nB = (size_t)B;
  std::vector<int32_t> zero;
  if (!charge) zero.assign(nB, 0);
  constexpr int kIn = 8;
  const size_t isz[kIn] = {sizeof(int) * nB * A, sizeof(int) * nB, sizeof(int) * nB * M * 2,   sizeof(int) * nB,
                           sizeof(int) * nB,     sizeof(int) * nB, sizeof(gaudi::HuckelTab), sizeof(float) * nB * A * 3};
  const void* ins[kIn] = {elem, n_atoms, bonds, n_bonds, charge ? charge : zero.data(), mol.data(), tab.data(), xyz};
  for (int i = 0; i < kIn; ++i) {
    HIPCHECK(h, h->d_ring[i].reserve(isz[i]));
    HIPCHECK(h, hipMemcpyAsync(h->d_ring[i].p, ins[i], isz[i], hipMemcpyHostToDevice, h->stream));
  }
  void* douts[gaudi::kRcOuts];
  for (int i = 0; i < gaudi::kRcOuts; ++i) {  // a refused molecule writes its status only: zero everywhere else
    HIPCHECK(h, h->d_ring[kIn + i].reserve(osz[i]));
    HIPCHECK(h, hipMemsetAsync(h->d_ring[kIn + i].p, 0, osz[i], h->stream));
    douts[i] = h->d_ring[kIn + i].p;
  }
  gaudi::RcParams Q{};
  gaudi::rc_params(Q, tables, B, A, M, douts);
  Q.in.elem = h->d_ring[0].as<int>();
  Q.in.n_atoms = h->d_ring[1].as<int>();
  Q.in.bonds = h->d_ring[2].as<int>();
  Q.in.n_bonds = h->d_ring[3].as<int>();
  Q.charge = h->d_ring[4].as<int>();
  Q.tab = h->d_ring[6].as<gaudi::HuckelTab>();
  Q.xyz = h->d_ring[7].as<float>();
  const int* dmol = h->d_ring[5].as<int>();
  if (int rc = gaudi::rc_launch<32>(h, Q, dmol, tier_n[0])) return rc;
  if (int rc = gaudi::rc_launch<64>(h, Q, dmol + tier_n[0], tier_n[1])) return rc;
  if (int rc = gaudi::rc_launch<128>(h, Q, dmol + tier_n[0] + tier_n[1], tier_n[2])) return rc;
  for (int i = 0; i < gaudi::kRcOuts; ++i)
    HIPCHECK(h, hipMemcpyAsync(outs[i], douts[i], osz[i], hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  return GAUDI_OK;
}

extern "C" int gaudi_host_ring_currents(GAUDI_RC_ARGS) {
  void* outs[gaudi::kRcOuts];
  size_t osz[gaudi::kRcOuts];
  gaudi::rc_out_list(GAUDI_RC_OUT, B > 0 ? B : 0, M, outs, osz);
  for (void* p : outs)
    if (!p) return GAUDI_E_INVALID;
  const char* why = "";
  std::vector<gaudi::HuckelTab> tab(1);
  std::vector<int> mol;
  int tier_n[3];
  bool table_ok = false;
  if (int rc = gaudi::rc_prepare(tables, B, A, M, elem, n_atoms, bonds, n_bonds, xyz, tab[0], table_ok, mol, tier_n, &why)) return rc;
  if (B == 0) return GAUDI_OK;
  for (int i = 0; i < gaudi::kRcOuts; ++i) memset(outs[i], 0, osz[i]);
  if (!table_ok) {
    for (int b = 0; b < B; ++b) status_out[b] = GAUDI_HUCKEL_BAD_TABLE;
    return GAUDI_OK;
  }
  std::vector<int32_t> zero;
  if (!charge) zero.assign((size_t)B, 0);
  gaudi::RcParams Q{};
  gaudi::rc_params(Q, tables, B, A, M, outs);
  Q.in.elem = elem;
  Q.in.n_atoms = n_atoms;
  Q.in.bonds = bonds;
  Q.in.n_bonds = n_bonds;
  Q.charge = charge ? charge : zero.data();
  Q.xyz = xyz;
  Q.tab = tab.data();
  gaudi::rc_host_tier<32>(Q, mol.data(), tier_n[0]);
  gaudi::rc_host_tier<64>(Q, mol.data() + tier_n[0], tier_n[1]);
  gaudi::rc_host_tier<128>(Q, mol.data() + tier_n[0] + tier_n[1], tier_n[2]);
  return GAUDI_OK;
}
#undef GAUDI_RC_ARGS
#undef GAUDI_RC_OUT

extern "C" int gaudi_ring_currents_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms) {
  if (!h || !n_launches || !total_ms) return GAUDI_E_INVALID;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, h->ring_log.fold(0));
  *n_launches = (int32_t)h->ring_log.n;
  *total_ms = h->ring_log.ms;
  return GAUDI_OK;
}
