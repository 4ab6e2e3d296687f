// atoms.inc -- graph of rings -> graph of atoms on the device (included after stability.inc at the end of gaudi_hip.hip).
//
// Replaces data/gor2goa.py:133-261 (gor2goa) with its helpers align_to_xy_plane (:54-85), rotation_2d (:99-105) and
// lineseg_dists (:108-130): the step between a sampled graph of rings and anything that names atoms.  The twin of
// stability.inc: one 64-lane wave per molecule, one launch per call, the fused pairs from the SAME ring_dist / ring_bonded.
//
// Per wave, 25 KB of LDS (two waves per workgroup):
//   1. nodes -> LDS; lane i builds row i of the adjacency; wave-uniform checks for the inputs the reference raises on;
//   2. every lane runs align_to_xy_plane redundantly on wave-uniform data (inertia terms in fp32 as numpy computes them from
//      the fp32 input, sums and everything after in double; the 3 x 3 eigenvectors with LAPACK's signs), lanes project their own nodes;
//   3. lane i places ring i (template, rotation, template H's at the origin, cyclic ring bonds) at the exclusive prefix of the
//      rings' atom counts, and lists its fused pairs (i, j > i) at the prefix of the upper-triangle row counts = np.triu order;
//   4. lane e picks, for fused pair e, the closest ring atom to the centre-to-centre segment on either side, on both rings;
//   5. lane 0 merges in list order (the reference zeroes merged atoms as it goes, so the order is part of the result);
//   6. survivors are renumbered by a wave prefix scan; bonds mapped, rank-sorted, de-duplicated;
//   7. optional hydrogens (lanes = atoms), optional fingerprint (lanes = breadth-first sources, 256-bit visited sets in registers).
// The discrete choices (4) compare doubles the reference also computes in double; contraction of a * b + c may differ from numpy
// in the last bit, which matters only on exact ties -- no implementation can be held to those (tools/make_golden.py g30 filters them).

namespace gaudi {

constexpr int kAtomWaves = 2;
constexpr int kAtomMaxNodes = 2 * kStabMaxRings + 2;  // hetero: 32 rings, 32 orientation nodes, one odd node
constexpr int kAtomRing = 6;                          // ring atoms per template
constexpr int kAtomMaxPre = kStabMaxRings * 8;        // atoms before merging: 6 ring atoms + 2 template H per ring
constexpr int kAtomMaxEdges = 96;                     // fused pairs (32 rings on a triangular lattice have at most 76)
constexpr int kAtomMaxWork = kAtomMaxPre + 2 * kAtomMaxEdges;
constexpr int kAtomMaxHeavy = 256;                    // atoms before hydrogens are placed: width of the fingerprint's bit sets
constexpr int kAtomMaxOut = GAUDI_ATOMS_MAX_ATOMS;
constexpr int kAtomMaxBonds = GAUDI_ATOMS_MAX_BONDS;
static_assert(kAtomMaxPre <= kAtomMaxBonds && kAtomMaxHeavy <= kAtomMaxOut, "capacities");

struct AtomTables {
  int ring_size[kStabMaxTypes], n_h[kStabMaxTypes], no_orient[kStabMaxTypes];
  int h_parent[kStabMaxTypes][2];
  int elem[kStabMaxTypes][kAtomRing];
  double extra[kStabMaxTypes];
  double templ[kStabMaxTypes][kAtomRing][2];
  int h_elem, c_elem;
  double h_bond;
};
struct AtomDevTables {
  StabTables S;
  AtomTables A;
};

struct AtomSmem {
  float x[kAtomMaxNodes][3];
  int type[kAtomMaxNodes];
  unsigned adj[kStabMaxRings];
  double ax[kAtomMaxNodes][2];      // nodes in the aligned frame
  unsigned short rbase[kStabMaxRings];
  unsigned char ei[kAtomMaxEdges], ej[kAtomMaxEdges];
  unsigned short iidx[2 * kAtomMaxEdges], jidx[2 * kAtomMaxEdges];
  unsigned short pb[kAtomMaxPre][2];  // bonds before merging
  unsigned char ftype[kAtomMaxOut];   // final elements
  unsigned keys[kAtomMaxBonds], sorted[kAtomMaxBonds];  // bonds as (min << 16 | max)
  unsigned hcnt[kAtomMaxHeavy];       // fingerprint: attached H's
  union {
    struct {  // construction
      double at[kAtomMaxWork][2];
      unsigned short map[kAtomMaxWork], newidx[kAtomMaxWork];
      unsigned char wtype[kAtomMaxWork], del[kAtomMaxWork];
    } w;
    unsigned adjb[kAtomMaxHeavy][8];  // fingerprint: heavy-atom adjacency as bit rows
  } u1;
  union {
    double fxy[kAtomMaxOut][2];                  // final atoms in the aligned frame
    unsigned long long colour[2][kAtomMaxHeavy];  // fingerprint (after the coordinates have been written out)
  } u2;
};

struct AtomParams {
  int B, N, flags, max_atoms, max_bonds;
  const float* x;
  const int* type;
  const int* n_nodes;
  int* n_atoms;
  int* atom_type;
  double* xy;
  double* xyz;
  int* n_bonds;
  int* bonds;
  int* status;
  unsigned long long* fp;
};

// exclusive prefix sum over the 64 lanes; total = the sum
__device__ __forceinline__ int wave_excl_scan(int v, int lane, int& total) {
  int inc = v;
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(inc, off);
    if (lane >= off) inc += t;
  }
  total = __shfl(inc, 63);
  return inc - v;
}

// ---- numpy.linalg.eigh of a symmetric 3 x 3, with LAPACK's eigenvector SIGNS.
// The reference keeps (e0 . x, e1 . x): the molecule seen along e0 x e1.  Seen from the other side every ring template runs the other
// way round and the `> 0` / `< 0` picks swap, so the ORDER of the merged atoms -- and with it the bond list -- depends on the signs
// LAPACK happens to return.  They are a deterministic function of the matrix, so the solver below restates what numpy calls for
// n = 3, step by step: dsyevd('V', 'L') = dsytd2 (one Householder reflector) + dsteqr('I') (implicit QL / QR with dlaev2 on 2 x 2
// blocks, the 3.10+ dlartg, selection sort) + dormtr.  Rounding may differ in the last bits; the signs do not.
// Host and device: gaudi_host_eigh3 runs the same text on the CPU, where the test suite holds it against np.linalg.eigh.
__host__ __device__ __forceinline__ double f_sign(double a, double b) { return b >= 0.0 ? fabs(a) : -fabs(a); }
__host__ __device__ __forceinline__ double lp_dlapy2(double x, double y) {
  const double w = fmax(fabs(x), fabs(y)), z = fmin(fabs(x), fabs(y));
  return z == 0.0 ? w : w * sqrt(1.0 + (z / w) * (z / w));
}
__host__ __device__ __forceinline__ void lp_dlartg(double f, double g, double& c, double& s, double& r) {
  if (g == 0.0) { c = 1.0; s = 0.0; r = f; return; }
  if (f == 0.0) { c = 0.0; s = f_sign(1.0, g); r = fabs(g); return; }
  const double d = sqrt(f * f + g * g);
  c = fabs(f) / d;
  r = f_sign(d, f);
  s = g / r;
}
__host__ __device__ inline void lp_dlaev2(double a, double b, double c, double& rt1, double& rt2, double& cs1, double& sn1) {
  const double sm = a + c, df = a - c, adf = fabs(df), tb = b + b, ab = fabs(tb);
  const double acmx = fabs(a) > fabs(c) ? a : c, acmn = fabs(a) > fabs(c) ? c : a;
  double rt;
  if (adf > ab) rt = adf * sqrt(1.0 + (ab / adf) * (ab / adf));
  else if (adf < ab) rt = ab * sqrt(1.0 + (adf / ab) * (adf / ab));
  else rt = ab * sqrt(2.0);
  int sgn1, sgn2;
  if (sm < 0.0) { rt1 = 0.5 * (sm - rt); sgn1 = -1; rt2 = (acmx / rt1) * acmn - (b / rt1) * b; }
  else if (sm > 0.0) { rt1 = 0.5 * (sm + rt); sgn1 = 1; rt2 = (acmx / rt1) * acmn - (b / rt1) * b; }
  else { rt1 = 0.5 * rt; rt2 = -0.5 * rt; sgn1 = 1; }
  double cs;
  if (df >= 0.0) { cs = df + rt; sgn2 = 1; }
  else { cs = df - rt; sgn2 = -1; }
  if (fabs(cs) > ab) { const double ct = -tb / cs; sn1 = 1.0 / sqrt(1.0 + ct * ct); cs1 = ct * sn1; }
  else if (ab == 0.0) { cs1 = 1.0; sn1 = 0.0; }
  else { const double tn = -cs / tb; cs1 = 1.0 / sqrt(1.0 + tn * tn); sn1 = tn * cs1; }
  if (sgn1 == sgn2) { const double tn = cs1; cs1 = -sn1; sn1 = tn; }
}
// dlasr('R', 'V', 'F' or 'B') on the 3 rows of Z, columns j0 .. j0 + cnt - 1, rotation k between columns j0 + k and j0 + k + 1
__host__ __device__ inline void lp_dlasr(double Z[3][3], const double* c, const double* s, int j0, int cnt, bool forward) {
  for (int q = 0; q < cnt - 1; ++q) {
    const int k = forward ? q : cnt - 2 - q, j = j0 + k;
    for (int i = 0; i < 3; ++i) {
      const double t = Z[i][j + 1];
      Z[i][j + 1] = c[k] * t - s[k] * Z[i][j];
      Z[i][j] = s[k] * t + c[k] * Z[i][j];
    }
  }
}
// A: symmetric, the lower triangle is read.  E[c][k] = component c of the eigenvector of the k-th smallest eigenvalue.
__host__ __device__ inline void eigh3(const double A[3][3], double E[3][3]) {
  constexpr double kEps = 1.1102230246251565e-16, kSafMin = 2.2250738585072014e-308;
  double a21 = A[1][0], a22 = A[1][1], a32 = A[2][1], a33 = A[2][2];
  const double a31 = A[2][0];
  // dsytd2, uplo = 'L': H = I - tau v v^T with v = (0, 1, v2) takes (a21, a31) to (beta, 0)
  double tau = 0.0, v2 = 0.0;
  if (a31 != 0.0) {
    const double beta = -f_sign(lp_dlapy2(a21, fabs(a31)), a21);
    tau = (beta - a21) / beta;
    v2 = a31 * (1.0 / (a21 - beta));
    a21 = beta;
    const double x1 = tau * (a22 + a32 * v2), x2 = tau * (a32 + a33 * v2);
    const double al = -0.5 * tau * (x1 + x2 * v2);
    const double w1 = x1 + al, w2 = x2 + al * v2;
    a22 -= 2.0 * w1;
    a32 -= v2 * w1 + w2;
    a33 -= 2.0 * v2 * w2;
  }
  double d[3] = {A[0][0], a22, a33}, e[2] = {a21, a32};
  double Z[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  // dsteqr, compz = 'I' (n = 3: no scaling needed for inertia tensors of Angstrom coordinates)
  const int n = 3, nmaxit = 90;
  int jtot = 0, l1 = 0;
  while (l1 < n && jtot < nmaxit) {
    if (l1 > 0) e[l1 - 1] = 0.0;
    int m = n - 1;
    for (int mm = l1; mm < n - 1; ++mm) {
      const double tst = fabs(e[mm]);
      if (tst == 0.0) { m = mm; break; }
      if (tst <= sqrt(fabs(d[mm])) * sqrt(fabs(d[mm + 1])) * kEps) { e[mm] = 0.0; m = mm; break; }
    }
    int l = l1, lend = m;
    const int lsv = l, lendsv = lend;
    l1 = m + 1;
    if (lend == l) continue;
    double anorm = 0.0;
    for (int i = l; i <= lend; ++i) anorm = fmax(anorm, fabs(d[i]));
    for (int i = l; i < lend; ++i) anorm = fmax(anorm, fabs(e[i]));
    if (!(anorm > 0.0)) continue;  // (zero, or NaN input: nothing to iterate on)
    if (fabs(d[lend]) < fabs(d[l])) { lend = lsv; l = lendsv; }
    double cs[2], ss[2];
    if (lend > l) {  // QL iteration
      while (true) {
        m = lend;
        if (l != lend)
          for (int mm = l; mm < lend; ++mm)
            if (fabs(e[mm]) * fabs(e[mm]) <= (kEps * kEps * fabs(d[mm])) * fabs(d[mm + 1]) + kSafMin) { m = mm; break; }
        if (m < lend) e[m] = 0.0;
        double p = d[l];
        if (m == l) {  // eigenvalue found
          ++l;
          if (l <= lend) continue;
          break;
        }
        if (m == l + 1) {
          double rt1, rt2, c, s;
          lp_dlaev2(d[l], e[l], d[l + 1], rt1, rt2, c, s);
          lp_dlasr(Z, &c, &s, l, 2, false);
          d[l] = rt1;
          d[l + 1] = rt2;
          e[l] = 0.0;
          l += 2;
          if (l <= lend) continue;
          break;
        }
        if (jtot == nmaxit) break;
        ++jtot;
        double g = (d[l + 1] - p) / (2.0 * e[l]), r = lp_dlapy2(g, 1.0);
        g = d[m] - p + (e[l] / (g + f_sign(r, g)));
        double s = 1.0, c = 1.0;
        p = 0.0;
        for (int i = m - 1; i >= l; --i) {
          const double f = s * e[i], b = c * e[i];
          lp_dlartg(g, f, c, s, r);
          if (i != m - 1) e[i + 1] = r;
          g = d[i + 1] - p;
          r = (d[i] - g) * s + 2.0 * c * b;
          p = s * r;
          d[i + 1] = g + p;
          g = c * r - b;
          cs[i - l] = c;
          ss[i - l] = -s;
        }
        lp_dlasr(Z, cs, ss, l, m - l + 1, false);
        d[l] -= p;
        e[l] = g;
      }
    } else {  // QR iteration
      while (true) {
        m = lend;
        if (l != lend)
          for (int mm = l; mm > lend; --mm)
            if (fabs(e[mm - 1]) * fabs(e[mm - 1]) <= (kEps * kEps * fabs(d[mm])) * fabs(d[mm - 1]) + kSafMin) { m = mm; break; }
        if (m > lend) e[m - 1] = 0.0;
        double p = d[l];
        if (m == l) {
          --l;
          if (l >= lend) continue;
          break;
        }
        if (m == l - 1) {
          double rt1, rt2, c, s;
          lp_dlaev2(d[l - 1], e[l - 1], d[l], rt1, rt2, c, s);
          lp_dlasr(Z, &c, &s, l - 1, 2, true);
          d[l - 1] = rt1;
          d[l] = rt2;
          e[l - 1] = 0.0;
          l -= 2;
          if (l >= lend) continue;
          break;
        }
        if (jtot == nmaxit) break;
        ++jtot;
        double g = (d[l - 1] - p) / (2.0 * e[l - 1]), r = lp_dlapy2(g, 1.0);
        g = d[m] - p + (e[l - 1] / (g + f_sign(r, g)));
        double s = 1.0, c = 1.0;
        p = 0.0;
        for (int i = m; i < l; ++i) {
          const double f = s * e[i], b = c * e[i];
          lp_dlartg(g, f, c, s, r);
          if (i != m) e[i - 1] = r;
          g = d[i] - p;
          r = (d[i + 1] - g) * s + 2.0 * c * b;
          p = s * r;
          d[i] = g + p;
          g = c * r - b;
          cs[i - m] = c;
          ss[i - m] = s;
        }
        lp_dlasr(Z, cs, ss, m, l - m + 1, true);
        d[l] -= p;
        e[l - 1] = g;
      }
    }
  }
  // selection sort into ascending order, columns along
  for (int ii = 1; ii < n; ++ii) {
    const int i = ii - 1;
    int k = i;
    double p = d[i];
    for (int j = ii; j < n; ++j)
      if (d[j] < p) { k = j; p = d[j]; }
    if (k != i) {
      d[k] = d[i];
      d[i] = p;
      for (int r = 0; r < 3; ++r) { const double t = Z[r][i]; Z[r][i] = Z[r][k]; Z[r][k] = t; }
    }
  }
  // dormtr: Z := H Z
  for (int j = 0; j < 3; ++j) {
    const double t = tau * (Z[1][j] + v2 * Z[2][j]);
    E[0][j] = Z[0][j];
    E[1][j] = Z[1][j] - t;
    E[2][j] = Z[2][j] - t * v2;
  }
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {  // the splitmix64 finaliser
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// rank-sort keys[0..n) into out (ties by index), then keep the first of every run of equal keys, back into keys; returns the count
__device__ inline int sort_unique(unsigned* keys, unsigned* out, int n, int lane) {
  for (int q = lane; q < n; q += 64) {
    const unsigned k = keys[q];
    int rank = 0;
    for (int r = 0; r < n; ++r) {
      const unsigned o = keys[r];
      rank += (o < k) || (o == k && r < q);
    }
    out[rank] = k;
  }
  wave_lds_fence();
  const int per = (n + 63) / 64, lo = lane * per, hi = min(n, lo + per);
  int cnt = 0;
  for (int q = lo; q < hi; ++q) cnt += q == 0 || out[q] != out[q - 1];
  int total;
  int pos = wave_excl_scan(cnt, lane, total);
  for (int q = lo; q < hi; ++q)
    if (q == 0 || out[q] != out[q - 1]) keys[pos++] = out[q];
  wave_lds_fence();
  return total;
}

// -(sum of unit vectors from atom a to its heavy neighbours), normalised: where a hydrogen on a goes.  nb bonds in keys.
__device__ inline void outward(const AtomSmem& s, const AtomTables& A, int a, int nb, double& dx, double& dy, int& heavy_deg) {
  double sx = 0.0, sy = 0.0, lx = 0.0, ly = 0.0;
  int deg = 0;
  const double px = s.u2.fxy[a][0], py = s.u2.fxy[a][1];
  for (int q = 0; q < nb; ++q) {
    const int i = (int)(s.keys[q] >> 16), j = (int)(s.keys[q] & 0xffffu);
    if ((i != a && j != a) || i == j) continue;
    const int o = i == a ? j : i;
    if (s.ftype[o] == A.h_elem) continue;
    const double vx = s.u2.fxy[o][0] - px, vy = s.u2.fxy[o][1] - py;
    const double r = sqrt(vx * vx + vy * vy);
    if (r > 0.0) {
      lx = vx / r;
      ly = vy / r;
      sx += lx;
      sy += ly;
    }
    ++deg;
  }
  heavy_deg = deg;
  double r = sqrt(sx * sx + sy * sy);
  if (!(r > 1e-9)) {  // no heavy neighbour, or neighbours that cancel (a straight angle): perpendicular to the last bond, or +x
    sx = deg ? ly : -1.0;
    sy = deg ? -lx : 0.0;
    r = 1.0;
  }
  dx = -sx / r;
  dy = -sy / r;
}

__global__ __launch_bounds__(64 * kAtomWaves) void atoms_kernel(const AtomParams P, const AtomDevTables* __restrict__ Tp) {
  const StabTables& T = Tp->S;
  const AtomTables& A = Tp->A;
  __shared__ AtomSmem smem[kAtomWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * kAtomWaves + w;
  if (b >= P.B) return;
  AtomSmem& s = smem[w];
  const int N = P.N;
  const int n = P.n_nodes[b];                   // 1 .. min(N, kAtomMaxNodes - 1): checked by the host
  const int nr = T.orientation ? n / 2 : n;     // <= kStabMaxRings: checked by the host
  const float* xb = P.x + (size_t)b * N * 3;
  const int* tb = P.type + (size_t)b * N;
  const int MA = P.max_atoms, MB = P.max_bonds;
  const bool place_h = (P.flags & GAUDI_ATOMS_PLACE_H) != 0, want_fp = (P.flags & GAUDI_ATOMS_FINGERPRINT) != 0;
  int status = GAUDI_ATOMS_BUILT, n_atoms = 0, n_bonds = 0;
  unsigned long long fp = 0ull;

  do {  // every `break` below is wave-uniform
    if (nr < 1) { status = GAUDI_ATOMS_NO_RINGS; break; }
    for (int i = lane; i < n * 3; i += 64) s.x[i / 3][i % 3] = xb[i];
    bool bad = false;
    for (int i = lane; i < n; i += 64) {
      const int t = tb[i];
      s.type[i] = t;
      if (i < nr) {
        const bool in_table = t >= 0 && t < T.n_types;
        // (a ring that needs an orientation node in a dataset without them: orientation[i] of an empty array)
        bad |= !in_table || A.ring_size[in_table ? t : 0] == 0 || (!T.orientation && !A.no_orient[in_table ? t : 0]);
      }
    }
    if (__ballot(bad) != 0ull) { status = GAUDI_ATOMS_BAD_TYPE; break; }
    wave_lds_fence();

    // ---- 1. adjacency of the rings: positions2adj, as stability_kernel computes it
    unsigned row = 0u;
    int my_type = 0;
    if (lane < nr) {
      my_type = s.type[lane];
      for (int j = 0; j < nr; ++j) {
        const float dist = ring_dist(s.x[lane], s.x[j]);
        row |= (j != lane && ring_bonded(T, my_type, s.type[j], dist)) ? (1u << j) : 0u;
      }
      s.adj[lane] = row;
    }
    // gor2goa.py:159: adj[i].nonzero()[0, 0] of a ring without neighbours -- reached by NO_ORIENTATION rings only
    if (__ballot(lane < nr && nr > 1 && A.no_orient[my_type] && row == 0u) != 0ull) { status = GAUDI_ATOMS_NO_NEIGHBOUR; break; }

    // ---- 2. align_to_xy_plane (gor2goa.py:54-85), redundantly in every lane
    double I[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, com[3] = {0, 0, 0}, E[3][3];
    for (int i = 0; i < n; ++i) {
      const float a0 = s.x[i][0], a1 = s.x[i][1], a2 = s.x[i][2];
      // numpy evaluates these on np.float32 scalars, then adds the float32 matrix to the float64 one
      const float q0 = mul_rn(a0, a0), q1 = mul_rn(a1, a1), q2 = mul_rn(a2, a2);
      I[0][0] += (double)add_rn(q1, q2);
      I[1][1] += (double)add_rn(q0, q2);
      I[2][2] += (double)add_rn(q0, q1);
      I[0][1] += (double)mul_rn(-a0, a1);
      I[0][2] += (double)mul_rn(-a0, a2);
      I[1][2] += (double)mul_rn(-a1, a2);
      com[0] += (double)a0;
      com[1] += (double)a1;
      com[2] += (double)a2;
    }
    I[1][0] = I[0][1];
    I[2][0] = I[0][2];
    I[2][1] = I[1][2];
    com[0] /= 3.0;  // `com / len(com)`: the length of the 3-vector, not the node count
    com[1] /= 3.0;
    com[2] /= 3.0;
    eigh3(I, E);
    for (int i = lane; i < n; i += 64) {
      const double d0 = (double)s.x[i][0] - com[0], d1 = (double)s.x[i][1] - com[1], d2 = (double)s.x[i][2] - com[2];
      s.ax[i][0] = E[0][0] * d0 + E[1][0] * d1 + E[2][0] * d2;
      s.ax[i][1] = E[0][1] * d0 + E[1][1] * d1 + E[2][1] * d2;
    }
    wave_lds_fence();

    // ---- 3. ring placement (gor2goa.py:151-198) and the list of fused pairs (:203-207)
    int cnt = 0, up = 0;
    if (lane < nr) {
      cnt = A.ring_size[my_type] + A.n_h[my_type];
      up = __popc(row & ~((2u << lane) - 1u));
    }
    int Ptot, Etot;
    const int base = wave_excl_scan(cnt, lane, Ptot);
    int ebase = wave_excl_scan(up, lane, Etot);
    if (Etot > kAtomMaxEdges) { status = GAUDI_ATOMS_OVERFLOW; break; }
    const int Wtot = Ptot + 2 * Etot;  // <= kAtomMaxWork
    for (int a = lane; a < Wtot; a += 64) {
      s.u1.w.map[a] = (unsigned short)a;
      s.u1.w.del[a] = 0;
    }
    if (lane < nr) {
      const int t = my_type, sz = A.ring_size[t];
      double angle;
      if (A.no_orient[t]) {
        angle = 0.0;
        if (nr > 1) {
          const int j = __ffs(row) - 1;
          angle = atan2(s.ax[j][1] - s.ax[lane][1], s.ax[j][0] - s.ax[lane][0]);
        }
        angle += A.extra[t];
      } else {
        angle = atan2(s.ax[nr + lane][1] - s.ax[lane][1], s.ax[nr + lane][0] - s.ax[lane][0]);
      }
      // ring @ rotation_2d(-angle): [[cos, -sin], [sin, cos]] of -angle, applied from the right
      const double c = cos(-angle), sn = sin(-angle);
      for (int k = 0; k < sz; ++k) {
        const double rx = A.templ[t][k][0], ry = A.templ[t][k][1];
        s.u1.w.at[base + k][0] = rx * c + ry * sn + s.ax[lane][0];
        s.u1.w.at[base + k][1] = rx * -sn + ry * c + s.ax[lane][1];
        s.u1.w.wtype[base + k] = (unsigned char)A.elem[t][k];
        s.pb[base + k][0] = (unsigned short)(base + k);
        s.pb[base + k][1] = (unsigned short)(base + (k + 1 == sz ? 0 : k + 1));
      }
      for (int q = 0; q < A.n_h[t]; ++q) {  // template H's stay at the origin (gor2goa.py:190-198)
        s.u1.w.at[base + sz + q][0] = 0.0;
        s.u1.w.at[base + sz + q][1] = 0.0;
        s.u1.w.wtype[base + sz + q] = (unsigned char)A.h_elem;
        s.pb[base + sz + q][0] = (unsigned short)(base + A.h_parent[t][q]);
        s.pb[base + sz + q][1] = (unsigned short)(base + sz + q);
      }
      s.rbase[lane] = (unsigned short)base;
      unsigned m = row & ~((2u << lane) - 1u);
      while (m) {
        s.ei[ebase] = (unsigned char)lane;
        s.ej[ebase] = (unsigned char)(__ffs(m) - 1);
        m &= m - 1;
        ++ebase;
      }
    }
    wave_lds_fence();

    // ---- 4. per fused pair: the closest ring atom to the centre-to-centre segment on either side (gor2goa.py:209-229)
    for (int e = lane; e < Etot; e += 64) {
      const int ri = s.ei[e], rj = s.ej[e];
      const double p1x = s.ax[ri][0], p1y = s.ax[ri][1], p2x = s.ax[rj][0], p2y = s.ax[rj][1];
      const double vx = p2x - p1x, vy = p2y - p1y;
      const double nv = sqrt(vx * vx + vy * vy);
      const double dx = vx / nv, dy = vy / nv;
      for (int side = 0; side < 2; ++side) {
        const int r = side ? rj : ri;
        const int rb = s.rbase[r], sz = A.ring_size[s.type[r]];
        double best1 = INFINITY, best2 = INFINITY;
        int k1 = 0, k2 = 0;
        for (int k = 0; k < sz; ++k) {
          const double px = s.u1.w.at[rb + k][0], py = s.u1.w.at[rb + k][1];
          // lineseg_dists (gor2goa.py:108-130)
          const double sp = (p1x - px) * dx + (p1y - py) * dy;
          const double tp = (px - p2x) * dx + (py - p2y) * dy;
          const double hh = fmax(fmax(sp, tp), 0.0);
          const double cc = (px - p1x) * dy - (py - p1y) * dx;
          const double dist = hypot(hh, cc);
          const double sd = (vx * (p1y - py) - vy * (p1x - px)) / nv;
          const double v1 = sd > 0.0 ? INFINITY : dist, v2 = sd < 0.0 ? INFINITY : dist;
          if (v1 < best1) { best1 = v1; k1 = k; }  // np.argmin: the first minimum, index 0 when everything is inf
          if (v2 < best2) { best2 = v2; k2 = k; }
        }
        unsigned short* dst = side ? s.jidx : s.iidx;
        dst[2 * e] = (unsigned short)(rb + k1);
        dst[2 * e + 1] = (unsigned short)(rb + k2);
      }
    }
    wave_lds_fence();

    // ---- 5. merge in list order (gor2goa.py:231-240): merged atoms are zeroed as the loop goes
    if (lane == 0) {
      for (int k = 0; k < 2 * Etot; ++k) {
        const int i = s.iidx[k], j = s.jidx[k];
        s.u1.w.at[Ptot + k][0] = (s.u1.w.at[i][0] + s.u1.w.at[j][0]) / 2.0;
        s.u1.w.at[Ptot + k][1] = (s.u1.w.at[i][1] + s.u1.w.at[j][1]) / 2.0;
        s.u1.w.wtype[Ptot + k] = s.u1.w.wtype[i];
        s.u1.w.map[i] = s.u1.w.map[j] = (unsigned short)(Ptot + k);
        s.u1.w.at[i][0] = s.u1.w.at[i][1] = s.u1.w.at[j][0] = s.u1.w.at[j][1] = 0.0;
        s.u1.w.del[i] = s.u1.w.del[j] = 1;
      }
    }
    wave_lds_fence();

    // ---- 6. delete, renumber (gor2goa.py:246-254), map and de-duplicate the bonds (:257-258)
    {
      const int per = (Wtot + 63) / 64, lo = lane * per, hi = min(Wtot, lo + per);
      int keep = 0;
      for (int a = lo; a < hi; ++a) keep += !s.u1.w.del[a];
      int pos = wave_excl_scan(keep, lane, n_atoms);
      if (n_atoms > kAtomMaxHeavy || n_atoms > MA || Ptot > MB) { status = GAUDI_ATOMS_OVERFLOW; break; }
      for (int a = lo; a < hi; ++a) {
        if (s.u1.w.del[a]) continue;
        s.u1.w.newidx[a] = (unsigned short)pos;
        s.u2.fxy[pos][0] = s.u1.w.at[a][0];
        s.u2.fxy[pos][1] = s.u1.w.at[a][1];
        s.ftype[pos] = s.u1.w.wtype[a];
        ++pos;
      }
    }
    wave_lds_fence();
    for (int q = lane; q < Ptot; q += 64) {
      const unsigned i = s.u1.w.newidx[s.u1.w.map[s.pb[q][0]]], j = s.u1.w.newidx[s.u1.w.map[s.pb[q][1]]];
      s.keys[q] = i < j ? (i << 16 | j) : (j << 16 | i);
    }
    wave_lds_fence();
    n_bonds = sort_unique(s.keys, s.sorted, Ptot, lane);
    const int n_pre = n_atoms, nb_pre = n_bonds;  // before hydrogens are placed

    // ---- 7a. hydrogens
    if (place_h) {
      const int per = (n_pre + 63) / 64, lo = lane * per, hi = min(n_pre, lo + per);
      int need = 0;
      for (int a = lo; a < hi; ++a) {
        if (s.ftype[a] != A.c_elem) continue;
        double dx, dy;
        int deg;
        outward(s, A, a, nb_pre, dx, dy, deg);
        need += deg == 2;
      }
      int added;
      int pos = wave_excl_scan(need, lane, added);
      if (n_pre + added > MA || n_pre + added > kAtomMaxOut || nb_pre + added > MB || nb_pre + added > kAtomMaxBonds) {
        status = GAUDI_ATOMS_OVERFLOW;
        break;
      }
      for (int a = lo; a < hi; ++a) {
        if (s.ftype[a] == A.h_elem) {  // a template H: from the origin to its ring atom's outward direction
          int parent = -1;
          for (int q = 0; q < nb_pre && parent < 0; ++q) {
            const int i = (int)(s.keys[q] >> 16), j = (int)(s.keys[q] & 0xffffu);
            if (i == a && j != a) parent = j;
            if (j == a && i != a) parent = i;
          }
          if (parent < 0) continue;
          double dx, dy;
          int deg;
          outward(s, A, parent, nb_pre, dx, dy, deg);
          s.u2.fxy[a][0] = s.u2.fxy[parent][0] + A.h_bond * dx;  // (H positions are never read by `outward`)
          s.u2.fxy[a][1] = s.u2.fxy[parent][1] + A.h_bond * dy;
        } else if (s.ftype[a] == A.c_elem) {
          double dx, dy;
          int deg;
          outward(s, A, a, nb_pre, dx, dy, deg);
          if (deg != 2) continue;
          const int hidx = n_pre + pos;
          s.u2.fxy[hidx][0] = s.u2.fxy[a][0] + A.h_bond * dx;
          s.u2.fxy[hidx][1] = s.u2.fxy[a][1] + A.h_bond * dy;
          s.ftype[hidx] = (unsigned char)A.h_elem;
          s.sorted[pos] = (unsigned)a << 16 | (unsigned)hidx;  // parked: keys is being read
          ++pos;
        }
      }
      wave_lds_fence();
      for (int q = lane; q < added; q += 64) s.keys[nb_pre + q] = s.sorted[q];
      wave_lds_fence();
      n_atoms = n_pre + added;
      n_bonds = sort_unique(s.keys, s.sorted, nb_pre + added, lane);
    }

    // ---- outputs
    {
      int* ty = P.atom_type + (size_t)b * MA;
      double* xy = P.xy + (size_t)b * MA * 2;
      double* xyz = P.xyz + (size_t)b * MA * 3;
      for (int a = lane; a < n_atoms; a += 64) {
        const double u = s.u2.fxy[a][0], v = s.u2.fxy[a][1];
        ty[a] = s.ftype[a];
        xy[2 * a] = u;
        xy[2 * a + 1] = v;
        xyz[3 * a] = com[0] + E[0][0] * u + E[0][1] * v;
        xyz[3 * a + 1] = com[1] + E[1][0] * u + E[1][1] * v;
        xyz[3 * a + 2] = com[2] + E[2][0] * u + E[2][1] * v;
      }
      int* bo = P.bonds + (size_t)b * MB * 2;
      for (int q = lane; q < n_bonds; q += 64) {
        bo[2 * q] = (int)(s.keys[q] >> 16);
        bo[2 * q + 1] = (int)(s.keys[q] & 0xffffu);
      }
    }

    // ---- 7b. fingerprint of the heavy-atom graph (atoms 0 .. n_pre; bonds to placed H's have an end beyond)
    if (want_fp) {
      wave_lds_fence();  // fxy has been read: u2 becomes the colours, u1 the bit rows
      for (int i = lane; i < n_pre * 8; i += 64) (&s.u1.adjb[0][0])[i] = 0u;
      for (int a = lane; a < n_pre; a += 64) s.hcnt[a] = 0u;
      wave_lds_fence();
      int hb = 0;
      for (int q = lane; q < n_bonds; q += 64) {
        const int i = (int)(s.keys[q] >> 16), j = (int)(s.keys[q] & 0xffffu);
        if (j >= n_pre || i == j) continue;
        const bool hi_ = s.ftype[i] == A.h_elem, hj = s.ftype[j] == A.h_elem;
        if (!hi_ && !hj) {
          atomicOr(&s.u1.adjb[i][j >> 5], 1u << (j & 31));
          atomicOr(&s.u1.adjb[j][i >> 5], 1u << (i & 31));
          ++hb;
        } else if (hi_ != hj) {
          atomicAdd(&s.hcnt[hi_ ? j : i], 1u);
        }
      }
      for (int off = 32; off > 0; off >>= 1) hb += __shfl_xor(hb, off);
      wave_lds_fence();
      int n_heavy = 0;
      for (int a = lane; a < n_pre; a += 64) n_heavy += s.ftype[a] != A.h_elem;
      for (int off = 32; off > 0; off >>= 1) n_heavy += __shfl_xor(n_heavy, off);
      // initial colour: element, heavy degree, attached H's, histogram of shortest-path lengths
      for (int a = lane; a < n_pre; a += 64) {
        if (s.ftype[a] == A.h_elem) continue;
        unsigned vis[8], fr[8], nx[8];
        int deg = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          vis[q] = fr[q] = (a >> 5) == q ? 1u << (a & 31) : 0u;
          deg += __popc(s.u1.adjb[a][q]);
        }
        unsigned long long ph = 0ull;
        int reached = 1;
        for (int level = 1; level <= n_pre; ++level) {
#pragma unroll
          for (int q = 0; q < 8; ++q) nx[q] = 0u;
#pragma unroll
          for (int wd = 0; wd < 8; ++wd) {
            unsigned f = fr[wd];
            while (f) {
              const int v = wd * 32 + __ffs(f) - 1;
              f &= f - 1;
#pragma unroll
              for (int q = 0; q < 8; ++q) nx[q] |= s.u1.adjb[v][q];
            }
          }
          int c = 0;
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            nx[q] &= ~vis[q];
            vis[q] |= nx[q];
            fr[q] = nx[q];
            c += __popc(nx[q]);
          }
          if (c == 0) break;
          reached += c;
          ph = mix64(ph ^ ((unsigned long long)level << 32 | (unsigned)c));
        }
        ph = mix64(ph ^ (unsigned long long)(n_heavy - reached));  // atoms of other fragments
        const unsigned hc = s.hcnt[a] + (s.ftype[a] == A.c_elem && deg == 2 ? 1u : 0u);
        s.u2.colour[0][a] = mix64(ph ^ ((unsigned long long)s.ftype[a] << 48 | (unsigned long long)deg << 32 | hc));
      }
      wave_lds_fence();
      // Weisfeiler-Lehman rounds until the number of colour classes stops growing
      int cur = 0, classes = -1;
      for (int round = 0; round <= n_heavy; ++round) {
        int distinct = 0;
        for (int a = lane; a < n_pre; a += 64) {
          if (s.ftype[a] == A.h_elem) continue;
          const unsigned long long ca = s.u2.colour[cur][a];
          bool first = true;
          for (int o = 0; o < a && first; ++o) first = s.ftype[o] == A.h_elem || s.u2.colour[cur][o] != ca;
          distinct += first;
        }
        for (int off = 32; off > 0; off >>= 1) distinct += __shfl_xor(distinct, off);
        if (distinct == classes) break;
        classes = distinct;
        for (int a = lane; a < n_pre; a += 64) {
          if (s.ftype[a] == A.h_elem) continue;
          unsigned long long acc = 0ull;  // the neighbours' colours as a multiset: a sum of mixed values
#pragma unroll
          for (int wd = 0; wd < 8; ++wd) {
            unsigned f = s.u1.adjb[a][wd];
            while (f) {
              const int v = wd * 32 + __ffs(f) - 1;
              f &= f - 1;
              acc += mix64(s.u2.colour[cur][v]);
            }
          }
          s.u2.colour[cur ^ 1][a] = mix64(s.u2.colour[cur][a] * 0x9e3779b97f4a7c15ull + acc);
        }
        wave_lds_fence();
        cur ^= 1;
      }
      unsigned long long acc = 0ull;
      for (int a = lane; a < n_pre; a += 64)
        if (s.ftype[a] != A.h_elem) acc += mix64(s.u2.colour[cur][a]);
      for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
      fp = mix64(acc ^ ((unsigned long long)n_heavy << 32 | (unsigned)hb));
      if (fp == 0ull) fp = 1ull;  // 0 means "not built"
    }
  } while (false);

  if (lane == 0) {
    P.status[b] = status;
    P.n_atoms[b] = status ? 0 : n_atoms;
    P.n_bonds[b] = status ? 0 : n_bonds;
    if (P.fp) P.fp[b] = status ? 0ull : fp;
  }
}

}  // namespace gaudi

extern "C" int gaudi_rings_to_atoms(gaudi_handle* h, const gaudi_ring_tables* tb, const gaudi_atom_tables* at, int B, int N,
                                    const float* x, const int32_t* ring_type, const int32_t* n_nodes, int flags, int max_atoms,
                                    int max_bonds, int32_t* n_atoms_out, int32_t* atom_type_out, double* xy_out, double* xyz_out,
                                    int32_t* n_bonds_out, int32_t* bonds_out, int32_t* status_out, uint64_t* fingerprint_out) {
  if (!h || !tb || !at || !x || !ring_type || !n_nodes || !n_atoms_out || !atom_type_out || !xy_out || !xyz_out || !n_bonds_out ||
      !bonds_out || !status_out || B < 0 || N < 1)
    return GAUDI_E_INVALID;
  if ((flags & GAUDI_ATOMS_FINGERPRINT) && !fingerprint_out) return fail(h, GAUDI_E_INVALID, "fingerprint asked for without a buffer");
  if (flags & ~(GAUDI_ATOMS_PLACE_H | GAUDI_ATOMS_FINGERPRINT)) return fail(h, GAUDI_E_INVALID, "unknown flag");
  if (tb->n_types < 1 || tb->n_types > gaudi::kStabMaxTypes || at->n_types != tb->n_types)
    return fail(h, GAUDI_E_INVALID, "n_types must be in 1..16 and the same in both tables");
  if (max_atoms < 1 || max_atoms > GAUDI_ATOMS_MAX_ATOMS || max_bonds < 1 || max_bonds > GAUDI_ATOMS_MAX_BONDS)
    return fail(h, GAUDI_E_INVALID, "max_atoms / max_bonds must be in 1..384");
  std::vector<gaudi::AtomDevTables> Dv(1);
  gaudi::AtomDevTables* D = Dv.data();
  gaudi::AtomTables& A = D->A;
  if (at->h_elem < 0 || at->h_elem > 255 || at->c_elem < 0 || at->c_elem > 255) return fail(h, GAUDI_E_INVALID, "element index outside 0..255");
  for (int t = 0; t < tb->n_types; ++t) {
    const int sz = at->ring_size[t], nh = at->n_template_h[t];
    if (sz != 0 && (sz < 3 || sz > gaudi::kAtomRing)) return fail(h, GAUDI_E_INVALID, "ring_size must be 0 or 3..6");
    if (nh < 0 || nh > 2) return fail(h, GAUDI_E_INVALID, "n_template_h must be in 0..2");
    A.ring_size[t] = sz;
    A.n_h[t] = nh;
    A.no_orient[t] = at->no_orientation[t] != 0;
    A.extra[t] = at->extra_angle[t];
    for (int q = 0; q < 2; ++q) {
      if (q < nh && (at->template_h_parent[t][q] < 0 || at->template_h_parent[t][q] >= sz))
        return fail(h, GAUDI_E_INVALID, "template_h_parent outside the ring");
      A.h_parent[t][q] = q < nh ? at->template_h_parent[t][q] : 0;
    }
    for (int k = 0; k < gaudi::kAtomRing; ++k) {
      if (k < sz && (at->ring_elem[t][k] < 0 || at->ring_elem[t][k] > 255)) return fail(h, GAUDI_E_INVALID, "element index outside 0..255");
      A.elem[t][k] = k < sz ? at->ring_elem[t][k] : 0;
      A.templ[t][k][0] = k < sz ? at->templ[t][k][0] : 0.0;
      A.templ[t][k][1] = k < sz ? at->templ[t][k][1] : 0.0;
    }
  }
  A.h_elem = at->h_elem;
  A.c_elem = at->c_elem;
  A.h_bond = at->h_bond;
  if (B == 0) return GAUDI_OK;
  for (int b = 0; b < B; ++b) {
    const int n = n_nodes[b];
    if (n < 1 || n > N) return fail(h, GAUDI_E_INVALID, "n_nodes must be in 1..N");
    if ((tb->orientation ? n / 2 : n) > gaudi::kStabMaxRings) return fail(h, GAUDI_E_CAPACITY, "more than 32 rings in one molecule");
  }
  HIPCHECK(h, hipSetDevice(h->device));
  if (int rc = stab_device_tables(h, tb, D->S)) return rc;

  const size_t nB = (size_t)B;
  const size_t sizes[] = {sizeof(float) * nB * N * 3,      sizeof(int) * nB * N,           sizeof(int) * nB,
                          sizeof(int) * nB,                sizeof(int) * nB * max_atoms,   sizeof(double) * nB * max_atoms * 2,
                          sizeof(double) * nB * max_atoms * 3, sizeof(int) * nB,           sizeof(int) * nB * max_bonds * 2,
                          sizeof(int) * nB,                sizeof(uint64_t) * nB,          sizeof(gaudi::AtomDevTables)};
  DevBuf* bufs[] = {&h->d_sx, &h->d_stype, &h->d_sn, &h->d_atoms[0], &h->d_atoms[1], &h->d_atoms[2],
                    &h->d_atoms[3], &h->d_atoms[4], &h->d_atoms[5], &h->d_atoms[6], &h->d_atoms[7], &h->d_atoms[8]};
  for (int i = 0; i < 12; ++i) HIPCHECK(h, bufs[i]->reserve(sizes[i]));
  HIPCHECK(h, hipMemcpyAsync(h->d_sx.p, x, sizes[0], hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(h->d_stype.p, ring_type, sizes[1], hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(h->d_sn.p, n_nodes, sizes[2], hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(h->d_atoms[8].p, D, sizes[11], hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));  // D is a local object
  // rows beyond a molecule's n_atoms / n_bonds are not written by the kernel: zero them once
  for (int i = 4; i <= 6; ++i) HIPCHECK(h, hipMemsetAsync(bufs[i]->p, 0, sizes[i], h->stream));
  HIPCHECK(h, hipMemsetAsync(bufs[8]->p, 0, sizes[8], h->stream));
  gaudi::AtomParams P{};
  P.B = B;
  P.N = N;
  P.flags = flags;
  P.max_atoms = max_atoms;
  P.max_bonds = max_bonds;
  P.x = h->d_sx.as<float>();
  P.type = h->d_stype.as<int>();
  P.n_nodes = h->d_sn.as<int>();
  P.n_atoms = h->d_atoms[0].as<int>();
  P.atom_type = h->d_atoms[1].as<int>();
  P.xy = h->d_atoms[2].as<double>();
  P.xyz = h->d_atoms[3].as<double>();
  P.n_bonds = h->d_atoms[4].as<int>();
  P.bonds = h->d_atoms[5].as<int>();
  P.status = h->d_atoms[6].as<int>();
  P.fp = (flags & GAUDI_ATOMS_FINGERPRINT) ? h->d_atoms[7].as<unsigned long long>() : nullptr;
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (h->prof) HIPCHECK(h, h->atoms_log.begin(h->stream, ev));
  hipLaunchKernelGGL(gaudi::atoms_kernel, dim3((B + gaudi::kAtomWaves - 1) / gaudi::kAtomWaves), dim3(64 * gaudi::kAtomWaves), 0,
                     h->stream, P, (const gaudi::AtomDevTables*)h->d_atoms[8].p);
  HIPCHECK(h, hipGetLastError());
  if (h->prof) HIPCHECK(h, h->atoms_log.end(h->stream, ev));
  void* outs[] = {n_atoms_out, atom_type_out, xy_out, xyz_out, n_bonds_out, bonds_out, status_out};
  for (int i = 0; i < 7; ++i) HIPCHECK(h, hipMemcpyAsync(outs[i], bufs[3 + i]->p, sizes[3 + i], hipMemcpyDeviceToHost, h->stream));
  if (P.fp) HIPCHECK(h, hipMemcpyAsync(fingerprint_out, h->d_atoms[7].p, sizes[10], hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  return GAUDI_OK;
}

extern "C" int gaudi_atoms_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms) {
  if (!h || !n_launches || !total_ms) return GAUDI_E_INVALID;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, h->atoms_log.fold(0));
  *n_launches = (int32_t)h->atoms_log.n;
  *total_ms = h->atoms_log.ms;
  return GAUDI_OK;
}

extern "C" int gaudi_host_eigh3(int n, const double* a, double* e_out) {
  if (n < 0 || (n > 0 && (!a || !e_out))) return GAUDI_E_INVALID;
  for (int q = 0; q < n; ++q) {
    double A[3][3], E[3][3];
    for (int i = 0; i < 9; ++i) A[i / 3][i % 3] = a[(size_t)q * 9 + i];
    gaudi::eigh3(A, E);
    for (int i = 0; i < 9; ++i) e_out[(size_t)q * 9 + i] = E[i / 3][i % 3];
  }
  return GAUDI_OK;
}
