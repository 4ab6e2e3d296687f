// reactivity.inc -- Hueckel localization energies of a graph of atoms: the pi energy lost when the attacked centres are taken out of
// conjugation (Wheland's atom localization energy, Brown's para-localization energy, the ortho / bond localization energy) and
// the free valence (included after ring_current.inc at the end of gaudi_hip.hip; DESIGN.md section 8r; the model is spelled out
// in include/gaudi_hip.h).
//
// The pi centres, the matrix and the levels are huckel.inc's, through its own routines: canon_graph, huckel_sites, huckel_matrix,
// jacobi_sweeps, huckel_rayleigh; the rings are ring_current.inc's rc_ring_enum.  ONE text, two builds, as huckel.inc: a 64-lane
// wave on the device, one lane that walks every index on the host (kRwLanes).  The grid is (molecule of the tier, slice), one wave
// per workgroup.  Every wave
//   1. classifies the sites and solves the parent itself (one solve out of dozens); keeps the parent's sparse matrix;
//   2. enumerates the chordless rings of 4 to 6 centres, a lane's centres a contiguous ascending range so that the order found is
//      the host's; the rings of a smallest centre are kept while the count through that centre stays within 32 (what is dropped
//      does not depend on the walk), ranked by sorted atom tuple and reported from the smallest centre in the order found;
//   3. lists the six-rings among them and (with_bonds) the listed bonds between two pi centres: the molecule's fixed job order is
//      the centres ascending, then (six-ring, pair k = 0..2) in ring order, then those bonds in list order;
//   4. runs the jobs j = slice (mod slices): the surviving centres are compacted into the reduced sparse matrix (rows, and a row's
//      bonds, in the parent's order), diagonalised, ranked and filled by the shared routines; the job's value is stored by lane 0.
// Slice 0 alone writes the per-molecule scalars, the rings, the free valence and the quiet NaN of every entry no job owns.  Every
// output element is written by exactly one wave with plain vector stores; no atomics; every branch around a fence or a reduction
// is lane-uniform; loop bounds come from n, the ring count and n_bonds only.  Every fp32 operation is individually rounded and
// every sum runs in one fixed order, so a job's bits do not depend on the tier, the batch, the molecule's place in it or `slices`,
// and the device gives the host build's bits.  The per-molecule sweep total and the flag of a residual solve at the sweep cap are
// folded on the host side of the entry point from one int per job (rx_fold): no second launch, no cross-wave reduction.

namespace gaudi {

constexpr int kRxKinds = GAUDI_REACTIVITY_KINDS;
constexpr int kRxMaxSlices = GAUDI_REACTIVITY_MAX_SLICES;
constexpr int kRxPairs = 3;                      // pairs of opposite positions of a six-ring
constexpr int kRxCapBit = 1 << 16;               // in a job's sweep word: the solve hit the sweep cap
constexpr int kRxNaN = 0x7fc00000;               // the quiet NaN of an entry that does not apply
constexpr float kRxMaxValence = 1.7320508f;      // sqrt(3): the largest sum of pi bond orders of a carbon centre
constexpr int kRxJobsFixed = kHuckelMaxPi + kRxPairs * kRcMaxRings;  // a row of job words holds these and M bond jobs
static_assert(kRxKinds == 3 && kRxMaxSlices == 16 && kHuckelSweeps < kRxCapBit, "kinds q = 0, 1, 2; a job word holds sweeps and the cap bit");

template <int P>
struct RxSmem : HuckelSmem<P> {
  float phd[P], pkn[P][kHuckelNbr];    // the parent's sparse matrix (a job overwrites hd, nb, kn with its own)
  kek_u64 uam[kRcMaxRings][2];         // a ring's centres as a mask, in the order found
  unsigned short pib[kCanonMaxBonds];  // the listed bonds between two pi centres, ascending
  unsigned char pnb[P][kHuckelNbr];
  unsigned char cyc[kRcMaxRings][kRcMaxSize], scyc[kRcMaxRings][kRcMaxSize];  // rings in cycle order: as found, as reported
  unsigned char csz[kRcMaxRings], ssz[kRcMaxRings];
  unsigned char six[kRcMaxRings];      // the six-rings among the reported rings, ascending
};
static_assert(sizeof(RxSmem<128>) <= 160 * 1024, "the largest tier fits the LDS of a CU");

struct RxParams {
  CanonParams in;  // the input fields only
  const int* mol;  // the molecules of this launch (one capacity tier)
  const int* charge;
  const HuckelTab* tab;
  int with_bonds, slices;
  float* atom_loc;      // [B][3][A]
  float* free_valence;  // [B][A]
  int* rings;           // [B][32][6]
  int* n_rings;         // [B]
  float* para;          // [B][32][3]
  float* ortho;         // [B][M]
  float* e_pi;          // [B]
  int *n_pi, *n_electrons, *n_jobs, *sweeps, *flags, *status;  // [B]
  int* job_word;        // [B][kRxJobsFixed + M]: a job's sweeps, and kRxCapBit
};

// the levels in s.x ranked by counting (ties: the smaller index first) into s.lev: huckel.inc, step 4
template <class S>
__host__ __device__ inline void rx_rank(S& s, int n, int lane) {
  for (int i = lane; i < n; i += kRwLanes) {
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
}

// the pi energy of n_el electrons on the ranked levels, two per level from the lowest energy, the last level may hold one: the
// sum huckel_molecule forms for e_pi, term by term, in fp32.  Every lane computes it alike.
template <class S>
__host__ __device__ inline float rx_energy(const S& s, int n_el) {
#pragma clang fp contract(off)
  const int n_occ = (n_el + 1) >> 1;
  float e = 0.0f;
  for (int k = 0; k < n_occ; ++k) e = e + (float)(2 * (k + 1) <= n_el ? 2 : 1) * s.lev[k];
  return e;
}

// ... and the same sum in fp64, where every product and (to 2^-53) every partial sum is exact: a localization energy is the
// difference of two such sums of the order of n_pi, and an fp32 accumulator's rounding (half an ulp of the running sum per term)
// would outweigh the error of the levels themselves.  Individually rounded, one fixed order: the same bits on both builds.
template <class S>
__host__ __device__ inline double rx_energy64(const S& s, int n_el) {
#pragma clang fp contract(off)
  const int n_occ = (n_el + 1) >> 1;
  double e = 0.0;
  for (int k = 0; k < n_occ; ++k) e = e + (double)(2 * (k + 1) <= n_el ? 2 : 1) * (double)s.lev[k];
  return e;
}

// The parent without centre d0, or without d0 < d1 (d1 = none: one centre): the m surviving centres compacted in ascending
// order into s.a, s.v and the sparse matrix, a row's bonds in the parent's order; diagonalised and ranked into s.lev.  false:
// the sweep cap.  Every lane calls it with the same arguments.
template <int P>
__host__ __device__ inline bool rx_residual(RxSmem<P>& s, int m, int d0, int d1, int lane, int& sweeps) {
  rw_fence();
  for (int r = 0; r < m; ++r)
    for (int c = lane; c < m; c += kRwLanes) {
      s.a[r][c] = 0.0f;
      s.v[r][c] = r == c ? 1.0f : 0.0f;
    }
  rw_fence();
  for (int r = lane; r < m; r += kRwLanes) {
    int o = r;
    o += o >= d0;
    o += o >= d1;
    const float hr = s.phd[o];
    s.a[r][r] = hr;
    s.hd[r] = hr;
    int d = 0;
    for (int q = 0; q < kHuckelNbr; ++q) {
      const int t = s.pnb[o][q];
      if (t == kCanonNone) break;
      if (t == d0 || t == d1) continue;
      const int nt = t - (t > d0) - (t > d1);
      const float kk = s.pkn[o][q];
      s.a[r][nt] = kk;
      s.nb[r][d] = (unsigned char)nt;
      s.kn[r][d] = kk;
      ++d;
    }
    for (; d < kHuckelNbr; ++d) {
      s.nb[r][d] = (unsigned char)kCanonNone;
      s.kn[r][d] = 0.0f;
    }
  }
  rw_fence();
  const bool converged = jacobi_sweeps<P>(s, m, lane, kHuckelOff, sweeps);
  huckel_rayleigh(s, m, lane);
  rx_rank(s, m, lane);
  return converged;
}

// the status of a molecule that leaves without a result: slice 0 writes it
#define GAUDI_RX_LEAVE(code)                        \
  {                                                 \
    if (first && lane == 0) Q.status[b] = (code);   \
    return;                                         \
  }

// One molecule's slice.  Every branch around a fence or a reduction is lane-uniform.
template <int P>
__host__ __device__ inline void reactivity_molecule(const RxParams& Q, RxSmem<P>& s, int b, int slice, int lane) {
#pragma clang fp contract(off)
  const int A = Q.in.A, M = Q.in.M;
  const bool first = slice == 0;
  int H = 0, E = 0;
  const int gstatus = canon_graph(Q.in, s.g, b, lane, H, E);
  if (gstatus != GAUDI_CANON_OK) GAUDI_RX_LEAVE(gstatus);
  const HuckelTab& T = *Q.tab;
  // ---- 1. the parent: huckel.inc's steps 1 to 4
  int n, n_el;
  const int refused = huckel_sites<P>(T, s, H, Q.charge[b], lane, n, n_el);
  if (refused != GAUDI_HUCKEL_OK) GAUDI_RX_LEAVE(refused);
  huckel_matrix(T, s, n, lane);
  int parent_sweeps = 0;
  if (!jacobi_sweeps<P>(s, n, lane, kHuckelOff, parent_sweeps)) GAUDI_RX_LEAVE(GAUDI_HUCKEL_NOT_CONVERGED);
  huckel_rayleigh(s, n, lane);
  rx_rank(s, n, lane);
  const float e_parent = rx_energy(s, n_el);
  const double e_parent64 = rx_energy64(s, n_el);
  for (int r = lane; r < n; r += kRwLanes) {
    s.phd[r] = s.hd[r];
    for (int d = 0; d < kHuckelNbr; ++d) {
      s.pnb[r][d] = s.nb[r][d];
      s.pkn[r][d] = s.kn[r][d];
    }
  }
  rw_fence();
  // ---- 2. the rings: counted, stored at the prefix of the counts while a centre's rings fit, ranked by their sorted atom tuple
  const int per = (n + kRwLanes - 1) / kRwLanes, lo = lane * per, hi = lo + per < n ? lo + per : n;
  int mine = 0;
  for (int a = lo; a < hi; ++a) mine += rc_ring_enum(s, a, false, 0);
  int found_all;
  int base = rw_scan(mine, lane, found_all);
  int kept = 0;
  for (int a = lo; a < hi; ++a) {
    const int c = rc_ring_enum(s, a, false, 0);
    if (base + c <= kRcMaxRings) kept += rc_ring_enum(s, a, true, base);
    base += c;
  }
  int R;
  (void)rw_scan(kept, lane, R);
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
  for (int r = lane; r < R; r += kRwLanes) {
    // of two chordless cycles (neither holds the other) the one with the lowest centre they differ in has the smaller sorted tuple
    const kek_u64 a0 = s.uam[r][0], a1 = s.uam[r][1];
    int rank = 0;
    for (int o = 0; o < R; ++o) {
      const kek_u64 d0 = a0 ^ s.uam[o][0], d1 = a1 ^ s.uam[o][1];
      rank += d0 ? ((d0 & (0 - d0)) & s.uam[o][0]) != 0 : d1 ? ((d1 & (0 - d1)) & s.uam[o][1]) != 0 : 0;
    }
    const int size = s.csz[r];
    for (int j = 0; j < kRcMaxSize; ++j) s.scyc[rank][j] = j < size ? s.cyc[r][j] : (unsigned char)kCanonNone;
    s.ssz[rank] = (unsigned char)size;
  }
  rw_fence();
  // ---- 3. the job lists
  int n6 = 0;
  for (int r = 0; r < R; ++r) {
    if (s.ssz[r] != kRcMaxSize) continue;
    if (lane == 0) s.six[n6] = (unsigned char)r;
    ++n6;
  }
  const int n_atoms = Q.in.n_atoms[b], n_bonds = Q.in.n_bonds[b];
  int n_pib = 0;
  if (Q.with_bonds) {
    const int bper = (n_bonds + kRwLanes - 1) / kRwLanes, blo = lane * bper, bhi = blo + bper < n_bonds ? blo + bper : n_bonds;
    int cnt = 0;
    for (int pass = 0; pass < 2; ++pass) {
      int at = pass == 0 ? 0 : rw_scan(cnt, lane, n_pib);
      for (int e = blo; e < bhi; ++e) {
        const int hi_ = s.g.hidx[s.g.bl[e][0]], hj = s.g.hidx[s.g.bl[e][1]];
        if (hi_ == kCanonNone || hj == kCanonNone) continue;
        if (s.pidx[hi_] == kCanonNone || s.pidx[hj] == kCanonNone) continue;
        if (pass == 0)
          ++cnt;
        else
          s.pib[at++] = (unsigned short)e;
      }
    }
  }
  rw_fence();
  const int n_pair_jobs = kRxPairs * n6, n_jobs = n + n_pair_jobs + n_pib;
  // ---- the parent's outputs and the quiet NaN of every entry no job owns: slice 0
  if (first) {
    const int n_occ = (n_el + 1) >> 1;
    float* loc = Q.atom_loc + (size_t)b * kRxKinds * A;
    for (int a = lane; a < A; a += kRwLanes) {
      const int hv = a < n_atoms ? (int)s.g.hidx[a] : kCanonNone;
      if (hv != kCanonNone && s.pidx[hv] != kCanonNone) continue;
      for (int q = 0; q < kRxKinds; ++q) loc[(size_t)q * A + a] = __builtin_bit_cast(float, kRxNaN);
      Q.free_valence[(size_t)b * A + a] = __builtin_bit_cast(float, kRxNaN);
    }
    for (int r = lane; r < n; r += kRwLanes) {  // the free valence: sqrt(3) less the pi bond orders to the centre's pi neighbours
      float sum = 0.0f;
      for (int d = 0; d < kHuckelNbr; ++d) {
        const int o = s.pnb[r][d];
        if (o == kCanonNone) break;
        float acc = 0.0f;
        for (int k = 0; k < n_occ; ++k) {
          const int i = s.ord[k];
          acc = acc + (float)(2 * (k + 1) <= n_el ? 2 : 1) * (s.v[r][i] * s.v[o][i]);
        }
        sum = sum + acc;
      }
      Q.free_valence[(size_t)b * A + s.g.hv[s.vert[r]]] = kRxMaxValence - sum;
    }
    int* rings = Q.rings + (size_t)b * kRcMaxRings * kRcMaxSize;
    for (int i = lane; i < kRcMaxRings * kRcMaxSize; i += kRwLanes) {
      const int r = i / kRcMaxSize, j = i - r * kRcMaxSize;
      rings[i] = r < R && j < s.ssz[r] ? (int)s.g.hv[s.vert[s.scyc[r][j]]] : -1;
    }
    for (int i = lane; i < kRcMaxRings * kRxPairs; i += kRwLanes) {
      const int r = i / kRxPairs;
      if (!(r < R && s.ssz[r] == kRcMaxSize)) Q.para[(size_t)b * kRcMaxRings * kRxPairs + i] = __builtin_bit_cast(float, kRxNaN);
    }
    for (int e = lane; e < M; e += kRwLanes) {
      bool job = Q.with_bonds && e < n_bonds;
      if (job) {
        const int hi_ = s.g.hidx[s.g.bl[e][0]], hj = s.g.hidx[s.g.bl[e][1]];
        job = hi_ != kCanonNone && hj != kCanonNone && s.pidx[hi_] != kCanonNone && s.pidx[hj] != kCanonNone;
      }
      if (!job) Q.ortho[(size_t)b * M + e] = __builtin_bit_cast(float, kRxNaN);
    }
    if (lane == 0) {
      Q.n_rings[b] = R;
      Q.e_pi[b] = e_parent;
      Q.n_pi[b] = n;
      Q.n_electrons[b] = n_el;
      Q.n_jobs[b] = n_jobs;
      Q.sweeps[b] = parent_sweeps;
      Q.flags[b] = R < found_all ? GAUDI_REACTIVITY_RINGS_TRUNCATED : 0;
      Q.status[b] = GAUDI_HUCKEL_OK;
    }
  }
  // ---- 4. this slice's jobs
  int* words = Q.job_word + (size_t)b * (kRxJobsFixed + M);
  for (int j = slice; j < n_jobs; j += Q.slices) {
    int x, y = kCanonNone;
    if (j < n) {
      x = j;
    } else if (j < n + n_pair_jobs) {
      const int t = j - n, ring = s.six[t / kRxPairs], k = t % kRxPairs;
      x = s.scyc[ring][k];
      y = s.scyc[ring][k + kRxPairs];
    } else {
      const int e = s.pib[j - n - n_pair_jobs];
      x = s.pidx[s.g.hidx[s.g.bl[e][0]]];
      y = s.pidx[s.g.hidx[s.g.bl[e][1]]];
    }
    const bool pair = y != kCanonNone;
    const int d0 = pair && y < x ? y : x, d1 = pair ? (y < x ? x : y) : kCanonNone;
    const int m = n - (pair ? 2 : 1);
    // the kinds to fill: q electrons stay on the deleted centre(s); a pair keeps two
    const int q_lo = pair ? 2 : 0, q_hi = 2;
    bool any = false;
    for (int q = q_lo; q <= q_hi; ++q) any = any || (n_el - q >= 0 && n_el - q <= 2 * m);
    int sw = 0;
    bool solved = true;
    if (any && m > 0) solved = rx_residual<P>(s, m, d0, d1, lane, sw);
    const double h_sum = pair ? (double)s.phd[d0] + (double)s.phd[d1] : (double)s.phd[d0];
    float val[kRxKinds];
    for (int q = 0; q < kRxKinds; ++q) {
      const int ne = n_el - q;
      val[q] = __builtin_bit_cast(float, kRxNaN);
      if (q < q_lo || !solved || ne < 0 || ne > 2 * m) continue;
      const double e = m > 0 ? rx_energy64(s, ne) : 0.0;
      val[q] = (float)(e_parent64 - (e + (pair ? h_sum : (double)q * h_sum)));
    }
    if (lane == 0) {
      if (j < n) {
        const size_t at = (size_t)b * kRxKinds * A + s.g.hv[s.vert[x]];
        for (int q = 0; q < kRxKinds; ++q) Q.atom_loc[at + (size_t)q * A] = val[q];
      } else if (j < n + n_pair_jobs) {
        const int t = j - n;
        Q.para[((size_t)b * kRcMaxRings + s.six[t / kRxPairs]) * kRxPairs + t % kRxPairs] = val[2];
      } else {
        Q.ortho[(size_t)b * M + s.pib[j - n - n_pair_jobs]] = val[2];
      }
      words[j] = sw | (solved ? 0 : kRxCapBit);
    }
  }
}
#undef GAUDI_RX_LEAVE

template <int P>
__global__ __launch_bounds__(64) void reactivity_kernel(const RxParams Q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char reactivity_lds[];
  reactivity_molecule<P>(Q, *reinterpret_cast<RxSmem<P>*>(reactivity_lds), Q.mol[blockIdx.x], (int)blockIdx.y, (int)threadIdx.x);
}

struct RxOut {
  float *atom_loc, *free_valence;
  int32_t *rings, *n_rings;
  float *para, *ortho, *e_pi;
  int32_t *n_pi, *n_electrons, *n_jobs, *sweeps, *flags, *status;
};
constexpr int kRxOuts = 13, kRxStatusOut = 12, kRxWordBuf = 20;  // d_react: seven inputs, thirteen outputs, the job words

static void rx_out_list(const RxOut& o, int B, int A, int M, void* (&p)[kRxOuts], size_t (&sz)[kRxOuts]) {
  const size_t nB = (size_t)B, rings = kRcMaxRings;
  void* ptrs[kRxOuts] = {o.atom_loc, o.free_valence, o.rings, o.n_rings, o.para, o.ortho, o.e_pi,
                         o.n_pi, o.n_electrons, o.n_jobs, o.sweeps, o.flags, o.status};
  const size_t sizes[kRxOuts] = {4 * nB * kRxKinds * A, 4 * nB * A, 4 * nB * rings * kRcMaxSize, 4 * nB, 4 * nB * rings * kRxPairs,
                                 4 * nB * M, 4 * nB, 4 * nB, 4 * nB, 4 * nB, 4 * nB, 4 * nB, 4 * nB};
  for (int i = 0; i < kRxOuts; ++i) {
    p[i] = ptrs[i];
    sz[i] = sizes[i];
  }
}

static void rx_params(RxParams& Q, const gaudi_huckel_tables* t, int B, int A, int M, int with_bonds, int slices, void* (&outs)[kRxOuts],
                      int* job_word) {
  Q.in.B = B;
  Q.in.A = A;
  Q.in.M = M;
  Q.in.n_elems = t->n_elems;
  Q.in.h_elem = t->h_elem;
  Q.in.c_elem = t->c_elem;
  Q.with_bonds = with_bonds != 0;
  Q.slices = slices;
  Q.atom_loc = (float*)outs[0];
  Q.free_valence = (float*)outs[1];
  Q.rings = (int*)outs[2];
  Q.n_rings = (int*)outs[3];
  Q.para = (float*)outs[4];
  Q.ortho = (float*)outs[5];
  Q.e_pi = (float*)outs[6];
  Q.n_pi = (int*)outs[7];
  Q.n_electrons = (int*)outs[8];
  Q.n_jobs = (int*)outs[9];
  Q.sweeps = (int*)outs[10];
  Q.flags = (int*)outs[11];
  Q.status = (int*)outs[kRxStatusOut];
  Q.job_word = job_word;
}

// the arguments checked, the molecules routed and the table read, as gaudi_huckel does
static int rx_prepare(const gaudi_huckel_tables* t, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                      const int32_t* bonds, const int32_t* n_bonds, int slices, HuckelTab& tab, bool& table_ok, std::vector<int>& mol,
                      int (&tier_n)[3], const char** why) {
  if (int rc = huckel_prepare(t, B, A, M, elem, n_atoms, bonds, n_bonds, tab, table_ok, mol, tier_n, why)) return rc;
  if (slices < 0 || slices > kRxMaxSlices) {
    *why = "slices outside 0..16";
    return GAUDI_E_INVALID;
  }
  if ((long long)B * kRxKinds * A > (1ll << 31) || (long long)B * (kRxJobsFixed + M) > (1ll << 31)) {
    *why = "B * max(3 A, 224 + M) beyond 2^31";
    return GAUDI_E_CAPACITY;
  }
  return GAUDI_OK;
}

// The per-molecule sums the waves of a molecule cannot form without meeting: the sweeps of every residual solve added to the
// parent's, and the flag of a residual solve at the sweep cap.  From the downloaded job words, on the host.
static void rx_fold(int B, int M, const int32_t* job_word, const int32_t* n_jobs, const int32_t* status, int32_t* sweeps, int32_t* flags) {
  for (int b = 0; b < B; ++b) {
    if (status[b] != GAUDI_HUCKEL_OK) continue;
    const int32_t* w = job_word + (size_t)b * (kRxJobsFixed + M);
    for (int j = 0; j < n_jobs[b]; ++j) {
      sweeps[b] += w[j] & (kRxCapBit - 1);
      if (w[j] & kRxCapBit) flags[b] |= GAUDI_REACTIVITY_SWEEP_CAP;
    }
  }
}

// Slices for a tier of `count` molecules when the caller leaves the choice (slices = 0): enough workgroups for two per CU, no
// more than kRxMaxSlices per molecule: ceil(2 * CUs / count) clamped to 1..16.  A batch of 2 * CUs molecules or more runs unsliced.
static int rx_slices(int num_cus, int count) {
  const int want = (2 * num_cus + count - 1) / count;
  return want < 1 ? 1 : want > kRxMaxSlices ? kRxMaxSlices : want;
}

template <int P>
static int rx_launch(gaudi_handle* h, RxParams Q, const int* mol, int count, int slices) {
  if (count == 0) return GAUDI_OK;
  Q.mol = mol;
  Q.slices = slices > 0 ? slices : rx_slices(h->num_cus, count);
  constexpr int lds = (int)sizeof(RxSmem<P>);
  {
    // the attribute belongs to the function: one process-wide record per device (see the sampler's launch)
    static std::mutex mu;
    static std::map<int, bool> raised;
    std::lock_guard<std::mutex> lock(mu);
    if (!raised[h->device]) {
      HIPCHECK(h, hipFuncSetAttribute((const void*)reactivity_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      raised[h->device] = true;
    }
  }
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (h->prof) HIPCHECK(h, h->react_log.begin(h->stream, ev));
  hipLaunchKernelGGL(reactivity_kernel<P>, dim3(count, Q.slices), dim3(64), lds, h->stream, Q);
  HIPCHECK(h, hipGetLastError());
  if (h->prof) HIPCHECK(h, h->react_log.end(h->stream, ev));
  return GAUDI_OK;
}

template <int P>
static void rx_host_tier(const RxParams& Q, const int* mol, int count) {
  if (count == 0) return;
  std::vector<RxSmem<P>> W(1);
  for (int i = 0; i < count; ++i)
    for (int slice = 0; slice < Q.slices; ++slice) reactivity_molecule<P>(Q, W[0], mol[i], slice, 0);
}

}  // namespace gaudi

#define GAUDI_RX_ARGS                                                                                                            \
  const gaudi_huckel_tables *tables, int B, int A, int M, const int32_t *elem, const int32_t *n_atoms, const int32_t *bonds,     \
      const int32_t *n_bonds, const int32_t *charge, int with_bonds, int slices, float *atom_localization_out,                   \
      float *free_valence_out, int32_t *rings_out, int32_t *n_rings_out, float *para_localization_out,                           \
      float *ortho_localization_out, float *e_pi_out, int32_t *n_pi_out, int32_t *n_electrons_out, int32_t *n_jobs_out,          \
      int32_t *sweeps_out, int32_t *flags_out, int32_t *status_out
#define GAUDI_RX_OUT                                                                                                             \
  gaudi::RxOut {                                                                                                                 \
    atom_localization_out, free_valence_out, rings_out, n_rings_out, para_localization_out, ortho_localization_out, e_pi_out,    \
        n_pi_out, n_electrons_out, n_jobs_out, sweeps_out, flags_out, status_out                                                 \
  }

extern "C" int gaudi_reactivity(gaudi_handle* h, GAUDI_RX_ARGS) {
  if (!h) return GAUDI_E_INVALID;
  void* outs[gaudi::kRxOuts];
  size_t osz[gaudi::kRxOuts];
  gaudi::rx_out_list(GAUDI_RX_OUT, B > 0 ? B : 0, A, M, outs, osz);
  for (void* p : outs)
    if (!p) return fail(h, GAUDI_E_INVALID, "every output array is required");
  const char* why = "";
  std::vector<gaudi::HuckelTab> tab(1);
  std::vector<int> mol;
  int tier_n[3];
  bool table_ok = false;
  if (int rc = gaudi::rx_prepare(tables, B, A, M, elem, n_atoms, bonds, n_bonds, slices, tab[0], table_ok, mol, tier_n, &why))
    return fail(h, rc, why);
  if (B == 0) return GAUDI_OK;
  if (!table_ok) {  // nothing runs on a table that cannot be read: every row zero
    for (int i = 0; i < gaudi::kRxOuts; ++i) memset(outs[i], 0, osz[i]);
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
    HIPCHECK(h, h->d_react[i].reserve(isz[i]));
    HIPCHECK(h, hipMemcpyAsync(h->d_react[i].p, ins[i], isz[i], hipMemcpyHostToDevice, h->stream));
  }
  void* douts[gaudi::kRxOuts];
  for (int i = 0; i < gaudi::kRxOuts; ++i) {  // a refused molecule writes its status only: zero everywhere else
    HIPCHECK(h, h->d_react[kIn + i].reserve(osz[i]));
    HIPCHECK(h, hipMemsetAsync(h->d_react[kIn + i].p, 0, osz[i], h->stream));
    douts[i] = h->d_react[kIn + i].p;
  }
  const size_t wsz = sizeof(int32_t) * nB * (gaudi::kRxJobsFixed + M);
  HIPCHECK(h, h->d_react[gaudi::kRxWordBuf].reserve(wsz));
  HIPCHECK(h, hipMemsetAsync(h->d_react[gaudi::kRxWordBuf].p, 0, wsz, h->stream));
  gaudi::RxParams Q{};
  gaudi::rx_params(Q, tables, B, A, M, with_bonds, slices, douts, h->d_react[gaudi::kRxWordBuf].as<int>());
  Q.in.elem = h->d_react[0].as<int>();
  Q.in.n_atoms = h->d_react[1].as<int>();
  Q.in.bonds = h->d_react[2].as<int>();
  Q.in.n_bonds = h->d_react[3].as<int>();
  Q.charge = h->d_react[4].as<int>();
  Q.tab = h->d_react[6].as<gaudi::HuckelTab>();
  const int* dmol = h->d_react[5].as<int>();
  if (int rc = gaudi::rx_launch<32>(h, Q, dmol, tier_n[0], slices)) return rc;
  if (int rc = gaudi::rx_launch<64>(h, Q, dmol + tier_n[0], tier_n[1], slices)) return rc;
  if (int rc = gaudi::rx_launch<128>(h, Q, dmol + tier_n[0] + tier_n[1], tier_n[2], slices)) return rc;
  std::vector<int32_t> words(nB * (gaudi::kRxJobsFixed + M));
  for (int i = 0; i < gaudi::kRxOuts; ++i)
    HIPCHECK(h, hipMemcpyAsync(outs[i], douts[i], osz[i], hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipMemcpyAsync(words.data(), h->d_react[gaudi::kRxWordBuf].p, wsz, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  gaudi::rx_fold(B, M, words.data(), n_jobs_out, status_out, sweeps_out, flags_out);
  return GAUDI_OK;
}

extern "C" int gaudi_host_reactivity(GAUDI_RX_ARGS) {
  void* outs[gaudi::kRxOuts];
  size_t osz[gaudi::kRxOuts];
  gaudi::rx_out_list(GAUDI_RX_OUT, B > 0 ? B : 0, A, M, outs, osz);
  for (void* p : outs)
    if (!p) return GAUDI_E_INVALID;
  const char* why = "";
  std::vector<gaudi::HuckelTab> tab(1);
  std::vector<int> mol;
  int tier_n[3];
  bool table_ok = false;
  if (int rc = gaudi::rx_prepare(tables, B, A, M, elem, n_atoms, bonds, n_bonds, slices, tab[0], table_ok, mol, tier_n, &why)) return rc;
  if (B == 0) return GAUDI_OK;
  for (int i = 0; i < gaudi::kRxOuts; ++i) memset(outs[i], 0, osz[i]);
  if (!table_ok) {
    for (int b = 0; b < B; ++b) status_out[b] = GAUDI_HUCKEL_BAD_TABLE;
    return GAUDI_OK;
  }
  std::vector<int32_t> zero;
  if (!charge) zero.assign((size_t)B, 0);
  std::vector<int32_t> words((size_t)B * (gaudi::kRxJobsFixed + M), 0);
  gaudi::RxParams Q{};
  gaudi::rx_params(Q, tables, B, A, M, with_bonds, slices > 0 ? slices : 1, outs, words.data());
  Q.in.elem = elem;
  Q.in.n_atoms = n_atoms;
  Q.in.bonds = bonds;
  Q.in.n_bonds = n_bonds;
  Q.charge = charge ? charge : zero.data();
  Q.tab = tab.data();
  gaudi::rx_host_tier<32>(Q, mol.data(), tier_n[0]);
  gaudi::rx_host_tier<64>(Q, mol.data() + tier_n[0], tier_n[1]);
  gaudi::rx_host_tier<128>(Q, mol.data() + tier_n[0] + tier_n[1], tier_n[2]);
  gaudi::rx_fold(B, M, words.data(), n_jobs_out, status_out, sweeps_out, flags_out);
  return GAUDI_OK;
}
#undef GAUDI_RX_ARGS
#undef GAUDI_RX_OUT

extern "C" int gaudi_reactivity_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms) {
  if (!h || !n_launches || !total_ms) return GAUDI_E_INVALID;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, h->react_log.fold(0));
  *n_launches = (int32_t)h->react_log.n;
  *total_ms = h->react_log.ms;
  return GAUDI_OK;
}
