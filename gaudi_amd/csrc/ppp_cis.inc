// ppp_cis.inc -- PPP-CIS excited states: singlet and triplet excitation energies, transition dipoles, oscillator strengths and the
// leading configuration of every singlet, from the PPP ground state (included after ppp.inc at the end of gaudi_hip.hip; DESIGN.md
// section 8n; the model is spelled out in include/gaudi_hip.h).
//
// A SECOND KERNEL after the SCF kernels of ppp.inc, one launch for all tiers: ppp_molecule hands a solved molecule over in a row of
// global scratch (ppp_cis_handover: n, n_occ, the two window-edge separations, the centres' coordinates and gamma, and the at most
// sixteen active levels with their eigenvector columns), and what a kernel wrote is visible to the next one on the stream.  ONE
// text, two builds, as ppp.inc: a 64-lane wave per molecule on the device, one lane that walks every index on the host (kRwLanes).
// Per molecule, with D = n_o * n_v <= 64 configurations (i -> a) ordered by (i ascending, a ascending):
//   1. lane = column jb.  For r ascending the wave forms the row gamma_r. once (lane = s), then lane jb forms
//      J_r = sum_s gamma_rs (C_sj C_sb) and the L^a_r = sum_s gamma_rs (C_sa C_sb), s ascending, and adds
//      (C_ri C_ra) J_r to (ia|jb) and (C_ri C_rj) L^a_r to (ij|ab) for ia <= jb: its column's upper part.  No integral table;
//   2. T = delta (eps_a - eps_i) - (ij|ab), S = T + 2 (ia|jb) on the upper triangle, mirrored below the diagonal: the same bits on
//      either side.  Both are stashed in the molecule's scratch row, a lane writing and later reading its own columns only;
//   3. per spin: a = the matrix, v = I, jacobi_sweeps<64> (huckel.inc) with ppp.inc's threshold rule on this matrix's diagonal; the
//      columns normalised; a = the matrix again; the excitation energies are the dense Rayleigh quotients v^T a v in one fixed
//      order, ranked by counting (ties: the smaller index first);
//   4. of singlet k: mu = sqrt2 sum_ia X_ia,k d_ia with d_ia = sum_r (C_ri C_ra)(x_r - x_0), f = (kCisOsc E) |mu|^2, and the
//      configuration of the largest X^2 (ties: the smaller index).
// Arithmetic as ppp.inc: individually rounded fp32, every sum in one fixed order, no atomics, lane-uniform branches around fences.

namespace gaudi {

constexpr int kCisDim = GAUDI_PPP_CIS_MAX_STATES;
constexpr float kCisOsc = 0.08748948f;   // (2 / 3) / 27.211386 / 0.52917721^2: eV and e Angstrom to atomic units
constexpr float kCisSqrt2 = 1.4142135f;
static_assert(kCisDim == kCisMaxWindow * kCisMaxWindow && kCisDim == 64, "lane = configuration; the solver's capacity tier is 64");

struct CisSmem {
  float a[kCisDim][kCisDim + 1], v[kCisDim][kCisDim + 1];
  float c[kCisAct][kHuckelMaxPi];  // the active columns of C: 0..7 occupied (ascending rank), 8..15 empty
  float xyz[kHuckelMaxPi][3], gam[kHuckelMaxPi];
  float eps[kCisAct];
  float g[kHuckelMaxPi];                // gamma_r. of the row in hand
  float l[kCisMaxWindow][kCisDim];      // L^a_r of a lane's column
  float d[kCisDim][3];                  // the transition dipole of a configuration
  float x[kCisDim];                     // an energy per column
  float rc[kCisDim / 2], rs[kCisDim / 2], rpp[kCisDim / 2], rqq[kCisDim / 2];  // jacobi_sweeps' rotations
  unsigned char rp[kCisDim / 2], rq[kCisDim / 2];
  float t1;
};
static_assert(sizeof(CisSmem) <= 48 * 1024, "three waves of the CIS stage share the LDS of a CU");

struct CisParams {
  int B, repulsion, window;
  float* rows;  // [B][kCisRow]: what ppp_molecule handed over, and the stash of S and T
  int *status, *flags;  // gaudi_ppp's: read; the CIS bits are added
  float *singlet, *triplet, *osc, *dipole;  // [B][64], [B][64], [B][64], [B][64][3]
  unsigned char* lead;                      // [B][64][2]
  float* lead_weight;                       // [B][64]
  int *n_states, *n_active_occ, *n_active_virt, *cis_sweeps;  // [B]
};

// One spin: the matrix `mat` (the lane's own columns of the scratch row) diagonalised, s.v = its normalised eigenvectors,
// s.x = the Rayleigh quotient of every column.  Every lane calls it with the same D.
__host__ __device__ inline bool cis_solve(CisSmem& s, const float* mat, int D, int lane, int& sweeps) {
#pragma clang fp contract(off)
  for (int c = lane; c < D; c += kRwLanes)
    for (int r = 0; r < D; ++r) {
      s.a[r][c] = mat[r * kCisDim + c];
      s.v[r][c] = r == c ? 1.0f : 0.0f;
    }
  rw_fence();
  float big = 0.0f;  // ppp.inc's rule: 2^-24 of the largest |diagonal|, rounded up to a power of two
  for (int r = lane; r < D; r += kRwLanes) {
    const float t = fabsf(s.a[r][r]);
    big = t > big ? t : big;
  }
  const int bits = -rw_min(-huckel_bits(big));
  int e = (bits >> 23) + ((bits & 0x7fffff) != 0) - 24;
  e = e < 1 ? 1 : e > 254 ? 254 : e;
  const bool ok = jacobi_sweeps<kCisDim>(s, D, lane, __builtin_bit_cast(float, e << 23), sweeps);
  for (int k = lane; k < D; k += kRwLanes) {
    float den = 0.0f;
    for (int r = 0; r < D; ++r) {
      const float vr = s.v[r][k];
      den = den + vr * vr;
    }
    const float norm = sqrtf(den);
    for (int r = 0; r < D; ++r) {
      s.v[r][k] = s.v[r][k] / norm;
      s.a[r][k] = mat[r * kCisDim + k];
    }
  }
  rw_fence();
  for (int k = lane; k < D; k += kRwLanes) {
    float num = 0.0f;
    for (int r = 0; r < D; ++r) {
      float row = 0.0f;
      for (int c = 0; c < D; ++c) row = row + s.a[r][c] * s.v[c][k];
      num = num + s.v[r][k] * row;
    }
    s.x[k] = num;
  }
  rw_fence();
  return ok;
}

// the rank of column k among s.x[0 .. D)
__host__ __device__ __forceinline__ int cis_rank(const CisSmem& s, int D, int k) {
  const float xi = s.x[k];
  int rk = 0;
  for (int j = 0; j < D; ++j) {
    const float xj = s.x[j];
    rk += xj < xi || (xj == xi && j < k);
  }
  return rk;
}

// One molecule.  Every branch around a fence or a reduction is lane-uniform.
__host__ __device__ inline void cis_molecule(const CisParams& Q, CisSmem& s, int b, int lane) {
#pragma clang fp contract(off)
  if (Q.status[b] != GAUDI_HUCKEL_OK) return;  // refused or not converged: no hand-over, zero rows
  float* row = Q.rows + (size_t)b * kCisRow;
  const int n = huckel_bits(row[0]), n_occ = huckel_bits(row[1]);
  if (n < 1 || n > kHuckelMaxPi || n_occ < 0 || n_occ > n) return;
  const int W = Q.window, n_virt = n - n_occ;
  const int n_o = n_occ < W ? n_occ : W, n_v = n_virt < W ? n_virt : W, D = n_o * n_v;
  int flags = 0;
  if (D < n_occ * n_virt) flags |= GAUDI_PPP_CIS_TRUNCATED;
  if ((row[2] >= 0.0f && row[2] < kPppDegenerate) || (row[3] >= 0.0f && row[3] < kPppDegenerate)) flags |= GAUDI_PPP_CIS_WINDOW_EDGE;
  if (D == 0) {
    if (lane == 0) {
      Q.n_active_occ[b] = n_o;
      Q.n_active_virt[b] = n_v;
      Q.flags[b] = Q.flags[b] | flags;
    }
    return;
  }
  for (int r = lane; r < n; r += kRwLanes) {
    for (int k = 0; k < 3; ++k) s.xyz[r][k] = row[kCisXyz + 3 * r + k];
    s.gam[r] = row[kCisGam + r];
    for (int q = 0; q < kCisAct; ++q) s.c[q][r] = row[kCisCoef + q * kHuckelMaxPi + r];
  }
  for (int q = lane; q < kCisAct; q += kRwLanes) s.eps[q] = row[kCisEps + q];
  for (int jb = lane; jb < D; jb += kRwLanes)
    for (int ia = 0; ia <= jb; ++ia) {
      s.a[ia][jb] = 0.0f;
      s.v[ia][jb] = 0.0f;
    }
  rw_fence();
  // ---- 1. the upper part of the lane's column of (ij|ab) in s.a and of (ia|jb) in s.v
  const int repulsion = Q.repulsion;
  for (int r = 0; r < n; ++r) {
    for (int t = lane; t < n; t += kRwLanes) s.g[t] = t == r ? s.gam[r] : ppp_gamma(s, r, t, repulsion);
    rw_fence();
    for (int jb = lane; jb < D; jb += kRwLanes) {
      const int j = jb / n_v, bb = jb - j * n_v;
      const float* cj = s.c[j];
      const float* cb = s.c[kCisMaxWindow + bb];
      float big_j = 0.0f, big_l[kCisMaxWindow];
      for (int a = 0; a < kCisMaxWindow; ++a) big_l[a] = 0.0f;
      for (int t = 0; t < n; ++t) {
        const float g = s.g[t], cbt = cb[t];
        big_j = big_j + g * (cj[t] * cbt);
        for (int a = 0; a < kCisMaxWindow; ++a)
          if (a < n_v) big_l[a] = big_l[a] + g * (s.c[kCisMaxWindow + a][t] * cbt);
      }
      for (int a = 0; a < kCisMaxWindow; ++a) s.l[a][jb] = big_l[a];
      const float crj = cj[r];
      int i = 0, a = 0;
      for (int ia = 0; ia <= jb; ++ia) {
        const float cri = s.c[i][r], cra = s.c[kCisMaxWindow + a][r];
        s.v[ia][jb] = s.v[ia][jb] + (cri * cra) * big_j;
        s.a[ia][jb] = s.a[ia][jb] + (cri * crj) * s.l[a][jb];
        if (++a == n_v) {
          a = 0;
          ++i;
        }
      }
    }
    rw_fence();
  }
  // ---- 2. S in s.a, T in s.v: the upper triangle, then its mirror; the transition dipole of every configuration
  for (int jb = lane; jb < D; jb += kRwLanes) {
    const int j = jb / n_v, bb = jb - j * n_v;
    for (int ia = 0; ia <= jb; ++ia) {
      const float coul = s.a[ia][jb], exch = s.v[ia][jb];
      const float t = ia == jb ? (s.eps[kCisMaxWindow + bb] - s.eps[j]) - coul : 0.0f - coul;
      s.a[ia][jb] = t + 2.0f * exch;
      s.v[ia][jb] = t;
    }
    const float* cj = s.c[j];
    const float* cb = s.c[kCisMaxWindow + bb];
    float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
    for (int r = 0; r < n; ++r) {
      const float w = cj[r] * cb[r];
      d0 = d0 + w * (s.xyz[r][0] - s.xyz[0][0]);
      d1 = d1 + w * (s.xyz[r][1] - s.xyz[0][1]);
      d2 = d2 + w * (s.xyz[r][2] - s.xyz[0][2]);
    }
    s.d[jb][0] = d0;
    s.d[jb][1] = d1;
    s.d[jb][2] = d2;
  }
  rw_fence();
  for (int c = lane; c < D; c += kRwLanes)
    for (int r = c + 1; r < D; ++r) {
      s.a[r][c] = s.a[c][r];
      s.v[r][c] = s.v[c][r];
    }
  rw_fence();
  float* mat_s = row + kCisMatS;
  float* mat_t = row + kCisMatT;
  for (int c = lane; c < D; c += kRwLanes)
    for (int r = 0; r < D; ++r) {
      mat_s[r * kCisDim + c] = s.a[r][c];
      mat_t[r * kCisDim + c] = s.v[r][c];
    }
  // ---- 3, 4. the singlets
  int sweeps = 0;
  bool ok = cis_solve(s, mat_s, D, lane, sweeps);
  const size_t at = (size_t)b * kCisDim;
  const int first = n_occ - n_o;
  for (int k = lane; k < D; k += kRwLanes) {
    const int rk = cis_rank(s, D, k);
    const float e = s.x[k];
    float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f, best = -1.0f;
    int lead = 0;
    for (int ia = 0; ia < D; ++ia) {
      const float xk = s.v[ia][k], w = xk * xk;
      m0 = m0 + xk * s.d[ia][0];
      m1 = m1 + xk * s.d[ia][1];
      m2 = m2 + xk * s.d[ia][2];
      if (w > best) {
        best = w;
        lead = ia;
      }
    }
    m0 = kCisSqrt2 * m0;
    m1 = kCisSqrt2 * m1;
    m2 = kCisSqrt2 * m2;
    const int li = lead / n_v;
    Q.singlet[at + rk] = e;
    Q.dipole[(at + rk) * 3 + 0] = m0;
    Q.dipole[(at + rk) * 3 + 1] = m1;
    Q.dipole[(at + rk) * 3 + 2] = m2;
    Q.osc[at + rk] = (kCisOsc * e) * ((m0 * m0 + m1 * m1) + m2 * m2);
    Q.lead[(at + rk) * 2 + 0] = (unsigned char)(first + li);
    Q.lead[(at + rk) * 2 + 1] = (unsigned char)(n_occ + (lead - li * n_v));
    Q.lead_weight[at + rk] = best;
  }
  rw_fence();
  // ---- 3. the triplets
  ok = cis_solve(s, mat_t, D, lane, sweeps) && ok;
  for (int k = lane; k < D; k += kRwLanes) {
    const int rk = cis_rank(s, D, k);
    Q.triplet[at + rk] = s.x[k];
    if (rk == 0) s.t1 = s.x[k];
  }
  rw_fence();
  if (lane == 0) {
    if (!(s.t1 > 0.0f)) flags |= GAUDI_PPP_CIS_TRIPLET_UNSTABLE;
    if (!ok) {
      flags |= GAUDI_PPP_CIS_JACOBI_CAP;
      Q.status[b] = GAUDI_HUCKEL_NOT_CONVERGED;
    }
    Q.n_states[b] = D;
    Q.n_active_occ[b] = n_o;
    Q.n_active_virt[b] = n_v;
    Q.cis_sweeps[b] = sweeps;
    Q.flags[b] = Q.flags[b] | flags;
  }
}

__global__ __launch_bounds__(64) void ppp_cis_kernel(const CisParams Q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ppp_cis_lds[];
  if ((int)blockIdx.x < Q.B) cis_molecule(Q, *reinterpret_cast<CisSmem*>(ppp_cis_lds), (int)blockIdx.x, (int)threadIdx.x);
}

static void cis_params(CisParams& C, const PppParams& Q, int B, void* (&outs)[kCisOuts]) {
  C.B = B;
  C.repulsion = Q.repulsion;
  C.window = Q.window;
  C.rows = Q.cis;
  C.status = Q.status;
  C.flags = Q.flags;
  C.singlet = (float*)outs[0];
  C.triplet = (float*)outs[1];
  C.osc = (float*)outs[2];
  C.dipole = (float*)outs[3];
  C.lead = (unsigned char*)outs[4];
  C.lead_weight = (float*)outs[5];
  C.n_states = (int*)outs[6];
  C.n_active_occ = (int*)outs[7];
  C.n_active_virt = (int*)outs[8];
  C.cis_sweeps = (int*)outs[9];
}

// the CIS launch of a call: one workgroup per molecule, all tiers; after the SCF launches on the same stream
static int cis_device(gaudi_handle* h, const PppParams& Q, int B, void* (&douts)[kCisOuts]) {
  CisParams C{};
  cis_params(C, Q, B, douts);
  constexpr int lds = (int)sizeof(CisSmem);
  {
    // the attribute belongs to the function: one process-wide record per device (see the sampler's launch)
    static std::mutex mu;
    static std::map<int, bool> raised;
    std::lock_guard<std::mutex> lock(mu);
    if (!raised[h->device]) {
      HIPCHECK(h, hipFuncSetAttribute((const void*)ppp_cis_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      raised[h->device] = true;
    }
  }
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (h->prof) HIPCHECK(h, h->ppp_cis_log.begin(h->stream, ev));
  hipLaunchKernelGGL(ppp_cis_kernel, dim3(B), dim3(64), lds, h->stream, C);
  HIPCHECK(h, hipGetLastError());
  if (h->prof) HIPCHECK(h, h->ppp_cis_log.end(h->stream, ev));
  return GAUDI_OK;
}

static void cis_host(const PppParams& Q, int B, void* (&outs)[kCisOuts]) {
  CisParams C{};
  cis_params(C, Q, B, outs);
  std::vector<CisSmem> W(1);
  for (int b = 0; b < B; ++b) cis_molecule(C, W[0], b, 0);
}

}  // namespace gaudi

#define GAUDI_CIS_OUT                                                                                                            \
  gaudi::CisOut {                                                                                                                \
    singlet_out, triplet_out, osc_out, dipole_out, lead_out, lead_weight_out, n_states_out, n_active_occ_out,                    \
        n_active_virt_out, cis_sweeps_out                                                                                        \
  }

extern "C" int gaudi_ppp_cis(gaudi_handle* h, GAUDI_PPP_ARGS, int window, GAUDI_PPP_CIS_ARGS) {
  const gaudi::CisOut cis = GAUDI_CIS_OUT;
  return gaudi::ppp_device(h, GAUDI_PPP_PASS, &cis, window);
}

extern "C" int gaudi_host_ppp_cis(GAUDI_PPP_ARGS, int window, GAUDI_PPP_CIS_ARGS) {
  const gaudi::CisOut cis = GAUDI_CIS_OUT;
  return gaudi::ppp_host(GAUDI_PPP_PASS, &cis, window);
}
#undef GAUDI_CIS_OUT
#undef GAUDI_PPP_CIS_ARGS
#undef GAUDI_PPP_PASS
#undef GAUDI_PPP_ARGS
#undef GAUDI_PPP_OUT

extern "C" int gaudi_ppp_cis_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms) {
  if (!h || !n_launches || !total_ms) return GAUDI_E_INVALID;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, h->ppp_cis_log.fold(0));
  *n_launches = (int32_t)h->ppp_cis_log.n;
  *total_ms = h->ppp_cis_log.ms;
  return GAUDI_OK;
}
