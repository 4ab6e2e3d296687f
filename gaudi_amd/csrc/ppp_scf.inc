// ppp_scf.inc -- the PPP SCF with Pulay's DIIS: the rows that the damped iteration leaves NOT_CONVERGED
// (included after ppp_open.inc; DESIGN.md section 8t; the model is spelled out in include/gaudi_hip.h).
//
// The kernel is ppp.inc's ppp_molecule with its third compile-time flag set: the model, the Fock formula, the Jacobi solver, the
// half-electron occupations and the fp64 state energy of gaudi_ppp_open, and between a = F(P) and the solver the four steps below.
// From iteration diis_start on (so P0 = diag(z), which commutes with every F of an all-carbon molecule, never enters):
//   ppp_diis_error     G = F P into s.v, e = G - G^T; F and e into the ring slot of the row's global scratch; max |e|;
//   ppp_diis_products  B_ij = sum e_i e_j of the new entry against every kept one, in fp64 from the fp32 elements;
//   ppp_diis_solve     the bordered system by Gaussian elimination with partial pivoting in fp64; a pivot below 2^-40 drops the
//                      oldest entry and solves again;
//   ppp_diis_combine   a = sum c_i F_i, oldest to newest.
// The scratch row is [1 + 2 * diis_size][P * P] floats: the density, the ring's Fock matrices, the ring's commutators.  Every lane
// writes and later reads only its own columns of them, as it does of the density, so global memory needs no cross-lane ordering.
// ONE text, two builds (kRwLanes 64 / 1), contraction off, every sum in one fixed order: the device equals the host build bit for
// bit.  One writer per output element, plain vector stores, no atomics; every branch around a fence or a reduction is lane-uniform.
// This file holds the four steps, the launch (split so that one launch's scratch stays within 512 MiB), the host build's driver and
// the three entry points.

namespace gaudi {

constexpr int kPppScfOuts = kPppOpenOuts + 2;
constexpr double kPppDiisPivot = 9.094947017729282e-13;  // 2^-40
constexpr size_t kPppScfScratch = (size_t)512 << 20;     // bytes of scratch one launch may hold

// G = F P into s.v (column c by the lane that owns column c of P: G_rc = sum over k ascending of a[r][k] P_kc), then e = G - G^T;
// F and e go to their ring slot.  Returns max |e|, reduced through its bits.
template <int P>
__host__ __device__ inline float ppp_diis_error(PppSmem<P>& s, const float* pm, float* f_slot, float* e_slot, int n, int lane) {
#pragma clang fp contract(off)
  constexpr int R = 8;  // rows of a column held in registers at a time (P is a multiple of it: rows n .. P - 1 are read, never kept)
  static_assert(P % R == 0, "a block of rows stays inside s.a");
  for (int c = lane; c < n; c += kRwLanes)
    for (int r0 = 0; r0 < n; r0 += R) {
      float acc[R];
#pragma unroll
      for (int i = 0; i < R; ++i) acc[i] = 0.0f;
      for (int k = 0; k < n; ++k) {
        const float p = pm[k * P + c];
#pragma unroll
        for (int i = 0; i < R; ++i) acc[i] = acc[i] + s.a[r0 + i][k] * p;
      }
#pragma unroll
      for (int i = 0; i < R; ++i)
        if (r0 + i < n) s.v[r0 + i][c] = acc[i];
    }
  rw_fence();
  float worst = 0.0f;
  for (int c = lane; c < n; c += kRwLanes)
    for (int r = 0; r < n; ++r) {
      const float e = s.v[r][c] - s.v[c][r], t = fabsf(e);
      worst = t > worst ? t : worst;
      e_slot[r * P + c] = e;
      f_slot[r * P + c] = s.a[r][c];
    }
  const float err = __builtin_bit_cast(float, -rw_min(-huckel_bits(worst)));
  rw_fence();  // (s.v is free again)
  return err;
}

// s.db[new][i] = s.db[i][new] = sum e_i e_new for every entry of the ring, the new one (the last) included: by columns over r
// ascending into s.xd, then over the columns ascending by one lane.  s.db is indexed by ring slot: kept entries keep their values.
template <int P>
__host__ __device__ inline void ppp_diis_products(PppSmem<P>& s, const float* es, int size, int head, int len, int n, int lane) {
#pragma clang fp contract(off)
  const int fresh = (head + len - 1) % size;
  const float* en = es + (size_t)fresh * (P * P);
  for (int q = 0; q < len; ++q) {
    const int slot = (head + q) % size;
    const float* ei = es + (size_t)slot * (P * P);
    for (int c = lane; c < n; c += kRwLanes) {
      double acc = 0.0;
      for (int r = 0; r < n; ++r) acc = acc + (double)ei[r * P + c] * (double)en[r * P + c];
      s.xd[c] = acc;
    }
    rw_fence();
    if (lane == 0) {
      double b = 0.0;
      for (int c = 0; c < n; ++c) b = b + s.xd[c];
      s.db[fresh][slot] = b;
      s.db[slot][fresh] = b;
    }
    rw_fence();
  }
}

// The coefficients of the ring's entries, oldest first, as floats in s.x[0 .. len - 1]; returns how many entries they combine.
// B is scaled by its largest diagonal element; the system is [[B, 1], [1^T, 0]] (c, lambda) = (0, 1).  Where a pivot is below
// 2^-40 (or B is all zero) the oldest entry is dropped for good and the rest solved again; with one entry left: 1, nothing written.
template <int P>
__host__ __device__ inline int ppp_diis_solve(PppSmem<P>& s, int size, int& head, int& len, int lane) {
#pragma clang fp contract(off)
  while (len >= 2) {
    const int N = len + 1;
    double top = 0.0;
    for (int q = 0; q < len; ++q) {
      const int slot = (head + q) % size;
      const double d = s.db[slot][slot];
      top = d > top ? d : top;
    }
    bool ok = top > 0.0;
    if (ok) {
      for (int idx = lane; idx < N * (N + 1); idx += kRwLanes) {
        const int i = idx / (N + 1), j = idx % (N + 1);
        double t = 0.0;
        if (i < len && j < len) t = s.db[(head + i) % size][(head + j) % size] / top;
        else if ((i < len && j == len) || (i == len && j < len) || (i == len && j == N)) t = 1.0;
        s.dm[i][j] = t;
      }
      rw_fence();
    }
    for (int p = 0; ok && p < N; ++p) {
      int pr = p;
      double big = fabs(s.dm[p][p]);
      for (int i = p + 1; i < N; ++i) {
        const double t = fabs(s.dm[i][p]);
        if (t > big) {
          big = t;
          pr = i;
        }
      }
      ok = big >= kPppDiisPivot;  // (every lane read the same column: lane-uniform)
      rw_fence();                 // (the search's reads before the swap)
      if (!ok) break;
      if (pr != p)
        for (int j = lane; j <= N; j += kRwLanes) {
          const double t = s.dm[p][j];
          s.dm[p][j] = s.dm[pr][j];
          s.dm[pr][j] = t;
        }
      rw_fence();
      for (int i = p + 1 + lane; i < N; i += kRwLanes) {
        const double f = s.dm[i][p] / s.dm[p][p];
        for (int j = p + 1; j <= N; ++j) s.dm[i][j] = s.dm[i][j] - f * s.dm[p][j];
      }
      rw_fence();
    }
    if (ok) {
      if (lane == 0) {
        for (int i = N - 1; i >= 0; --i) {  // the solution over the right-hand side
          double acc = s.dm[i][N];
          for (int j = i + 1; j < N; ++j) acc = acc - s.dm[i][j] * s.dm[j][N];
          s.dm[i][N] = acc / s.dm[i][i];
        }
        for (int i = 0; i < len; ++i) s.x[i] = (float)s.dm[i][N];  // rounded once
      }
      rw_fence();
      return len;
    }
    head = head + 1 == size ? 0 : head + 1;
    --len;
  }
  return 1;
}

// a = sum c_i F_i, oldest to newest: each lane its own columns.
template <int P>
__host__ __device__ inline void ppp_diis_combine(PppSmem<P>& s, const float* fs, int size, int head, int len, int n, int lane) {
#pragma clang fp contract(off)
  for (int c = lane; c < n; c += kRwLanes)
    for (int r = 0; r < n; ++r) {
      float acc = 0.0f;
      for (int q = 0; q < len; ++q) acc = acc + s.x[q] * fs[(size_t)((head + q) % size) * (P * P) + r * P + c];
      s.a[r][c] = acc;
    }
}

template <int P>
__global__ __launch_bounds__(64) void ppp_scf_kernel(const PppParams Q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ppp_scf_lds[];
  ppp_molecule<P, true, true>(Q, *reinterpret_cast<PppSmem<P>*>(ppp_scf_lds),
                              Q.scratch + (size_t)blockIdx.x * (size_t)(1 + 2 * Q.diis_size) * (P * P), Q.mol[blockIdx.x],
                              (int)threadIdx.x);
}

// the rows of one launch: as many as 512 MiB of scratch hold (at the 128 tier with the default history 630)
template <int P>
static int ppp_scf_chunk(int diis_size) {
  const size_t row = sizeof(float) * (size_t)(1 + 2 * diis_size) * (P * P);
  return (int)(kPppScfScratch / row);
}

template <int P>
static int ppp_scf_launch(gaudi_handle* h, PppParams Q, const int* mol, int count) {
  if (count == 0) return GAUDI_OK;
  constexpr int lds = (int)sizeof(PppSmem<P>);
  {
    static std::mutex mu;
    static std::map<int, bool> raised;
    std::lock_guard<std::mutex> lock(mu);
    if (!raised[h->device]) {
      HIPCHECK(h, hipFuncSetAttribute((const void*)ppp_scf_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      raised[h->device] = true;
    }
  }
  const int chunk = ppp_scf_chunk<P>(Q.diis_size);
  for (int at = 0; at < count; at += chunk) {  // the launches follow one another on the stream and share the scratch
    const int rows = count - at < chunk ? count - at : chunk;
    Q.mol = mol + at;
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    if (h->prof) HIPCHECK(h, h->ppp_scf_log.begin(h->stream, ev));
    hipLaunchKernelGGL(ppp_scf_kernel<P>, dim3(rows), dim3(64), lds, h->stream, Q);
    HIPCHECK(h, hipGetLastError());
    if (h->prof) HIPCHECK(h, h->ppp_scf_log.end(h->stream, ev));
  }
  return GAUDI_OK;
}

template <int P>
static void ppp_scf_host_tier(const PppParams& Q, const int* mol, int count) {
  if (count == 0) return;
  std::vector<PppSmem<P>> W(1);
  std::vector<float> pm((size_t)(1 + 2 * Q.diis_size) * P * P);
  for (int i = 0; i < count; ++i) ppp_molecule<P, true, true>(Q, W[0], pm.data(), mol[i], 0);
}

// the two outputs behind gaudi_ppp_open's twenty-three
static void ppp_scf_out_list(const PppOut& o, const PppOpenOut& x, float* diis_error, int32_t* n_extrapolated, int B, int A, int M,
                             void* (&p)[kPppScfOuts], size_t (&sz)[kPppScfOuts]) {
  void* p23[kPppOpenOuts];
  size_t sz23[kPppOpenOuts];
  ppp_open_out_list(o, x, B, A, M, p23, sz23);
  for (int i = 0; i < kPppOpenOuts; ++i) {
    p[i] = p23[i];
    sz[i] = sz23[i];
  }
  p[kPppOpenOuts] = diis_error;
  p[kPppOpenOuts + 1] = n_extrapolated;
  sz[kPppOpenOuts] = sz[kPppOpenOuts + 1] = 4 * (size_t)B;
}

static void ppp_scf_params(PppParams& Q, const gaudi_ppp_tables* t, int B, int A, int M, int repulsion, int diis_size, int diis_start,
                           float damping, void* (&outs)[kPppScfOuts]) {
  void* o23[kPppOpenOuts];
  for (int i = 0; i < kPppOpenOuts; ++i) o23[i] = outs[i];
  ppp_open_params(Q, t, B, A, M, repulsion, damping, o23);
  Q.diis_size = diis_size;
  Q.diis_start = diis_start;
  Q.diis_error = (float*)outs[kPppOpenOuts];
  Q.n_extrapolated = (int*)outs[kPppOpenOuts + 1];
}

// a history or a first iteration the kernel cannot run with: every row is refused
static bool ppp_scf_settings(int diis_size, int diis_start) {
  return diis_size >= 2 && diis_size <= kPppDiisMax && diis_start >= 2 && diis_start <= kPppIterations;
}

#define GAUDI_PPP_SCF_ARGS                                                                                                       \
  const gaudi_ppp_tables *tables, int B, int A, int M, const int32_t *elem, const int32_t *n_atoms, const int32_t *bonds,        \
      const int32_t *n_bonds, const float *xyz, const int32_t *charge, const int32_t *multiplicity, int repulsion,               \
      int32_t diis_size, int32_t diis_start, float damping, float *levels_out, uint8_t *occupation_out, float *pi_charge_out,    \
      float *pi_bond_order_out, int8_t *site_class_out, int32_t *n_pi_out, int32_t *n_electrons_out, int32_t *n_excluded_out,    \
      int32_t *iterations_out, int32_t *sweeps_out, int32_t *flags_out, int32_t *status_out, float *homo_out, float *lumo_out,   \
      float *gap_out, float *e_electronic_out, float *e_core_out, float *delta_p_out, float *spin_density_out,                   \
      double *e_state_out, double *he_correction_out, int32_t *n_open_out, int32_t *somo_out, float *diis_error_out,             \
      int32_t *n_extrapolated_out
#define GAUDI_PPP_SCF_PASS                                                                                                       \
  tables, B, A, M, elem, n_atoms, bonds, n_bonds, xyz, charge, multiplicity, repulsion, diis_size, diis_start, damping,          \
      levels_out, occupation_out, pi_charge_out, pi_bond_order_out, site_class_out, n_pi_out, n_electrons_out, n_excluded_out,   \
      iterations_out, sweeps_out, flags_out, status_out, homo_out, lumo_out, gap_out, e_electronic_out, e_core_out, delta_p_out, \
      spin_density_out, e_state_out, he_correction_out, n_open_out, somo_out, diis_error_out, n_extrapolated_out
#define GAUDI_PPP_SCF_OUT GAUDI_PPP_OUT, gaudi::PppOpenOut{spin_density_out, e_state_out, he_correction_out, n_open_out, somo_out}, \
                          diis_error_out, n_extrapolated_out

static int ppp_scf_device(gaudi_handle* h, GAUDI_PPP_SCF_ARGS) {
  if (!h) return GAUDI_E_INVALID;
  void* outs[kPppScfOuts];
  size_t osz[kPppScfOuts];
  ppp_scf_out_list(GAUDI_PPP_SCF_OUT, B > 0 ? B : 0, A, M, outs, osz);
  for (void* p : outs)
    if (!p) return fail(h, GAUDI_E_INVALID, "every output array is required");
  if (!tables || !xyz) return fail(h, GAUDI_E_INVALID, "invalid argument");
  const char* why = "";
  std::vector<int> mol;
  int tier_n[3];
  if (int rc = huckel_route(tables->n_elems, tables->h_elem, tables->c_elem, B, A, M, elem, n_atoms, bonds, n_bonds, mol,
                            tier_n, &why))
    return fail(h, rc, why);
  if (B == 0) return GAUDI_OK;
  std::vector<PppTab> tab(1);
  const bool table_ok = ppp_table(tables, repulsion, damping, tab[0]);
  if (!table_ok || !ppp_scf_settings(diis_size, diis_start)) {  // nothing runs: every row zero
    for (int i = 0; i < kPppScfOuts; ++i) memset(outs[i], 0, osz[i]);
    for (int b = 0; b < B; ++b) status_out[b] = table_ok ? GAUDI_HUCKEL_BAD_INPUT : GAUDI_HUCKEL_BAD_TABLE;
    return GAUDI_OK;
  }
  HIPCHECK(h, hipSetDevice(h->device));
  const size_t nB = (size_t)B;
  std::vector<int32_t> zero;
  if (!charge || !multiplicity) zero.assign(nB, 0);
  constexpr int kIn = 9;
  const size_t isz[kIn] = {sizeof(int) * nB * A, sizeof(int) * nB, sizeof(int) * nB * M * 2, sizeof(int) * nB, sizeof(int) * nB,
                           sizeof(int) * nB,     sizeof(PppTab),   sizeof(float) * nB * A * 3, sizeof(int) * nB};
  const void* ins[kIn] = {elem,       n_atoms, bonds, n_bonds, charge ? charge : zero.data(), mol.data(),
                          tab.data(), xyz,     multiplicity ? multiplicity : zero.data()};
  DevBuf* buf = h->d_ppp_scf;
  for (int i = 0; i < kIn; ++i) {
    HIPCHECK(h, buf[i].reserve(isz[i]));
    HIPCHECK(h, hipMemcpyAsync(buf[i].p, ins[i], isz[i], hipMemcpyHostToDevice, h->stream));
  }
  void* douts[kPppScfOuts];
  for (int i = 0; i < kPppScfOuts; ++i) {  // a refused row writes its status only: zero everywhere else
    HIPCHECK(h, buf[kIn + i].reserve(osz[i]));
    HIPCHECK(h, hipMemsetAsync(buf[kIn + i].p, 0, osz[i], h->stream));
    douts[i] = buf[kIn + i].p;
  }
  // the scratch rows: the launches follow one another on the stream, so they share the largest launch's
  const size_t per = (size_t)(1 + 2 * diis_size);
  const size_t launch_rows[3] = {(size_t)std::min(tier_n[0], ppp_scf_chunk<32>(diis_size)), (size_t)std::min(tier_n[1], ppp_scf_chunk<64>(diis_size)),
                                 (size_t)std::min(tier_n[2], ppp_scf_chunk<128>(diis_size))};
  const int cap[3] = {32, 64, 128};
  size_t floats = 0;
  for (int k = 0; k < 3; ++k) floats = std::max(floats, launch_rows[k] * per * cap[k] * cap[k]);
  DevBuf& scratch = buf[kIn + kPppScfOuts];
  HIPCHECK(h, scratch.reserve(sizeof(float) * floats));
  PppParams Q{};
  ppp_scf_params(Q, tables, B, A, M, repulsion, diis_size, diis_start, damping, douts);
  Q.in.elem = buf[0].as<int>();
  Q.in.n_atoms = buf[1].as<int>();
  Q.in.bonds = buf[2].as<int>();
  Q.in.n_bonds = buf[3].as<int>();
  Q.charge = buf[4].as<int>();
  Q.tab = buf[6].as<PppTab>();
  Q.xyz = buf[7].as<float>();
  Q.multiplicity = buf[8].as<int>();
  Q.scratch = scratch.as<float>();
  const int* dmol = buf[5].as<int>();
  if (int rc = ppp_scf_launch<32>(h, Q, dmol, tier_n[0])) return rc;
  if (int rc = ppp_scf_launch<64>(h, Q, dmol + tier_n[0], tier_n[1])) return rc;
  if (int rc = ppp_scf_launch<128>(h, Q, dmol + tier_n[0] + tier_n[1], tier_n[2])) return rc;
  for (int i = 0; i < kPppScfOuts; ++i)
    HIPCHECK(h, hipMemcpyAsync(outs[i], douts[i], osz[i], hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  return GAUDI_OK;
}

static int ppp_scf_host(GAUDI_PPP_SCF_ARGS) {
  void* outs[kPppScfOuts];
  size_t osz[kPppScfOuts];
  ppp_scf_out_list(GAUDI_PPP_SCF_OUT, B > 0 ? B : 0, A, M, outs, osz);
  for (void* p : outs)
    if (!p) return GAUDI_E_INVALID;
  if (!tables || !xyz) return GAUDI_E_INVALID;
  const char* why = "";
  std::vector<int> mol;
  int tier_n[3];
  if (int rc = huckel_route(tables->n_elems, tables->h_elem, tables->c_elem, B, A, M, elem, n_atoms, bonds, n_bonds, mol,
                            tier_n, &why))
    return rc;
  if (B == 0) return GAUDI_OK;
  for (int i = 0; i < kPppScfOuts; ++i) memset(outs[i], 0, osz[i]);
  std::vector<PppTab> tab(1);
  const bool table_ok = ppp_table(tables, repulsion, damping, tab[0]);
  if (!table_ok || !ppp_scf_settings(diis_size, diis_start)) {
    for (int b = 0; b < B; ++b) status_out[b] = table_ok ? GAUDI_HUCKEL_BAD_INPUT : GAUDI_HUCKEL_BAD_TABLE;
    return GAUDI_OK;
  }
  std::vector<int32_t> zero;
  if (!charge || !multiplicity) zero.assign((size_t)B, 0);
  PppParams Q{};
  ppp_scf_params(Q, tables, B, A, M, repulsion, diis_size, diis_start, damping, outs);
  Q.in.elem = elem;
  Q.in.n_atoms = n_atoms;
  Q.in.bonds = bonds;
  Q.in.n_bonds = n_bonds;
  Q.charge = charge ? charge : zero.data();
  Q.multiplicity = multiplicity ? multiplicity : zero.data();
  Q.xyz = xyz;
  Q.tab = tab.data();
  ppp_scf_host_tier<32>(Q, mol.data(), tier_n[0]);
  ppp_scf_host_tier<64>(Q, mol.data() + tier_n[0], tier_n[1]);
  ppp_scf_host_tier<128>(Q, mol.data() + tier_n[0] + tier_n[1], tier_n[2]);
  return GAUDI_OK;
}

}  // namespace gaudi

extern "C" int gaudi_ppp_scf(gaudi_handle* h, GAUDI_PPP_SCF_ARGS) { return gaudi::ppp_scf_device(h, GAUDI_PPP_SCF_PASS); }

extern "C" int gaudi_host_ppp_scf(GAUDI_PPP_SCF_ARGS) { return gaudi::ppp_scf_host(GAUDI_PPP_SCF_PASS); }
#undef GAUDI_PPP_SCF_ARGS
#undef GAUDI_PPP_SCF_PASS
#undef GAUDI_PPP_SCF_OUT

extern "C" int gaudi_ppp_scf_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms) {
  if (!h || !n_launches || !total_ms) return GAUDI_E_INVALID;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, h->ppp_scf_log.fold(0));
  *n_launches = (int32_t)h->ppp_scf_log.n;
  *total_ms = h->ppp_scf_log.ms;
  return GAUDI_OK;
}
