// ppp_open.inc -- PPP for open shells by Dewar's half-electron method: radical ions, delta-SCF IP / EA and triplets
// (included after ppp.inc; DESIGN.md section 8s; the model is spelled out in include/gaudi_hip.h).
//
// The kernel is ppp.inc's ppp_molecule with its compile-time flag set: one restricted SCF with occupations 2 / 1 / 0, the same Fock
// formula, the same Jacobi solver, one solution per state, and a closed-form energy correction accumulated in fp64.  A row is
// (molecule, charge, multiplicity).  Tiers, routing, the scratch row and the rules (one writer per output element, plain vector
// stores, no atomics, lane-uniform branches around fences and reductions) are gaudi_ppp's.  This file holds the launch, the host
// build's driver and the three entry points.

namespace gaudi {

constexpr int kPppOpenOuts = kPppOuts + 5;

template <int P>
__global__ __launch_bounds__(64) void ppp_open_kernel(const PppParams Q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ppp_open_lds[];
  ppp_molecule<P, true>(Q, *reinterpret_cast<PppSmem<P>*>(ppp_open_lds), Q.scratch + (size_t)blockIdx.x * (P * P), Q.mol[blockIdx.x],
                        (int)threadIdx.x);
}

template <int P>
static int ppp_open_launch(gaudi_handle* h, PppParams Q, const int* mol, int count) {
  if (count == 0) return GAUDI_OK;
  Q.mol = mol;
  constexpr int lds = (int)sizeof(PppSmem<P>);
  {
    static std::mutex mu;
    static std::map<int, bool> raised;
    std::lock_guard<std::mutex> lock(mu);
    if (!raised[h->device]) {
      HIPCHECK(h, hipFuncSetAttribute((const void*)ppp_open_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      raised[h->device] = true;
    }
  }
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (h->prof) HIPCHECK(h, h->ppp_open_log.begin(h->stream, ev));
  hipLaunchKernelGGL(ppp_open_kernel<P>, dim3(count), dim3(64), lds, h->stream, Q);
  HIPCHECK(h, hipGetLastError());
  if (h->prof) HIPCHECK(h, h->ppp_open_log.end(h->stream, ev));
  return GAUDI_OK;
}

template <int P>
static void ppp_open_host_tier(const PppParams& Q, const int* mol, int count) {
  if (count == 0) return;
  std::vector<PppSmem<P>> W(1);
  std::vector<float> pm((size_t)P * P);
  for (int i = 0; i < count; ++i) ppp_molecule<P, true>(Q, W[0], pm.data(), mol[i], 0);
}

// the five outputs behind gaudi_ppp's eighteen
struct PppOpenOut {
  float* spin_density;
  double *e_state, *he_correction;
  int32_t *n_open, *somo;
};

static void ppp_open_out_list(const PppOut& o, const PppOpenOut& x, int B, int A, int M, void* (&p)[kPppOpenOuts],
                              size_t (&sz)[kPppOpenOuts]) {
  void* p18[kPppOuts];
  size_t sz18[kPppOuts];
  ppp_out_list(o, B, A, M, p18, sz18);
  for (int i = 0; i < kPppOuts; ++i) {
    p[i] = p18[i];
    sz[i] = sz18[i];
  }
  const size_t nB = (size_t)B;
  void* ptrs[5] = {x.spin_density, x.e_state, x.he_correction, x.n_open, x.somo};
  const size_t sizes[5] = {4 * nB * A, 8 * nB, 8 * nB, 4 * nB, 8 * nB};
  for (int i = 0; i < 5; ++i) {
    p[kPppOuts + i] = ptrs[i];
    sz[kPppOuts + i] = sizes[i];
  }
}

static void ppp_open_params(PppParams& Q, const gaudi_ppp_tables* t, int B, int A, int M, int repulsion, float damping,
                            void* (&outs)[kPppOpenOuts]) {
  void* o18[kPppOuts];
  for (int i = 0; i < kPppOuts; ++i) o18[i] = outs[i];
  ppp_params(Q, t, B, A, M, repulsion, damping, o18);
  Q.spin_density = (float*)outs[kPppOuts];
  Q.e_state = (double*)outs[kPppOuts + 1];
  Q.he_correction = (double*)outs[kPppOuts + 2];
  Q.n_open = (int*)outs[kPppOuts + 3];
  Q.somo = (int*)outs[kPppOuts + 4];
}

#define GAUDI_PPP_OPEN_ARGS                                                                                                      \
  const gaudi_ppp_tables *tables, int B, int A, int M, const int32_t *elem, const int32_t *n_atoms, const int32_t *bonds,        \
      const int32_t *n_bonds, const float *xyz, const int32_t *charge, const int32_t *multiplicity, int repulsion,               \
      float damping, float *levels_out, uint8_t *occupation_out, float *pi_charge_out, float *pi_bond_order_out,                 \
      int8_t *site_class_out, int32_t *n_pi_out, int32_t *n_electrons_out, int32_t *n_excluded_out, int32_t *iterations_out,     \
      int32_t *sweeps_out, int32_t *flags_out, int32_t *status_out, float *homo_out, float *lumo_out, float *gap_out,            \
      float *e_electronic_out, float *e_core_out, float *delta_p_out, float *spin_density_out, double *e_state_out,              \
      double *he_correction_out, int32_t *n_open_out, int32_t *somo_out
#define GAUDI_PPP_OPEN_PASS                                                                                                      \
  tables, B, A, M, elem, n_atoms, bonds, n_bonds, xyz, charge, multiplicity, repulsion, damping, levels_out, occupation_out,     \
      pi_charge_out, pi_bond_order_out, site_class_out, n_pi_out, n_electrons_out, n_excluded_out, iterations_out, sweeps_out,   \
      flags_out, status_out, homo_out, lumo_out, gap_out, e_electronic_out, e_core_out, delta_p_out, spin_density_out,           \
      e_state_out, he_correction_out, n_open_out, somo_out
#define GAUDI_PPP_OPEN_OUT \
  gaudi::PppOpenOut { spin_density_out, e_state_out, he_correction_out, n_open_out, somo_out }

static int ppp_open_device(gaudi_handle* h, GAUDI_PPP_OPEN_ARGS) {
  if (!h) return GAUDI_E_INVALID;
  void* outs[kPppOpenOuts];
  size_t osz[kPppOpenOuts];
  ppp_open_out_list(GAUDI_PPP_OUT, GAUDI_PPP_OPEN_OUT, B > 0 ? B : 0, A, M, outs, osz);
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
  if (!ppp_table(tables, repulsion, damping, tab[0])) {  // nothing runs on a table that cannot be read: every row zero
    for (int i = 0; i < kPppOpenOuts; ++i) memset(outs[i], 0, osz[i]);
    for (int b = 0; b < B; ++b) status_out[b] = GAUDI_HUCKEL_BAD_TABLE;
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
  DevBuf* buf = h->d_ppp_open;
  for (int i = 0; i < kIn; ++i) {
    HIPCHECK(h, buf[i].reserve(isz[i]));
    HIPCHECK(h, hipMemcpyAsync(buf[i].p, ins[i], isz[i], hipMemcpyHostToDevice, h->stream));
  }
  void* douts[kPppOpenOuts];
  for (int i = 0; i < kPppOpenOuts; ++i) {  // a refused row writes its status only: zero everywhere else
    HIPCHECK(h, buf[kIn + i].reserve(osz[i]));
    HIPCHECK(h, hipMemsetAsync(buf[kIn + i].p, 0, osz[i], h->stream));
    douts[i] = buf[kIn + i].p;
  }
  size_t rows = 0;  // the density rows: the launches follow one another on the stream, so they share the largest tier's
  const int cap[3] = {32, 64, 128};
  for (int k = 0; k < 3; ++k) rows = std::max(rows, (size_t)tier_n[k] * cap[k] * cap[k]);
  DevBuf& scratch = buf[kIn + kPppOpenOuts];
  HIPCHECK(h, scratch.reserve(sizeof(float) * rows));
  PppParams Q{};
  ppp_open_params(Q, tables, B, A, M, repulsion, damping, douts);
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
  if (int rc = ppp_open_launch<32>(h, Q, dmol, tier_n[0])) return rc;
  if (int rc = ppp_open_launch<64>(h, Q, dmol + tier_n[0], tier_n[1])) return rc;
  if (int rc = ppp_open_launch<128>(h, Q, dmol + tier_n[0] + tier_n[1], tier_n[2])) return rc;
  for (int i = 0; i < kPppOpenOuts; ++i)
    HIPCHECK(h, hipMemcpyAsync(outs[i], douts[i], osz[i], hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  return GAUDI_OK;
}

static int ppp_open_host(GAUDI_PPP_OPEN_ARGS) {
  void* outs[kPppOpenOuts];
  size_t osz[kPppOpenOuts];
  ppp_open_out_list(GAUDI_PPP_OUT, GAUDI_PPP_OPEN_OUT, B > 0 ? B : 0, A, M, outs, osz);
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
  for (int i = 0; i < kPppOpenOuts; ++i) memset(outs[i], 0, osz[i]);
  std::vector<PppTab> tab(1);
  if (!ppp_table(tables, repulsion, damping, tab[0])) {
    for (int b = 0; b < B; ++b) status_out[b] = GAUDI_HUCKEL_BAD_TABLE;
    return GAUDI_OK;
  }
  std::vector<int32_t> zero;
  if (!charge || !multiplicity) zero.assign((size_t)B, 0);
  PppParams Q{};
  ppp_open_params(Q, tables, B, A, M, repulsion, damping, outs);
  Q.in.elem = elem;
  Q.in.n_atoms = n_atoms;
  Q.in.bonds = bonds;
  Q.in.n_bonds = n_bonds;
  Q.charge = charge ? charge : zero.data();
  Q.multiplicity = multiplicity ? multiplicity : zero.data();
  Q.xyz = xyz;
  Q.tab = tab.data();
  ppp_open_host_tier<32>(Q, mol.data(), tier_n[0]);
  ppp_open_host_tier<64>(Q, mol.data() + tier_n[0], tier_n[1]);
  ppp_open_host_tier<128>(Q, mol.data() + tier_n[0] + tier_n[1], tier_n[2]);
  return GAUDI_OK;
}

}  // namespace gaudi

extern "C" int gaudi_ppp_open(gaudi_handle* h, GAUDI_PPP_OPEN_ARGS) { return gaudi::ppp_open_device(h, GAUDI_PPP_OPEN_PASS); }

extern "C" int gaudi_host_ppp_open(GAUDI_PPP_OPEN_ARGS) { return gaudi::ppp_open_host(GAUDI_PPP_OPEN_PASS); }
#undef GAUDI_PPP_OPEN_ARGS
#undef GAUDI_PPP_OPEN_PASS
#undef GAUDI_PPP_OPEN_OUT

extern "C" int gaudi_ppp_open_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms) {
  if (!h || !n_launches || !total_ms) return GAUDI_E_INVALID;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, h->ppp_open_log.fold(0));
  *n_launches = (int32_t)h->ppp_open_log.n;
  *total_ms = h->ppp_open_log.ms;
  return GAUDI_OK;
}
