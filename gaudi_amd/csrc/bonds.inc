// bonds.inc -- bond orders and formal charges of a graph of atoms on the device (included after rings.inc at the end of gaudi_hip.hip).
//
// The step between gor2goa and RDKit's sanitiser in the reference (data/gor2goa.py:298-324 -> data/xyz2mol.py:538-634, AC2BO): from
// elements and connectivity alone, give every atom a valence and a formal charge and place the double bonds.  The reference's
// answer depends on the atom numbering (networkx.max_weight_matching returns whichever maximum matching it finds), so this is not
// a restatement of its steps but of the question it answers, as a rule of its own (DESIGN.md section 8h):
//
//   sigma degree d = number of bonds, one more for a carbon with exactly two (the H build_molecule_aromatic adds);
//   options of an atom = the (added bonds a <= 1, formal charge q) pairs of its (element, d) in the valence table (at most two;
//     of two, the first is neutral and the second charged);
//   valid = connected, every atom has an option, and one option per atom can be chosen such that the charges sum to zero and the
//     atoms with a = 1 have a perfect matching among themselves (the double bonds);
//   returned = such a choice with the fewest charged atoms, the first in a fixed order of the molecule's own arrays.
//
// ONE text, two builds, as rings.inc: assign_bond_orders is __host__ __device__, the `lanes` of a phase are the 64 lanes of a wave on
// the device and one lane on the host (kRwLanes and the rw_* helpers of rings.inc).  Per wave 13.9 KB of LDS, two waves per workgroup:
//   1. lanes = atoms / bonds: elements and bond indices checked, the bond list staged in LDS; lane a collects atom a's neighbours
//      (at most 4 are kept: more has no option anyway), its sigma degree and its row of the table;
//   2. lanes = atoms: components by min-label propagation; the atoms with two options compacted in ascending index (prefix scan);
//   3. lane 0: a maximum matching of the atoms whose first option adds a bond -- greedy, then Edmonds' augmenting search with
//      blossom contraction (general graphs: a five-ring with its heteroatom selected is an odd cycle), every search confined to
//      the vertices it touched;
//   4. lane 0: if that is not a neutral perfect matching, subsets of the two-option atoms switched to their charged option, by
//      increasing size and in lexicographic order, pruned by the charge balance still reachable, by parity and by the deficiency of
//      the first matching (one switched atom changes it by one); a surviving subset is tried by augmenting from the first
//      matching, and the first exposed atom without an augmenting path refutes it.  A size that would look at more than 16 384
//      subsets ends the search with GAVE_UP: undecided, and the one status that can depend on the atom numbering (another
//      numbering may reach a structure before the budget is spent).  With at most 25 two-option atoms sizes 1..4 always fit;
//   5. lanes = atoms / bonds: charges and orders out.
// Integer arithmetic only; nothing depends on the molecule's place in the batch.

namespace gaudi {

constexpr int kBondWaves = 2;
constexpr int kBondMaxAtoms = GAUDI_BONDS_MAX_ATOMS;
constexpr int kBondMaxHeavy = GAUDI_BONDS_MAX_HEAVY;
constexpr int kBondMaxBonds = GAUDI_BONDS_MAX_BONDS;
constexpr int kBondMaxElems = 8;
constexpr int kBondDegrees = 5;           // sigma degrees 0..4 have a row in the table
constexpr int kBondNbr = 4;               // neighbours kept per atom
constexpr int kBondCap = GAUDI_BONDS_MAX_CHARGED;
constexpr int kBondSearch = GAUDI_BONDS_SEARCH_CHARGED;  // beyond the cap the search only asks whether a structure exists
constexpr int kBondBudget = 1 << 14;      // subsets looked at per molecule and subset size, pruned ones included
constexpr unsigned short kBondNone = 0xffff;
static_assert(kBondMaxAtoms == kRingMaxAtoms && kBondMaxHeavy == kRingMaxHeavy && kBondMaxAtoms < kBondNone, "capacities");
static_assert(kBondCap <= kBondSearch && kBondSearch <= 8, "the subset stack holds 8 entries");

struct BondTables {
  int n_elems, h_elem, c_elem;
  signed char n_opt[kBondMaxElems * kBondDegrees];
  signed char add[kBondMaxElems * kBondDegrees][2], chg[kBondMaxElems * kBondDegrees][2];
};

struct BondSmem {
  unsigned short nbr[kBondMaxAtoms][kBondNbr];
  unsigned short bl[kBondMaxBonds][2];
  unsigned short mate[kBondMaxAtoms], mate0[kBondMaxAtoms];  // the working matching; the first one
  unsigned short par[kBondMaxAtoms], base[kBondMaxAtoms], queue[kBondMaxAtoms], touch[kBondMaxAtoms];
  unsigned short label[kBondMaxAtoms + 1];                     // components; then the positive charge still to come at flex[i ...]
  unsigned short flex[kBondMaxAtoms], negsuf[kBondMaxAtoms + 1];
  unsigned char row[kBondMaxAtoms];                          // element * 5 + sigma degree: the atom's row of the table
  unsigned char sel[kBondMaxAtoms], pick[kBondMaxAtoms];     // takes a double bond; the option chosen
  unsigned char used[kBondMaxAtoms], blos[kBondMaxAtoms], seen[kBondMaxAtoms];
  int result[2];
  short c[8], sum[8];                                        // the subset being built: indices into flex, running charge
};

struct BondParams {
  int B, A, M;
  const int* elem;
  const int* n_atoms;
  const int* bonds;
  const int* n_bonds;
  unsigned char* order;
  signed char* charge;
  int* n_charged;
  int* status;
};

// ---- Edmonds' matching on the selected atoms (s.sel), run by ONE lane.  Between searches par = none, base = identity and
// used = blos = seen = 0 hold for every atom; a search restores that for the atoms it touched.
__host__ __device__ inline int bond_lca(BondSmem& s, int a, int b) {
  for (int x = a;;) {
    x = s.base[x];
    s.seen[x] = 1;
    if (s.mate[x] == kBondNone) break;  // the root
    x = s.par[s.mate[x]];
  }
  int r = b;
  for (;;) {
    r = s.base[r];
    if (s.seen[r]) break;
    r = s.par[s.mate[r]];
  }
  for (int x = a;;) {
    x = s.base[x];
    s.seen[x] = 0;
    if (s.mate[x] == kBondNone) break;
    x = s.par[s.mate[x]];
  }
  return r;
}

__host__ __device__ inline void bond_mark_path(BondSmem& s, int v, int b, int child) {
  while (s.base[v] != b) {
    s.blos[s.base[v]] = 1;
    s.blos[s.base[s.mate[v]]] = 1;
    s.par[v] = (unsigned short)child;
    child = s.mate[v];
    v = s.par[s.mate[v]];
  }
}

// An augmenting path from the exposed atom `root`: true, and the matching is augmented.  false: none exists, and some maximum
// matching leaves `root` exposed.
__host__ __device__ inline bool bond_augment(BondSmem& s, int root) {
  int qh = 0, qt = 0, nt = 0, found = -1;
  s.queue[qt++] = (unsigned short)root;
  s.touch[nt++] = (unsigned short)root;
  s.used[root] = 1;
  while (qh < qt && found < 0) {
    const int v = s.queue[qh++];
    for (int k = 0; k < kBondNbr && found < 0; ++k) {
      const int to = s.nbr[v][k];
      if (to == kBondNone) break;
      if (!s.sel[to] || s.base[v] == s.base[to] || s.mate[v] == to) continue;
      if (to == root || (s.mate[to] != kBondNone && s.par[s.mate[to]] != kBondNone)) {  // an outer atom: an odd cycle, contracted
        const int cb = bond_lca(s, v, to);
        for (int i = 0; i < nt; ++i) s.blos[s.touch[i]] = 0;
        bond_mark_path(s, v, cb, to);
        bond_mark_path(s, to, cb, v);
        for (int i = 0; i < nt; ++i) {
          const int u = s.touch[i];
          if (!s.blos[s.base[u]]) continue;
          s.base[u] = (unsigned short)cb;
          if (!s.used[u]) {
            s.used[u] = 1;
            s.queue[qt++] = (unsigned short)u;
          }
        }
      } else if (s.par[to] == kBondNone) {
        s.par[to] = (unsigned short)v;
        s.touch[nt++] = (unsigned short)to;
        if (s.mate[to] == kBondNone) {
          found = to;
        } else {
          const int w = s.mate[to];
          s.used[w] = 1;
          s.queue[qt++] = (unsigned short)w;
          s.touch[nt++] = (unsigned short)w;
        }
      }
    }
  }
  for (int v = found; v >= 0;) {
    const int pv = s.par[v], ppv = s.mate[pv];
    s.mate[v] = (unsigned short)pv;
    s.mate[pv] = (unsigned short)v;
    v = ppv == kBondNone ? -1 : ppv;
  }
  for (int i = 0; i < nt; ++i) {
    const int u = s.touch[i];
    s.par[u] = kBondNone;
    s.base[u] = (unsigned short)u;
    s.used[u] = 0;
    s.blos[u] = 0;
  }
  return found >= 0;
}

// Steps 3 and 4 for one molecule, by one lane: -> status, and the number of charged atoms of the structure in s.pick / s.sel / s.mate.
__host__ __device__ inline int bond_search(const BondTables& T, BondSmem& s, int n, int F, int forced, int q0, int& n_charged) {
  // ---- 3. the first matching: greedy in ascending atom index, then augmenting searches
  int n_sel = 0, deficiency = 0;
  for (int a = 0; a < n; ++a) {
    if (!s.sel[a]) continue;
    ++n_sel;
    if (s.mate[a] != kBondNone) continue;
    for (int k = 0; k < kBondNbr; ++k) {
      const int to = s.nbr[a][k];
      if (to == kBondNone) break;
      if (s.sel[to] && s.mate[to] == kBondNone) {
        s.mate[a] = (unsigned short)to;
        s.mate[to] = (unsigned short)a;
        break;
      }
    }
  }
  for (int a = 0; a < n; ++a)
    if (s.sel[a] && s.mate[a] == kBondNone && !bond_augment(s, a)) ++deficiency;
  n_charged = forced;
  if (q0 == 0 && deficiency == 0) return forced <= kBondCap ? GAUDI_BONDS_OK : GAUDI_BONDS_CAPPED;
  for (int a = 0; a < n; ++a) s.mate0[a] = s.mate[a];

  // ---- 4. subsets of the two-option atoms on their charged option.  label[i] / negsuf[i]: the positive / negative charge the
  // atoms flex[i ...] could still bring
  int qmax = 0;
  s.label[F] = 0;
  s.negsuf[F] = 0;
  for (int i = F - 1; i >= 0; --i) {
    const int q = T.chg[s.row[s.flex[i]]][1];
    s.label[i] = (unsigned short)(s.label[i + 1] + (q > 0 ? q : 0));
    s.negsuf[i] = (unsigned short)(s.negsuf[i + 1] + (q < 0 ? -q : 0));
    qmax = q > qmax ? q : -q > qmax ? -q : qmax;
  }
  for (int t = 1; t <= F && forced + t <= kBondSearch; ++t) {
    if (t < deficiency) continue;  // every switched atom changes the deficiency by exactly one
    int budget = kBondBudget;      // per size: sizes 1..4 of F <= 25 atoms are at most 15 275 subsets and always fit
    short* c = s.c;
    short* sum = s.sum;
    int d = 0;
    c[0] = 0;
    sum[0] = (short)q0;
    while (d >= 0) {
      if (c[d] > F - (t - d)) {
        if (--d >= 0) ++c[d];
        continue;
      }
      if (--budget < 0) {
        n_charged = 0;
        return GAUDI_BONDS_GAVE_UP;
      }
      const int now = sum[d] + T.chg[s.row[s.flex[c[d]]]][1], left = t - d - 1;
      const int need = -now;  // what the `left` atoms after c[d] must bring
      if (need > (int)s.label[c[d] + 1] || -need > (int)s.negsuf[c[d] + 1] || (need < 0 ? -need : need) > left * qmax) {
        ++c[d];
        continue;
      }
      if (left > 0) {
        sum[d + 1] = (short)now;
        c[d + 1] = (short)(c[d] + 1);
        ++d;
        continue;
      }
      // a balanced subset: switch, check the parity, match
      int cnt = n_sel;
      for (int i = 0; i < t; ++i) {
        const int a = s.flex[c[i]];
        cnt += T.add[s.row[a]][1] - T.add[s.row[a]][0];
        s.sel[a] = (unsigned char)T.add[s.row[a]][1];
      }
      bool ok = (cnt & 1) == 0;
      if (ok) {
        for (int a = 0; a < n; ++a) {
          const int m = s.mate0[a];
          s.mate[a] = (unsigned short)(s.sel[a] && m != kBondNone && s.sel[m] ? m : kBondNone);
        }
        for (int a = 0; a < n && ok; ++a)
          if (s.sel[a] && s.mate[a] == kBondNone) ok = bond_augment(s, a);
      }
      if (ok) {
        if (forced + t > kBondCap) {
          n_charged = 0;
          return GAUDI_BONDS_CAPPED;
        }
        for (int i = 0; i < t; ++i) s.pick[s.flex[c[i]]] = 1;
        n_charged = forced + t;
        return GAUDI_BONDS_OK;
      }
      for (int i = 0; i < t; ++i) s.sel[s.flex[c[i]]] = (unsigned char)T.add[s.row[s.flex[c[i]]]][0];
      ++c[d];
    }
  }
  n_charged = 0;
  return GAUDI_BONDS_NO_STRUCTURE;
}

// One molecule.  `s` is this wave's (host: this call's) working state; every `break` is lane-uniform.
__host__ __device__ inline void assign_bond_orders(const BondParams& P, const BondTables& T, BondSmem& s, int b, int lane) {
  const int A = P.A, M = P.M;
  const int n = P.n_atoms[b], m = P.n_bonds[b];
  const int* eb = P.elem + (size_t)b * A;
  const int* bb = P.bonds + (size_t)b * M * 2;
  int status = GAUDI_BONDS_OK, n_charged = 0;

  do {
    if (n <= 0) { status = GAUDI_BONDS_EMPTY; break; }
    if (n > A || m < 0 || m > M) { status = GAUDI_BONDS_BAD_INPUT; break; }  // (the entry points refuse these)
    if (n > kBondMaxAtoms || m > kBondMaxBonds) { status = GAUDI_BONDS_OVERFLOW; break; }
    // ---- 1. inputs checked; the bond list staged
    bool bad = false;
    int heavy = 0;
    for (int a = lane; a < n; a += kRwLanes) {
      const int e = eb[a];
      bad = bad || e < 0 || e >= T.n_elems;
      heavy += e != T.h_elem;
    }
    for (int k = lane; k < m; k += kRwLanes) {
      const int i = bb[2 * k], j = bb[2 * k + 1];
      const bool in = i >= 0 && i < n && j >= 0 && j < n && i != j;
      bad = bad || !in;
      s.bl[k][0] = (unsigned short)(in ? i : 0);
      s.bl[k][1] = (unsigned short)(in ? j : 0);
    }
    int H;
    (void)rw_scan(heavy, lane, H);
    rw_fence();
    if (rw_any(bad)) { status = GAUDI_BONDS_BAD_INPUT; break; }
    if (H > kBondMaxHeavy) { status = GAUDI_BONDS_OVERFLOW; break; }
    bool no_option = false;
    for (int a = lane; a < n; a += kRwLanes) {
      int d = 0;
      unsigned short nb[kBondNbr] = {kBondNone, kBondNone, kBondNone, kBondNone};
      for (int k = 0; k < m; ++k) {
        const int i = s.bl[k][0], j = s.bl[k][1];
        if (i != a && j != a) continue;
        const unsigned short o = (unsigned short)(i == a ? j : i);
        for (int q = 0; q < kBondNbr; ++q) bad = bad || nb[q] == o;  // the same bond twice
        for (int q = 0; q < kBondNbr; ++q)
          if (q == d) nb[q] = o;
        ++d;
      }
      for (int q = 0; q < kBondNbr; ++q) s.nbr[a][q] = nb[q];
      const int e = eb[a];
      const int sd = d + (e == T.c_elem && d == 2);
      const int r = e * kBondDegrees + (sd < kBondDegrees ? sd : 0);
      const bool has = sd < kBondDegrees && T.n_opt[r] > 0;
      no_option = no_option || !has;
      s.row[a] = (unsigned char)r;
      s.sel[a] = (unsigned char)(has ? T.add[r][0] : 0);
      s.pick[a] = 0;
      s.mate[a] = kBondNone;
      s.par[a] = kBondNone;
      s.base[a] = (unsigned short)a;
      s.used[a] = 0;
      s.blos[a] = 0;
      s.seen[a] = 0;
      s.label[a] = (unsigned short)a;
    }
    rw_fence();
    if (rw_any(bad)) { status = GAUDI_BONDS_BAD_INPUT; break; }
    if (rw_any(no_option)) { status = GAUDI_BONDS_BAD_VALENCE; break; }

    // ---- 2. one component (labels only fall, so racing reads are harmless)
    while (true) {
      bool changed = false;
      for (int a = lane; a < n; a += kRwLanes) {
        unsigned short lo = s.label[a];
        for (int q = 0; q < kBondNbr; ++q) {
          const int o = s.nbr[a][q];
          if (o == kBondNone) break;
          const unsigned short l = s.label[o];
          lo = l < lo ? l : lo;
        }
        if (lo < s.label[a]) {
          s.label[a] = lo;
          changed = true;
        }
      }
      rw_fence();
      if (!rw_any(changed)) break;
    }
    int comp = 0;
    for (int a = lane; a < n; a += kRwLanes) comp += s.label[a] == a;
    int C;
    (void)rw_scan(comp, lane, C);
    if (C != 1) { status = GAUDI_BONDS_NOT_CONNECTED; break; }
    // the two-option atoms in ascending index; the charge and the number of the atoms charged by their only option
    const int per = (n + kRwLanes - 1) / kRwLanes, lo = lane * per, hi = lo + per < n ? lo + per : n;
    int nflex = 0, forced = 0, q0 = 0;
    for (int a = lo; a < hi; ++a) {
      const int r = s.row[a];
      nflex += T.n_opt[r] == 2;
      forced += T.chg[r][0] != 0;
      q0 += T.chg[r][0];
    }
    int F, forced_all, q0_all;
    int pos = rw_scan(nflex, lane, F);
    (void)rw_scan(forced, lane, forced_all);
    (void)rw_scan(q0, lane, q0_all);
    rw_fence();  // label is read above and rewritten by the search
    for (int a = lo; a < hi; ++a)
      if (T.n_opt[s.row[a]] == 2) s.flex[pos++] = (unsigned short)a;
    rw_fence();

    // ---- 3, 4. the matching and the search, by one lane
    if (lane == 0) {
      int nc = 0;
      s.result[0] = bond_search(T, s, n, F, forced_all, q0_all, nc);
      s.result[1] = nc;
    }
    rw_fence();
    status = s.result[0];
    n_charged = s.result[1];
    if (status != GAUDI_BONDS_OK) break;

    // ---- 5. outputs
    for (int a = lane; a < n; a += kRwLanes) P.charge[(size_t)b * A + a] = T.chg[s.row[a]][s.pick[a]];
    for (int k = lane; k < m; k += kRwLanes) {
      const int i = s.bl[k][0], j = s.bl[k][1];
      P.order[(size_t)b * M + k] = (unsigned char)(s.sel[i] && s.mate[i] == j ? 2 : 1);
    }
  } while (false);

  if (lane == 0) {
    P.status[b] = status;
    P.n_charged[b] = status ? 0 : n_charged;
  }
}

__global__ __launch_bounds__(64 * kBondWaves) void bonds_kernel(const BondParams P, const BondTables* __restrict__ Tp) {
  __shared__ BondSmem smem[kBondWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * kBondWaves + w;
  if (b >= P.B) return;
  assign_bond_orders(P, *Tp, smem[w], b, lane);
}

// the arguments both entry points share, checked and turned into the kernel's tables
static int bonds_prepare(const gaudi_valence_tables* vt, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                         const int32_t* bonds, const int32_t* n_bonds, BondTables& T, const char** why) {
  *why = "invalid argument";
  if (!vt || !elem || !n_atoms || !bonds || !n_bonds || B < 0 || A < 1 || M < 1) return GAUDI_E_INVALID;
  if (vt->n_elems < 1 || vt->n_elems > kBondMaxElems) { *why = "n_elems must be in 1..8"; return GAUDI_E_INVALID; }
  if (vt->h_elem < 0 || vt->h_elem >= vt->n_elems || vt->c_elem < 0 || vt->c_elem >= vt->n_elems) { *why = "h_elem / c_elem outside the element list"; return GAUDI_E_INVALID; }
  T = BondTables{};
  T.n_elems = vt->n_elems;
  T.h_elem = vt->h_elem;
  T.c_elem = vt->c_elem;
  for (int e = 0; e < vt->n_elems; ++e)
    for (int d = 0; d < kBondDegrees; ++d) {
      const int r = e * kBondDegrees + d, no = vt->n_options[e][d];
      if (no < 0 || no > 2) { *why = "n_options must be in 0..2"; return GAUDI_E_INVALID; }
      T.n_opt[r] = (signed char)no;
      for (int k = 0; k < no; ++k) {
        const int a = vt->option[e][d][k][0], q = vt->option[e][d][k][1];
        if (a < 0 || a > 1 || q < -3 || q > 3) { *why = "an option adds 0 or 1 bonds and carries a charge in -3..3"; return GAUDI_E_INVALID; }
        T.add[r][k] = (signed char)a;
        T.chg[r][k] = (signed char)q;
      }
      if (no == 2 && (T.chg[r][0] != 0 || T.chg[r][1] == 0)) { *why = "of two options the first is neutral and the second charged"; return GAUDI_E_INVALID; }
    }
  for (int b = 0; b < B; ++b)
    if (n_atoms[b] < 0 || n_atoms[b] > A || n_bonds[b] < 0 || n_bonds[b] > M) { *why = "n_atoms must be in 0..A and n_bonds in 0..M"; return GAUDI_E_INVALID; }
  return GAUDI_OK;
}

}  // namespace gaudi

#define GAUDI_BONDS_ARGS                                                                                                          \
  int B, int A, int M, const int32_t *elem, const int32_t *n_atoms, const int32_t *bonds, const int32_t *n_bonds,                 \
      uint8_t *order_out, int8_t *charge_out, int32_t *n_charged_out, int32_t *status_out

extern "C" int gaudi_bond_orders(gaudi_handle* h, const gaudi_valence_tables* vt, GAUDI_BONDS_ARGS) {
  if (!h || !order_out || !charge_out || !n_charged_out || !status_out) return GAUDI_E_INVALID;
  gaudi::BondTables T;
  const char* why = "";
  if (int rc = gaudi::bonds_prepare(vt, B, A, M, elem, n_atoms, bonds, n_bonds, T, &why)) return fail(h, rc, why);
  if (B == 0) return GAUDI_OK;
  HIPCHECK(h, hipSetDevice(h->device));
  const size_t nB = (size_t)B;
  const size_t isz[5] = {sizeof(int) * nB * A, sizeof(int) * nB, sizeof(int) * nB * M * 2, sizeof(int) * nB, sizeof(gaudi::BondTables)};
  const size_t osz[4] = {nB * M, nB * A, sizeof(int) * nB, sizeof(int) * nB};
  const void* ins[5] = {elem, n_atoms, bonds, n_bonds, &T};
  for (int i = 0; i < 5; ++i) {
    HIPCHECK(h, h->d_bonds[i].reserve(isz[i]));
    HIPCHECK(h, hipMemcpyAsync(h->d_bonds[i].p, ins[i], isz[i], hipMemcpyHostToDevice, h->stream));
  }
  // a molecule without a structure writes its status only: zero everywhere else
  for (int i = 0; i < 4; ++i) {
    HIPCHECK(h, h->d_bonds[5 + i].reserve(osz[i]));
    HIPCHECK(h, hipMemsetAsync(h->d_bonds[5 + i].p, 0, osz[i], h->stream));
  }
  HIPCHECK(h, hipStreamSynchronize(h->stream));  // T is a local object
  gaudi::BondParams P{};
  P.B = B;
  P.A = A;
  P.M = M;
  P.elem = h->d_bonds[0].as<int>();
  P.n_atoms = h->d_bonds[1].as<int>();
  P.bonds = h->d_bonds[2].as<int>();
  P.n_bonds = h->d_bonds[3].as<int>();
  P.order = h->d_bonds[5].as<unsigned char>();
  P.charge = h->d_bonds[6].as<signed char>();
  P.n_charged = h->d_bonds[7].as<int>();
  P.status = h->d_bonds[8].as<int>();
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (h->prof) HIPCHECK(h, h->bonds_log.begin(h->stream, ev));
  hipLaunchKernelGGL(gaudi::bonds_kernel, dim3((B + gaudi::kBondWaves - 1) / gaudi::kBondWaves), dim3(64 * gaudi::kBondWaves), 0,
                     h->stream, P, (const gaudi::BondTables*)h->d_bonds[4].p);
  HIPCHECK(h, hipGetLastError());
  if (h->prof) HIPCHECK(h, h->bonds_log.end(h->stream, ev));
  void* outs[4] = {order_out, charge_out, n_charged_out, status_out};
  for (int i = 0; i < 4; ++i) HIPCHECK(h, hipMemcpyAsync(outs[i], h->d_bonds[5 + i].p, osz[i], hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  return GAUDI_OK;
}

extern "C" int gaudi_bonds_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms) {
  if (!h || !n_launches || !total_ms) return GAUDI_E_INVALID;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, h->bonds_log.fold(0));
  *n_launches = (int32_t)h->bonds_log.n;
  *total_ms = h->bonds_log.ms;
  return GAUDI_OK;
}

extern "C" int gaudi_host_bond_orders(const gaudi_valence_tables* vt, GAUDI_BONDS_ARGS) {
  if (!order_out || !charge_out || !n_charged_out || !status_out) return GAUDI_E_INVALID;
  std::vector<gaudi::BondTables> Tv(1);
  const char* why = "";
  if (int rc = gaudi::bonds_prepare(vt, B, A, M, elem, n_atoms, bonds, n_bonds, Tv[0], &why)) return rc;
  if (B == 0) return GAUDI_OK;
  const size_t nB = (size_t)B;
  memset(order_out, 0, nB * M);
  memset(charge_out, 0, nB * A);
  memset(n_charged_out, 0, sizeof(int) * nB);
  memset(status_out, 0, sizeof(int) * nB);
  gaudi::BondParams P{};
  P.B = B;
  P.A = A;
  P.M = M;
  P.elem = elem;
  P.n_atoms = n_atoms;
  P.bonds = bonds;
  P.n_bonds = n_bonds;
  P.order = order_out;
  P.charge = (signed char*)charge_out;
  P.n_charged = n_charged_out;
  P.status = status_out;
  std::vector<gaudi::BondSmem> S(1);
  for (int b = 0; b < B; ++b) gaudi::assign_bond_orders(P, Tv[0], S[0], b, 0);
  return GAUDI_OK;
}
#undef GAUDI_BONDS_ARGS
