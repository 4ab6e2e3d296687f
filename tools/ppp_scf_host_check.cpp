// Stand-alone host program for sanitizer runs of the PPP SCF with DIIS (csrc/ppp_scf.inc, ppp_molecule<P, true, true> of csrc/ppp.inc;
// AddressSanitizer + UndefinedBehaviorSanitizer on the HOST build, never on the device and never inside python):
// tools/ppp_scf_host_check.py builds and runs it.  Input: the flat file of tools/ppp_host_check.cpp -- the bytes of a
// gaudi_ppp_tables, then int32 B, A, M, then elem [B][A], n_atoms [B], bonds [B][M][2], n_bonds [B], xyz [B][A][3] float32: the
// molecules of the g30 fixture.  It runs gaudi_host_ppp_scf on the fixture under the four state kinds, then on inputs of its own in
// exactly-sized buffers (A = n, M = m, every output sized exactly, so any access past an array is past its allocation; the host
// build's scratch row is a vector of exactly (1 + 2 diis_size) P^2 floats): carbon chains at every tier edge with histories of 2, 6
// and 8 entries and first iterations 2, 3 and 5, and histories, first iterations, multiplicities, tables and settings that must be
// refused.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "gaudi_hip.h"

constexpr int kStatuses = 9;

struct Graph {
  std::vector<int32_t> e, b;
  std::vector<float> x;
};

struct Out {
  std::vector<float> levels, q, p, homo, lumo, gap, e_el, e_core, dp, spin, derr;
  std::vector<double> e_state, he;
  std::vector<uint8_t> occ;
  std::vector<int8_t> site;
  std::vector<int32_t> n_pi, n_el, n_exc, iters, sweeps, flags, status, n_open, somo, n_ex;
  Out(int B, int A, int M)
      : levels((size_t)B * 128, 7.f), q((size_t)B * A, 7.f), p((size_t)B * M, 7.f), homo(B, 7.f), lumo(B, 7.f), gap(B, 7.f), e_el(B, 7.f),
        e_core(B, 7.f), dp(B, 7.f), spin((size_t)B * A, 7.f), derr(B, 7.f), e_state(B, 7.0), he(B, 7.0), occ((size_t)B * 128, 7),
        site((size_t)B * A, 7), n_pi(B, 7), n_el(B, 7), n_exc(B, 7), iters(B, 7), sweeps(B, 7), flags(B, 7), status(B, 7), n_open(B, 7),
        somo((size_t)B * 2, 7), n_ex(B, 7) {}
};

static int run(const gaudi_ppp_tables& t, int B, int A, int M, const int32_t* elem, const int32_t* na, const int32_t* bonds,
               const int32_t* nb, const float* xyz, const int32_t* charge, const int32_t* mult, int repulsion, int size, int start,
               float damping, Out& o) {
  return gaudi_host_ppp_scf(&t, B, A, M, elem, na, bonds, nb, xyz, charge, mult, repulsion, size, start, damping, o.levels.data(),
                            o.occ.data(), o.q.data(), o.p.data(), o.site.data(), o.n_pi.data(), o.n_el.data(), o.n_exc.data(),
                            o.iters.data(), o.sweeps.data(), o.flags.data(), o.status.data(), o.homo.data(), o.lumo.data(), o.gap.data(),
                            o.e_el.data(), o.e_core.data(), o.dp.data(), o.spin.data(), o.e_state.data(), o.he.data(), o.n_open.data(),
                            o.somo.data(), o.derr.data(), o.n_ex.data());
}

// what a call writes must be consistent with what it says
static int check(int B, int A, int M, int start, const Out& o, int hist[kStatuses]) {
  for (int b = 0; b < B; ++b) {
    const int st = o.status[b];
    if (st < 0 || st >= kStatuses || st == GAUDI_PPP_OPEN_SHELL) return 10;
    hist[st]++;
    const bool solved = st == GAUDI_HUCKEL_OK || st == GAUDI_HUCKEL_NOT_CONVERGED;
    const int n = o.n_pi[b], open = o.n_open[b];
    if (n < 0 || n > GAUDI_HUCKEL_MAX_PI || (solved && n == 0) || open < 0 || open > 2) return 11;
    int el = 0;
    for (int k = 0; k < 128; ++k) {
      const float x = o.levels[(size_t)b * 128 + k];
      const int oc = o.occ[(size_t)b * 128 + k];
      if (!std::isfinite(x) || oc < 0 || oc > 2) return 12;
      if (k >= n && (x != 0.f || oc)) return 13;
      if (k > 0 && k < n && (x < o.levels[(size_t)b * 128 + k - 1] || oc > o.occ[(size_t)b * 128 + k - 1])) return 14;
      el += oc;
    }
    if (el != o.n_el[b] || !std::isfinite(o.e_state[b]) || !std::isfinite(o.he[b]) || !std::isfinite(o.dp[b]) || !(o.derr[b] >= 0.f)) return 15;
    for (int a = 0; a < A; ++a)
      if (!std::isfinite(o.q[(size_t)b * A + a]) || !std::isfinite(o.spin[(size_t)b * A + a]) ||
          (!solved && (o.site[(size_t)b * A + a] || o.q[(size_t)b * A + a] != 0.f || o.spin[(size_t)b * A + a] != 0.f)))
        return 16;
    for (int k = 0; k < M; ++k)
      if (!std::isfinite(o.p[(size_t)b * M + k]) || (!solved && o.p[(size_t)b * M + k] != 0.f)) return 18;
    if (!solved && (n || o.n_el[b] || o.n_exc[b] || o.iters[b] || o.sweeps[b] || o.flags[b] || o.homo[b] != 0.f || o.lumo[b] != 0.f ||
                    o.e_el[b] != 0.f || o.e_core[b] != 0.f || o.dp[b] != 0.f || o.e_state[b] != 0.0 || o.he[b] != 0.0 || open ||
                    o.somo[(size_t)b * 2] || o.somo[(size_t)b * 2 + 1] || o.derr[b] != 0.f || o.n_ex[b]))
      return 20;
    if (o.iters[b] < 0 || o.iters[b] > GAUDI_PPP_MAX_ITERATIONS || o.n_ex[b] < 0 ||
        (long long)o.n_ex[b] > std::max(0ll, (long long)o.iters[b] - start + 1))
      return 21;
    if (st == GAUDI_HUCKEL_OK && !(o.dp[b] <= 1.52587890625e-5f && o.derr[b] <= GAUDI_PPP_DIIS_ERROR)) return 22;
  }
  return 0;
}

// a zig-zag chain of n carbons, hydrogens listed at either end (parked at the origin: they are not pi centres)
static Graph chain(int n) {
  Graph g;
  g.e.assign(n, 1);
  for (int a = 0; a + 1 < n; ++a) { g.b.push_back(a); g.b.push_back(a + 1); }
  for (int a = 0; a < n; ++a) {
    g.x.push_back(1.2124f * a + 5.f);
    g.x.push_back((a & 1) ? 0.7f : 0.f);
    g.x.push_back(0.f);
  }
  const int ends[2] = {0, n - 1};
  for (int s = 0; s < (n == 1 ? 1 : 2); ++s)
    for (int k = 0; k < (n == 1 ? 3 : 2); ++k) {
      g.b.push_back(ends[s]);
      g.b.push_back((int)g.e.size());
      g.e.push_back(0);
      for (int d = 0; d < 3; ++d) g.x.push_back(0.f);
    }
  return g;
}

static int one(const gaudi_ppp_tables& t, const Graph& g, int charge, int mult, int size, int start, float damping, int hist[kStatuses],
               int want_rc = 0) {
  const int A = g.e.empty() ? 1 : (int)g.e.size(), M = g.b.empty() ? 1 : (int)g.b.size() / 2;
  std::vector<int32_t> e(g.e), b(g.b);
  std::vector<float> x(g.x);
  e.resize(A);
  b.resize((size_t)M * 2);
  x.resize((size_t)A * 3);
  const int32_t na = (int32_t)g.e.size(), nb = (int32_t)g.b.size() / 2, ch = charge, mu = mult;
  Out o(1, A, M);
  const int rc = run(t, 1, A, M, e.data(), &na, b.data(), &nb, x.data(), &ch, &mu, 0, size, start, damping, o);
  if (rc != want_rc) return 30;
  return rc == 0 ? check(1, A, M, start, o, hist) : 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  gaudi_ppp_tables t;
  int32_t head[3];
  if (fread(&t, sizeof(t), 1, f) != 1 || fread(head, sizeof(int32_t), 3, f) != 3) return 2;
  const int B = head[0], A = head[1], M = head[2];
  std::vector<int32_t> elem((size_t)B * A), na(B), bonds((size_t)B * M * 2), nb(B);
  std::vector<float> xyz((size_t)B * A * 3);
  if (fread(elem.data(), 4, elem.size(), f) != elem.size() || fread(na.data(), 4, B, f) != (size_t)B ||
      fread(bonds.data(), 4, bonds.size(), f) != bonds.size() || fread(nb.data(), 4, B, f) != (size_t)B ||
      fread(xyz.data(), 4, xyz.size(), f) != xyz.size())
    return 2;
  fclose(f);
  int hist[kStatuses] = {0};
  const int kinds[4][2] = {{1, 2}, {-1, 2}, {0, 3}, {0, 1}};  // charge, multiplicity: the four state kinds
  for (int kind = 0; kind < 4; ++kind) {
    std::vector<int32_t> ch(B, kinds[kind][0]), mu(B, kinds[kind][1]);
    Out o(B, A, M);
    if (run(t, B, A, M, elem.data(), na.data(), bonds.data(), nb.data(), xyz.data(), ch.data(), mu.data(), kind & 1, 6, 3, 0.25f, o)) return 3;
    if (int rc = check(B, A, M, 3, o, hist)) return rc;
  }
  printf("fixture x 4 state kinds: status counts");
  for (int s = 0; s < kStatuses; ++s) printf(" %d", hist[s]);
  printf("\n");
  int own[kStatuses] = {0};
  // chains at every tier edge, as cations and as triplets, with the shortest, the default and the longest history
  for (int n : {1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129}) {
    const int big = n > 100;  // (the largest tier is slow under the sanitizers: fewer cases)
    const int settings[][2] = {{2, 3}, {8, 3}, {6, 2}, {6, 5}, {8, 2}};
    for (int k = 0; k < 5; ++k) {
      if (big && k != 1) continue;
      if (int rc = one(t, chain(n), 1, 0, settings[k][0], settings[k][1], 0.25f, own)) return 200 + rc;
      if (!big)
        if (int rc = one(t, chain(n), 0, 3, settings[k][0], settings[k][1], 0.f, own)) return 220 + rc;
    }
    const int refused[][2] = {{0, 3}, {1, 3}, {9, 3}, {-1, 3}, {6, 1}, {6, 0}, {6, -4}, {6, 65}, {1 << 30, 3}, {6, std::numeric_limits<int>::min()}};
    for (const auto& c : refused) {
      int h2[kStatuses] = {0};
      if (int rc = one(t, chain(n), 0, 0, c[0], c[1], 0.25f, h2)) return 240 + rc;
      if (h2[GAUDI_HUCKEL_BAD_INPUT] != 1) return 260;
      own[GAUDI_HUCKEL_BAD_INPUT]++;
    }
    int h2[kStatuses] = {0};
    if (int rc = one(t, chain(n), n, 3, 6, 3, 0.25f, h2)) return 270 + rc;  // no electron as a triplet
    if (h2[n > 128 ? GAUDI_HUCKEL_OVERFLOW : GAUDI_HUCKEL_BAD_INPUT] != 1) return 280;
  }
  if (int rc = one(t, Graph{}, 0, 0, 6, 3, 0.25f, own)) return 300 + rc;
  for (int kind = 0; kind < 4; ++kind) {  // a table or a setting that must be refused: BAD_TABLE, before the history's BAD_INPUT
    gaudi_ppp_tables bad = t;
    float damping = 0.25f;
    if (kind == 0) bad.gamma[0] = 0.f;
    if (kind == 1) bad.z[0] = 3;
    if (kind == 2) damping = 1.f;
    if (kind == 3) damping = std::numeric_limits<float>::quiet_NaN();
    int h2[kStatuses] = {0};
    if (int rc = one(bad, chain(7), 0, 0, kind & 1 ? 0 : 6, 3, damping, h2)) return 400 + rc;
    if (h2[GAUDI_HUCKEL_BAD_TABLE] != 1) return 450 + kind;
  }
  gaudi_ppp_tables wrong = t;
  wrong.n_elems = 9;
  if (int rc = one(wrong, chain(6), 1, 0, 6, 3, 0.25f, own, GAUDI_E_INVALID)) return 500 + rc;
  printf("own inputs: status counts");
  for (int s = 0; s < kStatuses; ++s) printf(" %d", own[s]);
  printf("\n");
  return own[GAUDI_HUCKEL_OK] + own[GAUDI_HUCKEL_NOT_CONVERGED] > 60 && own[GAUDI_HUCKEL_BAD_INPUT] >= 100 && own[GAUDI_HUCKEL_OVERFLOW] > 0 &&
                 own[GAUDI_HUCKEL_EMPTY] > 0
             ? 0
             : 4;
}
