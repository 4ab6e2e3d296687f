// Stand-alone host program for sanitizer runs of the open-shell PPP kernel (csrc/ppp_open.inc, ppp_molecule<P, true> of csrc/ppp.inc;
// AddressSanitizer + UndefinedBehaviorSanitizer on the HOST build, never on the device and never inside python):
// tools/ppp_open_host_check.py builds and runs it.  Input: the flat file of tools/ppp_host_check.cpp -- the bytes of a
// gaudi_ppp_tables, then int32 B, A, M, then elem [B][A], n_atoms [B], bonds [B][M][2], n_bonds [B], xyz [B][A][3] float32: the
// molecules of the g30 fixture.  It runs gaudi_host_ppp_open on the fixture under the four state kinds (cation and anion doublets,
// the triplet, the singlet) and at the lowest multiplicity, the repulsion formulas alternating, then on inputs of its own in exactly-sized buffers (A = n, M = m, every
// output sized exactly, so any access past an array is past its allocation): carbon chains at every tier edge under charges and
// multiplicities that fit, that just fit (every level filled, no level filled, the open set at either end of the spectrum) and that
// do not, random graphs with out-of-range elements and indices and random planar coordinates (some coincident, some not finite)
// under random charges and multiplicities, and tables, settings and multiplicities that must be refused.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "gaudi_hip.h"

constexpr int kStatuses = 9;

struct Graph {
  std::vector<int32_t> e, b;
  std::vector<float> x;
};

struct Out {
  std::vector<float> levels, q, p, homo, lumo, gap, e_el, e_core, dp, spin;
  std::vector<double> e_state, he;
  std::vector<uint8_t> occ;
  std::vector<int8_t> site;
  std::vector<int32_t> n_pi, n_el, n_exc, iters, sweeps, flags, status, n_open, somo;
  Out(int B, int A, int M)
      : levels((size_t)B * 128, 7.f), q((size_t)B * A, 7.f), p((size_t)B * M, 7.f), homo(B, 7.f), lumo(B, 7.f), gap(B, 7.f), e_el(B, 7.f),
        e_core(B, 7.f), dp(B, 7.f), spin((size_t)B * A, 7.f), e_state(B, 7.0), he(B, 7.0), occ((size_t)B * 128, 7), site((size_t)B * A, 7),
        n_pi(B, 7), n_el(B, 7), n_exc(B, 7), iters(B, 7), sweeps(B, 7), flags(B, 7), status(B, 7), n_open(B, 7), somo((size_t)B * 2, 7) {}
};

static int run(const gaudi_ppp_tables& t, int B, int A, int M, const int32_t* elem, const int32_t* na, const int32_t* bonds,
               const int32_t* nb, const float* xyz, const int32_t* charge, const int32_t* mult, int repulsion, float damping, Out& o) {
  return gaudi_host_ppp_open(&t, B, A, M, elem, na, bonds, nb, xyz, charge, mult, repulsion, damping, o.levels.data(), o.occ.data(),
                             o.q.data(), o.p.data(), o.site.data(), o.n_pi.data(), o.n_el.data(), o.n_exc.data(), o.iters.data(),
                             o.sweeps.data(), o.flags.data(), o.status.data(), o.homo.data(), o.lumo.data(), o.gap.data(), o.e_el.data(),
                             o.e_core.data(), o.dp.data(), o.spin.data(), o.e_state.data(), o.he.data(), o.n_open.data(), o.somo.data());
}

// what a call writes must be consistent with what it says; mult: what was asked for (null: all zero)
static int check(int B, int A, int M, const int32_t* na, const int32_t* mult, const Out& o, int hist[kStatuses]) {
  for (int b = 0; b < B; ++b) {
    const int st = o.status[b];
    if (st < 0 || st >= kStatuses || st == GAUDI_PPP_OPEN_SHELL) return 10;  // (the new entry never says OPEN_SHELL)
    hist[st]++;
    const bool solved = st == GAUDI_HUCKEL_OK || st == GAUDI_HUCKEL_NOT_CONVERGED;
    const int n = o.n_pi[b], open = o.n_open[b];
    if (n < 0 || n > GAUDI_HUCKEL_MAX_PI || (solved && n == 0) || open < 0 || open > 2) return 11;
    if (solved && mult && mult[b] && open != mult[b] - 1) return 11;
    if (solved && (!mult || !mult[b]) && open != (o.n_el[b] & 1)) return 11;
    int el = 0, singles = 0;
    for (int k = 0; k < 128; ++k) {
      const float x = o.levels[(size_t)b * 128 + k];
      const int oc = o.occ[(size_t)b * 128 + k];
      if (!std::isfinite(x) || oc < 0 || oc > 2) return 12;
      if (k >= n && (x != 0.f || oc)) return 13;
      if (k > 0 && k < n && (x < o.levels[(size_t)b * 128 + k - 1] || oc > o.occ[(size_t)b * 128 + k - 1])) return 14;
      if (oc == 1 && (singles >= 2 || o.somo[(size_t)b * 2 + singles] != k)) return 14;
      singles += oc == 1;
      el += oc;
    }
    if (el != o.n_el[b] || singles != open || o.gap[b] < 0.f || !std::isfinite(o.e_el[b]) || !std::isfinite(o.e_core[b]) ||
        !std::isfinite(o.dp[b]) || !std::isfinite(o.e_state[b]) || !std::isfinite(o.he[b]))
      return 15;
    for (int k = open; solved && k < 2; ++k)
      if (o.somo[(size_t)b * 2 + k] != -1) return 15;
    int sites = 0;
    double spin = 0.0;
    for (int a = 0; a < A; ++a) {
      const int c = o.site[(size_t)b * A + a];
      const float sd = o.spin[(size_t)b * A + a];
      if (c < -1 || c >= GAUDI_HUCKEL_MAX_CLASSES || !std::isfinite(o.q[(size_t)b * A + a]) || !(sd >= 0.f && sd <= 1.001f)) return 16;
      if (!solved && (c || o.q[(size_t)b * A + a] != 0.f || sd != 0.f)) return 17;
      if (sd != 0.f && (c < 0 || a >= na[b])) return 17;
      sites += solved && c >= 0 && a < na[b];  // (padding behind a molecule's atoms stays zero)
      spin += sd;
    }
    if (solved && std::fabs(spin - open) > 1e-3) return 17;
    for (int k = 0; k < M; ++k)
      if (!std::isfinite(o.p[(size_t)b * M + k]) || (!solved && o.p[(size_t)b * M + k] != 0.f)) return 18;
    if (solved && sites != n) return 19;
    if (!solved && (n || o.n_el[b] || o.n_exc[b] || o.iters[b] || o.sweeps[b] || o.flags[b] || o.homo[b] != 0.f || o.lumo[b] != 0.f ||
                    o.e_el[b] != 0.f || o.e_core[b] != 0.f || o.dp[b] != 0.f || o.e_state[b] != 0.0 || o.he[b] != 0.0 || open ||
                    o.somo[(size_t)b * 2] || o.somo[(size_t)b * 2 + 1]))
      return 20;
    if (o.iters[b] < 0 || o.iters[b] > GAUDI_PPP_MAX_ITERATIONS || o.sweeps[b] < 0 ||
        o.sweeps[b] > GAUDI_PPP_MAX_ITERATIONS * GAUDI_HUCKEL_MAX_SWEEPS || (o.flags[b] & ~(14 | GAUDI_PPP_OPEN_TIE)) ||
        (open == 0 && ((o.flags[b] & GAUDI_PPP_OPEN_TIE) || o.he[b] != 0.0)))
      return 21;
    if (solved && (o.iters[b] < 1 || (st == GAUDI_HUCKEL_OK) != !(o.flags[b] & (GAUDI_PPP_SCF_CAP | GAUDI_PPP_JACOBI_CAP)))) return 22;
  }
  return 0;
}

// random planar coordinates on a jittered grid of 1.4 A: distinct atoms at least 0.7 A apart; a fault breaks one of them
static void place(std::mt19937& rng, Graph& g, int fault) {
  const int n = (int)g.e.size(), side = 1 + (int)std::ceil(std::sqrt((double)n));
  std::vector<int> cell(side * side);
  for (int k = 0; k < side * side; ++k) cell[k] = k;
  std::shuffle(cell.begin(), cell.end(), rng);
  std::uniform_real_distribution<float> jitter(-0.35f, 0.35f);
  g.x.resize((size_t)n * 3);
  for (int a = 0; a < n; ++a) {
    g.x[3 * a] = 1.4f * (cell[a] % side) + jitter(rng);
    g.x[3 * a + 1] = 1.4f * (cell[a] / side) + jitter(rng);
    g.x[3 * a + 2] = 0.f;
  }
  if (fault && n > 1) {
    const int a = rng() % n, c = (a + 1 + rng() % (n - 1)) % n;
    switch (rng() % 3) {
      case 0: g.x[3 * a + 1] = std::numeric_limits<float>::quiet_NaN(); break;
      case 1: g.x[3 * a] = std::numeric_limits<float>::infinity(); break;
      default: for (int k = 0; k < 3; ++k) g.x[3 * a + k] = g.x[3 * c + k]; break;
    }
  }
}

static Graph random_graph(std::mt19937& rng, int n, int mode) {
  Graph g;
  g.e.resize(n);
  for (auto& v : g.e) v = mode == 2 ? (int)(rng() % 7) : (rng() % 4 ? 1 : (int)(rng() % 6));
  if (mode < 2) {  // a tree plus chords; mode 1 with a fault
    for (int a = 1; a < n; ++a) { g.b.push_back(rng() % a); g.b.push_back(a); }
    for (int k = 0; k < n / 3; ++k) {
      const int a = rng() % n, c = rng() % n;
      if (a != c) { g.b.push_back(a); g.b.push_back(c); }
    }
    if (mode == 1 && !g.b.empty()) {
      const int k = rng() % (g.b.size() / 2);
      switch (rng() % 3) {
        case 0: g.b[2 * k + 1] = n; break;
        case 1: g.b[2 * k] = -1; break;
        default: g.b[2 * k + 1] = g.b[2 * k]; break;
      }
    }
  } else if (mode == 2) {  // noise
    const int m = 1 + rng() % 90;
    for (int k = 0; k < 2 * m; ++k) g.b.push_back((int)(rng() % (n + 1)) - (rng() % 50 == 0));
  } else {  // well-formed: a ladder of carbons and heteroatoms, every inner atom three-coordinate, no bond twice
    for (auto& v : g.e) v = rng() % 5 ? 1 : 2 + (int)(rng() % 4);
    for (int a = 0; a + 2 < n; ++a) { g.b.push_back(a); g.b.push_back(a + 2); }
    for (int a = 0; a + 1 < n; a += 2) { g.b.push_back(a); g.b.push_back(a + 1); }
  }
  place(rng, g, mode == 3 ? 0 : rng() % 4 == 0);
  return g;
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

static int one(const gaudi_ppp_tables& t, const Graph& g, int charge, int mult, int repulsion, float damping, int hist[kStatuses],
               int want_rc = 0) {
  const int A = g.e.empty() ? 1 : (int)g.e.size(), M = g.b.empty() ? 1 : (int)g.b.size() / 2;
  std::vector<int32_t> e(g.e), b(g.b);
  std::vector<float> x(g.x);
  e.resize(A);
  b.resize((size_t)M * 2);
  x.resize((size_t)A * 3);
  const int32_t na = (int32_t)g.e.size(), nb = (int32_t)g.b.size() / 2, ch = charge, mu = mult;
  Out o(1, A, M);
  const int rc = run(t, 1, A, M, e.data(), &na, b.data(), &nb, x.data(), &ch, &mu, repulsion, damping, o);
  if (rc != want_rc) return 30;
  return rc == 0 ? check(1, A, M, &na, &mu, o, hist) : 0;
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
  const int kinds[5][2] = {{1, 2}, {-1, 2}, {0, 3}, {0, 1}, {1, 0}};  // charge, multiplicity: the four state kinds, and "the lowest"
  for (int kind = 0; kind < 5; ++kind)
    for (int repulsion = kind & 1; repulsion <= (kind & 1); ++repulsion) {  // (the formulas alternate: a run takes a while here)
      std::vector<int32_t> ch(B, kinds[kind][0]), mu(B, kinds[kind][1]);
      Out o(B, A, M);
      if (run(t, B, A, M, elem.data(), na.data(), bonds.data(), nb.data(), xyz.data(), kinds[kind][0] ? ch.data() : nullptr,
              kinds[kind][1] ? mu.data() : nullptr, repulsion, repulsion ? 0.f : 0.25f, o))
        return 3;
      if (int rc = check(B, A, M, na.data(), kinds[kind][1] ? mu.data() : nullptr, o, hist)) return rc;
    }
  printf("fixture x 5 state kinds: status counts");
  for (int s = 0; s < kStatuses; ++s) printf(" %d", hist[s]);
  printf("\n");
  std::mt19937 rng(20261021u);
  int own[kStatuses] = {0};
  for (int it = 0; it < 240; ++it) {
    const int mode = it % 4;  // (a few large ladders: a random geometry rarely converges, and 64 iterations of 128 centres are slow here)
    const int n = mode == 3 ? (it % 40 == 3 ? 100 + (int)(rng() % 90) : 1 + (int)(rng() % 50)) : 1 + (int)(rng() % 60);
    if (int rc = one(t, random_graph(rng, n, mode), (int)(rng() % 5) - 2, (int)(rng() % 6) - 1, (int)(rng() % 2), 0.25f * (float)(rng() % 3),
                     own))
      return 100 + rc;
  }
  // chains at every tier edge.  A chain of n carbons has n electrons at charge 0: multiplicities that fit, that just fit (charge
  // n - 1: one electron, a doublet in the lowest level; charge n - 2 as a triplet: the open set IS the bottom; charge -(n - 1) and
  // -(n - 2): the open set at the top, every level occupied; charge -n: every level filled), and that do not.
  for (int n : {1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129}) {
    const int big = n > 100;  // (the largest tier is slow under the sanitizers: fewer cases)
    for (int mult = 0; mult <= 3; ++mult)
      for (int charge : {0, 1, -1})
        if (!big || (mult == 0 && charge == 1) || (mult == 3 && charge == 0))
          if (int rc = one(t, chain(n), charge, mult, n & 1, 0.25f, own)) return 200 + rc;
    const int fits[][2] = {{n - 1, 2}, {n - 1, 0}, {n - 2, 3}, {-(n - 1), 2}, {-(n - 2), 3}, {-n, 1}, {-n, 0}, {n, 1}, {n, 0}};
    for (int k = 0; k < 9; ++k) {
      const int* c = fits[k];
      if (big && k != 0 && k != 4 && k != 6) continue;
      if (int rc = one(t, chain(n), c[0], c[1], 0, 0.25f, own)) return 220 + rc;
    }
    const int misfits[][2] = {{n, 2}, {n, 3}, {n - 1, 3}, {-n, 2}, {-n, 3}, {-(n - 1), 3}, {n + 1, 0}, {-(n + 1), 0}, {1000, 0}, {-1000, 2},
                              {0, 4}, {0, -1}, {1, 4}, {0, 1 << 30}, {0, -(1 << 30)},
                              {0, std::numeric_limits<int>::max()}, {0, std::numeric_limits<int>::min()}};
    for (const auto& c : misfits) {
      int h2[kStatuses] = {0};
      if (int rc = one(t, chain(n), c[0], c[1], 0, 0.25f, h2)) return 240 + rc;
      if (h2[n > 128 ? GAUDI_HUCKEL_OVERFLOW : GAUDI_HUCKEL_BAD_INPUT] != 1) return 260;
      own[n > 128 ? GAUDI_HUCKEL_OVERFLOW : GAUDI_HUCKEL_BAD_INPUT]++;
    }
  }
  for (int n : {2, 33})  // a coordinate of a pi centre that is not finite, two centres in one place: BAD_GEOMETRY
    for (int kind = 0; kind < 3; ++kind) {
      Graph g = chain(n);
      const int a = n / 2;
      if (kind == 0) g.x[3 * a + 2] = std::numeric_limits<float>::quiet_NaN();
      if (kind == 1) g.x[3 * a] = -std::numeric_limits<float>::infinity();
      if (kind == 2) for (int k = 0; k < 3; ++k) g.x[3 * a + k] = g.x[k];
      int h2[kStatuses] = {0};
      if (int rc = one(t, g, 1, 0, kind & 1, 0.25f, h2)) return 270 + rc;
      if (h2[GAUDI_PPP_BAD_GEOMETRY] != 1) return 290 + kind;
      own[GAUDI_PPP_BAD_GEOMETRY]++;
    }
  if (int rc = one(t, Graph{}, 0, 0, 0, 0.25f, own)) return 300 + rc;
  // tables and settings that must be refused: every row BAD_TABLE and nothing else written
  for (int kind = 0; kind < 12; ++kind) {
    gaudi_ppp_tables bad = t;
    int repulsion = 0;
    float damping = 0.25f;
    if (kind == 0) bad.site_class[1][3] = bad.n_classes;
    if (kind == 1) bad.site_class[1][3] = -2;
    if (kind == 2) bad.n_classes = GAUDI_HUCKEL_MAX_CLASSES + 1;
    if (kind == 3) bad.z[0] = 3;
    if (kind == 4) { bad.beta_pair[0][1] = -1.f; bad.beta_pair[1][0] = -2.f; }
    if (kind == 5) bad.gamma[0] = 0.f;
    if (kind == 6) bad.gamma[1] = std::numeric_limits<float>::quiet_NaN();
    if (kind == 7) bad.I[0] = std::numeric_limits<float>::infinity();
    if (kind == 8) bad.beta0 = std::numeric_limits<float>::quiet_NaN();
    if (kind == 9) damping = 1.f;
    if (kind == 10) damping = -0.5f;
    if (kind == 11) repulsion = 2;
    int h2[kStatuses] = {0};
    if (int rc = one(bad, chain(7), 0, kind % 3 ? 2 : 0, repulsion, damping, h2)) return 400 + rc;
    if (h2[GAUDI_HUCKEL_BAD_TABLE] != 1) return 450 + kind;
  }
  gaudi_ppp_tables wrong = t;
  wrong.n_elems = 9;
  if (int rc = one(wrong, chain(6), 1, 0, 0, 0.25f, own, GAUDI_E_INVALID)) return 500 + rc;
  printf("own inputs: status counts");
  for (int s = 0; s < kStatuses; ++s) printf(" %d", own[s]);
  printf("\n");
  return own[GAUDI_HUCKEL_OK] + own[GAUDI_HUCKEL_NOT_CONVERGED] > 150 && own[GAUDI_HUCKEL_BAD_INPUT] > 150 && own[GAUDI_HUCKEL_OVERFLOW] > 0 &&
                 own[GAUDI_HUCKEL_EMPTY] > 0 && own[GAUDI_PPP_BAD_GEOMETRY] > 5
             ? 0
             : 4;
}
