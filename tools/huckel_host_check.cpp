// Stand-alone host program for sanitizer runs of csrc/huckel.inc (AddressSanitizer + UndefinedBehaviorSanitizer on the HOST build,
// never on the device and never inside python): tools/huckel_host_check.py builds and runs it.  Input: a flat file -- the bytes of
// a gaudi_huckel_tables, then int32 B, A, M, then elem [B][A], n_atoms [B], bonds [B][M][2], n_bonds [B]: the g32 fixture.  It
// runs gaudi_host_huckel on the fixture with charges -1, 0, 1, then on inputs of its own in exactly-sized buffers (A = n, M = m,
// every output sized exactly, so any access past an array is past its allocation): random graphs with out-of-range elements and
// indices, repeated bonds and degree-8 vertices, well-formed random molecules of up to 190 atoms, carbon paths at every tier
// edge, charges far outside what a molecule can carry, and tables that must be refused.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gaudi_hip.h"

struct Graph {
  std::vector<int32_t> e, b;
};

struct Out {
  std::vector<float> levels, homo, lumo, gap, e_pi, q, p;
  std::vector<uint8_t> occ;
  std::vector<int32_t> n_pi, n_el, n_exc, sweeps, flags, status;
  std::vector<int8_t> site;
  Out(int B, int A, int M)
      : levels((size_t)B * 128, 7.f), homo(B, 7.f), lumo(B, 7.f), gap(B, 7.f), e_pi(B, 7.f), q((size_t)B * A, 7.f), p((size_t)B * M, 7.f),
        occ((size_t)B * 128, 7), n_pi(B, 7), n_el(B, 7), n_exc(B, 7), sweeps(B, 7), flags(B, 7), status(B, 7), site((size_t)B * A, 7) {}
};

static int run(const gaudi_huckel_tables& t, int B, int A, int M, const int32_t* elem, const int32_t* na, const int32_t* bonds,
               const int32_t* nb, const int32_t* charge, Out& o) {
  return gaudi_host_huckel(&t, B, A, M, elem, na, bonds, nb, charge, o.levels.data(), o.occ.data(), o.n_pi.data(), o.n_el.data(),
                           o.n_exc.data(), o.sweeps.data(), o.flags.data(), o.status.data(), o.homo.data(), o.lumo.data(),
                           o.gap.data(), o.e_pi.data(), o.q.data(), o.p.data(), o.site.data());
}

// what a call writes must be consistent with what it says
static int check(int B, int A, int M, const int32_t* na, const Out& o, int hist[7]) {
  for (int b = 0; b < B; ++b) {
    const int st = o.status[b];
    if (st < 0 || st > 6) return 10;
    hist[st]++;
    const bool solved = st == GAUDI_HUCKEL_OK || st == GAUDI_HUCKEL_NOT_CONVERGED;
    const int n = o.n_pi[b];
    if (n < 0 || n > GAUDI_HUCKEL_MAX_PI || (solved && n == 0)) return 11;
    int el = 0;
    for (int k = 0; k < 128; ++k) {
      const float x = o.levels[(size_t)b * 128 + k];
      const int oc = o.occ[(size_t)b * 128 + k];
      if (!std::isfinite(x) || oc > 2) return 12;
      if (k >= n && (x != 0.f || oc)) return 13;
      if (k > 0 && k < n && (x > o.levels[(size_t)b * 128 + k - 1] || oc > o.occ[(size_t)b * 128 + k - 1])) return 14;
      el += oc;
    }
    if (el != o.n_el[b] || o.gap[b] < 0.f || !std::isfinite(o.e_pi[b])) return 15;
    int sites = 0;
    for (int a = 0; a < A; ++a) {
      const int c = o.site[(size_t)b * A + a];
      if (c < -1 || c >= GAUDI_HUCKEL_MAX_CLASSES || !std::isfinite(o.q[(size_t)b * A + a])) return 16;
      if (!solved && (c || o.q[(size_t)b * A + a] != 0.f)) return 17;
      sites += solved && c >= 0 && a < na[b];  // (padding behind a molecule's atoms stays zero)
    }
    for (int k = 0; k < M; ++k)
      if (!std::isfinite(o.p[(size_t)b * M + k]) || (!solved && o.p[(size_t)b * M + k] != 0.f)) return 18;
    if (solved && sites != n) return 19;
    if (!solved && (n || o.n_el[b] || o.n_exc[b] || o.sweeps[b] || o.flags[b] || o.homo[b] != 0.f || o.lumo[b] != 0.f)) return 20;
    if (o.sweeps[b] < 0 || o.sweeps[b] > GAUDI_HUCKEL_MAX_SWEEPS || (o.flags[b] & ~3)) return 21;
  }
  return 0;
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
  } else if (mode == 3) {  // few atoms, many bonds: degrees up to 8 and beyond
    const int k = n < 10 ? n : 10;
    for (int a = 0; a < k; ++a)
      for (int c = 0; c < a; ++c)
        if (rng() % 3) { g.b.push_back(a); g.b.push_back(c); }
    for (int a = k; a < n; ++a) { g.b.push_back(rng() % a); g.b.push_back(a); }
  } else {  // well-formed: a ladder of carbons and heteroatoms, every inner atom three-coordinate, no bond twice
    for (auto& v : g.e) v = rng() % 5 ? 1 : 2 + (int)(rng() % 4);
    for (int a = 0; a + 2 < n; ++a) { g.b.push_back(a); g.b.push_back(a + 2); }
    for (int a = 0; a + 1 < n; a += 2) { g.b.push_back(a); g.b.push_back(a + 1); }
  }
  return g;
}

// a path of n carbons, two hydrogens listed at either end
static Graph polyene(int n) {
  Graph g;
  g.e.assign(n, 1);
  for (int a = 0; a + 1 < n; ++a) { g.b.push_back(a); g.b.push_back(a + 1); }
  const int ends[2] = {0, n - 1};
  for (int s = 0; s < (n == 1 ? 1 : 2); ++s)
    for (int k = 0; k < (n == 1 ? 3 : 2); ++k) {
      g.b.push_back(ends[s]);
      g.b.push_back((int)g.e.size());
      g.e.push_back(0);
    }
  return g;
}

static int one(const gaudi_huckel_tables& t, const Graph& g, int charge, int hist[7], int want_rc = 0) {
  const int A = g.e.empty() ? 1 : (int)g.e.size(), M = g.b.empty() ? 1 : (int)g.b.size() / 2;
  std::vector<int32_t> e(g.e), b(g.b);
  e.resize(A);
  b.resize((size_t)M * 2);
  const int32_t na = (int32_t)g.e.size(), nb = (int32_t)g.b.size() / 2, ch = charge;
  Out o(1, A, M);
  const int rc = run(t, 1, A, M, e.data(), &na, b.data(), &nb, &ch, o);
  if (rc != want_rc) return 30;
  return rc == 0 ? check(1, A, M, &na, o, hist) : 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  gaudi_huckel_tables t;
  int32_t head[3];
  if (fread(&t, sizeof(t), 1, f) != 1 || fread(head, sizeof(int32_t), 3, f) != 3) return 2;
  const int B = head[0], A = head[1], M = head[2];
  std::vector<int32_t> elem((size_t)B * A), na(B), bonds((size_t)B * M * 2), nb(B);
  if (fread(elem.data(), 4, elem.size(), f) != elem.size() || fread(na.data(), 4, B, f) != (size_t)B ||
      fread(bonds.data(), 4, bonds.size(), f) != bonds.size() || fread(nb.data(), 4, B, f) != (size_t)B)
    return 2;
  fclose(f);
  int hist[7] = {0};
  for (int charge = -1; charge <= 1; ++charge) {
    std::vector<int32_t> ch(B, charge);
    Out o(B, A, M);
    if (run(t, B, A, M, elem.data(), na.data(), bonds.data(), nb.data(), charge ? ch.data() : nullptr, o)) return 3;
    if (int rc = check(B, A, M, na.data(), o, hist)) return rc;
  }
  printf("fixture x 3 charges: status counts");
  for (int s = 0; s < 7; ++s) printf(" %d", hist[s]);
  printf("\n");
  std::mt19937 rng(20261020u);
  int own[7] = {0};
  for (int it = 0; it < 400; ++it) {
    const int mode = it % 5, n = mode == 4 ? 1 + (int)(rng() % 190) : 1 + (int)(rng() % (mode == 3 ? 40 : 120));
    if (int rc = one(t, random_graph(rng, n, mode), (int)(rng() % 5) - 2, own)) return 100 + rc;
  }
  for (int n : {1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129})
    for (int charge : {0, 1, -1, 1000, -1000})
      if (int rc = one(t, polyene(n), charge, own)) return 200 + rc;
  if (int rc = one(t, Graph{}, 0, own)) return 300 + rc;
  // tables that must be refused: every molecule BAD_TABLE and nothing else written
  for (int kind = 0; kind < 5; ++kind) {
    gaudi_huckel_tables bad = t;
    if (kind == 0) bad.site_class[1][3] = bad.n_classes;
    if (kind == 1) bad.site_class[1][3] = -2;
    if (kind == 2) bad.n_classes = GAUDI_HUCKEL_MAX_CLASSES + 1;
    if (kind == 3) bad.n_e[0] = 3;
    if (kind == 4) { bad.k_pair[0][1] = 1.f; bad.k_pair[1][0] = 2.f; }
    int h2[7] = {0};
    if (int rc = one(bad, polyene(6), 0, h2)) return 400 + rc;
    if (h2[GAUDI_HUCKEL_BAD_TABLE] != 1) return 450 + kind;
  }
  gaudi_huckel_tables wrong = t;
  wrong.n_elems = 9;
  if (int rc = one(wrong, polyene(6), 0, own, GAUDI_E_INVALID)) return 500 + rc;
  printf("own inputs: status counts");
  for (int s = 0; s < 7; ++s) printf(" %d", own[s]);
  printf("\n");
  return own[GAUDI_HUCKEL_OK] > 100 && own[GAUDI_HUCKEL_BAD_INPUT] > 50 && own[GAUDI_HUCKEL_OVERFLOW] > 0 && own[GAUDI_HUCKEL_EMPTY] > 0 ? 0 : 4;
}
