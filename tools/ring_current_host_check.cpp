// Stand-alone host program for sanitizer runs of csrc/ring_current.inc (AddressSanitizer + UndefinedBehaviorSanitizer on the HOST
// build, never on the device and never inside python): tools/ring_current_host_check.py builds and runs it.  Input: a flat file --
// the bytes of a gaudi_huckel_tables, then int32 B, A, M, then elem [B][A], n_atoms [B], bonds [B][M][2], n_bonds [B], charge [B],
// the expected status [B] (-1: any) and xyz [B][A][3] float.  It runs gaudi_host_ring_currents on the batch, then on every molecule
// of it alone in exactly-sized buffers (A = n, M = m, every output sized exactly, so any access past an array is past its
// allocation) and compares with the batch's row, then on inputs of its own in exactly-sized buffers: random graphs with
// out-of-range elements and indices, repeated bonds and degree-8 vertices, well-formed random ladders of up to 190 atoms with
// random, coincident and non-finite coordinates, charges far outside what a molecule can carry, and tables that must be refused.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gaudi_hip.h"

constexpr int kRings = GAUDI_RING_CURRENT_MAX_RINGS, kSize = GAUDI_RING_CURRENT_MAX_SIZE, kStatuses = 10;

struct Graph {
  std::vector<int32_t> e, b;
  std::vector<float> x;
};

struct Out {
  std::vector<float> bond, cur, area, normal, rms, gap, res;
  std::vector<int32_t> n_rings, atoms, size, n_pi, n_el, sweeps, flags, status;
  Out(int B, int M)
      : bond((size_t)B * M, 7.f), cur((size_t)B * kRings, 7.f), area((size_t)B * kRings, 7.f), normal((size_t)B * 3, 7.f), rms(B, 7.f),
        gap(B, 7.f), res(B, 7.f), n_rings(B, 7), atoms((size_t)B * kRings * kSize, 7), size((size_t)B * kRings, 7), n_pi(B, 7), n_el(B, 7),
        sweeps(B, 7), flags(B, 7), status(B, 7) {}
};

static int run(const gaudi_huckel_tables& t, int B, int A, int M, const int32_t* elem, const int32_t* na, const int32_t* bonds,
               const int32_t* nb, const float* xyz, const int32_t* charge, Out& o) {
  return gaudi_host_ring_currents(&t, B, A, M, elem, na, bonds, nb, xyz, charge, o.bond.data(), o.n_rings.data(), o.atoms.data(),
                                  o.size.data(), o.cur.data(), o.area.data(), o.normal.data(), o.rms.data(), o.gap.data(), o.res.data(),
                                  o.n_pi.data(), o.n_el.data(), o.sweeps.data(), o.flags.data(), o.status.data());
}

// what a call writes must be consistent with what it says
static int check(int B, int M, const int32_t* na, const Out& o, int hist[kStatuses]) {
  for (int b = 0; b < B; ++b) {
    const int st = o.status[b];
    if (st < 0 || st >= kStatuses) return 10;
    hist[st]++;
    const bool ok = st == GAUDI_HUCKEL_OK;
    const int R = o.n_rings[b];
    if (R < 0 || R > kRings || (o.flags[b] & ~GAUDI_RING_CURRENT_RINGS_UNDEFINED)) return 11;
    if (!ok && (R || o.flags[b] || o.n_pi[b] || o.n_el[b] || o.sweeps[b] || o.gap[b] != 0.f || o.rms[b] != 0.f || o.res[b] != 0.f)) return 12;
    if (ok && (o.n_pi[b] < 1 || o.n_pi[b] > GAUDI_HUCKEL_MAX_PI || (o.n_el[b] & 1) || o.sweeps[b] > GAUDI_HUCKEL_MAX_SWEEPS)) return 13;
    if ((o.flags[b] & GAUDI_RING_CURRENT_RINGS_UNDEFINED) && R) return 14;
    for (int k = 0; k < M; ++k)
      if (!std::isfinite(o.bond[(size_t)b * M + k]) || (!ok && o.bond[(size_t)b * M + k] != 0.f)) return 15;
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(o.normal[(size_t)b * 3 + k]) || (!ok && o.normal[(size_t)b * 3 + k] != 0.f)) return 16;
    const bool rows = ok && !(o.flags[b] & GAUDI_RING_CURRENT_RINGS_UNDEFINED);
    for (int r = 0; r < kRings; ++r) {
      const size_t at = (size_t)b * kRings + r;
      const int sz = o.size[at];
      if (r < R ? (sz < 4 || sz > kSize || !(o.area[at] > 1e-3f) || !std::isfinite(o.cur[at])) : (sz || o.area[at] != 0.f || o.cur[at] != 0.f))
        return 17;
      for (int j = 0; j < kSize; ++j) {
        const int a = o.atoms[at * kSize + j];
        if (rows ? (j < sz ? (a < 0 || a >= na[b]) : a != -1) : a != 0) return 18;
      }
    }
    if (!std::isfinite(o.res[b]) || o.res[b] < 0.f || o.rms[b] < 0.f || !std::isfinite(o.rms[b]) || !std::isfinite(o.gap[b])) return 19;
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
  } else {  // well-formed: a ladder of carbons and heteroatoms, every inner atom three-coordinate, no bond twice: fused four-rings
    for (auto& v : g.e) v = rng() % 5 ? 1 : 2 + (int)(rng() % 4);
    for (int a = 0; a + 2 < n; ++a) { g.b.push_back(a); g.b.push_back(a + 2); }
    for (int a = 0; a + 1 < n; a += 2) { g.b.push_back(a); g.b.push_back(a + 1); }
  }
  // coordinates: a ladder in the plane for the well-formed, random points otherwise; now and then two equal points or a NaN
  g.x.resize((size_t)n * 3);
  std::uniform_real_distribution<float> u(-6.f, 6.f);
  for (int a = 0; a < n; ++a) {
    g.x[3 * a] = mode == 4 ? 1.4f * (a / 2) : u(rng);
    g.x[3 * a + 1] = mode == 4 ? 1.4f * (a & 1) : u(rng);
    g.x[3 * a + 2] = mode == 4 ? 0.05f * u(rng) : u(rng);
  }
  if (n > 1 && rng() % 8 == 0) for (int k = 0; k < 3; ++k) g.x[3 + k] = g.x[k];
  if (rng() % 8 == 0) g.x[rng() % g.x.size()] = rng() % 2 ? NAN : INFINITY;
  return g;
}

static int one(const gaudi_huckel_tables& t, const Graph& g, int charge, int hist[kStatuses], Out* keep = nullptr, int want_rc = 0) {
  const int A = g.e.empty() ? 1 : (int)g.e.size(), M = g.b.empty() ? 1 : (int)g.b.size() / 2;
  std::vector<int32_t> e(g.e), b(g.b);
  std::vector<float> x(g.x);
  e.resize(A);
  b.resize((size_t)M * 2);
  x.resize((size_t)A * 3);
  const int32_t na = (int32_t)g.e.size(), nb = (int32_t)g.b.size() / 2, ch = charge;
  Out o(1, M);
  const int rc = run(t, 1, A, M, e.data(), &na, b.data(), &nb, x.data(), &ch, o);
  if (rc != want_rc) return 30;
  if (keep) *keep = o;
  return rc == 0 ? check(1, M, &na, o, hist) : 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  gaudi_huckel_tables t;
  int32_t head[3];
  if (fread(&t, sizeof(t), 1, f) != 1 || fread(head, sizeof(int32_t), 3, f) != 3) return 2;
  const int B = head[0], A = head[1], M = head[2];
  std::vector<int32_t> elem((size_t)B * A), na(B), bonds((size_t)B * M * 2), nb(B), charge(B), want(B);
  std::vector<float> xyz((size_t)B * A * 3);
  if (fread(elem.data(), 4, elem.size(), f) != elem.size() || fread(na.data(), 4, B, f) != (size_t)B ||
      fread(bonds.data(), 4, bonds.size(), f) != bonds.size() || fread(nb.data(), 4, B, f) != (size_t)B ||
      fread(charge.data(), 4, B, f) != (size_t)B || fread(want.data(), 4, B, f) != (size_t)B ||
      fread(xyz.data(), 4, xyz.size(), f) != xyz.size())
    return 2;
  fclose(f);
  int hist[kStatuses] = {0};
  Out all(B, M);
  if (run(t, B, A, M, elem.data(), na.data(), bonds.data(), nb.data(), xyz.data(), charge.data(), all)) return 3;
  if (int rc = check(B, M, na.data(), all, hist)) return rc;
  int undefined = 0;
  for (int b = 0; b < B; ++b) {
    if (want[b] >= 0 && all.status[b] != want[b]) return 5;
    undefined += all.flags[b] & GAUDI_RING_CURRENT_RINGS_UNDEFINED;
  }
  printf("the batch: status counts");
  for (int s = 0; s < kStatuses; ++s) printf(" %d", hist[s]);
  printf(", rings undefined %d\n", undefined);
  if (undefined < 1) return 6;
  // every molecule alone, in buffers of exactly its size: the same bits as its row of the batch
  int alone[kStatuses] = {0};
  for (int b = 0; b < B; ++b) {
    Graph g;
    g.e.assign(elem.begin() + (size_t)b * A, elem.begin() + (size_t)b * A + na[b]);
    g.b.assign(bonds.begin() + (size_t)b * M * 2, bonds.begin() + (size_t)b * M * 2 + 2 * nb[b]);
    g.x.assign(xyz.begin() + (size_t)b * A * 3, xyz.begin() + (size_t)b * A * 3 + 3 * na[b]);
    Out o(1, 1);
    if (int rc = one(t, g, charge[b], alone, &o)) return 50 + rc;
    if (o.status[0] != all.status[b] || o.n_rings[0] != all.n_rings[b] || o.flags[0] != all.flags[b] || o.sweeps[0] != all.sweeps[b] ||
        memcmp(o.cur.data(), &all.cur[(size_t)b * kRings], sizeof(float) * kRings) ||
        memcmp(o.area.data(), &all.area[(size_t)b * kRings], sizeof(float) * kRings) ||
        memcmp(o.atoms.data(), &all.atoms[(size_t)b * kRings * kSize], sizeof(int32_t) * kRings * kSize) ||
        memcmp(o.bond.data(), &all.bond[(size_t)b * M], sizeof(float) * nb[b]) || memcmp(&o.res[0], &all.res[b], sizeof(float)))
      return 7;
  }
  std::mt19937 rng(20261020u);
  int own[kStatuses] = {0};
  for (int it = 0; it < 400; ++it) {
    const int mode = it % 5, n = mode == 4 ? 1 + (int)(rng() % 190) : 1 + (int)(rng() % (mode == 3 ? 40 : 120));
    if (int rc = one(t, random_graph(rng, n, mode), (int)(rng() % 5) - 2, own)) return 100 + rc;
  }
  for (int n : {4, 6, 8, 30, 32, 34, 62, 64, 66, 126, 128, 130})  // ladders at every tier edge, with the charges that may or may not fit
    for (int charge : {0, 2, -2, 1000, -1000}) {
      Graph g = random_graph(rng, n, 4);
      for (auto& v : g.e) v = 1;
      for (int a = 0; a < n; ++a) g.x[3 * a] = 1.4f * (a / 2), g.x[3 * a + 1] = 1.4f * (a & 1), g.x[3 * a + 2] = 0.f;
      if (int rc = one(t, g, charge, own)) return 200 + rc;
    }
  if (int rc = one(t, Graph{}, 0, own)) return 300 + rc;
  for (int kind = 0; kind < 5; ++kind) {  // tables that must be refused: every molecule BAD_TABLE and nothing else written
    gaudi_huckel_tables bad = t;
    if (kind == 0) bad.site_class[1][3] = bad.n_classes;
    if (kind == 1) bad.site_class[1][3] = -2;
    if (kind == 2) bad.n_classes = GAUDI_HUCKEL_MAX_CLASSES + 1;
    if (kind == 3) bad.n_e[0] = 3;
    if (kind == 4) { bad.k_pair[0][1] = 1.f; bad.k_pair[1][0] = 2.f; }
    int h2[kStatuses] = {0};
    Graph g = random_graph(rng, 6, 4);
    if (int rc = one(bad, g, 0, h2)) return 400 + rc;
    if (h2[GAUDI_HUCKEL_BAD_TABLE] != 1) return 450 + kind;
  }
  gaudi_huckel_tables wrong = t;
  wrong.n_elems = 9;
  if (int rc = one(wrong, random_graph(rng, 6, 4), 0, own, nullptr, GAUDI_E_INVALID)) return 500 + rc;
  printf("own inputs: status counts");
  for (int s = 0; s < kStatuses; ++s) printf(" %d", own[s]);
  printf("\n");
  return own[GAUDI_HUCKEL_OK] > 20 && own[GAUDI_HUCKEL_BAD_INPUT] > 50 && own[GAUDI_HUCKEL_OVERFLOW] > 0 && own[GAUDI_HUCKEL_EMPTY] > 0 &&
                 own[GAUDI_PPP_BAD_GEOMETRY] > 0 && own[GAUDI_PPP_OPEN_SHELL] > 0 && own[GAUDI_RING_CURRENT_SMALL_GAP] > 0
             ? 0
             : 4;
}
