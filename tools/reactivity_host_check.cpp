// Stand-alone host program for sanitizer runs of csrc/reactivity.inc (AddressSanitizer + UndefinedBehaviorSanitizer on the HOST
// build, never on the device and never inside python): tools/reactivity_host_check.py builds and runs it.  Input: a flat file --
// the bytes of a gaudi_huckel_tables, then int32 B, A, M, then elem [B][A], n_atoms [B], bonds [B][M][2], n_bonds [B], charge [B]
// and the expected status [B] (-1: any).  It runs gaudi_host_reactivity on the batch, then on every molecule of it alone in
// exactly-sized buffers (A = n, M = m, every output sized exactly, so any access past an array is past its allocation) with
// another `slices` and compares with the batch's row, then on inputs of its own in exactly-sized buffers: chains at every tier
// edge under charges that may or may not fit, random graphs with out-of-range elements and indices, repeated bonds and degree-8
// vertices, well-formed random ladders of up to 190 atoms (more than 32 rings), and tables that must be refused.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gaudi_hip.h"

constexpr int kRings = GAUDI_RING_CURRENT_MAX_RINGS, kSize = GAUDI_RING_CURRENT_MAX_SIZE, kKinds = GAUDI_REACTIVITY_KINDS, kStatuses = 7;
constexpr uint32_t kNaN = 0x7fc00000u;

struct Graph {
  std::vector<int32_t> e, b;
};

struct Out {
  std::vector<float> atom, fv, para, ortho, e_pi;
  std::vector<int32_t> rings, n_rings, n_pi, n_el, n_jobs, sweeps, flags, status;
  Out(int B, int A, int M)
      : atom((size_t)B * kKinds * A, 7.f), fv((size_t)B * A, 7.f), para((size_t)B * kRings * 3, 7.f), ortho((size_t)B * M, 7.f), e_pi(B, 7.f),
        rings((size_t)B * kRings * kSize, 7), n_rings(B, 7), n_pi(B, 7), n_el(B, 7), n_jobs(B, 7), sweeps(B, 7), flags(B, 7), status(B, 7) {}
};

static int run(const gaudi_huckel_tables& t, int B, int A, int M, const int32_t* elem, const int32_t* na, const int32_t* bonds,
               const int32_t* nb, const int32_t* charge, int with_bonds, int slices, Out& o) {
  return gaudi_host_reactivity(&t, B, A, M, elem, na, bonds, nb, charge, with_bonds, slices, o.atom.data(), o.fv.data(), o.rings.data(),
                               o.n_rings.data(), o.para.data(), o.ortho.data(), o.e_pi.data(), o.n_pi.data(), o.n_el.data(),
                               o.n_jobs.data(), o.sweeps.data(), o.flags.data(), o.status.data());
}

static uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
// a value, or THE quiet NaN
static bool fine(float f) { return std::isfinite(f) || bits(f) == kNaN; }

// what a call writes must be consistent with what it says
static int check(int B, int A, int M, const int32_t* na, const int32_t* nb, int with_bonds, const Out& o, int hist[kStatuses]) {
  for (int b = 0; b < B; ++b) {
    const int st = o.status[b];
    if (st < 0 || st >= kStatuses) return 10;
    hist[st]++;
    const bool ok = st == GAUDI_HUCKEL_OK;
    const int R = o.n_rings[b];
    if (R < 0 || R > kRings || (o.flags[b] & ~(GAUDI_REACTIVITY_SWEEP_CAP | GAUDI_REACTIVITY_RINGS_TRUNCATED))) return 11;
    if (!ok && (R || o.flags[b] || o.n_pi[b] || o.n_el[b] || o.n_jobs[b] || o.sweeps[b] || o.e_pi[b] != 0.f)) return 12;
    if (ok && (o.n_pi[b] < 1 || o.n_pi[b] > GAUDI_HUCKEL_MAX_PI || o.n_jobs[b] < o.n_pi[b] || o.n_jobs[b] > o.n_pi[b] + 3 * R + nb[b] ||
               o.sweeps[b] < 0 || o.sweeps[b] > (o.n_jobs[b] + 1) * GAUDI_HUCKEL_MAX_SWEEPS || !std::isfinite(o.e_pi[b])))
      return 13;
    int centres = 0;
    for (int a = 0; a < A; ++a) {
      const float v = o.fv[(size_t)b * A + a];
      if (ok ? !fine(v) : bits(v) != 0u) return 14;
      if (ok && a >= na[b] && bits(v) != kNaN) return 14;
      centres += ok && std::isfinite(v);
      for (int q = 0; q < kKinds; ++q) {
        const float l = o.atom[((size_t)b * kKinds + q) * A + a];
        if (ok ? !fine(l) : bits(l) != 0u) return 15;
        if (ok && std::isfinite(l) && !std::isfinite(v)) return 15;  // a localization energy only on a pi centre
      }
    }
    if (ok && centres != o.n_pi[b]) return 16;
    for (int r = 0; r < kRings; ++r) {
      int size = 0;
      for (int j = 0; j < kSize; ++j) {
        const int a = o.rings[((size_t)b * kRings + r) * kSize + j];
        if (!ok ? a != 0 : (r >= R ? a != -1 : (a < -1 || a >= na[b]))) return 17;
        size += ok && a >= 0;
      }
      if (ok && r < R && (size < 4 || size > kSize)) return 17;
      for (int k = 0; k < 3; ++k) {
        const float v = o.para[((size_t)b * kRings + r) * 3 + k];
        if (ok ? !fine(v) : bits(v) != 0u) return 18;
        if (ok && std::isfinite(v) && !(r < R && size == kSize)) return 18;
      }
    }
    for (int k = 0; k < M; ++k) {
      const float v = o.ortho[(size_t)b * M + k];
      if (ok ? !fine(v) : bits(v) != 0u) return 19;
      if (ok && std::isfinite(v) && (!with_bonds || k >= nb[b])) return 19;
    }
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
  return g;
}

// a chain of n three-coordinate carbons: two listed hydrogens at either end (three on a single carbon)
static Graph chain(int n) {
  Graph g;
  g.e.assign(n, 1);
  for (int a = 0; a + 1 < n; ++a) { g.b.push_back(a); g.b.push_back(a + 1); }
  auto add_h = [&](int parent, int count) {
    for (int k = 0; k < count; ++k) {
      g.b.push_back(parent);
      g.b.push_back((int)g.e.size());
      g.e.push_back(0);
    }
  };
  if (n == 1) {
    add_h(0, 3);
  } else {
    add_h(0, 2);
    add_h(n - 1, 2);
  }
  return g;
}

static int one(const gaudi_huckel_tables& t, const Graph& g, int charge, int with_bonds, int slices, int hist[kStatuses], Out* keep = nullptr,
               int want_rc = 0) {
  const int A = g.e.empty() ? 1 : (int)g.e.size(), M = g.b.empty() ? 1 : (int)g.b.size() / 2;
  std::vector<int32_t> e(g.e), b(g.b);
  e.resize(A);
  b.resize((size_t)M * 2);
  const int32_t na = (int32_t)g.e.size(), nb = (int32_t)g.b.size() / 2, ch = charge;
  Out o(1, A, M);
  const int rc = run(t, 1, A, M, e.data(), &na, b.data(), &nb, &ch, with_bonds, slices, o);
  if (rc != want_rc) return 30;
  if (keep) *keep = o;
  return rc == 0 ? check(1, A, M, &na, &nb, with_bonds, o, hist) : 0;
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
  if (fread(elem.data(), 4, elem.size(), f) != elem.size() || fread(na.data(), 4, B, f) != (size_t)B ||
      fread(bonds.data(), 4, bonds.size(), f) != bonds.size() || fread(nb.data(), 4, B, f) != (size_t)B ||
      fread(charge.data(), 4, B, f) != (size_t)B || fread(want.data(), 4, B, f) != (size_t)B)
    return 2;
  fclose(f);
  int hist[kStatuses] = {0};
  Out all(B, A, M);
  if (run(t, B, A, M, elem.data(), na.data(), bonds.data(), nb.data(), charge.data(), 1, 0, all)) return 3;
  if (int rc = check(B, A, M, na.data(), nb.data(), 1, all, hist)) return rc;
  int truncated = 0;
  for (int b = 0; b < B; ++b) {
    if (want[b] >= 0 && all.status[b] != want[b]) return 5;
    truncated += (all.flags[b] & GAUDI_REACTIVITY_RINGS_TRUNCATED) != 0;
  }
  printf("the batch: status counts");
  for (int s = 0; s < kStatuses; ++s) printf(" %d", hist[s]);
  printf(", rings truncated %d\n", truncated);
  if (truncated < 1) return 6;
  // every molecule alone, in buffers of exactly its size and cut into other slices: the same bits as its row of the batch
  int alone[kStatuses] = {0};
  for (int b = 0; b < B; ++b) {
    Graph g;
    g.e.assign(elem.begin() + (size_t)b * A, elem.begin() + (size_t)b * A + na[b]);
    g.b.assign(bonds.begin() + (size_t)b * M * 2, bonds.begin() + (size_t)b * M * 2 + 2 * nb[b]);
    Out o(1, 1, 1);
    if (int rc = one(t, g, charge[b], 1, 1 + b % GAUDI_REACTIVITY_MAX_SLICES, alone, &o)) return 50 + rc;
    if (o.status[0] != all.status[b] || o.n_rings[0] != all.n_rings[b] || o.flags[0] != all.flags[b] || o.sweeps[0] != all.sweeps[b] ||
        o.n_jobs[0] != all.n_jobs[b] || memcmp(&o.e_pi[0], &all.e_pi[b], 4) ||
        memcmp(o.para.data(), &all.para[(size_t)b * kRings * 3], sizeof(float) * kRings * 3) ||
        memcmp(o.rings.data(), &all.rings[(size_t)b * kRings * kSize], sizeof(int32_t) * kRings * kSize) ||
        memcmp(o.ortho.data(), &all.ortho[(size_t)b * M], sizeof(float) * nb[b]) ||
        memcmp(o.fv.data(), &all.fv[(size_t)b * A], sizeof(float) * na[b]))
      return 7;
    const int n = na[b] > 0 ? na[b] : 1;
    for (int q = 0; q < kKinds; ++q)
      if (memcmp(&o.atom[(size_t)q * n], &all.atom[((size_t)b * kKinds + q) * A], sizeof(float) * na[b])) return 8;
  }
  std::mt19937 rng(20261021u);
  int own[kStatuses] = {0};
  for (int n : {1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129})  // chains at every tier edge, with charges that may or may not fit
    for (int ch : {0, 1, -1, n, -n, n - 1, 1 - n, 1000, -1000}) {
      if (n > 33 && ch != 0 && ch != 1000) continue;  // (the host build runs every solve serially: the large chains once, without their bond jobs)
      if (int rc = one(t, chain(n), ch, ch == 0 && n <= 33, 1 + (int)(rng() % GAUDI_REACTIVITY_MAX_SLICES), own)) return 200 + rc;
    }
  for (int it = 0; it < 150; ++it) {
    const int mode = it % 5, n = mode == 4 ? 1 + (int)(rng() % 190) : 1 + (int)(rng() % (mode == 3 ? 40 : 120));
    // (the large well-formed ladders without their bond jobs: the host build runs every solve serially)
    if (int rc = one(t, random_graph(rng, n, mode), (int)(rng() % 5) - 2, mode != 4 || n < 60, (int)(rng() % (GAUDI_REACTIVITY_MAX_SLICES + 1)), own))
      return 100 + rc;
  }
  if (int rc = one(t, Graph{}, 0, 1, 0, own)) return 300 + rc;
  for (int kind = 0; kind < 5; ++kind) {  // tables that must be refused: every molecule BAD_TABLE and nothing else written
    gaudi_huckel_tables bad = t;
    if (kind == 0) bad.site_class[1][3] = bad.n_classes;
    if (kind == 1) bad.site_class[1][3] = -2;
    if (kind == 2) bad.n_classes = GAUDI_HUCKEL_MAX_CLASSES + 1;
    if (kind == 3) bad.n_e[0] = 3;
    if (kind == 4) { bad.k_pair[0][1] = 1.f; bad.k_pair[1][0] = 2.f; }
    int h2[kStatuses] = {0};
    if (int rc = one(bad, random_graph(rng, 6, 4), 0, 1, 0, h2)) return 400 + rc;
    if (h2[GAUDI_HUCKEL_BAD_TABLE] != 1) return 450 + kind;
  }
  gaudi_huckel_tables wrong = t;
  wrong.n_elems = 9;
  if (int rc = one(wrong, random_graph(rng, 6, 4), 0, 1, 0, own, nullptr, GAUDI_E_INVALID)) return 500 + rc;
  if (int rc = one(t, chain(6), 0, 1, GAUDI_REACTIVITY_MAX_SLICES + 1, own, nullptr, GAUDI_E_INVALID)) return 510 + rc;
  if (int rc = one(t, chain(6), 0, 1, -1, own, nullptr, GAUDI_E_INVALID)) return 520 + rc;
  printf("own inputs: status counts");
  for (int s = 0; s < kStatuses; ++s) printf(" %d", own[s]);
  printf("\n");
  return own[GAUDI_HUCKEL_OK] > 40 && own[GAUDI_HUCKEL_BAD_INPUT] > 40 && own[GAUDI_HUCKEL_OVERFLOW] > 0 && own[GAUDI_HUCKEL_EMPTY] > 0 ? 0 : 4;
}
