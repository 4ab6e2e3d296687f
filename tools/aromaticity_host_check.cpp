// Stand-alone host program for sanitizer runs of csrc/kekule.inc (AddressSanitizer + UndefinedBehaviorSanitizer on the HOST build,
// never on the device and never inside python): tools/aromaticity_host_check.py builds and runs it.  Input: a flat file -- int32
// n_elems, h_elem, c_elem, B, A, M, then the valence table (n_options [8][5], option [8][5][2][2]), then elem [B][A], n_atoms [B],
// bonds [B][M][2], n_bonds [B]: the g32 fixture.  It runs gaudi_host_kekule on the fixture, then on inputs of its own in
// exactly-sized buffers (A = n, M = m, every output sized exactly, so any access past an array is past its allocation): random
// graphs with out-of-range elements and indices, repeated bonds and degree-8 vertices, well-formed random molecules of up to 190
// atoms, carbon ladders up to the capacity of 128 sel atoms and one beyond it, fused-hexagon strips up to and beyond 32 hexagons,
// and a ladder beyond the budget.
#include <cstdio>
#include <random>
#include <vector>

#include "gaudi_hip.h"

struct Graph {
  std::vector<int32_t> e, b;
};

struct Out {
  std::vector<int64_t> k, nodes;
  std::vector<uint32_t> dc, sc;
  std::vector<int32_t> nhex, hex, fries, clar, st;
  Out(int B, int M)
      : k(B), nodes(B), dc((size_t)B * M), sc((size_t)B * GAUDI_RINGS_MAX_RINGS), nhex(B), hex((size_t)B * GAUDI_RINGS_MAX_RINGS * 6),
        fries(B), clar(B), st(B) {}
};

static int run(const gaudi_valence_tables& vt, int B, int A, int M, const std::vector<int32_t>& elem, const std::vector<int32_t>& na,
               const std::vector<int32_t>& bonds, const std::vector<int32_t>& nb, Out& o) {
  return gaudi_host_kekule(&vt, B, A, M, elem.data(), na.data(), bonds.data(), nb.data(), o.k.data(), o.dc.data(), o.nhex.data(),
                           o.hex.data(), o.sc.data(), o.fries.data(), o.clar.data(), o.nodes.data(), o.st.data());
}

// what a call writes must be consistent with what it says
static int check(int B, int A, int M, const std::vector<int32_t>& na, const std::vector<int32_t>& nb, const Out& o, int hist[9]) {
  for (int b = 0; b < B; ++b) {
    const int st = o.st[b];
    if (st < 0 || st > 8) return 10;
    hist[st]++;
    uint64_t dsum = 0, ssum = 0, hsum = 0;
    for (int k = 0; k < M; ++k) {
      const uint32_t d = o.dc[(size_t)b * M + k];
      if (d > o.k[b] || (k >= nb[b] && d)) return 11;
      dsum += d;
    }
    for (int r = 0; r < GAUDI_RINGS_MAX_RINGS; ++r) {
      const uint32_t s = o.sc[(size_t)b * GAUDI_RINGS_MAX_RINGS + r];
      if (s > o.k[b] || (r >= o.nhex[b] && s)) return 12;
      ssum += s;
      for (int j = 0; j < 6; ++j) {
        const int a = o.hex[((size_t)b * GAUDI_RINGS_MAX_RINGS + r) * 6 + j];
        if (a < 0 || a >= A || (r >= o.nhex[b] && a) || (r < o.nhex[b] && a >= na[b])) return 13;
        hsum += a;
      }
    }
    if (st != GAUDI_KEKULE_OK && (o.k[b] || o.nodes[b] || o.nhex[b] || o.fries[b] || o.clar[b] || dsum || ssum || hsum)) return 14;
    if (st == GAUDI_KEKULE_OK) {
      if (o.k[b] < 1 || o.nodes[b] < 1 || o.nodes[b] > GAUDI_KEKULE_BUDGET || o.k[b] > o.nodes[b]) return 15;
      if (o.nhex[b] < 0 || o.nhex[b] > GAUDI_RINGS_MAX_RINGS || o.clar[b] > o.fries[b] || o.fries[b] > o.nhex[b] || o.clar[b] < 0) return 16;
      if (dsum % (uint64_t)o.k[b]) return 17;  // every structure has the same number of double bonds
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
  } else {  // well-formed and connected: degree at most 3, a tree plus chords, no bond twice; elements that have an option at
           // their degree (H, O or S at the ends, mostly carbon inside; rarely a three-coordinate O, whose only option is charged)
    std::vector<char> seen((size_t)n * n, 0);
    std::vector<int> deg(n, 0);
    for (int a = 1; a < n; ++a) {
      int c = rng() % a;
      for (int t = 0; t < 8 && deg[c] >= 3; ++t) c = rng() % a;
      seen[(size_t)a * n + c] = seen[(size_t)c * n + a] = 1;
      ++deg[a];
      ++deg[c];
      g.b.push_back(c);
      g.b.push_back(a);
    }
    for (int k = 0; k < n / 2; ++k) {
      const int a = rng() % n, c = rng() % n;
      if (a == c || seen[(size_t)a * n + c] || deg[a] >= 3 || deg[c] >= 3) continue;
      seen[(size_t)a * n + c] = seen[(size_t)c * n + a] = 1;
      ++deg[a];
      ++deg[c];
      g.b.push_back(a);
      g.b.push_back(c);
    }
    for (int a = 0; a < n; ++a) {
      const int r = rng() % 40;
      g.e[a] = deg[a] <= 1 ? (r < 20 ? 0 : r < 30 ? 4 : 5) : deg[a] == 2 ? (r < 30 ? 1 : r < 34 ? 3 : 4 + r % 2) : (r < 36 ? 1 : r < 39 ? 2 + r % 2 : 4);
    }
  }
  return g;
}

// two graphs in one record
static Graph both(const Graph& x, const Graph& y) {
  Graph g = x;
  g.e.insert(g.e.end(), y.e.begin(), y.e.end());
  for (int32_t v : y.b) g.b.push_back(v + (int32_t)x.e.size());
  return g;
}

// 2 x n three-coordinate carbons; with a shuffled numbering when asked
static Graph ladder(std::mt19937& rng, int n, bool shuffle) {
  Graph g;
  g.e.assign(2 * n, 1);
  std::vector<int> p(2 * n);
  for (int i = 0; i < 2 * n; ++i) p[i] = i;
  if (shuffle)
    for (int i = 2 * n - 1; i > 0; --i) std::swap(p[i], p[rng() % (i + 1)]);
  for (int k = 0; k < n; ++k) { g.b.push_back(p[2 * k]); g.b.push_back(p[2 * k + 1]); }
  for (int k = 0; k + 1 < n; ++k) {
    g.b.push_back(p[2 * k]); g.b.push_back(p[2 * k + 2]);
    g.b.push_back(p[2 * k + 1]); g.b.push_back(p[2 * k + 3]);
  }
  return g;
}

// a row of `rings` fused six-rings (an acene): 4 * rings + 2 carbons
static Graph acene(int rings) {
  Graph g;
  const int n = 4 * rings + 2, top = 2 * rings + 1;
  g.e.assign(n, 1);
  for (int a = 0; a + 1 < top; ++a) { g.b.push_back(a); g.b.push_back(a + 1); }
  for (int a = top; a + 1 < n; ++a) { g.b.push_back(a); g.b.push_back(a + 1); }
  for (int k = 0; k <= rings; ++k) { g.b.push_back(2 * k); g.b.push_back(top + 2 * k); }
  return g;
}

// graphs into exactly-sized packed arrays
static void pack(const std::vector<Graph>& gs, int& A, int& M, std::vector<int32_t>& elem, std::vector<int32_t>& na,
                 std::vector<int32_t>& bonds, std::vector<int32_t>& nb) {
  A = 1;
  M = 1;
  for (const Graph& g : gs) {
    if ((int)g.e.size() > A) A = (int)g.e.size();
    if ((int)g.b.size() / 2 > M) M = (int)g.b.size() / 2;
  }
  const size_t n = gs.size();
  elem.assign(n * A, 0);
  bonds.assign(n * M * 2, 0);
  na.resize(n);
  nb.resize(n);
  for (size_t i = 0; i < n; ++i) {
    na[i] = (int32_t)gs[i].e.size();
    nb[i] = (int32_t)gs[i].b.size() / 2;
    for (size_t k = 0; k < gs[i].e.size(); ++k) elem[i * A + k] = gs[i].e[k];
    for (size_t k = 0; k < gs[i].b.size(); ++k) bonds[i * M * 2 + k] = gs[i].b[k];
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  int32_t hdr[6];
  gaudi_valence_tables vt{};
  if (!f || fread(hdr, sizeof hdr, 1, f) != 1) return 2;
  if (fread(vt.n_options, sizeof vt.n_options, 1, f) != 1 || fread(vt.option, sizeof vt.option, 1, f) != 1) return 2;
  vt.n_elems = hdr[0];
  vt.h_elem = hdr[1];
  vt.c_elem = hdr[2];
  const int B = hdr[3], A = hdr[4], M = hdr[5];
  std::vector<int32_t> elem((size_t)B * A), na(B), bonds((size_t)B * M * 2), nb(B);
  if (fread(elem.data(), 4, elem.size(), f) != elem.size() || fread(na.data(), 4, B, f) != (size_t)B ||
      fread(bonds.data(), 4, bonds.size(), f) != bonds.size() || fread(nb.data(), 4, B, f) != (size_t)B)
    return 2;
  fclose(f);

  {
    Out o(B, M);
    int hist[9] = {0};
    const int rc = run(vt, B, A, M, elem, na, bonds, nb, o);
    const int bad = rc ? rc : check(B, A, M, na, nb, o, hist);
    int64_t kmax = 0, nmax = 0;
    for (int b = 0; b < B; ++b) {
      if (o.k[b] > kmax) kmax = o.k[b];
      if (o.nodes[b] > nmax) nmax = o.nodes[b];
    }
    printf("fixture: rc %d, statuses 0..8: %d %d %d %d %d %d %d %d %d, largest K %lld, largest tree %lld nodes\n", bad, hist[0], hist[1],
           hist[2], hist[3], hist[4], hist[5], hist[6], hist[7], hist[8], (long long)kmax, (long long)nmax);
    if (bad || hist[GAUDI_KEKULE_UNDECIDED] || !hist[GAUDI_KEKULE_OK]) return 3;
  }

  std::mt19937 rng(12);
  int hist[9] = {0};
  long calls = 0, graphs = 0;
  for (int it = 0; it < 400; ++it) {
    const int nb_ = 1 + rng() % 6;
    std::vector<Graph> mols;
    for (int k = 0; k < nb_; ++k) {
      const int r = rng() % 16;
      if (r == 0) mols.push_back(Graph{});
      else if (r == 1) mols.push_back(ladder(rng, 2 + rng() % 14, rng() % 2));          // up to 2 x 15: at most 987 structures
      else if (r == 2) mols.push_back(ladder(rng, it % 8 ? 3 : 64 + (int)(rng() % 2), false));  // 128 sel atoms: within the capacity
                                                                                        // and beyond the budget; 130: refused
      else if (r == 3) mols.push_back(acene(1 + rng() % 34));                           // up to 34 hexagons: 33 and 34 are refused
      else if (r == 4) mols.push_back(both(acene(1 + rng() % 3), random_graph(rng, 2 + rng() % 20, 4)));
      else if (r < 10) mols.push_back(random_graph(rng, 1 + rng() % 190, 4));
      else mols.push_back(random_graph(rng, 1 + rng() % 70, (int)(rng() % 4)));
    }
    graphs += nb_;
    int A2, M2;
    std::vector<int32_t> e2, na2, b2, nb2;
    pack(mols, A2, M2, e2, na2, b2, nb2);
    Out o(nb_, M2);
    if (run(vt, nb_, A2, M2, e2, na2, b2, nb2, o)) return 4;
    ++calls;
    if (int bad = check(nb_, A2, M2, na2, nb2, o, hist)) return bad;
  }
  {  // beyond the budget, between two molecules that are not
    std::vector<Graph> mols{acene(3), ladder(rng, 30, false), acene(2)};
    int A2, M2;
    std::vector<int32_t> e2, na2, b2, nb2;
    pack(mols, A2, M2, e2, na2, b2, nb2);
    Out o(3, M2);
    if (run(vt, 3, A2, M2, e2, na2, b2, nb2, o)) return 4;
    if (int bad = check(3, A2, M2, na2, nb2, o, hist)) return bad;
    if (o.st[0] != GAUDI_KEKULE_OK || o.st[1] != GAUDI_KEKULE_UNDECIDED || o.st[2] != GAUDI_KEKULE_OK || o.k[0] != 4 || o.k[2] != 3) return 6;
    ++calls;
    graphs += 3;
  }
  printf("stress: %ld calls, %ld graphs, statuses 0..8: %d %d %d %d %d %d %d %d %d\n", calls, graphs, hist[0], hist[1], hist[2], hist[3],
         hist[4], hist[5], hist[6], hist[7], hist[8]);
  for (int s = 0; s < 9; ++s)
    if (!hist[s]) return 5;  // every status was met
  // a null output: refused, nothing written
  {
    std::vector<Graph> mols(1, acene(1));
    int A2, M2;
    std::vector<int32_t> e2, na2, b2, nb2;
    pack(mols, A2, M2, e2, na2, b2, nb2);
    Out o(1, M2);
    if (gaudi_host_kekule(&vt, 1, A2, M2, e2.data(), na2.data(), b2.data(), nb2.data(), nullptr, o.dc.data(), o.nhex.data(), o.hex.data(),
                          o.sc.data(), o.fries.data(), o.clar.data(), o.nodes.data(), o.st.data()) != GAUDI_E_INVALID)
      return 7;
  }
  printf("done\n");
  return 0;
}
