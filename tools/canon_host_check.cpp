// Stand-alone host program for sanitizer runs of csrc/canon.inc (AddressSanitizer + UndefinedBehaviorSanitizer on the HOST build,
// never on the device and never inside python): tools/canon_host_check.py builds and runs it.  Input: a flat file holding int32
// n_elems, h_elem, c_elem, B, A, M, then elem [B][A], n_atoms [B], bonds [B][M][2], n_bonds [B] -- the g32 fixture.
// It runs gaudi_host_canonical_order on that, then on inputs of its own: random graphs in exactly-sized buffers (A = n, M = m,
// so any access past a molecule's arrays is past the allocation) with out-of-range elements and indices, repeated bonds,
// degrees up to and beyond 8 and full-capacity sizes; and the symmetric graphs whose search trees are the large ones -- rings,
// disjoint rings up to the node cap, the cube, Petersen, Heawood, the dodecahedron, K3,3 and a star whose tree hits the depth.
#include <cstdio>
#include <random>
#include <vector>

#include "gaudi_hip.h"

struct Out {
  int32_t status = 0, nodes = 0, n_heavy = 0, n_hbonds = 0;
};

static int one(int n_elems, std::vector<int32_t>& e, std::vector<int32_t>& bd, Out& o) {
  int32_t n = (int32_t)e.size(), m = (int32_t)bd.size() / 2;
  const int A = n > 0 ? n : 1, M = m > 0 ? m : 1;
  std::vector<int32_t> rank(A);
  std::vector<uint8_t> label(A);
  std::vector<uint16_t> cb((size_t)M * 2);
  if (n == 0) e.resize(1);
  if (m == 0) bd.resize(2);
  return gaudi_host_canonical_order(n_elems, 0, 1, 1, A, M, e.data(), &n, bd.data(), &m, rank.data(), &o.n_heavy, label.data(),
                                    &o.n_hbonds, cb.data(), &o.nodes, &o.status);
}

static int carbons(const char* name, int n, const std::vector<int32_t>& edges) {
  std::vector<int32_t> e(n, 1), bd(edges);
  Out o;
  if (one(6, e, bd, o)) return 1;
  printf("%s: status %d, nodes %d\n", name, o.status, o.nodes);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  int32_t hdr[6];
  if (!f || fread(hdr, sizeof hdr, 1, f) != 1) return 2;
  const int n_elems = hdr[0], B = hdr[3], A = hdr[4], M = hdr[5];
  std::vector<int32_t> elem((size_t)B * A), na(B), bonds((size_t)B * M * 2), nb(B);
  if (fread(elem.data(), 4, elem.size(), f) != elem.size() || fread(na.data(), 4, B, f) != (size_t)B ||
      fread(bonds.data(), 4, bonds.size(), f) != bonds.size() || fread(nb.data(), 4, B, f) != (size_t)B)
    return 2;
  fclose(f);
  std::vector<int32_t> rank((size_t)B * A), nh(B), ne(B), nodes(B), st(B);
  std::vector<uint8_t> label((size_t)B * A);
  std::vector<uint16_t> cb((size_t)B * M * 2);
  int rc = gaudi_host_canonical_order(n_elems, hdr[1], hdr[2], B, A, M, elem.data(), na.data(), bonds.data(), nb.data(), rank.data(),
                                      nh.data(), label.data(), ne.data(), cb.data(), nodes.data(), st.data());
  int hist[5] = {0}, most = 0;
  for (int b = 0; b < B; ++b) {
    hist[st[b]]++;
    most = nodes[b] > most ? nodes[b] : most;
  }
  printf("fixture: rc %d, statuses 0..4:", rc);
  for (int k = 0; k < 5; ++k) printf(" %d", hist[k]);
  printf(", most nodes %d\n", most);
  if (rc) return 3;

  std::mt19937 rng(7);
  int hist2[5] = {0};
  for (int it = 0; it < 4000; ++it) {
    const bool full = it % 11 == 0;
    const int n = full ? 384 : 1 + rng() % 60;
    std::vector<int32_t> e(n), bd;
    const int mode = it % 4;  // 0: a tree plus chords; 1: the same with faults; 2: noise; 3: few atoms, many bonds (high degrees)
    for (auto& v : e) v = mode == 2 ? (int)(rng() % 7) : (full ? (rng() % 2 ? 1 : 0) : (int)(rng() % 6));
    if (mode < 2) {
      for (int a = 1; a < n; ++a) { bd.push_back(rng() % a); bd.push_back(a); }
      for (int k = 0; k < n / 3 && (int)bd.size() / 2 < 384; ++k) {
        const int a = rng() % n, b = rng() % n;
        if (a != b) { bd.push_back(a); bd.push_back(b); }  // (may repeat a bond: BAD_INPUT)
      }
      while ((int)bd.size() / 2 > 384) { bd.pop_back(); bd.pop_back(); }
      if (mode == 1 && !bd.empty()) {
        const int k = rng() % (bd.size() / 2);
        switch (rng() % 4) {
          case 0: bd[2 * k + 1] = n; break;                      // one past the atoms
          case 1: bd[2 * k] = -1; break;
          case 2: bd[2 * k + 1] = bd[2 * k]; break;              // an atom bonded to itself
          default: if (bd.size() / 2 < 384) { bd.push_back(bd[2 * k + 1]); bd.push_back(bd[2 * k]); }  // the same bond twice
        }
      }
    } else if (mode == 2) {
      const int m = full ? 384 : 1 + rng() % 90;
      for (int k = 0; k < 2 * m; ++k) bd.push_back((int)(rng() % (n + 1)) - (rng() % 50 == 0));
    } else {
      const int k = n < 12 ? n : 12;
      for (int a = 0; a < k; ++a)
        for (int b = 0; b < a; ++b)
          if (rng() % 3) { bd.push_back(a); bd.push_back(b); }
    }
    Out o;
    if (one(6, e, bd, o)) return 3;
    hist2[o.status]++;
  }
  printf("stress: statuses 0..4:");
  for (int k = 0; k < 5; ++k) printf(" %d", hist2[k]);
  printf("\n");

  // full capacity, every label alike: a ring of 192 carbons, and 32 disjoint six-rings (the node cap)
  std::vector<int32_t> ring;
  for (int a = 0; a < 192; ++a) { ring.push_back(a); ring.push_back((a + 1) % 192); }
  if (carbons("ring of 192", 192, ring)) return 3;
  for (int k : {1, 2, 3, 32}) {
    std::vector<int32_t> bz;
    for (int r = 0; r < k; ++r)
      for (int a = 0; a < 6; ++a) { bz.push_back(6 * r + a); bz.push_back(6 * r + (a + 1) % 6); }
    char name[32];
    snprintf(name, sizeof name, "%d six-rings", k);
    if (carbons(name, 6 * k, bz)) return 3;
  }
  std::vector<int32_t> g;
  for (int a = 0; a < 8; ++a)
    for (int k = 0; k < 3; ++k)
      if (a < (a ^ (1 << k))) { g.push_back(a); g.push_back(a ^ (1 << k)); }
  if (carbons("cube", 8, g)) return 3;
  g.clear();
  for (int a = 0; a < 5; ++a) {
    g.insert(g.end(), {a, (a + 1) % 5, a, a + 5, a + 5, (a + 2) % 5 + 5});
  }
  if (carbons("petersen", 10, g)) return 3;
  g.clear();
  for (int a = 0; a < 14; ++a) {
    g.push_back(a); g.push_back((a + 1) % 14);
    if (a % 2 == 0) { g.push_back(a); g.push_back((a + 5) % 14); }
  }
  if (carbons("heawood", 14, g)) return 3;
  g.clear();
  for (int a = 0; a < 5; ++a) {  // the dodecahedron: two five-rings joined through a ten-ring
    g.insert(g.end(), {a, (a + 1) % 5, a, 5 + 2 * a, 15 + a, 15 + (a + 1) % 5, 15 + a, 6 + 2 * a});
    g.insert(g.end(), {5 + 2 * a, 6 + 2 * a, 6 + 2 * a, 5 + (2 * a + 2) % 10});
  }
  if (carbons("dodecahedron", 20, g)) return 3;
  g.clear();
  for (int a = 0; a < 3; ++a)
    for (int b = 3; b < 6; ++b) { g.push_back(a); g.push_back(b); }
  if (carbons("k33", 6, g)) return 3;
  g.clear();
  for (int a = 1; a <= 8; ++a) { g.push_back(0); g.push_back(a); }
  if (carbons("star of 8", 9, g)) return 3;
  g.clear();
  for (int a = 0; a < 20; ++a) { g.push_back(2 * a); g.push_back(2 * a + 1); }  // 20 disjoint pairs: the depth cap
  if (carbons("20 pairs", 40, g)) return 3;
  return 0;
}
