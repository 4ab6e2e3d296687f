// Stand-alone host program for sanitizer runs of csrc/bonds.inc (AddressSanitizer + UndefinedBehaviorSanitizer on the HOST build,
// never on the device and never inside python): tools/bonds_host_check.py builds and runs it.  Input: a flat file holding
// gaudi_valence_tables, then int32 B, A, M, then elem [B][A], n_atoms [B], bonds [B][M][2], n_bonds [B] -- the g32 fixture.
// It runs gaudi_host_bond_orders on that, then on stress inputs of its own: random graphs in exactly-sized buffers (A = n,
// M = m, so any access past a molecule's arrays is past the allocation) with out-of-range elements and indices, repeated
// bonds and full-capacity sizes, and ladders of two-option atoms that drive the subset search to its budget.
#include <cstdio>
#include <random>
#include <vector>

#include "gaudi_hip.h"

static int one(const gaudi_valence_tables& T, std::vector<int32_t>& e, std::vector<int32_t>& bd, int32_t* status, int32_t* n_charged) {
  int32_t n = (int32_t)e.size(), m = (int32_t)bd.size() / 2;
  std::vector<uint8_t> o(m > 0 ? m : 1);
  std::vector<int8_t> q(n);
  if (m == 0) bd.resize(2);
  return gaudi_host_bond_orders(&T, 1, n, m > 0 ? m : 1, e.data(), &n, bd.data(), &m, o.data(), q.data(), n_charged, status);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  gaudi_valence_tables T;
  int32_t hdr[3];
  if (!f || fread(&T, sizeof T, 1, f) != 1 || fread(hdr, sizeof hdr, 1, f) != 1) return 2;
  const int B = hdr[0], A = hdr[1], M = hdr[2];
  std::vector<int32_t> elem((size_t)B * A), na(B), bonds((size_t)B * M * 2), nb(B), nc(B), st(B);
  if (fread(elem.data(), 4, elem.size(), f) != elem.size() || fread(na.data(), 4, B, f) != (size_t)B ||
      fread(bonds.data(), 4, bonds.size(), f) != bonds.size() || fread(nb.data(), 4, B, f) != (size_t)B)
    return 2;
  fclose(f);
  std::vector<uint8_t> order((size_t)B * M);
  std::vector<int8_t> charge((size_t)B * A);
  int rc = gaudi_host_bond_orders(&T, B, A, M, elem.data(), na.data(), bonds.data(), nb.data(), order.data(), charge.data(), nc.data(), st.data());
  int hist[9] = {0};
  for (int b = 0; b < B; ++b) hist[st[b]]++;
  printf("fixture: rc %d, statuses 0..8:", rc);
  for (int k = 0; k < 9; ++k) printf(" %d", hist[k]);
  printf("\n");
  if (rc) return 3;

  std::mt19937 rng(7);
  int hist2[9] = {0};
  for (int it = 0; it < 6000; ++it) {
    const bool full = it % 11 == 0;
    const int n = full ? 384 : 2 + rng() % 60;
    std::vector<int32_t> e(n), bd;
    const int mode = it % 3;  // 0: a tree plus chords of hetero atoms (mostly well-formed); 1: the same with faults; 2: noise
    for (auto& v : e) v = mode == 2 ? (int)(rng() % 7) : (rng() % 3 ? 1 : 2 + (int)(rng() % 4));
    std::vector<int> deg(n, 0);
    if (mode < 2) {
      for (int a = 1; a < n; ++a) {
        int p = rng() % a;
        for (int tries = 0; deg[p] >= 3 && tries < 8; ++tries) p = rng() % a;
        bd.push_back(p); bd.push_back(a); ++deg[p]; ++deg[a];
      }
      for (int k = 0; k < n / 3 && (int)bd.size() / 2 < 384; ++k) {
        const int a = rng() % n, b = rng() % n;
        if (a != b && deg[a] < 3 && deg[b] < 3) { bd.push_back(a); bd.push_back(b); ++deg[a]; ++deg[b]; }
      }
      while ((int)bd.size() / 2 > 384) { bd.pop_back(); bd.pop_back(); }
      for (int a = 0; a < n; ++a) {  // elements that have an option at the atom's degree, so that the search runs
        static const int at2[4] = {1, 3, 4, 5}, at3[3] = {1, 2, 3};
        e[a] = deg[a] <= 1 ? 0 : deg[a] == 2 ? at2[rng() % 4] : deg[a] == 3 ? at3[rng() % 3] : 1;
      }
      if (mode == 1 && !bd.empty()) {
        const int k = rng() % (bd.size() / 2);
        switch (rng() % 4) {
          case 0: bd[2 * k + 1] = n; break;                      // one past the atoms
          case 1: bd[2 * k] = -1; break;
          case 2: bd[2 * k + 1] = bd[2 * k]; break;              // an atom bonded to itself
          default: if (bd.size() / 2 < 384) { bd.push_back(bd[2 * k + 1]); bd.push_back(bd[2 * k]); }  // the same bond twice
        }
      }
    } else {
      const int m = full ? 384 : 1 + rng() % 90;
      for (int k = 0; k < 2 * m; ++k) bd.push_back((int)(rng() % (n + 1)) - (rng() % 50 == 0));
    }
    int32_t s1 = 0, c1 = 0;
    if (one(T, e, bd, &s1, &c1)) return 3;
    hist2[s1]++;
  }
  printf("stress: statuses 0..8:");
  for (int k = 0; k < 9; ++k) printf(" %d", hist2[k]);
  printf("\n");

  for (int n : {24, 60, 192}) {  // B / N ladders between carbon pairs: the subset search, up to its budget
    std::vector<int32_t> e(n), bd;
    for (int k = 0; k < n; ++k) e[k] = (k % 4 == 0 || k % 4 == 3) ? 2 : 3;
    for (int k = 2; k < n - 2; k += 2) { bd.push_back(k); bd.push_back(k + 1); }
    for (int k = 0; k < n - 2; k += 2) { bd.push_back(k); bd.push_back(k + 2); bd.push_back(k + 1); bd.push_back(k + 3); }
    for (int c : {0, 1, n - 2, n - 1}) { e[c] = 1; bd.push_back(c); bd.push_back((int)e.size()); e.push_back(0); }
    int32_t s1 = 0, c1 = 0;
    if (one(T, e, bd, &s1, &c1)) return 3;
    printf("ladder of %d: status %d, n_charged %d\n", n, s1, c1);
  }
  return 0;
}
