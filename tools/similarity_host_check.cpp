// Stand-alone host program for sanitizer runs of csrc/fp.inc (AddressSanitizer + UndefinedBehaviorSanitizer on the HOST builds,
// never on the device and never inside python): tools/similarity_host_check.py builds and runs it.  Input: the flat file of
// tools/canon_host_check.cpp -- int32 n_elems, h_elem, c_elem, B, A, M, then elem [B][A], n_atoms [B], bonds [B][M][2],
// n_bonds [B]: the g32 fixture.  It runs gaudi_host_circular_fingerprint on that at every (radius, n_bins), then
// gaudi_host_fp_nearest with the rows as queries and library at k = 1, 5 and 16, then both on inputs of their own: random graphs in
// exactly-sized buffers (A = n, M = m, so any access past a molecule's arrays is past the allocation) with out-of-range elements
// and indices, repeated bonds and high degrees; full-capacity stars that saturate bins; and libraries of 1..5 rows with zero
// rows and k beyond M, every output buffer sized exactly.
#include <cstdio>
#include <random>
#include <vector>

#include "gaudi_hip.h"

static int one(std::vector<int32_t>& e, std::vector<int32_t>& bd, int radius, int n_bins, int32_t& status, int32_t& total) {
  int32_t n = (int32_t)e.size(), m = (int32_t)bd.size() / 2;
  const int A = n > 0 ? n : 1, M = m > 0 ? m : 1;
  if (n == 0) e.resize(1);
  if (m == 0) bd.resize(2);
  std::vector<uint8_t> fp(n_bins);
  const int rc = gaudi_host_circular_fingerprint(6, 0, 1, 1, A, M, e.data(), &n, bd.data(), &m, radius, n_bins, fp.data(), &total, &status);
  long sum = 0;
  for (uint8_t v : fp) sum += v;
  return rc ? rc : (sum == total ? 0 : 100);
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
  const int bins[3] = {256, 512, 1024};
  std::vector<uint8_t> rows;
  for (int radius = 0; radius <= 3; ++radius)
    for (int n_bins : bins) {
      std::vector<uint8_t> fp((size_t)B * n_bins);
      std::vector<int32_t> total(B), st(B);
      const int rc = gaudi_host_circular_fingerprint(n_elems, hdr[1], hdr[2], B, A, M, elem.data(), na.data(), bonds.data(), nb.data(),
                                                     radius, n_bins, fp.data(), total.data(), st.data());
      int hist[5] = {0}, most = 0;
      for (int b = 0; b < B; ++b) hist[st[b]]++;
      for (uint8_t v : fp) most = v > most ? v : most;
      printf("fixture radius %d bins %4d: rc %d, statuses 0..4: %d %d %d %d %d, largest count %d\n", radius, n_bins, rc, hist[0], hist[1],
             hist[2], hist[3], hist[4], most);
      if (rc) return 3;
      if (radius == 2 && n_bins == 256) rows = fp;
    }
  for (int k : {1, 5, 16}) {
    std::vector<int32_t> idx((size_t)B * k), co((size_t)B * k), un((size_t)B * k);
    const int rc = gaudi_host_fp_nearest(256, B, rows.data(), B, rows.data(), k, idx.data(), co.data(), un.data());
    int self = 0;
    for (int b = 0; b < B; ++b) self += co[(size_t)b * k] == un[(size_t)b * k];
    printf("nearest k %2d: rc %d, %d of %d queries with a row at similarity 1 (or 0 / 0)\n", k, rc, self, B);
    if (rc) return 3;
  }

  std::mt19937 rng(11);
  int hist2[5] = {0};
  for (int it = 0; it < 3000; ++it) {
    const bool full = it % 13 == 0;
    const int n = full ? 384 : 1 + rng() % 60;
    std::vector<int32_t> e(n), bd;
    const int mode = it % 4;  // 0: a tree plus chords; 1: the same with faults; 2: noise; 3: few atoms, many bonds (high degrees)
    for (auto& v : e) v = mode == 2 ? (int)(rng() % 7) : (full ? (rng() % 2 ? 1 : 0) : (int)(rng() % 6));
    if (mode < 2) {
      for (int a = 1; a < n; ++a) { bd.push_back(rng() % a); bd.push_back(a); }
      for (int k = 0; k < n / 3 && (int)bd.size() / 2 < 384; ++k) {
        const int a = rng() % n, b = rng() % n;
        if (a != b) { bd.push_back(a); bd.push_back(b); }
      }
      while ((int)bd.size() / 2 > 384) { bd.pop_back(); bd.pop_back(); }
      if (mode == 1 && !bd.empty()) {
        const int k = rng() % (bd.size() / 2);
        switch (rng() % 3) {
          case 0: bd[2 * k + 1] = n; break;
          case 1: bd[2 * k] = -1; break;
          default: bd[2 * k + 1] = bd[2 * k]; break;
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
    int32_t st = 0, total = 0;
    if (one(e, bd, it % 4, bins[it % 3], st, total)) return 3;
    if (st != 0 && total != 0) return 4;
    hist2[st]++;
  }
  printf("stress: statuses 0..4: %d %d %d %d %d\n", hist2[0], hist2[1], hist2[2], hist2[3], hist2[4]);

  // full capacity, every leaf alike: 38 stars of a centre with four leaves, and 192 lone atoms (three of four ids in 256 bins)
  {
    std::vector<int32_t> e, bd;
    for (int s = 0; s < 38; ++s) {
      const int c = (int)e.size();
      e.push_back(3);
      for (int l = 0; l < 4; ++l) { e.push_back(2); bd.push_back(c); bd.push_back((int)e.size() - 1); }
    }
    int32_t st = 0, total = 0;
    if (one(e, bd, 3, 256, st, total)) return 3;
    printf("38 stars: status %d, total %d of %d features\n", st, total, 190 * 4);
    std::vector<int32_t> lone(192, 1), none;
    if (one(lone, none, 3, 256, st, total)) return 3;
    printf("192 lone carbons: status %d, total %d of %d features\n", st, total, 192 * 4);
  }

  // small libraries, exact buffers
  for (int it = 0; it < 400; ++it) {
    const int n_bins = bins[it % 3], Bq = 1 + rng() % 4, Ml = 1 + rng() % 5, k = 1 + rng() % 16;
    std::vector<uint8_t> q((size_t)Bq * n_bins), lib((size_t)Ml * n_bins);
    for (auto& v : q) v = rng() % 5 == 0 ? rng() % 256 : 0;
    for (auto& v : lib) v = rng() % 5 == 0 ? rng() % 256 : 0;
    if (it % 7 == 0) std::fill(q.begin(), q.begin() + n_bins, 0);
    if (it % 5 == 0) std::fill(lib.begin(), lib.begin() + n_bins, 0);
    if (it % 11 == 0) std::fill(lib.begin(), lib.end(), 255);  // the largest totals: common * union needs 64 bits
    if (it % 11 == 0) std::fill(q.begin(), q.end(), 255);
    std::vector<int32_t> idx((size_t)Bq * k), co((size_t)Bq * k), un((size_t)Bq * k);
    if (gaudi_host_fp_nearest(n_bins, Bq, q.data(), Ml, lib.data(), k, idx.data(), co.data(), un.data())) return 3;
    for (int b = 0; b < Bq; ++b)
      for (int j = 0; j < k; ++j)
        if ((j < Ml) != (idx[(size_t)b * k + j] >= 0)) return 5;
  }
  printf("small libraries: done\n");
  return 0;
}
