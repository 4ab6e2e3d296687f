// Stand-alone host program for sanitizer runs of csrc/fp_select.inc (AddressSanitizer + UndefinedBehaviorSanitizer on the HOST
// twins gaudi_host_fp_neighbours, gaudi_host_fp_cluster and gaudi_host_fp_pick_diverse, never on the device and never inside
// python): tools/diversity_host_check.py builds and runs it.  Input: a flat file -- int32 N, n_bins, then rows [N][n_bins] of
// uint8: the fingerprints of the g32 fixture.  It runs the three twins on those rows at the thresholds 0/1, 7/10 and 1/1, with
// and without seeds, then on inputs of their own with EVERY buffer sized exactly (so any access past an array is past the
// allocation): random sparse rows with zero rows and all-255 rows, k = 0 and k beyond N, a first row given, seeds of 1..70 rows,
// and the capacity refusals (no list, a list one entry short, the exact size; more than 2^20 rows; thresholds out of range).
#include <cstdio>
#include <random>
#include <vector>

#include "gaudi_hip.h"

struct Picks {
  std::vector<int32_t> picked, pc, pu, owner, oc, ou;
  int32_t n = 0;
  Picks(int N, int k) : picked(k), pc(k), pu(k), owner(N), oc(N), ou(N) {}
};

static int pick(int n_bins, int N, const uint8_t* rows, int S, const uint8_t* seeds, int first, int k, int num, int den, Picks& P) {
  return gaudi_host_fp_pick_diverse(n_bins, N, rows, S, seeds, first, k, num, den, P.picked.data(), P.pc.data(), P.pu.data(), &P.n,
                                    P.owner.data(), P.oc.data(), P.ou.data());
}

// counts first, then the lists into a buffer of exactly offsets[N] entries; a buffer one entry short must be refused
static int lists(int n_bins, int N, const uint8_t* rows, int num, int den, long long& total) {
  std::vector<int32_t> count(N);
  std::vector<int64_t> off((size_t)N + 1);
  if (int rc = gaudi_host_fp_neighbours(n_bins, N, rows, num, den, count.data(), 0, off.data(), nullptr)) return rc;
  total = N ? off[N] : 0;
  std::vector<int32_t> list((size_t)total);
  if (total > 0) {
    std::vector<int32_t> small((size_t)total - 1);
    if (total > 1 && gaudi_host_fp_neighbours(n_bins, N, rows, num, den, count.data(), total - 1, off.data(), small.data()) != GAUDI_E_CAPACITY)
      return 100;
    if (int rc = gaudi_host_fp_neighbours(n_bins, N, rows, num, den, count.data(), total, off.data(), list.data())) return rc;
    for (int i = 0; i < N; ++i)
      for (int64_t p = off[i]; p < off[i + 1]; ++p)
        if (list[p] < 0 || list[p] >= N || (p > off[i] && list[p] <= list[p - 1])) return 101;
  }
  return 0;
}

static int clusters(int n_bins, int N, const uint8_t* rows, int num, int den, int32_t& n) {
  std::vector<int32_t> cl(N), ce(N), sz(N), co(N);
  if (int rc = gaudi_host_fp_cluster(n_bins, N, rows, num, den, cl.data(), ce.data(), sz.data(), co.data(), &n)) return rc;
  long members = 0, live = 0;
  for (int i = 0; i < N; ++i) {
    members += sz[i];
    live += cl[i] >= 0;
    if (cl[i] >= n || (i < n) != (ce[i] >= 0)) return 102;
  }
  return members == live ? 0 : 103;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  int32_t hdr[2];
  if (!f || fread(hdr, sizeof hdr, 1, f) != 1) return 2;
  const int N = hdr[0], n_bins = hdr[1];
  std::vector<uint8_t> rows((size_t)N * n_bins);
  if (fread(rows.data(), 1, rows.size(), f) != rows.size()) return 2;
  fclose(f);
  const int thr[3][2] = {{0, 1}, {7, 10}, {1, 1}};
  for (auto& t : thr) {
    long long total = 0;
    int32_t n = 0;
    if (int rc = lists(n_bins, N, rows.data(), t[0], t[1], total)) return printf("fixture lists: %d\n", rc), 3;
    if (int rc = clusters(n_bins, N, rows.data(), t[0], t[1], n)) return printf("fixture clusters: %d\n", rc), 3;
    Picks P(N, N + 5), Q(N, 40);
    if (int rc = pick(n_bins, N, rows.data(), 0, nullptr, -1, N + 5, t[0], t[1], P)) return printf("fixture picks: %d\n", rc), 3;
    if (int rc = pick(n_bins, N, rows.data(), 70, rows.data() + (size_t)100 * n_bins, -1, 40, t[0], t[1], Q)) return printf("fixture seeded picks: %d\n", rc), 3;
    printf("fixture thr %d/%d: %lld entries, %d clusters, %d picks of %d asked, %d behind 70 seeds\n", t[0], t[1], total, n, P.n, N + 5, Q.n);
  }

  std::mt19937 rng(17);
  const int bins[3] = {256, 512, 1024};
  long done = 0;
  for (int it = 0; it < 600; ++it) {
    const int nb = bins[it % 3], n = 1 + rng() % 40, num = rng() % 11, den = 10;
    std::vector<uint8_t> r((size_t)n * nb);
    for (auto& v : r) v = rng() % 6 == 0 ? rng() % 256 : 0;
    for (int i = 0; i < n; ++i) {
      if (rng() % 5 == 0) std::fill(r.begin() + (size_t)i * nb, r.begin() + (size_t)(i + 1) * nb, 0);      // zero rows
      if (rng() % 9 == 0) std::fill(r.begin() + (size_t)i * nb, r.begin() + (size_t)(i + 1) * nb, 255);    // the largest totals
      if (i > 0 && rng() % 4 == 0) std::copy(r.begin(), r.begin() + nb, r.begin() + (size_t)i * nb);       // duplicates of row 0
    }
    if (it % 29 == 0) std::fill(r.begin(), r.end(), 0);
    if (it % 31 == 0) std::fill(r.begin(), r.end(), 255);
    long long total = 0;
    int32_t nc = 0;
    if (int rc = lists(nb, n, r.data(), num, den, total)) return printf("stress lists: %d\n", rc), 4;
    if (int rc = clusters(nb, n, r.data(), num, den, nc)) return printf("stress clusters: %d\n", rc), 4;
    const int ks[4] = {0, 1, n, n + 7};
    for (int k : ks) {
      Picks P(n, k);
      if (pick(nb, n, r.data(), 0, nullptr, -1, k, it % 2 ? num : 0, it % 2 ? den : 0, P)) return 4;
      if (P.n > k || P.n > n) return 5;
      const int S = 1 + rng() % 70;
      std::vector<uint8_t> s((size_t)S * nb);
      for (auto& v : s) v = rng() % 6 == 0 ? rng() % 256 : 0;
      if (rng() % 3 == 0) std::fill(s.begin(), s.begin() + nb, 0);
      if (rng() % 3 == 0) std::copy(r.begin(), r.begin() + nb, s.begin() + (size_t)(S - 1) * nb);  // a seed equal to a batch row
      if (pick(nb, n, r.data(), S, s.data(), -1, k, num, den, P)) return 4;
      for (int i = 0; i < n; ++i)
        if (P.owner[i] < -1 - S || P.owner[i] >= n) return 6;
    }
    // a first row: accepted when live, refused otherwise and out of range
    const int first = rng() % n;
    bool live = false;
    for (int b = 0; b < nb; ++b) live |= r[(size_t)first * nb + b] != 0;
    Picks P(n, 3);
    if (pick(nb, n, r.data(), 0, nullptr, first, 3, 0, 0, P) != (live ? GAUDI_OK : GAUDI_E_INVALID)) return 7;
    if (live && P.picked[0] != first) return 7;
    if (pick(nb, n, r.data(), 0, nullptr, n, 3, 0, 0, P) != GAUDI_E_INVALID) return 7;
    ++done;
  }
  printf("stress: %ld batches done\n", done);

  // refusals that must come before any row is read
  {
    uint8_t one[256] = {1};
    int32_t c = 0, n = 0;
    int64_t off[2];
    if (gaudi_host_fp_neighbours(256, (1 << 20) + 1, one, 1, 2, &c, 0, off, nullptr) != GAUDI_E_CAPACITY) return 8;
    if (gaudi_host_fp_cluster(256, (1 << 20) + 1, one, 1, 2, &c, &c, &c, &c, &n) != GAUDI_E_CAPACITY) return 8;
    const int bad[4][2] = {{1, 0}, {2, 1}, {-1, 2}, {1, 65537}};
    for (auto& t : bad)
      if (gaudi_host_fp_neighbours(256, 1, one, t[0], t[1], &c, 0, off, nullptr) != GAUDI_E_INVALID) return 8;
    if (gaudi_host_fp_neighbours(128, 1, one, 1, 2, &c, 0, off, nullptr) != GAUDI_E_INVALID) return 8;
    if (gaudi_host_fp_neighbours(256, 1, one, 1, 2, &c, 3, off, nullptr) != GAUDI_E_INVALID) return 8;
    if (gaudi_host_fp_neighbours(256, 0, nullptr, 1, 2, nullptr, 0, nullptr, nullptr) != GAUDI_OK) return 8;
    Picks P(1, 1);
    if (pick(256, 1, one, 2, nullptr, -1, 1, 0, 0, P) != GAUDI_E_INVALID) return 8;  // seeds missing: no resident library here
    printf("refusals: done\n");
  }
  return 0;
}
