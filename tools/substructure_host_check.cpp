// Stand-alone host program for sanitizer runs of csrc/sub.inc (AddressSanitizer + UndefinedBehaviorSanitizer on the HOST build,
// never on the device and never inside python): tools/substructure_host_check.py builds and runs it.  Input: the flat file of
// tools/canon_host_check.cpp -- int32 n_elems, h_elem, c_elem, B, A, M, then elem [B][A], n_atoms [B], bonds [B][M][2],
// n_bonds [B]: the g32 fixture -- followed by the named patterns of tests/substructure_helpers.py in the same layout: int32 P, QA,
// QM, then p_elem [P][QA], p_n_atoms [P], p_bonds [P][QM][2], p_n_bonds [P].  It runs gaudi_host_substructure_search on the
// fixture under the four flag settings, then on inputs of its own in exactly-sized buffers (A = n, M = m, QA, QM likewise, every
// output sized exactly, so any access past an array is past its allocation): random graphs with out-of-range elements and
// indices, repeated bonds and degree-8 vertices as molecules AND as patterns, 32- and 33-vertex patterns, refused patterns, P
// from 1 to 64, well-formed random molecules of up to 190 atoms against well-formed random patterns of up to 32, and calls without
// first / covered.
#include <cstdio>
#include <random>
#include <vector>

#include "gaudi_hip.h"

struct Graph {
  std::vector<int32_t> e, b;
};

// what a call writes must be consistent with what it says
static int check(int B, int P, int A, int QA, const std::vector<int32_t>& count, const std::vector<int32_t>& first,
                 const std::vector<uint8_t>& covered, const std::vector<int32_t>& steps, const std::vector<int32_t>& st, int hist[6]) {
  for (int c = 0; c < B * P; ++c) {
    if (st[c] < 0 || st[c] > 5) return 10;
    hist[st[c]]++;
    int cov = 0, set = 0;
    for (int a = 0; a < A; ++a) cov += covered[(size_t)c * A + a];
    for (int a = 0; a < QA; ++a) {
      const int v = first[(size_t)c * QA + a];
      if (v < -1 || v >= A) return 11;
      set += v >= 0;
    }
    if (st[c] > GAUDI_SUB_GAVE_UP && (count[c] || steps[c] || cov || set)) return 12;
    if ((count[c] > 0) != (set > 0) || (count[c] > 0) != (cov > 0) || count[c] < 0 || steps[c] < 0) return 13;
    if (set > cov) return 14;
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
  } else if (mode == 5) {  // well-formed and connected: mostly carbon, a tree plus chords, no bond twice
    for (auto& v : g.e) v = rng() % 5 ? 1 : 2 + (int)(rng() % 4);
    std::vector<char> seen((size_t)n * n, 0);
    for (int a = 1; a < n; ++a) {
      const int c = rng() % a;
      seen[(size_t)a * n + c] = seen[(size_t)c * n + a] = 1;
      g.b.push_back(c);
      g.b.push_back(a);
    }
    for (int k = 0; k < n / 2; ++k) {
      const int a = rng() % n, c = rng() % n;
      if (a == c || seen[(size_t)a * n + c]) continue;
      seen[(size_t)a * n + c] = seen[(size_t)c * n + a] = 1;
      g.b.push_back(a);
      g.b.push_back(c);
    }
  } else {  // a path: connected, every size a pattern may have and one more
    for (int a = 1; a < n; ++a) { g.b.push_back(a - 1); g.b.push_back(a); }
    for (auto& v : g.e) v = 1;
  }
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
  int32_t hdr[6], ph[3];
  if (!f || fread(hdr, sizeof hdr, 1, f) != 1) return 2;
  const int n_elems = hdr[0], B = hdr[3], A = hdr[4], M = hdr[5];
  std::vector<int32_t> elem((size_t)B * A), na(B), bonds((size_t)B * M * 2), nb(B);
  if (fread(elem.data(), 4, elem.size(), f) != elem.size() || fread(na.data(), 4, B, f) != (size_t)B ||
      fread(bonds.data(), 4, bonds.size(), f) != bonds.size() || fread(nb.data(), 4, B, f) != (size_t)B)
    return 2;
  if (fread(ph, sizeof ph, 1, f) != 1) return 2;
  const int P = ph[0], QA = ph[1], QM = ph[2];
  std::vector<int32_t> pe((size_t)P * QA), pna(P), pb((size_t)P * QM * 2), pnb(P);
  if (fread(pe.data(), 4, pe.size(), f) != pe.size() || fread(pna.data(), 4, P, f) != (size_t)P ||
      fread(pb.data(), 4, pb.size(), f) != pb.size() || fread(pnb.data(), 4, P, f) != (size_t)P)
    return 2;
  fclose(f);

  (void)gaudi_host_substructure_root_steps(1);
  for (int flags = 0; flags < 4; ++flags) {
    const size_t cells = (size_t)B * P;
    std::vector<int32_t> fl(P, flags), count(cells), first(cells * QA), steps(cells), st(cells);
    std::vector<uint8_t> covered(cells * A);
    const int rc = gaudi_host_substructure_search(n_elems, hdr[1], hdr[2], B, A, M, elem.data(), na.data(), bonds.data(), nb.data(), P, QA,
                                                  QM, pe.data(), pna.data(), pb.data(), pnb.data(), fl.data(), count.data(), first.data(),
                                                  covered.data(), steps.data(), st.data());
    int hist[6] = {0};
    long hits = 0;
    for (int32_t c : count) hits += c > 0;
    const int bad = rc ? rc : check(B, P, A, QA, count, first, covered, steps, st, hist);
    printf("fixture flags %d: rc %d, statuses 0..5: %d %d %d %d %d %d, %ld cells with a hit\n", flags, bad, hist[0], hist[1], hist[2],
           hist[3], hist[4], hist[5], hits);
    if (bad || hist[GAUDI_SUB_GAVE_UP] || hist[GAUDI_SUB_BAD_PATTERN]) return 3;
  }
  printf("fixture: the largest per-root step count %d, the cap %d\n", gaudi_host_substructure_root_steps(1), GAUDI_SUB_MAX_STEPS);

  std::mt19937 rng(12);
  int hist[6] = {0};
  long calls = 0, graphs = 0;
  for (int it = 0; it < 600; ++it) {
    const int nb_ = 1 + rng() % 6, np_ = it % 40 == 0 ? 64 : 1 + rng() % 5;
    std::vector<Graph> mols, pats;
    for (int k = 0; k < nb_; ++k) {
      const int r = rng() % 16;
      mols.push_back(r == 0 ? Graph{} : r == 1 ? random_graph(rng, 192 + (int)(rng() % 3), 4) : r < 10 ? random_graph(rng, 1 + rng() % 190, 5)
                                                                                                 : random_graph(rng, 1 + rng() % 70, (int)(rng() % 4)));
    }
    for (int k = 0; k < np_; ++k) {
      const int r = rng() % 12;
      if (r == 0) pats.push_back(Graph{});
      else if (r == 1) pats.push_back(random_graph(rng, 32 + (int)(rng() % 2), 4));      // 32 vertices: taken; 33: refused
      else if (r == 2) pats.push_back(random_graph(rng, 2 + rng() % 30, 2));             // noise: refused
      else if (r == 3) pats.push_back(random_graph(rng, 9, 3));                          // degree up to 8
      else if (r == 4) pats.push_back(random_graph(rng, 1 + rng() % 9, (int)(rng() % 2)));
      else pats.push_back(random_graph(rng, 1 + rng() % (r == 5 ? 32 : 8), 5));
    }
    graphs += nb_ + np_;
    int A2, M2, QA2, QM2;
    std::vector<int32_t> e2, na2, b2, nb2, pe2, pna2, pb2, pnb2, fl(np_);
    pack(mols, A2, M2, e2, na2, b2, nb2);
    pack(pats, QA2, QM2, pe2, pna2, pb2, pnb2);
    for (auto& v : fl) v = rng() % 20 == 0 ? 4 : (int)(rng() % 4);
    const size_t cells = (size_t)nb_ * np_;
    std::vector<int32_t> count(cells), first(cells * QA2), steps(cells), st(cells);
    std::vector<uint8_t> covered(cells * A2);
    const bool lean = it % 5 == 0;
    const int rc = gaudi_host_substructure_search(7, 0, 1, nb_, A2, M2, e2.data(), na2.data(), b2.data(), nb2.data(), np_, QA2, QM2,
                                                  pe2.data(), pna2.data(), pb2.data(), pnb2.data(), fl.data(), count.data(),
                                                  lean ? nullptr : first.data(), lean ? nullptr : covered.data(), steps.data(), st.data());
    if (rc) return 4;
    ++calls;
    if (!lean) {
      if (int bad = check(nb_, np_, A2, QA2, count, first, covered, steps, st, hist)) return bad;
    } else {
      for (int32_t s : st) hist[s]++;
    }
  }
  printf("stress: %ld calls, %ld graphs, statuses 0..5: %d %d %d %d %d %d\n", calls, graphs, hist[0], hist[1], hist[2], hist[3], hist[4],
         hist[5]);
  for (int s = 0; s < 6; ++s)
    if (!hist[s]) return 5;  // every status was met
  // 65 patterns: refused whole, nothing written
  {
    std::vector<Graph> mols(1, random_graph(rng, 10, 4)), pats(65, random_graph(rng, 3, 4));
    int A2, M2, QA2, QM2;
    std::vector<int32_t> e2, na2, b2, nb2, pe2, pna2, pb2, pnb2, fl(65, 0), out(65);
    pack(mols, A2, M2, e2, na2, b2, nb2);
    pack(pats, QA2, QM2, pe2, pna2, pb2, pnb2);
    if (gaudi_host_substructure_search(6, 0, 1, 1, A2, M2, e2.data(), na2.data(), b2.data(), nb2.data(), 65, QA2, QM2, pe2.data(),
                                       pna2.data(), pb2.data(), pnb2.data(), fl.data(), out.data(), nullptr, nullptr, out.data(),
                                       out.data()) != GAUDI_E_CAPACITY)
      return 6;
  }
  printf("done\n");
  return 0;
}
