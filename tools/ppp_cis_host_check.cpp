// Stand-alone host program for sanitizer runs of csrc/ppp_cis.inc (AddressSanitizer + UndefinedBehaviorSanitizer on the HOST build,
// never on the device and never inside python): tools/ppp_cis_host_check.py builds and runs it.  Input: a flat file -- the bytes of
// a gaudi_ppp_tables, then two batches, each int32 B, A, M, then elem [B][A], n_atoms [B], bonds [B][M][2], n_bonds [B],
// xyz [B][A][3] float32 and charge [B]: the molecules of the g30 fixture and the tier-edge set.  It runs gaudi_host_ppp_cis on
// either batch as packed, under charges 0 and +-2 (added to the batch's own) and windows 1, 3 and 8, then on every molecule alone
// in exactly-sized buffers (A = n, M = m, every output sized exactly, so any access past an array is past its allocation), then
// with windows that must be refused, and checks that what a call writes is consistent with what it says.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gaudi_hip.h"

constexpr int kS = GAUDI_PPP_CIS_MAX_STATES;

struct Batch {
  int B = 0, A = 0, M = 0;
  std::vector<int32_t> elem, na, bonds, nb, charge;
  std::vector<float> xyz;
};

struct Out {
  std::vector<float> levels, q, p, homo, lumo, gap, e_el, e_core, dp, singlet, triplet, osc, dipole, weight;
  std::vector<uint8_t> occ, lead;
  std::vector<int8_t> site;
  std::vector<int32_t> n_pi, n_el, n_exc, iters, sweeps, flags, status, n_states, n_o, n_v, cis_sweeps;
  Out(int B, int A, int M)
      : levels((size_t)B * 128, 7.f), q((size_t)B * A, 7.f), p((size_t)B * M, 7.f), homo(B, 7.f), lumo(B, 7.f), gap(B, 7.f), e_el(B, 7.f),
        e_core(B, 7.f), dp(B, 7.f), singlet((size_t)B * kS, 7.f), triplet((size_t)B * kS, 7.f), osc((size_t)B * kS, 7.f),
        dipole((size_t)B * kS * 3, 7.f), weight((size_t)B * kS, 7.f), occ((size_t)B * 128, 7), lead((size_t)B * kS * 2, 7),
        site((size_t)B * A, 7), n_pi(B, 7), n_el(B, 7), n_exc(B, 7), iters(B, 7), sweeps(B, 7), flags(B, 7), status(B, 7), n_states(B, 7),
        n_o(B, 7), n_v(B, 7), cis_sweeps(B, 7) {}
};

static int run(const gaudi_ppp_tables& t, int B, int A, int M, const int32_t* elem, const int32_t* na, const int32_t* bonds,
               const int32_t* nb, const float* xyz, const int32_t* charge, int repulsion, int window, Out& o) {
  return gaudi_host_ppp_cis(&t, B, A, M, elem, na, bonds, nb, xyz, charge, repulsion, 0.25f, o.levels.data(), o.occ.data(), o.q.data(),
                            o.p.data(), o.site.data(), o.n_pi.data(), o.n_el.data(), o.n_exc.data(), o.iters.data(), o.sweeps.data(),
                            o.flags.data(), o.status.data(), o.homo.data(), o.lumo.data(), o.gap.data(), o.e_el.data(), o.e_core.data(),
                            o.dp.data(), window, o.singlet.data(), o.triplet.data(), o.osc.data(), o.dipole.data(), o.lead.data(),
                            o.weight.data(), o.n_states.data(), o.n_o.data(), o.n_v.data(), o.cis_sweeps.data());
}

// what a call writes must be consistent with what it says; counts[0] solved with states, [1] without, [2] refused or not converged
static int check(int B, int window, const Out& o, int counts[3]) {
  for (int b = 0; b < B; ++b) {
    const int st = o.status[b], D = o.n_states[b], n = o.n_pi[b], n_occ = o.n_el[b] / 2;
    if (st < 0 || st > 8 || D < 0 || D > kS) return 10;
    if (st != GAUDI_HUCKEL_OK && (D || o.n_o[b] || o.n_v[b] || o.cis_sweeps[b] || (o.flags[b] & ~14))) return 11;
    if (st == GAUDI_HUCKEL_OK) {
      const int n_o = n_occ < window ? n_occ : window, n_v = n - n_occ < window ? n - n_occ : window;
      if (o.n_o[b] != n_o || o.n_v[b] != n_v || D != n_o * n_v) return 12;
      if (((o.flags[b] & GAUDI_PPP_CIS_TRUNCATED) != 0) != (D < n_occ * (n - n_occ))) return 13;
      if (o.flags[b] & GAUDI_PPP_CIS_JACOBI_CAP) return 14;
      if (D && ((o.flags[b] & GAUDI_PPP_CIS_TRIPLET_UNSTABLE) != 0) != (o.triplet[(size_t)b * kS] <= 0.f)) return 15;
      if (o.cis_sweeps[b] < 0 || o.cis_sweeps[b] > 2 * GAUDI_HUCKEL_MAX_SWEEPS) return 16;
    }
    for (int k = 0; k < kS; ++k) {
      const size_t at = (size_t)b * kS + k;
      const float s = o.singlet[at], t = o.triplet[at], f = o.osc[at], w = o.weight[at];
      if (!std::isfinite(s) || !std::isfinite(t) || !std::isfinite(f) || !std::isfinite(w)) return 20;
      for (int c = 0; c < 3; ++c)
        if (!std::isfinite(o.dipole[at * 3 + c]) || (k >= D && o.dipole[at * 3 + c] != 0.f)) return 21;
      if (k >= D && (s != 0.f || t != 0.f || f != 0.f || w != 0.f || o.lead[at * 2] || o.lead[at * 2 + 1])) return 22;
      if (k < D) {
        if (k > 0 && (s < o.singlet[at - 1] || t < o.triplet[at - 1])) return 23;
        if (!(w > 0.f && w <= 1.0001f) || t > s + 1e-3f) return 24;
        const int i = o.lead[at * 2], a = o.lead[at * 2 + 1];
        if (i < n_occ - o.n_o[b] || i >= n_occ || a < n_occ || a >= n_occ + o.n_v[b]) return 25;
      }
    }
    counts[st != GAUDI_HUCKEL_OK ? 2 : D ? 0 : 1]++;
  }
  return 0;
}

static bool read_batch(FILE* f, Batch& g) {
  int32_t head[3];
  if (fread(head, sizeof(int32_t), 3, f) != 3) return false;
  g.B = head[0], g.A = head[1], g.M = head[2];
  g.elem.resize((size_t)g.B * g.A), g.na.resize(g.B), g.bonds.resize((size_t)g.B * g.M * 2), g.nb.resize(g.B), g.charge.resize(g.B);
  g.xyz.resize((size_t)g.B * g.A * 3);
  return fread(g.elem.data(), 4, g.elem.size(), f) == g.elem.size() && fread(g.na.data(), 4, g.B, f) == (size_t)g.B &&
         fread(g.bonds.data(), 4, g.bonds.size(), f) == g.bonds.size() && fread(g.nb.data(), 4, g.B, f) == (size_t)g.B &&
         fread(g.xyz.data(), 4, g.xyz.size(), f) == g.xyz.size() && fread(g.charge.data(), 4, g.B, f) == (size_t)g.B;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  gaudi_ppp_tables t;
  Batch batch[2];
  if (fread(&t, sizeof(t), 1, f) != 1 || !read_batch(f, batch[0]) || !read_batch(f, batch[1])) return 2;
  fclose(f);
  const int windows[3] = {1, 3, 8};
  int packed[3] = {0}, alone[3] = {0};
  for (int k = 0; k < 2; ++k) {
    const Batch& g = batch[k];
    for (int extra = -2; extra <= 2; extra += 2)
      for (int w = 0; w < 3; ++w) {
        if (k == 1 && extra && w != 2) continue;  // (the 128-centre molecules are slow here: the charged edge set at window 8 only)
        std::vector<int32_t> ch(g.charge);
        for (auto& c : ch) c += extra;
        Out o(g.B, g.A, g.M);
        if (run(t, g.B, g.A, g.M, g.elem.data(), g.na.data(), g.bonds.data(), g.nb.data(), g.xyz.data(), ch.data(), (extra + w) & 1,
                windows[w], o))
          return 3;
        if (int rc = check(g.B, windows[w], o, packed)) return rc;
      }
    // every molecule alone in exactly-sized buffers
    for (int b = 0; b < g.B; ++b) {
      const int n = g.na[b], m = g.nb[b];
      if (n == 0 || (k == 1 && n > 70)) continue;  // (the large edge molecules ran exactly sized enough above: B = 12, A = their own)
      const int A = n, M = m > 0 ? m : 1;
      std::vector<int32_t> e(g.elem.begin() + (size_t)b * g.A, g.elem.begin() + (size_t)b * g.A + n), bo((size_t)M * 2, 0);
      std::vector<float> x(g.xyz.begin() + (size_t)b * g.A * 3, g.xyz.begin() + ((size_t)b * g.A + n) * 3);
      memcpy(bo.data(), g.bonds.data() + (size_t)b * g.M * 2, sizeof(int32_t) * 2 * m);
      const int32_t na = n, nb = m, ch = g.charge[b];
      const int w = windows[b % 3];
      Out o(1, A, M);
      if (run(t, 1, A, M, e.data(), &na, bo.data(), &nb, x.data(), &ch, b & 1, w, o)) return 4;
      if (int rc = check(1, w, o, alone)) return 100 + rc;
    }
  }
  // windows that must be refused: every molecule BAD_TABLE and nothing else written
  for (int window : {0, 9, -3}) {
    const Batch& g = batch[0];
    Out o(g.B, g.A, g.M);
    if (run(t, g.B, g.A, g.M, g.elem.data(), g.na.data(), g.bonds.data(), g.nb.data(), g.xyz.data(), nullptr, 0, window, o)) return 5;
    for (int b = 0; b < g.B; ++b)
      if (o.status[b] != GAUDI_HUCKEL_BAD_TABLE || o.n_states[b] || o.flags[b] || o.n_pi[b]) return 6;
    for (float v : o.singlet)
      if (v != 0.f) return 7;
  }
  printf("packed: with states %d, without %d, refused or not converged %d\n", packed[0], packed[1], packed[2]);
  printf("alone, exactly sized: with states %d, without %d, refused or not converged %d\n", alone[0], alone[1], alone[2]);
  return packed[0] > 1000 && alone[0] > 150 && packed[2] > 10 ? 0 : 8;
}
