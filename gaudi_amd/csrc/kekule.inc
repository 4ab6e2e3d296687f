// kekule.inc -- all Kekule structures of a graph of atoms on the device (included after ppp_cis.inc at the end of gaudi_hip.hip).
//
// bonds.inc returns ONE Kekule structure, whichever its matching finds.  This file enumerates them all and returns what the
// classical descriptors of a polycyclic aromatic system are made of (DESIGN.md section 8o): their number K, for every bond the
// number of structures in which it is double (the Pauling bond order is that over K), the hexagons, for every hexagon the number
// of structures in which it is a sextet, the Fries number and the Clar number.  Atoms, bonds, the sigma degree and the valence
// table are those of bonds.inc; every atom takes its FIRST option, which must be neutral; `sel` is the set of atoms whose option
// adds a bond, G[sel] the graph of the bonds between them, a Kekule structure a perfect matching of G[sel].
//
// The search tree, which also defines the budget: the root is the empty matching; at a node v is the lowest unmatched atom of
// sel; without one the node is a structure; otherwise it has one child per unmatched sel neighbour of v in ascending order; a
// node without a child is a dead end.  More than GAUDI_KEKULE_BUDGET nodes: UNDECIDED.
//
// ONE text, two builds, as bonds.inc: kekule_molecule is __host__ __device__, the `lanes` of a phase are the 64 lanes of a wave on
// the device and one lane on the host (kRwLanes and the rw_* helpers of rings.inc).  Per wave 21 256 bytes of LDS, two waves per workgroup:
//   1. lanes = atoms / bonds: the checks and the neighbour lists of bonds.inc; components by min-label propagation; sel numbered
//      compactly in ascending atom index (prefix scan), the bonds of G[sel] numbered in bond-list order (prefix scan); lane c
//      collects the at most three sel neighbours of compact atom c in ascending order, with their edge numbers, into two words;
//   2. lanes = atoms: the chordless 6-cycles of G[sel] -- lane a walks the chordless paths from a through larger atoms only and
//      closes them on a with second atom < last atom, every cycle once and already in its reported order; counted, then stored at
//      the prefix of the counts; ranked by the sorted atom tuple; per hexagon a 192-bit edge mask, a 128-bit atom mask and the
//      32-bit mask of the hexagons it shares an atom with;
//   3. the search on all lanes: the tree is expanded level by level in an LDS ring (one open node per lane, children at the prefix
//      of their counts) until 64 nodes are open or none is; then every lane takes open nodes through one LDS counter and walks the
//      subtree below depth-first.  A lane's state is registers only: the matched atoms (128 bits), the atoms that were `v` (128
//      bits: the highest is the level to undo), the double bonds (192 bits) and the child taken per level (2 bits each).  At a
//      structure the lane adds to the bond and hexagon counters in LDS and keeps K, the Fries and the Clar maximum in registers;
//      the Clar number of a structure is an exact maximum independent set of its sextets under share-an-atom, by branching on
//      the lowest candidate, skipped when the sextet count cannot beat the lane's maximum.  Every kKekSlice steps the wave sums the
//      lanes' node counts and stops once the sum passes the budget: a tree within the budget is never cut short, a tree beyond
//      it is UNDECIDED whatever the schedule;
//   4. lanes = bonds / hexagon atoms: the counts out.
// Integer arithmetic only, plain vector stores and LDS atomics only; sums and maxima commute, so nothing depends on how the search
// is split over lanes, on the molecule's place in the batch, or on host versus device.

namespace gaudi {

typedef unsigned long long kek_u64;

constexpr int kKekWaves = 2;
constexpr int kKekMaxSel = GAUDI_KEKULE_MAX_SEL;
constexpr int kKekMaxEdges = GAUDI_KEKULE_MAX_EDGES;
constexpr int kKekMaxHex = GAUDI_RINGS_MAX_RINGS;
constexpr int kKekBudget = GAUDI_KEKULE_BUDGET;
constexpr int kKekOpen = 64;     // the level-by-level expansion ends with this many open nodes (or none)
constexpr int kKekQueue = 256;   // ring slots: fewer than kKekOpen nodes being read and at most three children of each
constexpr int kKekSlice = 256;   // steps of a lane between two sums of the node counts
constexpr unsigned kKekNone = 0xff;
static_assert(kKekMaxSel == 128 && kKekMaxEdges == 192 && kKekMaxHex == 32, "the masks are 2 x 64, 3 x 64 and 32 bits wide");
static_assert(4 * (kKekOpen - 1) <= kKekQueue && (kKekQueue & (kKekQueue - 1)) == 0, "the ring holds a level and its children");
static_assert(kKekMaxSel < kKekNone && kKekMaxEdges < kKekNone, "compact indices and edge numbers are bytes");

struct KekSmem {
  kek_u64 qm[kKekQueue][2], qe[kKekQueue][3];         // open nodes: matched atoms, double bonds
  kek_u64 hmask[kKekMaxHex][3], amask[kKekMaxHex][2];  // the hexagons in reported order: edges, atoms
  kek_u64 uam[kKekMaxHex][2];                          // atom masks in the order found
  unsigned dc[kKekMaxEdges], sc[kKekMaxHex], conf[kKekMaxHex];
  unsigned cnb[kKekMaxSel], ced[kKekMaxSel];           // compact atom -> its sel neighbours ascending / their edges, a byte each
  unsigned short nbr[kBondMaxAtoms][kBondNbr];
  unsigned short bl[kBondMaxBonds][2];
  unsigned short label[kBondMaxAtoms];
  unsigned short catom[kKekMaxSel];                    // compact index -> atom
  unsigned char sel[kBondMaxAtoms], cidx[kBondMaxAtoms], eidx[kBondMaxBonds];  // atom -> compact index, bond -> edge number
  unsigned char cyc[kKekMaxHex][6], scyc[kKekMaxHex][6];                       // hexagons in cycle order: as found, as reported
  int qnext;
};

struct KekParams {
  int B, A, M;
  const int* elem;
  const int* n_atoms;
  const int* bonds;
  const int* n_bonds;
  long long* k;
  unsigned* double_count;
  int* n_hex;
  int* hex_atoms;
  unsigned* sextet_count;
  int* fries;
  int* clar;
  long long* n_nodes;
  int* status;
};

__host__ __device__ __forceinline__ unsigned kek_byte(unsigned w, int q) { return (w >> (8 * q)) & 0xffu; }
__host__ __device__ __forceinline__ kek_u64 kek_lo(int i) { return i < 64 ? 1ull << (i & 63) : 0ull; }
__host__ __device__ __forceinline__ kek_u64 kek_hi(int i) { return i >= 64 && i < 128 ? 1ull << (i & 63) : 0ull; }
__host__ __device__ __forceinline__ kek_u64 kek_top(int i) { return i >= 128 ? 1ull << (i & 63) : 0ull; }
__host__ __device__ __forceinline__ int kek_pop(kek_u64 w) { return __builtin_popcountll(w); }
__host__ __device__ __forceinline__ int kek_ctz(kek_u64 w) { return __builtin_ctzll(w); }
__host__ __device__ __forceinline__ bool kek_adj(const KekSmem& s, int x, unsigned y) {
  const unsigned w = s.cnb[x];
  return kek_byte(w, 0) == y || kek_byte(w, 1) == y || kek_byte(w, 2) == y;
}
// the number of the edge x - y of G[sel] (the caller knows it exists)
__host__ __device__ __forceinline__ int kek_edge(const KekSmem& s, int x, unsigned y) {
  const unsigned w = s.cnb[x], d = s.ced[x];
  return (int)(kek_byte(w, 0) == y ? kek_byte(d, 0) : kek_byte(w, 1) == y ? kek_byte(d, 1) : kek_byte(d, 2));
}
__host__ __device__ __forceinline__ void kek_inc(unsigned* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(p, 1u);
#else
  ++*p;
#endif
}
__host__ __device__ __forceinline__ int kek_take(int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicAdd(p, 1);
#else
  return (*p)++;
#endif
}
__host__ __device__ __forceinline__ int kek_max(int v) { return -rw_min(-v); }

// Chordless 6-cycles of G[sel] whose smallest atom is a, each once and from a towards the smaller of its two ring neighbours.
// Returns their number; with `store` they are written to s.cyc[base ...] while base + found stays below kKekMaxHex.
__host__ __device__ inline int kek_hex_enum(KekSmem& s, int a, bool store, int base) {
  int found = 0;
  const unsigned w0 = s.cnb[a];
  for (int q1 = 0; q1 < 3; ++q1) {
    const unsigned p1 = kek_byte(w0, q1);
    if (p1 == kKekNone) break;
    if ((int)p1 <= a) continue;
    const unsigned w1 = s.cnb[p1];
    for (int q2 = 0; q2 < 3; ++q2) {
      const unsigned p2 = kek_byte(w1, q2);
      if (p2 == kKekNone) break;
      if ((int)p2 <= a || kek_adj(s, p2, a)) continue;
      const unsigned w2 = s.cnb[p2];
      for (int q3 = 0; q3 < 3; ++q3) {
        const unsigned p3 = kek_byte(w2, q3);
        if (p3 == kKekNone) break;
        if ((int)p3 <= a || p3 == p1 || kek_adj(s, p3, a) || kek_adj(s, p3, p1)) continue;
        const unsigned w3 = s.cnb[p3];
        for (int q4 = 0; q4 < 3; ++q4) {
          const unsigned p4 = kek_byte(w3, q4);
          if (p4 == kKekNone) break;
          if ((int)p4 <= a || p4 == p2 || kek_adj(s, p4, a) || kek_adj(s, p4, p1) || kek_adj(s, p4, p2)) continue;
          const unsigned w4 = s.cnb[p4];
          for (int q5 = 0; q5 < 3; ++q5) {
            const unsigned p5 = kek_byte(w4, q5);
            if (p5 == kKekNone) break;
            if ((int)p5 <= a || p5 == p3 || p5 < p1 || !kek_adj(s, p5, a)) continue;
            if (kek_adj(s, p5, p1) || kek_adj(s, p5, p2) || kek_adj(s, p5, p3)) continue;
            if (store && base + found < kKekMaxHex) {
              unsigned char* c = s.cyc[base + found];
              c[0] = (unsigned char)a;
              c[1] = (unsigned char)p1;
              c[2] = (unsigned char)p2;
              c[3] = (unsigned char)p3;
              c[4] = (unsigned char)p4;
              c[5] = (unsigned char)p5;
            }
            ++found;
          }
        }
      }
    }
  }
  return found;
}

// The largest set of pairwise atom-disjoint hexagons within A, if it beats `best`: the independent subsets of A in lexicographic
// order -- I the hexagons taken, every hexagon below p decided -- cut where even all remaining candidates would not beat best.
__host__ __device__ inline int kek_mis(const KekSmem& s, unsigned A, int best) {
  unsigned I = 0;
  int p = 0;
  for (;;) {
    unsigned blocked = I;
    for (unsigned w = I; w; w &= w - 1) blocked |= s.conf[__builtin_ctz(w)];
    const unsigned C = A & ~blocked & (unsigned)(~0ull << p);
    const int ni = __builtin_popcount(I);
    if (C && ni + __builtin_popcount(C) > best) {
      const int r = __builtin_ctz(C);
      I |= 1u << r;
      p = r + 1;
      continue;
    }
    best = ni > best ? ni : best;
    if (!I) break;
    const int r = 31 - __builtin_clz(I);  // the last hexagon taken is now left out
    I &= ~(1u << r);
    p = r + 1;
  }
  return best;
}

// One structure, with double bonds e0..e2, into the counters.
__host__ __device__ inline void kek_record(KekSmem& s, int R, kek_u64 e0, kek_u64 e1, kek_u64 e2, int& K, int& fries, int& clar) {
  ++K;
  for (kek_u64 w = e0; w; w &= w - 1) kek_inc(&s.dc[kek_ctz(w)]);
  for (kek_u64 w = e1; w; w &= w - 1) kek_inc(&s.dc[64 + kek_ctz(w)]);
  for (kek_u64 w = e2; w; w &= w - 1) kek_inc(&s.dc[128 + kek_ctz(w)]);
  unsigned sextets = 0;
  for (int r = 0; r < R; ++r)
    if (kek_pop(e0 & s.hmask[r][0]) + kek_pop(e1 & s.hmask[r][1]) + kek_pop(e2 & s.hmask[r][2]) == 3) {
      sextets |= 1u << r;
      kek_inc(&s.sc[r]);
    }
  const int ns = __builtin_popcount(sextets);
  fries = ns > fries ? ns : fries;
  if (ns > clar) clar = kek_mis(s, sextets, clar);
}

// One molecule.  `s` is this wave's (host: this call's) working state; every `break` of the outer block is lane-uniform.
__host__ __device__ inline void kekule_molecule(const KekParams& P, const BondTables& T, KekSmem& s, int b, int lane) {
  const int A = P.A, M = P.M;
  const int n = P.n_atoms[b], m = P.n_bonds[b];
  const int* eb = P.elem + (size_t)b * A;
  const int* bb = P.bonds + (size_t)b * M * 2;
  int status = GAUDI_KEKULE_OK;

  do {
    if (n <= 0) { status = GAUDI_KEKULE_EMPTY; break; }
    if (n > A || m < 0 || m > M) { status = GAUDI_KEKULE_BAD_INPUT; break; }  // (the entry points refuse these)
    if (n > kBondMaxAtoms || m > kBondMaxBonds) { status = GAUDI_KEKULE_OVERFLOW; break; }
    // ---- 1. inputs checked, the bond list staged, neighbours, sigma degree, sel (as bonds.inc)
    bool bad = false;
    int heavy = 0;
    for (int a = lane; a < n; a += kRwLanes) {
      const int e = eb[a];
      bad = bad || e < 0 || e >= T.n_elems;
      heavy += e != T.h_elem;
    }
    for (int k = lane; k < m; k += kRwLanes) {
      const int i = bb[2 * k], j = bb[2 * k + 1];
      const bool in = i >= 0 && i < n && j >= 0 && j < n && i != j;
      bad = bad || !in;
      s.bl[k][0] = (unsigned short)(in ? i : 0);
      s.bl[k][1] = (unsigned short)(in ? j : 0);
    }
    int H;
    (void)rw_scan(heavy, lane, H);
    rw_fence();
    if (rw_any(bad)) { status = GAUDI_KEKULE_BAD_INPUT; break; }
    if (H > kBondMaxHeavy) { status = GAUDI_KEKULE_OVERFLOW; break; }
    bool no_option = false, charged = false;
    for (int a = lane; a < n; a += kRwLanes) {
      int d = 0;
      unsigned short nb[kBondNbr] = {kBondNone, kBondNone, kBondNone, kBondNone};
      for (int k = 0; k < m; ++k) {
        const int i = s.bl[k][0], j = s.bl[k][1];
        if (i != a && j != a) continue;
        const unsigned short o = (unsigned short)(i == a ? j : i);
        for (int q = 0; q < kBondNbr; ++q) bad = bad || nb[q] == o;  // the same bond twice
        for (int q = 0; q < kBondNbr; ++q)
          if (q == d) nb[q] = o;
        ++d;
      }
      for (int q = 0; q < kBondNbr; ++q) s.nbr[a][q] = nb[q];
      const int e = eb[a];
      const int sd = d + (e == T.c_elem && d == 2);
      const int r = e * kBondDegrees + (sd < kBondDegrees ? sd : 0);
      const bool has = sd < kBondDegrees && T.n_opt[r] > 0;
      no_option = no_option || !has;
      charged = charged || (has && T.chg[r][0] != 0);
      s.sel[a] = (unsigned char)(has ? T.add[r][0] : 0);
      s.cidx[a] = (unsigned char)kKekNone;
      s.label[a] = (unsigned short)a;
    }
    rw_fence();
    if (rw_any(bad)) { status = GAUDI_KEKULE_BAD_INPUT; break; }
    if (rw_any(no_option)) { status = GAUDI_KEKULE_BAD_VALENCE; break; }
    // one component (labels only fall, so racing reads are harmless)
    while (true) {
      bool changed = false;
      for (int a = lane; a < n; a += kRwLanes) {
        unsigned short lo = s.label[a];
        for (int q = 0; q < kBondNbr; ++q) {
          const int o = s.nbr[a][q];
          if (o == kBondNone) break;
          const unsigned short l = s.label[o];
          lo = l < lo ? l : lo;
        }
        if (lo < s.label[a]) {
          s.label[a] = lo;
          changed = true;
        }
      }
      rw_fence();
      if (!rw_any(changed)) break;
    }
    int comp = 0;
    for (int a = lane; a < n; a += kRwLanes) comp += s.label[a] == a;
    int C;
    (void)rw_scan(comp, lane, C);
    if (C != 1) { status = GAUDI_KEKULE_NOT_CONNECTED; break; }
    if (rw_any(charged)) { status = GAUDI_KEKULE_NOT_NEUTRAL; break; }
    // sel numbered in ascending atom index, the bonds of G[sel] in bond-list order
    const int per = (n + kRwLanes - 1) / kRwLanes, lo = lane * per, hi = lo + per < n ? lo + per : n;
    const int bper = (m + kRwLanes - 1) / kRwLanes, blo = lane * bper, bhi = blo + bper < m ? blo + bper : m;
    int cnt = 0, ecnt = 0;
    for (int a = lo; a < hi; ++a) cnt += s.sel[a];
    for (int k = blo; k < bhi; ++k) ecnt += s.sel[s.bl[k][0]] && s.sel[s.bl[k][1]];
    int S, E;
    int pos = rw_scan(cnt, lane, S);
    int epos = rw_scan(ecnt, lane, E);
    if (S > kKekMaxSel || E > kKekMaxEdges) { status = GAUDI_KEKULE_OVERFLOW; break; }
    for (int a = lo; a < hi; ++a)
      if (s.sel[a]) {
        s.cidx[a] = (unsigned char)pos;
        s.catom[pos++] = (unsigned short)a;
      }
    for (int k = blo; k < bhi; ++k) s.eidx[k] = (unsigned char)(s.sel[s.bl[k][0]] && s.sel[s.bl[k][1]] ? epos++ : kKekNone);
    for (int e = lane; e < kKekMaxEdges; e += kRwLanes) s.dc[e] = 0;
    for (int r = lane; r < kKekMaxHex; r += kRwLanes) s.sc[r] = 0;
    rw_fence();
    bool crowded = false;  // a sel atom with more than three sel neighbours: beyond what a node's two path bits can name
    for (int c = lane; c < S; c += kRwLanes) {
      const int a = s.catom[c];
      unsigned n0 = kKekNone, n1 = kKekNone, n2 = kKekNone, e0 = 0, e1 = 0, e2 = 0;
      int deg = 0;
      for (int k = 0; k < m; ++k) {
        const int i = s.bl[k][0], j = s.bl[k][1];
        if ((i != a && j != a) || s.eidx[k] == kKekNone) continue;
        const unsigned u = s.cidx[i == a ? j : i], e = s.eidx[k];
        if (u < n0) {
          n2 = n1; e2 = e1; n1 = n0; e1 = e0; n0 = u; e0 = e;
        } else if (u < n1) {
          n2 = n1; e2 = e1; n1 = u; e1 = e;
        } else if (u < n2) {
          n2 = u; e2 = e;
        }
        ++deg;
      }
      crowded = crowded || deg > 3;
      s.cnb[c] = n0 | n1 << 8 | n2 << 16 | kKekNone << 24;
      s.ced[c] = e0 | e1 << 8 | e2 << 16;
    }
    rw_fence();
    if (rw_any(crowded)) { status = GAUDI_KEKULE_OVERFLOW; break; }

    // ---- 2. the hexagons: counted, stored at the prefix of the counts, ranked by their sorted atom tuple
    int mine = 0;
    for (int a = lane; a < S; a += kRwLanes) mine += kek_hex_enum(s, a, false, 0);
    int R;
    int base = rw_scan(mine, lane, R);
    if (R > kKekMaxHex) { status = GAUDI_KEKULE_OVERFLOW; break; }
    for (int a = lane; a < S; a += kRwLanes) base += kek_hex_enum(s, a, true, base);
    rw_fence();
    for (int r = lane; r < R; r += kRwLanes) {
      kek_u64 a0 = 0, a1 = 0;
      for (int j = 0; j < 6; ++j) {
        a0 |= kek_lo(s.cyc[r][j]);
        a1 |= kek_hi(s.cyc[r][j]);
      }
      s.uam[r][0] = a0;
      s.uam[r][1] = a1;
    }
    rw_fence();
    for (int r = lane; r < R; r += kRwLanes) {
      // of two atom sets of one size the one that holds the lowest atom they differ in has the smaller sorted tuple
      const kek_u64 a0 = s.uam[r][0], a1 = s.uam[r][1];
      int rank = 0;
      for (int o = 0; o < R; ++o) {
        const kek_u64 d0 = a0 ^ s.uam[o][0], d1 = a1 ^ s.uam[o][1];
        rank += d0 ? ((d0 & (0 - d0)) & s.uam[o][0]) != 0 : d1 ? ((d1 & (0 - d1)) & s.uam[o][1]) != 0 : 0;
      }
      kek_u64 h0 = 0, h1 = 0, h2 = 0;
      for (int j = 0; j < 6; ++j) {
        const int x = s.cyc[r][j], e = kek_edge(s, x, s.cyc[r][j == 5 ? 0 : j + 1]);
        s.scyc[rank][j] = (unsigned char)x;
        h0 |= kek_lo(e);
        h1 |= kek_hi(e);
        h2 |= kek_top(e);
      }
      s.amask[rank][0] = a0;
      s.amask[rank][1] = a1;
      s.hmask[rank][0] = h0;
      s.hmask[rank][1] = h1;
      s.hmask[rank][2] = h2;
    }
    rw_fence();
    for (int r = lane; r < R; r += kRwLanes) {
      unsigned c = 0;
      for (int o = 0; o < R; ++o)
        if (o != r && ((s.amask[r][0] & s.amask[o][0]) | (s.amask[r][1] & s.amask[o][1]))) c |= 1u << o;
      s.conf[r] = c;
    }
    if (lane == 0) {
      // the root: the empty matching; the bits beyond S count as matched, so a node is a structure when no bit is clear
      s.qm[0][0] = S >= 64 ? 0ull : ~0ull << S;
      s.qm[0][1] = S >= 128 ? 0ull : S <= 64 ? ~0ull : ~0ull << (S - 64);
      s.qe[0][0] = s.qe[0][1] = s.qe[0][2] = 0ull;
      s.qnext = 0;
    }
    rw_fence();
    if (S & 1) { status = GAUDI_KEKULE_NO_KEKULE; break; }

    // ---- 3. the search.  Level by level until kKekOpen nodes are open ...
    int K = 0, fries = 0, clar = 0, nodes = 0;
    int head = 0, open = 1;
    while (open > 0 && open < kKekOpen) {
      int kids = 0;
      for (int i = lane; i < open; i += kRwLanes) {
        const int slot = (head + i) & (kKekQueue - 1);
        const kek_u64 m0 = s.qm[slot][0], m1 = s.qm[slot][1];
        ++nodes;
        if (!~m0 && !~m1) {
          kek_record(s, R, s.qe[slot][0], s.qe[slot][1], s.qe[slot][2], K, fries, clar);
          continue;
        }
        const int v = ~m0 ? kek_ctz(~m0) : 64 + kek_ctz(~m1);
        const unsigned w = s.cnb[v];
        for (int q = 0; q < 3; ++q) {
          const unsigned u = kek_byte(w, q);
          if (u == kKekNone) break;
          kids += !((m0 & kek_lo(u)) | (m1 & kek_hi(u)));
        }
      }
      int total;
      int at = head + open + rw_scan(kids, lane, total);
      for (int i = lane; i < open; i += kRwLanes) {
        const int slot = (head + i) & (kKekQueue - 1);
        const kek_u64 m0 = s.qm[slot][0], m1 = s.qm[slot][1];
        if (!~m0 && !~m1) continue;
        const int v = ~m0 ? kek_ctz(~m0) : 64 + kek_ctz(~m1);
        const unsigned w = s.cnb[v], d = s.ced[v];
        for (int q = 0; q < 3; ++q) {
          const unsigned u = kek_byte(w, q);
          if (u == kKekNone) break;
          if ((m0 & kek_lo(u)) | (m1 & kek_hi(u))) continue;
          const int to = at++ & (kKekQueue - 1), e = kek_byte(d, q);
          s.qm[to][0] = m0 | kek_lo(v) | kek_lo(u);
          s.qm[to][1] = m1 | kek_hi(v) | kek_hi(u);
          s.qe[to][0] = s.qe[slot][0] | kek_lo(e);
          s.qe[to][1] = s.qe[slot][1] | kek_hi(e);
          s.qe[to][2] = s.qe[slot][2] | kek_top(e);
        }
      }
      rw_fence();
      head = (head + open) & (kKekQueue - 1);
      open = total;
    }
    // ... then every lane takes open nodes and walks the subtree below.  q: -1 = enter the node, 0..2 = the next child of v to
    // try, 3 = undo the last level
    kek_u64 m0 = 0, m1 = 0, v0 = 0, v1 = 0, e0 = 0, e1 = 0, e2 = 0, p0 = 0, p1 = 0;
    int depth = 0, q = -1, v = 0;
    bool busy = false, done = open == 0, undecided = false;
    for (;;) {
      for (int step = 0; step < kKekSlice; ++step) {
        if (!busy) {
          if (done) break;
          const int i = kek_take(&s.qnext);
          if (i >= open) {
            done = true;
            break;
          }
          const int slot = (head + i) & (kKekQueue - 1);
          m0 = s.qm[slot][0];
          m1 = s.qm[slot][1];
          e0 = s.qe[slot][0];
          e1 = s.qe[slot][1];
          e2 = s.qe[slot][2];
          v0 = v1 = p0 = p1 = 0;
          depth = 0;
          q = -1;
          busy = true;
        }
        if (q < 0) {
          ++nodes;
          if (!~m0 && !~m1) {
            kek_record(s, R, e0, e1, e2, K, fries, clar);
            q = 3;
          } else {
            v = ~m0 ? kek_ctz(~m0) : 64 + kek_ctz(~m1);
            q = 0;
          }
        }
        if (q < 3) {
          const unsigned w = s.cnb[v];
          unsigned u = kKekNone;
          for (; q < 3; ++q) {
            u = kek_byte(w, q);
            if (u == kKekNone) q = 2;  // (the neighbours are sorted: none follows)
            else if (!((m0 & kek_lo(u)) | (m1 & kek_hi(u)))) break;
          }
          if (q < 3) {
            const int e = kek_byte(s.ced[v], q), sh = 2 * (depth & 31);
            m0 |= kek_lo(v) | kek_lo(u);
            m1 |= kek_hi(v) | kek_hi(u);
            v0 |= kek_lo(v);
            v1 |= kek_hi(v);
            e0 |= kek_lo(e);
            e1 |= kek_hi(e);
            e2 |= kek_top(e);
            if (depth < 32) p0 = (p0 & ~(3ull << sh)) | (kek_u64)q << sh;
            else p1 = (p1 & ~(3ull << sh)) | (kek_u64)q << sh;
            ++depth;
            q = -1;
            continue;
          }
        }
        if (depth == 0) {
          busy = false;
          continue;
        }
        --depth;
        {
          v = v1 ? 127 - __builtin_clzll(v1) : 63 - __builtin_clzll(v0);
          const int sh = 2 * (depth & 31), was = (int)(((depth < 32 ? p0 : p1) >> sh) & 3);
          const int u = kek_byte(s.cnb[v], was), e = kek_byte(s.ced[v], was);
          m0 &= ~(kek_lo(v) | kek_lo(u));
          m1 &= ~(kek_hi(v) | kek_hi(u));
          v0 &= ~kek_lo(v);
          v1 &= ~kek_hi(v);
          e0 &= ~kek_lo(e);
          e1 &= ~kek_hi(e);
          e2 &= ~kek_top(e);
          q = was + 1;
        }
      }
      int sum;
      (void)rw_scan(nodes, lane, sum);
      if (sum > kKekBudget) { undecided = true; break; }
      if (!rw_any(busy || !done)) break;
    }
    rw_fence();
    if (undecided) { status = GAUDI_KEKULE_UNDECIDED; break; }
    int K_all, N_all;
    (void)rw_scan(K, lane, K_all);
    (void)rw_scan(nodes, lane, N_all);
    fries = kek_max(fries);
    clar = kek_max(clar);
    if (K_all == 0) { status = GAUDI_KEKULE_NO_KEKULE; break; }

    // ---- 4. outputs
    for (int k = lane; k < m; k += kRwLanes)
      if (s.eidx[k] != kKekNone) P.double_count[(size_t)b * M + k] = s.dc[s.eidx[k]];
    for (int i = lane; i < R * 6; i += kRwLanes) P.hex_atoms[(size_t)b * kKekMaxHex * 6 + i] = s.catom[s.scyc[i / 6][i % 6]];
    for (int r = lane; r < R; r += kRwLanes) P.sextet_count[(size_t)b * kKekMaxHex + r] = s.sc[r];
    if (lane == 0) {
      P.k[b] = K_all;
      P.n_hex[b] = R;
      P.fries[b] = fries;
      P.clar[b] = clar;
      P.n_nodes[b] = N_all;
    }
  } while (false);

  if (lane == 0) P.status[b] = status;
}

__global__ __launch_bounds__(64 * kKekWaves) void kekule_kernel(const KekParams P, const BondTables* __restrict__ Tp) {
  __shared__ KekSmem smem[kKekWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * kKekWaves + w;
  if (b >= P.B) return;
  kekule_molecule(P, *Tp, smem[w], b, lane);
}

// the nine outputs in argument order: bytes per molecule
static void kekule_sizes(int M, size_t osz[9]) {
  const size_t per[9] = {sizeof(long long), sizeof(unsigned) * (size_t)M, sizeof(int), sizeof(int) * kKekMaxHex * 6,
                         sizeof(unsigned) * kKekMaxHex, sizeof(int), sizeof(int), sizeof(long long), sizeof(int)};
  for (int i = 0; i < 9; ++i) osz[i] = per[i];
}

}  // namespace gaudi

#define GAUDI_KEKULE_ARGS                                                                                                         \
  int B, int A, int M, const int32_t *elem, const int32_t *n_atoms, const int32_t *bonds, const int32_t *n_bonds,                 \
      int64_t *k_out, uint32_t *double_count_out, int32_t *n_hex_out, int32_t *hex_atoms_out, uint32_t *sextet_count_out,         \
      int32_t *fries_out, int32_t *clar_out, int64_t *n_nodes_out, int32_t *status_out
#define GAUDI_KEKULE_OUTS \
  { k_out, double_count_out, n_hex_out, hex_atoms_out, sextet_count_out, fries_out, clar_out, n_nodes_out, status_out }

static void kekule_point(gaudi::KekParams& P, void* const o[9]) {
  P.k = (long long*)o[0];
  P.double_count = (unsigned*)o[1];
  P.n_hex = (int*)o[2];
  P.hex_atoms = (int*)o[3];
  P.sextet_count = (unsigned*)o[4];
  P.fries = (int*)o[5];
  P.clar = (int*)o[6];
  P.n_nodes = (long long*)o[7];
  P.status = (int*)o[8];
}

extern "C" int gaudi_kekule(gaudi_handle* h, const gaudi_valence_tables* vt, GAUDI_KEKULE_ARGS) {
  void* const outs[9] = GAUDI_KEKULE_OUTS;
  if (!h) return GAUDI_E_INVALID;
  for (void* o : outs)
    if (!o) return fail(h, GAUDI_E_INVALID, "invalid argument");
  gaudi::BondTables T;
  const char* why = "";
  if (int rc = gaudi::bonds_prepare(vt, B, A, M, elem, n_atoms, bonds, n_bonds, T, &why)) return fail(h, rc, why);
  if (B == 0) return GAUDI_OK;
  HIPCHECK(h, hipSetDevice(h->device));
  const size_t nB = (size_t)B;
  const size_t isz[5] = {sizeof(int) * nB * A, sizeof(int) * nB, sizeof(int) * nB * M * 2, sizeof(int) * nB, sizeof(gaudi::BondTables)};
  size_t osz[9];
  gaudi::kekule_sizes(M, osz);
  const void* ins[5] = {elem, n_atoms, bonds, n_bonds, &T};
  for (int i = 0; i < 5; ++i) {
    HIPCHECK(h, h->d_kekule[i].reserve(isz[i]));
    HIPCHECK(h, hipMemcpyAsync(h->d_kekule[i].p, ins[i], isz[i], hipMemcpyHostToDevice, h->stream));
  }
  // a molecule with any status but OK writes its status only: zero everywhere else
  void* dev[9];
  for (int i = 0; i < 9; ++i) {
    HIPCHECK(h, h->d_kekule[5 + i].reserve(osz[i] * nB));
    HIPCHECK(h, hipMemsetAsync(h->d_kekule[5 + i].p, 0, osz[i] * nB, h->stream));
    dev[i] = h->d_kekule[5 + i].p;
  }
  HIPCHECK(h, hipStreamSynchronize(h->stream));  // T is a local object
  gaudi::KekParams P{};
  P.B = B;
  P.A = A;
  P.M = M;
  P.elem = h->d_kekule[0].as<int>();
  P.n_atoms = h->d_kekule[1].as<int>();
  P.bonds = h->d_kekule[2].as<int>();
  P.n_bonds = h->d_kekule[3].as<int>();
  kekule_point(P, dev);
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (h->prof) HIPCHECK(h, h->kekule_log.begin(h->stream, ev));
  hipLaunchKernelGGL(gaudi::kekule_kernel, dim3((B + gaudi::kKekWaves - 1) / gaudi::kKekWaves), dim3(64 * gaudi::kKekWaves), 0,
                     h->stream, P, (const gaudi::BondTables*)h->d_kekule[4].p);
  HIPCHECK(h, hipGetLastError());
  if (h->prof) HIPCHECK(h, h->kekule_log.end(h->stream, ev));
  for (int i = 0; i < 9; ++i) HIPCHECK(h, hipMemcpyAsync(outs[i], dev[i], osz[i] * nB, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  return GAUDI_OK;
}

extern "C" int gaudi_kekule_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms) {
  if (!h || !n_launches || !total_ms) return GAUDI_E_INVALID;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, h->kekule_log.fold(0));
  *n_launches = (int32_t)h->kekule_log.n;
  *total_ms = h->kekule_log.ms;
  return GAUDI_OK;
}

extern "C" int gaudi_host_kekule(const gaudi_valence_tables* vt, GAUDI_KEKULE_ARGS) {
  void* const outs[9] = GAUDI_KEKULE_OUTS;
  for (void* o : outs)
    if (!o) return GAUDI_E_INVALID;
  std::vector<gaudi::BondTables> Tv(1);
  const char* why = "";
  if (int rc = gaudi::bonds_prepare(vt, B, A, M, elem, n_atoms, bonds, n_bonds, Tv[0], &why)) return rc;
  if (B == 0) return GAUDI_OK;
  size_t osz[9];
  gaudi::kekule_sizes(M, osz);
  for (int i = 0; i < 9; ++i) memset(outs[i], 0, osz[i] * (size_t)B);
  gaudi::KekParams P{};
  P.B = B;
  P.A = A;
  P.M = M;
  P.elem = elem;
  P.n_atoms = n_atoms;
  P.bonds = bonds;
  P.n_bonds = n_bonds;
  kekule_point(P, outs);
  std::vector<gaudi::KekSmem> S(1);
  for (int b = 0; b < B; ++b) gaudi::kekule_molecule(P, Tv[0], S[0], b, 0);
  return GAUDI_OK;
}
#undef GAUDI_KEKULE_ARGS
#undef GAUDI_KEKULE_OUTS
