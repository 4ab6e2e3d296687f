// canon.inc -- canonical numbering of a graph of atoms on the device (included after bonds.inc at the end of gaudi_hip.hip).
//
// What the reference gets from the InChI string when it counts distinct and novel molecules (analyze/analyze.py:180-231): an
// identity that does not depend on the atom numbering.  Here it is the canonical form of the labelled heavy-atom graph
// (DESIGN.md section 8i):
//
//   vertices = the non-hydrogen atoms; label = element * 8 + H count, the H count being the listed H neighbours plus one for a
//     carbon with exactly two bonds (the H build_molecule_aromatic adds: the sigma degree rule of bonds.inc);
//   edges = the bonds between non-hydrogen atoms, unlabelled (bond orders and charges belong to a resonance structure);
//   code of a numbering = n_heavy, the labels in rank order, the edges as sorted (lo, hi) pairs of ranks;
//   canonical = the numbering with the lexicographically smallest code among the leaves of the search tree below.
//
// Individualisation-refinement.  A colour is always "the number of vertices with a smaller colour", so it never depends on the
// numbering.  Refinement: colour <- colour + the number of vertices of the same colour whose sorted neighbour colours compare
// smaller, until nothing changes (the colouring is equitable).  A colouring with a class of two or more vertices branches on the
// first such class in colour order: each of its vertices in turn keeps the colour, the others move up by one.  A discrete
// colouring is a numbering.  The whole tree is walked (no pruning: the labels in rank order are the same at every leaf, and the
// edge lists are compared whole), within kCanonNodes refinements and kCanonDepth individualisations; beyond either the status is
// GAVE_UP and the best numbering met so far comes back -- valid, but not canonical.
//
// ONE text, two builds, as rings.inc and bonds.inc (kRwLanes and the rw_* helpers).  Per wave 11.2 KB of LDS, two waves per
// workgroup.  Lanes are atoms / bonds while the inputs are read, vertices for signatures, ranking and codes; every branch of the
// search control is taken on values all lanes hold alike (reductions, or LDS words lane 0 wrote), so the wave never diverges
// around a fence.  Integer arithmetic only; nothing depends on the molecule's place in the batch.

namespace gaudi {

constexpr int kCanonWaves = 2;
constexpr int kCanonMaxAtoms = GAUDI_CANON_MAX_ATOMS;
constexpr int kCanonMaxHeavy = GAUDI_CANON_MAX_HEAVY;
constexpr int kCanonMaxBonds = GAUDI_CANON_MAX_BONDS;
constexpr int kCanonDeg = GAUDI_CANON_MAX_DEGREE;
constexpr int kCanonNodes = GAUDI_CANON_MAX_NODES;
constexpr int kCanonDepth = GAUDI_CANON_MAX_DEPTH;
constexpr int kCanonMaxElems = 8;
constexpr int kCanonNone = 0xff;    // no vertex / no colour (vertices and colours are below 192)
constexpr int kCanonFar = 1 << 20;  // above every index: the identity of the min reductions
static_assert(kCanonMaxAtoms == kBondMaxAtoms && kCanonMaxHeavy == kBondMaxHeavy && kCanonMaxBonds == kBondMaxBonds, "capacities");
static_assert(kCanonMaxHeavy < kCanonNone && kCanonDeg == 8, "a vertex fits a byte; eight neighbour colours fit 64 bits");

struct CanonSmem {
  unsigned long long sig[kCanonMaxHeavy];            // a vertex's neighbour colours, ascending, most significant byte first
  unsigned short bl[kCanonMaxBonds][2];
  unsigned short hv[kCanonMaxHeavy];                 // vertex -> atom
  unsigned char hidx[kCanonMaxAtoms];                // atom -> vertex; none for a hydrogen
  unsigned char adj[kCanonMaxHeavy][kCanonDeg];      // a vertex's neighbours, none-padded
  unsigned char label[kCanonMaxHeavy];
  unsigned char col[kCanonDepth + 1][kCanonMaxHeavy];  // the colouring of every level of the path being walked
  unsigned char newc[kCanonMaxHeavy], size[kCanonMaxHeavy];  // the next colour; the size of the vertex's class
  unsigned char inv[kCanonMaxHeavy], bestcol[kCanonMaxHeavy];
  unsigned char code[kCanonMaxBonds][2], best[kCanonMaxBonds][2];
  short target[kCanonDepth + 1], cursor[kCanonDepth + 1];  // per level: the class branched on; its last vertex tried
};

struct CanonParams {
  int B, A, M, n_elems, h_elem, c_elem;
  const int* elem;
  const int* n_atoms;
  const int* bonds;
  const int* n_bonds;
  int* rank;
  int* n_heavy;
  unsigned char* label;
  int* n_hbonds;
  unsigned short* cbonds;
  int* nodes;
  int* status;
};

// eight values ascending: a sorting network (19 exchanges), every index a constant
__host__ __device__ __forceinline__ void canon_sort8(int (&c)[8]) {
#define GAUDI_CX(i, j)                       \
  {                                          \
    const int lo_ = c[i] < c[j] ? c[i] : c[j]; \
    c[j] = c[i] < c[j] ? c[j] : c[i];        \
    c[i] = lo_;                              \
  }
  GAUDI_CX(0, 2) GAUDI_CX(1, 3) GAUDI_CX(4, 6) GAUDI_CX(5, 7)
  GAUDI_CX(0, 4) GAUDI_CX(1, 5) GAUDI_CX(2, 6) GAUDI_CX(3, 7)
  GAUDI_CX(0, 1) GAUDI_CX(2, 3) GAUDI_CX(4, 5) GAUDI_CX(6, 7)
  GAUDI_CX(2, 4) GAUDI_CX(3, 5)
  GAUDI_CX(1, 4) GAUDI_CX(3, 6)
  GAUDI_CX(1, 2) GAUDI_CX(3, 4) GAUDI_CX(5, 6)
#undef GAUDI_CX
}

// Refine `col` (H vertices) in place to an equitable colouring.  -> the smallest colour whose class has two or more vertices,
// kCanonFar if the colouring is discrete.
__host__ __device__ inline int canon_refine(CanonSmem& s, unsigned char* col, int H, int lane) {
  for (;;) {
    for (int v = lane; v < H; v += kRwLanes) {
      int c[8];
      for (int k = 0; k < 8; ++k) {
        const int o = s.adj[v][k];
        c[k] = o == kCanonNone ? kCanonNone : (int)col[o];
      }
      canon_sort8(c);
      const unsigned hi = (unsigned)c[0] << 24 | (unsigned)c[1] << 16 | (unsigned)c[2] << 8 | (unsigned)c[3];
      const unsigned lo = (unsigned)c[4] << 24 | (unsigned)c[5] << 16 | (unsigned)c[6] << 8 | (unsigned)c[7];
      s.sig[v] = (unsigned long long)hi << 32 | lo;
    }
    rw_fence();
    bool changed = false;
    for (int v = lane; v < H; v += kRwLanes) {
      const int cv = col[v];
      const unsigned long long sv = s.sig[v];
      int lt = 0, eq = 0;
      for (int u = 0; u < H; ++u) {
        const bool same = col[u] == cv;
        eq += same;
        lt += same && s.sig[u] < sv;
      }
      s.newc[v] = (unsigned char)(cv + lt);
      s.size[v] = (unsigned char)eq;
      changed = changed || lt != 0;
    }
    rw_fence();
    if (!rw_any(changed)) break;
    for (int v = lane; v < H; v += kRwLanes) col[v] = s.newc[v];
    rw_fence();
  }
  int t = kCanonFar;
  for (int v = lane; v < H; v += kRwLanes)
    if (s.size[v] > 1 && col[v] < t) t = col[v];
  return rw_min(t);
}

// The edge list of the numbering `col` (discrete) into s.code: (lo, hi) rank pairs, sorted.
__host__ __device__ inline void canon_code(CanonSmem& s, const unsigned char* col, int H, int lane) {
  for (int v = lane; v < H; v += kRwLanes) s.inv[col[v]] = (unsigned char)v;
  rw_fence();
  const int per = (H + kRwLanes - 1) / kRwLanes, lo = lane * per, hi = lo + per < H ? lo + per : H;
  int cnt = 0;
  for (int r = lo; r < hi; ++r) {
    const int v = s.inv[r];
    for (int k = 0; k < 8; ++k) {
      const int o = s.adj[v][k];
      cnt += o != kCanonNone && col[o] > r;
    }
  }
  int total;
  int pos = rw_scan(cnt, lane, total);
  for (int r = lo; r < hi; ++r) {
    const int v = s.inv[r];
    int c[8];
    for (int k = 0; k < 8; ++k) {
      const int o = s.adj[v][k];
      c[k] = o != kCanonNone && col[o] > r ? (int)col[o] : kCanonNone;
    }
    canon_sort8(c);
    for (int k = 0; k < 8; ++k)
      if (c[k] != kCanonNone) {
        s.code[pos][0] = (unsigned char)r;
        s.code[pos][1] = (unsigned char)c[k];
        ++pos;
      }
  }
  rw_fence();
}

// The labelled graph of molecule b into s (bl, hv, hidx, adj, label): the inputs read and checked.  Only the input fields of P are
// used, so fp.inc reads its molecules through this too.  -> GAUDI_CANON_OK with H vertices and E edges, or the status that refuses
// the molecule; every exit is lane-uniform.
__host__ __device__ inline int canon_graph(const CanonParams& P, CanonSmem& s, int b, int lane, int& H_out, int& E_out) {
  const int A = P.A, M = P.M;
  const int n = P.n_atoms[b], m = P.n_bonds[b];
  const int* eb = P.elem + (size_t)b * A;
  const int* bb = P.bonds + (size_t)b * M * 2;
  int status = GAUDI_CANON_OK;
  H_out = 0;
  E_out = 0;
  do {
    if (n <= 0) { status = GAUDI_CANON_EMPTY; break; }
    if (n > A || m < 0 || m > M) { status = GAUDI_CANON_BAD_INPUT; break; }  // (the entry points refuse these)
    if (n > kCanonMaxAtoms || m > kCanonMaxBonds) { status = GAUDI_CANON_OVERFLOW; break; }
    // ---- 1. inputs checked; the bond list staged; the non-hydrogen atoms numbered in ascending index
    bool bad = false;
    const int aper = (n + kRwLanes - 1) / kRwLanes, alo = lane * aper, ahi = alo + aper < n ? alo + aper : n;
    int heavy = 0;
    for (int a = alo; a < ahi; ++a) {
      const int e = eb[a];
      bad = bad || e < 0 || e >= P.n_elems;
      heavy += e != P.h_elem;
    }
    for (int k = lane; k < m; k += kRwLanes) {
      const int i = bb[2 * k], j = bb[2 * k + 1];
      const bool in = i >= 0 && i < n && j >= 0 && j < n && i != j;
      bad = bad || !in;
      s.bl[k][0] = (unsigned short)(in ? i : 0);
      s.bl[k][1] = (unsigned short)(in ? j : 0);
    }
    int H;
    int hpos = rw_scan(heavy, lane, H);
    if (rw_any(bad)) { status = GAUDI_CANON_BAD_INPUT; break; }
    if (H > kCanonMaxHeavy) { status = GAUDI_CANON_OVERFLOW; break; }
    for (int a = alo; a < ahi; ++a) {
      const bool hy = eb[a] == P.h_elem;
      s.hidx[a] = (unsigned char)(hy ? kCanonNone : hpos);
      if (!hy) s.hv[hpos++] = (unsigned short)a;
    }
    rw_fence();
    // ---- 2. lane a collects atom a's neighbours (at most 8 are kept: more is OVERFLOW); a vertex gets its row and its label
    bool over = false;
    int ends = 0;
    for (int a = lane; a < n; a += kRwLanes) {
      int d = 0;
      int nb[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
      for (int k = 0; k < m; ++k) {
        const int i = s.bl[k][0], j = s.bl[k][1];
        if (i != a && j != a) continue;
        const int o = i == a ? j : i;
        for (int q = 0; q < 8; ++q) bad = bad || nb[q] == o;  // the same bond twice
        for (int q = 0; q < 8; ++q)
          if (q == d) nb[q] = o;
        ++d;
      }
      over = over || d > kCanonDeg;
      const int h = s.hidx[a];
      if (h == kCanonNone) continue;
      int hc = 0, hd = 0;
      int row[8] = {kCanonNone, kCanonNone, kCanonNone, kCanonNone, kCanonNone, kCanonNone, kCanonNone, kCanonNone};
      for (int q = 0; q < 8; ++q) {
        if (nb[q] < 0) continue;
        const int oh = s.hidx[nb[q]];
        if (oh == kCanonNone) {
          ++hc;
        } else {
          for (int r = 0; r < 8; ++r)
            if (r == hd) row[r] = oh;
          ++hd;
        }
      }
      const int e = eb[a];
      hc += e == P.c_elem && d == 2;
      over = over || hc > 7;
      for (int q = 0; q < 8; ++q) s.adj[h][q] = (unsigned char)row[q];
      s.label[h] = (unsigned char)(e * 8 + (hc & 7));
      ends += hd;
    }
    int E2;
    (void)rw_scan(ends, lane, E2);
    rw_fence();
    if (rw_any(bad)) { status = GAUDI_CANON_BAD_INPUT; break; }
    if (rw_any(over)) { status = GAUDI_CANON_OVERFLOW; break; }
    H_out = H;
    E_out = E2 / 2;
  } while (false);
  return status;
}

// One molecule.  `s` is this wave's (host: this call's) working state; every `break` is lane-uniform.
__host__ __device__ inline void canonical_order(const CanonParams& P, CanonSmem& s, int b, int lane) {
  const int A = P.A, M = P.M;
  const int n = P.n_atoms[b];
  int nodes = 0, H = 0, E = 0;
  int status = canon_graph(P, s, b, lane, H, E);

  do {
    if (status != GAUDI_CANON_OK) break;
    // ---- 3. the first colouring: the rank of the label
    for (int v = lane; v < H; v += kRwLanes) {
      const int lv = s.label[v];
      int c = 0;
      for (int u = 0; u < H; ++u) c += s.label[u] < lv;
      s.col[0][v] = (unsigned char)c;
    }
    rw_fence();

    // ---- 4. the search tree, depth first; one node = one refinement
    int level = 0;
    bool have = false, gave_up = false;
    for (;;) {
      if (nodes == kCanonNodes) { gave_up = true; break; }
      ++nodes;
      const int tgt = canon_refine(s, s.col[level], H, lane);
      if (tgt == kCanonFar) {  // a leaf: keep its numbering if its code is the smallest so far
        const unsigned char* col = s.col[level];
        canon_code(s, col, H, lane);
        bool better = !have;
        if (have) {
          int first = kCanonFar;
          for (int k = lane; k < E; k += kRwLanes)
            if (first == kCanonFar && (s.code[k][0] != s.best[k][0] || s.code[k][1] != s.best[k][1])) first = k;
          first = rw_min(first);
          if (first != kCanonFar) {
            const int c0 = s.code[first][0], b0 = s.best[first][0];
            better = c0 < b0 || (c0 == b0 && s.code[first][1] < s.best[first][1]);
          }
        }
        if (better) {
          rw_fence();  // (the comparison's reads before the copy)
          for (int k = lane; k < E; k += kRwLanes) {
            s.best[k][0] = s.code[k][0];
            s.best[k][1] = s.code[k][1];
          }
          for (int v = lane; v < H; v += kRwLanes) s.bestcol[v] = col[v];
          rw_fence();
        }
        have = true;
        --level;
      } else if (level == kCanonDepth) {
        gave_up = true;
        break;
      } else {
        if (lane == 0) {
          s.target[level] = (short)tgt;
          s.cursor[level] = -1;
        }
        rw_fence();
      }
      // the next child: up while a level's class is spent, then its next vertex (ascending index) individualised one level down
      while (level >= 0) {
        const unsigned char* col = s.col[level];
        const int t = s.target[level], c = s.cursor[level];
        int nx = kCanonFar;
        for (int v = lane; v < H; v += kRwLanes)
          if (nx == kCanonFar && col[v] == t && v > c) nx = v;
        nx = rw_min(nx);
        if (nx == kCanonFar) {
          --level;
          continue;
        }
        rw_fence();
        if (lane == 0) s.cursor[level] = (short)nx;
        for (int v = lane; v < H; v += kRwLanes) {
          const int cv = col[v];
          s.col[level + 1][v] = (unsigned char)(cv + (cv == t && v != nx));
        }
        rw_fence();
        ++level;
        break;
      }
      if (level < 0) break;
    }
    if (!have) {  // gave up before the first leaf: the root's classes in ascending vertex index
      for (int v = lane; v < H; v += kRwLanes) {
        const int cv = s.col[0][v];
        int c = cv;
        for (int u = 0; u < v; ++u) c += s.col[0][u] == cv;
        s.bestcol[v] = (unsigned char)c;
      }
      rw_fence();
      canon_code(s, s.bestcol, H, lane);
      for (int k = lane; k < E; k += kRwLanes) {
        s.best[k][0] = s.code[k][0];
        s.best[k][1] = s.code[k][1];
      }
      rw_fence();
    }
    status = gave_up ? GAUDI_CANON_GAVE_UP : GAUDI_CANON_OK;

    // ---- 5. outputs
    for (int a = lane; a < A; a += kRwLanes) {
      const int h = a < n ? (int)s.hidx[a] : kCanonNone;
      P.rank[(size_t)b * A + a] = h == kCanonNone ? -1 : (int)s.bestcol[h];
    }
    for (int v = lane; v < H; v += kRwLanes) P.label[(size_t)b * A + s.bestcol[v]] = s.label[v];
    for (int k = lane; k < E; k += kRwLanes) {
      P.cbonds[((size_t)b * M + k) * 2] = s.best[k][0];
      P.cbonds[((size_t)b * M + k) * 2 + 1] = s.best[k][1];
    }
    if (lane == 0) {
      P.n_heavy[b] = H;
      P.n_hbonds[b] = E;
    }
  } while (false);

  if (lane == 0) {
    P.status[b] = status;
    P.nodes[b] = nodes;
  }
}

__global__ __launch_bounds__(64 * kCanonWaves) void canon_kernel(const CanonParams P) {
  __shared__ CanonSmem smem[kCanonWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * kCanonWaves + w;
  if (b >= P.B) return;
  canonical_order(P, smem[w], b, lane);
}

// the arguments both entry points share, checked
static int canon_prepare(int n_elems, int h_elem, int c_elem, int B, int A, int M, const int32_t* elem, const int32_t* n_atoms,
                         const int32_t* bonds, const int32_t* n_bonds, const char** why) {
  *why = "invalid argument";
  if (!elem || !n_atoms || !bonds || !n_bonds || B < 0 || A < 1 || M < 1) return GAUDI_E_INVALID;
  if (n_elems < 1 || n_elems > kCanonMaxElems) { *why = "n_elems must be in 1..8"; return GAUDI_E_INVALID; }
  if (h_elem < 0 || h_elem >= n_elems || c_elem < 0 || c_elem >= n_elems) { *why = "h_elem / c_elem outside the element list"; return GAUDI_E_INVALID; }
  for (int b = 0; b < B; ++b)
    if (n_atoms[b] < 0 || n_atoms[b] > A || n_bonds[b] < 0 || n_bonds[b] > M) { *why = "n_atoms must be in 0..A and n_bonds in 0..M"; return GAUDI_E_INVALID; }
  return GAUDI_OK;
}

}  // namespace gaudi

#define GAUDI_CANON_ARGS                                                                                                          \
  int n_elems, int h_elem, int c_elem, int B, int A, int M, const int32_t *elem, const int32_t *n_atoms, const int32_t *bonds,    \
      const int32_t *n_bonds, int32_t *rank_out, int32_t *n_heavy_out, uint8_t *label_out, int32_t *n_hbonds_out,                 \
      uint16_t *cbonds_out, int32_t *nodes_out, int32_t *status_out

extern "C" int gaudi_canonical_order(gaudi_handle* h, GAUDI_CANON_ARGS) {
  if (!h || !rank_out || !n_heavy_out || !label_out || !n_hbonds_out || !cbonds_out || !nodes_out || !status_out) return GAUDI_E_INVALID;
  const char* why = "";
  if (int rc = gaudi::canon_prepare(n_elems, h_elem, c_elem, B, A, M, elem, n_atoms, bonds, n_bonds, &why)) return fail(h, rc, why);
  if (B == 0) return GAUDI_OK;
  HIPCHECK(h, hipSetDevice(h->device));
  const size_t nB = (size_t)B;
  const size_t isz[4] = {sizeof(int) * nB * A, sizeof(int) * nB, sizeof(int) * nB * M * 2, sizeof(int) * nB};
  const size_t osz[7] = {sizeof(int) * nB * A, sizeof(int) * nB, nB * A, sizeof(int) * nB, sizeof(uint16_t) * nB * M * 2,
                         sizeof(int) * nB, sizeof(int) * nB};
  const void* ins[4] = {elem, n_atoms, bonds, n_bonds};
  for (int i = 0; i < 4; ++i) {
    HIPCHECK(h, h->d_canon[i].reserve(isz[i]));
    HIPCHECK(h, hipMemcpyAsync(h->d_canon[i].p, ins[i], isz[i], hipMemcpyHostToDevice, h->stream));
  }
  // a molecule without a numbering writes its status only: zero everywhere else
  for (int i = 0; i < 7; ++i) {
    HIPCHECK(h, h->d_canon[4 + i].reserve(osz[i]));
    HIPCHECK(h, hipMemsetAsync(h->d_canon[4 + i].p, 0, osz[i], h->stream));
  }
  gaudi::CanonParams P{};
  P.B = B;
  P.A = A;
  P.M = M;
  P.n_elems = n_elems;
  P.h_elem = h_elem;
  P.c_elem = c_elem;
  P.elem = h->d_canon[0].as<int>();
  P.n_atoms = h->d_canon[1].as<int>();
  P.bonds = h->d_canon[2].as<int>();
  P.n_bonds = h->d_canon[3].as<int>();
  P.rank = h->d_canon[4].as<int>();
  P.n_heavy = h->d_canon[5].as<int>();
  P.label = h->d_canon[6].as<unsigned char>();
  P.n_hbonds = h->d_canon[7].as<int>();
  P.cbonds = h->d_canon[8].as<unsigned short>();
  P.nodes = h->d_canon[9].as<int>();
  P.status = h->d_canon[10].as<int>();
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (h->prof) HIPCHECK(h, h->canon_log.begin(h->stream, ev));
  hipLaunchKernelGGL(gaudi::canon_kernel, dim3((B + gaudi::kCanonWaves - 1) / gaudi::kCanonWaves), dim3(64 * gaudi::kCanonWaves), 0,
                     h->stream, P);
  HIPCHECK(h, hipGetLastError());
  if (h->prof) HIPCHECK(h, h->canon_log.end(h->stream, ev));
  void* outs[7] = {rank_out, n_heavy_out, label_out, n_hbonds_out, cbonds_out, nodes_out, status_out};
  for (int i = 0; i < 7; ++i) HIPCHECK(h, hipMemcpyAsync(outs[i], h->d_canon[4 + i].p, osz[i], hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  return GAUDI_OK;
}

extern "C" int gaudi_canon_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms) {
  if (!h || !n_launches || !total_ms) return GAUDI_E_INVALID;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, h->canon_log.fold(0));
  *n_launches = (int32_t)h->canon_log.n;
  *total_ms = h->canon_log.ms;
  return GAUDI_OK;
}

extern "C" int gaudi_host_canonical_order(GAUDI_CANON_ARGS) {
  if (!rank_out || !n_heavy_out || !label_out || !n_hbonds_out || !cbonds_out || !nodes_out || !status_out) return GAUDI_E_INVALID;
  const char* why = "";
  if (int rc = gaudi::canon_prepare(n_elems, h_elem, c_elem, B, A, M, elem, n_atoms, bonds, n_bonds, &why)) return rc;
  if (B == 0) return GAUDI_OK;
  const size_t nB = (size_t)B;
  memset(rank_out, 0, sizeof(int) * nB * A);
  memset(n_heavy_out, 0, sizeof(int) * nB);
  memset(label_out, 0, nB * A);
  memset(n_hbonds_out, 0, sizeof(int) * nB);
  memset(cbonds_out, 0, sizeof(uint16_t) * nB * M * 2);
  memset(nodes_out, 0, sizeof(int) * nB);
  memset(status_out, 0, sizeof(int) * nB);
  gaudi::CanonParams P{};
  P.B = B;
  P.A = A;
  P.M = M;
  P.n_elems = n_elems;
  P.h_elem = h_elem;
  P.c_elem = c_elem;
  P.elem = elem;
  P.n_atoms = n_atoms;
  P.bonds = bonds;
  P.n_bonds = n_bonds;
  P.rank = rank_out;
  P.n_heavy = n_heavy_out;
  P.label = label_out;
  P.n_hbonds = n_hbonds_out;
  P.cbonds = cbonds_out;
  P.nodes = nodes_out;
  P.status = status_out;
  std::vector<gaudi::CanonSmem> S(1);
  for (int b = 0; b < B; ++b) gaudi::canonical_order(P, S[0], b, 0);
  return GAUDI_OK;
}
#undef GAUDI_CANON_ARGS
