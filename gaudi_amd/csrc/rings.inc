// rings.inc -- graph of atoms -> graph of rings on the device (included after atoms.inc at the end of gaudi_hip.hip).
//
// The inverse of atoms.inc.  Replaces, per molecule, utils/molgraph.py:37-80 (get_connectivity_matrix, skip_hydrogen=True),
// utils/ring_graph.py:12-93 (get_ring_type, get_rings) and :120-128 (get_rings_adj): what data/aromatic_dataloader.py:131-152 runs in
// Python and caches to disk.  One 64-lane wave per molecule, one launch per call, statuses in place of exceptions.
//
// ONE text, two builds: perceive_rings is __host__ __device__.  On the device the `lanes` of a phase are the 64 lanes of a wave, on
// the host there is one lane that walks every index of a phase serially (kRwLanes); the cross-lane helpers (rw_scan, rw_min,
// rw_any, rw_fence) are wave operations there and identities here.  Every per-item result is computed by ONE lane from LDS state the
// previous phase completed, and every order-dependent output is sorted, so the result does not depend on the lane count: the device
// output is bit-identical to gaudi_host_atoms_to_rings, which the CPU suite holds against the reference.
//
// Per wave, 12.4 KB of LDS (two waves per workgroup):
//   1. heavy atoms compacted by a prefix scan (ascending atom index), coordinates and elements -> LDS;
//   2. lane h builds row h of the heavy-atom adjacency (192-bit rows): sqrt(dx^2 + dy^2 + dz^2) <= (r_i + r_j) * factor in float64,
//      without contraction, which is symmetric in (i, j) bit for bit;
//   3. components C by min-label propagation to the fixpoint; E from the row popcounts; cyclomatic number E - V + C;
//   4. chordless cycles of 4..6 atoms: lane a walks the chordless paths that start at atom a and visit larger atoms only, and closes
//      them on a with second atom < last atom -- every cycle once.  Counted first, then stored at the prefix of the counts;
//   5. there must be no triangle, the count must be the cyclomatic number and the cycles independent over GF(2) (elimination on
//      their edge-incidence rows, one row per lane, at most 32 pivot steps).  Then they span the cycle space, every other cycle is a
//      sum of SHORTER-or-equal chordless ones that come first in the greedy (matroid) order, and the set is THE minimum cycle
//      basis, whatever the tie-breaking of networkx.  Otherwise: NOT_A_BASIS;
//   6. rank sort by the sorted atom tuple (54-bit keys); lane r: type of ring r from the element multiset, Db / DhDb by the H
//      neighbours of its B atoms, centre (sum in ascending atom index, then / size), orientation candidates; ring-ring adjacency.

namespace gaudi {

constexpr int kRingWaves = 2;
constexpr int kRingMaxAtoms = GAUDI_RINGS_MAX_ATOMS;
constexpr int kRingMaxHeavy = GAUDI_RINGS_MAX_HEAVY;
constexpr int kRingMaxRings = GAUDI_RINGS_MAX_RINGS;
constexpr int kRingWords = kRingMaxHeavy / 32;  // words of an adjacency row
constexpr int kRingEdgeWords = 8;               // E = V - C + rings <= 192 + 32 edges once the count check has passed
constexpr int kRingMaxElems = 8;
static_assert(kRingMaxHeavy % 32 == 0 && kRingMaxHeavy + kRingMaxRings <= 32 * kRingEdgeWords && kRingMaxHeavy <= 256, "capacities");

struct RingPerceiveTables {
  int n_elems, n_types, h_elem, c_elem, b_elem, db_type, dhdb_type;
  double radius[kRingMaxElems];
  unsigned sig[kStabMaxTypes];  // element multiset of the type: 4-bit counts by element index; 0 = not a ring of this dataset
  int no_orient[kStabMaxTypes];
};

struct RingSmem {
  double hx[kRingMaxHeavy][3];
  unsigned adj[kRingMaxHeavy][kRingWords];
  unsigned short hv[kRingMaxHeavy];     // heavy index -> atom index
  unsigned short label[kRingMaxHeavy];  // components; then the edge-number base of each row
  unsigned char he[kRingMaxHeavy];
  unsigned char ring[kRingMaxRings][6], sring[kRingMaxRings][6];  // heavy indices ascending; as found, and sorted by key
  unsigned char rsize[kRingMaxRings], ssize[kRingMaxRings];
  unsigned long long key[kRingMaxRings];
  unsigned ev[kRingMaxRings][kRingEdgeWords];
  unsigned char used[kRingMaxRings];
  unsigned amask[kRingMaxRings][kRingWords];  // atom sets of the sorted rings
};

struct RingParams {
  int B, A, flags, max_rings;
  double factor;
  const double* xyz;
  const int* elem;
  const int* n_atoms;
  int* status;
  int* n_rings;
  int* ring_size;
  int* ring_atoms;
  int* ring_type;
  double* centre;
  int* n_orient;
  double* orient;
  unsigned char* adj;
};

#if defined(__HIP_DEVICE_COMPILE__)
constexpr int kRwLanes = 64;
#else
constexpr int kRwLanes = 1;
#endif

__host__ __device__ __forceinline__ void rw_fence() {
#if defined(__HIP_DEVICE_COMPILE__)
  wave_lds_fence();
#endif
}
// exclusive prefix sum over the lanes; total = the sum
__host__ __device__ __forceinline__ int rw_scan(int v, int lane, int& total) {
#if defined(__HIP_DEVICE_COMPILE__)
  return wave_excl_scan(v, lane, total);
#else
  (void)lane;
  total = v;
  return 0;
#endif
}
__host__ __device__ __forceinline__ int rw_min(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
#endif
  return v;
}
__host__ __device__ __forceinline__ bool rw_any(bool p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ballot(p) != 0ull;
#else
  return p;
#endif
}

__host__ __device__ __forceinline__ bool ring_bit(const RingSmem& s, int u, int v) { return (s.adj[u][v >> 5] >> (v & 31)) & 1u; }

// Chordless cycles of 4..6 atoms whose smallest atom is a0, each once (second atom < last atom).  Returns their number; with
// `store` they are written, atoms ascending, to s.ring[base ...] (the caller has checked the capacity).
__host__ __device__ inline int ring_enum(RingSmem& s, int a0, bool store, int base, bool& triangle) {
  int path[5], word[5];
  unsigned bits[5];
  int count = 0, k = 0;
  path[0] = a0;
  word[0] = 0;
  bits[0] = s.adj[a0][0];
  while (k >= 0) {
    while (bits[k] == 0u && word[k] < kRingWords - 1) {
      ++word[k];
      bits[k] = s.adj[path[k]][word[k]];
    }
    if (bits[k] == 0u) {
      --k;
      continue;
    }
    const int w = word[k] * 32 + __builtin_ctz(bits[k]);
    bits[k] &= bits[k] - 1u;
    if (w <= a0) continue;
    bool ok = true;  // not on the path, no chord to the path's inner atoms (path[k] is w's predecessor)
    for (int q = 1; q < k; ++q) ok = ok && w != path[q] && !ring_bit(s, path[q], w);
    if (!ok) continue;
    if (k >= 1 && ring_bit(s, a0, w)) {  // closes on a0; a triangle (k == 1) is no ring and cannot be extended either
      triangle = triangle || k == 1;
      if (k >= 2 && path[1] < w) {
        if (store) {
          unsigned char* r = s.ring[base + count];
          const int n = k + 2;
          for (int q = 0; q <= k; ++q) r[q] = (unsigned char)path[q];
          r[k + 1] = (unsigned char)w;
          for (int i = 1; i < n; ++i) {  // insertion sort
            const unsigned char v = r[i];
            int j = i - 1;
            while (j >= 0 && r[j] > v) {
              r[j + 1] = r[j];
              --j;
            }
            r[j + 1] = v;
          }
          for (int q = n; q < 6; ++q) r[q] = 0;
          s.rsize[base + count] = (unsigned char)n;
        }
        ++count;
      }
      continue;
    }
    if (k <= 3) {  // k + 2 atoms on the path: one more closes a ring of at most 6
      ++k;
      path[k] = w;
      word[k] = 0;
      bits[k] = s.adj[w][0];
    }
  }
  return count;
}

// One molecule.  `s` is this wave's (host: this call's) working state; every `break` is lane-uniform.
__host__ __device__ inline void perceive_rings(const RingParams& P, const RingPerceiveTables& T, RingSmem& s, int b, int lane) {
#pragma clang fp contract(off)
  const int A = P.A, MR = P.max_rings;
  const int n = P.n_atoms[b];
  const double* xb = P.xyz + (size_t)b * A * 3;
  const int* eb = P.elem + (size_t)b * A;
  int status = GAUDI_RINGS_OK, R = 0;

  do {
    if (n > kRingMaxAtoms) { status = GAUDI_RINGS_OVERFLOW; break; }
    // ---- 1. heavy atoms, ascending
    const int per = (n + kRwLanes - 1) / kRwLanes, lo = lane * per, hi = lo + per < n ? lo + per : n;
    int cnt = 0;
    for (int a = lo; a < hi; ++a) cnt += eb[a] != T.h_elem;
    int H;
    int pos = rw_scan(cnt, lane, H);
    if (H > kRingMaxHeavy) { status = GAUDI_RINGS_OVERFLOW; break; }
    if (H == 0) { status = GAUDI_RINGS_NO_RINGS; break; }
    for (int a = lo; a < hi; ++a) {
      if (eb[a] == T.h_elem) continue;
      s.hv[pos] = (unsigned short)a;
      s.he[pos] = (unsigned char)eb[a];
      s.hx[pos][0] = xb[3 * a];
      s.hx[pos][1] = xb[3 * a + 1];
      s.hx[pos][2] = xb[3 * a + 2];
      ++pos;
    }
    rw_fence();

    // ---- 2. bonds (get_connectivity_matrix): row h of the adjacency by one lane
    int deg_sum = 0;
    for (int h = lane; h < H; h += kRwLanes) {
      const double x0 = s.hx[h][0], x1 = s.hx[h][1], x2 = s.hx[h][2], rh = T.radius[s.he[h]];
      unsigned row[kRingWords];
      for (int q = 0; q < kRingWords; ++q) row[q] = 0u;
      for (int j = 0; j < H; ++j) {
        if (j == h) continue;
        const double d0 = x0 - s.hx[j][0], d1 = x1 - s.hx[j][1], d2 = x2 - s.hx[j][2];
        const double cutoff = (rh + T.radius[s.he[j]]) * P.factor;
        const double dist = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        if (dist <= cutoff) {
          row[j >> 5] |= 1u << (j & 31);
          ++deg_sum;
        }
      }
      for (int q = 0; q < kRingWords; ++q) s.adj[h][q] = row[q];
      s.label[h] = (unsigned short)h;
    }
    rw_fence();

    // ---- 3. components: min-label propagation to the fixpoint (labels only fall, so racing reads are harmless)
    while (true) {
      bool changed = false;
      for (int h = lane; h < H; h += kRwLanes) {
        unsigned short m = s.label[h];
        for (int q = 0; q < kRingWords; ++q) {
          unsigned f = s.adj[h][q];
          while (f) {
            const unsigned short o = s.label[q * 32 + __builtin_ctz(f)];
            f &= f - 1u;
            m = o < m ? o : m;
          }
        }
        if (m < s.label[h]) {
          s.label[h] = m;
          changed = true;
        }
      }
      rw_fence();
      if (!rw_any(changed)) break;
    }
    int comp = 0;
    for (int h = lane; h < H; h += kRwLanes) comp += s.label[h] == h;
    int C, E2;
    (void)rw_scan(comp, lane, C);
    (void)rw_scan(deg_sum, lane, E2);
    const int E = E2 / 2, cyclo = E - H + C;
    rw_fence();

    // ---- 4. chordless cycles of 4..6 atoms, counted
    int mine = 0;
    bool triangle = false;
    for (int a = lane; a < H; a += kRwLanes) mine += ring_enum(s, a, false, 0, triangle);
    int base = rw_scan(mine, lane, R);
    // ---- 5a. as many as the cyclomatic number, and no triangle (a shorter cycle, which a minimum basis would take first)
    if (rw_any(triangle) || R != cyclo) { status = GAUDI_RINGS_NOT_A_BASIS; break; }
    if (R == 0) { status = GAUDI_RINGS_NO_RINGS; break; }
    if (R > kRingMaxRings || R > MR) { status = GAUDI_RINGS_OVERFLOW; break; }
    for (int a = lane; a < H; a += kRwLanes) base += ring_enum(s, a, true, base, triangle);
    // edge numbers: edge (u < v) = base of row u + rank of v among u's larger neighbours
    {
      const int hper = (H + kRwLanes - 1) / kRwLanes, hlo = lane * hper, hhi = hlo + hper < H ? hlo + hper : H;
      int up = 0;
      for (int h = hlo; h < hhi; ++h)
        for (int q = 0; q < kRingWords; ++q) {
          const unsigned above = q > (h >> 5) ? ~0u : q == (h >> 5) ? ~((2u << (h & 31)) - 1u) : 0u;
          up += __builtin_popcount(s.adj[h][q] & above);
        }
      int tot;
      int eb0 = rw_scan(up, lane, tot);
      for (int h = hlo; h < hhi; ++h) {
        s.label[h] = (unsigned short)eb0;
        for (int q = 0; q < kRingWords; ++q) {
          const unsigned above = q > (h >> 5) ? ~0u : q == (h >> 5) ? ~((2u << (h & 31)) - 1u) : 0u;
          eb0 += __builtin_popcount(s.adj[h][q] & above);
        }
      }
    }
    rw_fence();

    // ---- 5b. independent over GF(2).  A chordless cycle's edges are all the bonded pairs among its atoms.
    for (int r = lane; r < R; r += kRwLanes) {
      unsigned v[kRingEdgeWords];
      for (int q = 0; q < kRingEdgeWords; ++q) v[q] = 0u;
      const int sz = s.rsize[r];
      unsigned long long key = 0ull;
      for (int i = 0; i < sz; ++i) {
        const int u = s.ring[r][i];
        key |= (unsigned long long)(u + 1) << (9 * (5 - i));
        for (int j = i + 1; j < sz; ++j) {
          const int w = s.ring[r][j];
          if (!ring_bit(s, u, w)) continue;
          int rank = 0;  // neighbours of u in (u, w)
          for (int q = u >> 5; q <= (w >> 5); ++q) {
            unsigned m = s.adj[u][q];
            if (q == (u >> 5)) m &= ~((2u << (u & 31)) - 1u);
            if (q == (w >> 5)) m &= (1u << (w & 31)) - 1u;
            rank += __builtin_popcount(m);
          }
          const int e = s.label[u] + rank;
          v[e >> 5] ^= 1u << (e & 31);
        }
      }
      for (int q = 0; q < kRingEdgeWords; ++q) s.ev[r][q] = v[q];
      s.key[r] = key;
      s.used[r] = 0;
    }
    rw_fence();
    bool independent = true;
    for (int step = 0; step < R; ++step) {
      // the unused row with the lowest leading edge; a zero row among the unused ones is a dependency
      int best = 0x7fffffff;
      bool zero = false;
      for (int r = lane; r < R; r += kRwLanes) {
        if (s.used[r]) continue;
        int c = -1;
        for (int q = 0; q < kRingEdgeWords && c < 0; ++q)
          if (s.ev[r][q]) c = q * 32 + __builtin_ctz(s.ev[r][q]);
        if (c < 0) zero = true;
        else if (((c << 8) | r) < best) best = (c << 8) | r;
      }
      if (rw_any(zero)) { independent = false; break; }
      best = rw_min(best);
      const int p = best & 0xff, c = best >> 8;
      for (int r = lane; r < R; r += kRwLanes) {
        if (r == p || s.used[r] || !((s.ev[r][c >> 5] >> (c & 31)) & 1u)) continue;
        for (int q = 0; q < kRingEdgeWords; ++q) s.ev[r][q] ^= s.ev[p][q];
      }
      if (lane == 0) s.used[p] = 1;
      rw_fence();
    }
    if (!independent) { status = GAUDI_RINGS_NOT_A_BASIS; break; }

    // ---- 6. ring order: ascending by the sorted atom tuple
    for (int r = lane; r < R; r += kRwLanes) {
      const unsigned long long k = s.key[r];
      int rank = 0;
      for (int o = 0; o < R; ++o) rank += s.key[o] < k;
      for (int i = 0; i < 6; ++i) s.sring[rank][i] = s.ring[r][i];
      s.ssize[rank] = s.rsize[r];
      unsigned m[kRingWords];
      for (int q = 0; q < kRingWords; ++q) m[q] = 0u;
      for (int i = 0; i < s.rsize[r]; ++i) m[s.ring[r][i] >> 5] |= 1u << (s.ring[r][i] & 31);
      for (int q = 0; q < kRingWords; ++q) s.amask[rank][q] = m[q];
    }
    rw_fence();

    // ---- per ring: type (get_ring_type, the Db / DhDb rule), centre, orientation candidates (get_rings)
    bool bad = false;
    int my_type[(kRingMaxRings + kRwLanes - 1) / kRwLanes];
    for (int r = lane, it = 0; r < R; r += kRwLanes, ++it) {
      const int sz = s.ssize[r];
      unsigned sig = 0u;
      for (int i = 0; i < sz; ++i) sig += 1u << (4 * s.he[s.sring[r][i]]);
      int t = -1;
      for (int q = 0; q < T.n_types && t < 0; ++q)
        if (T.sig[q] == sig) t = q;
      if (t >= 0 && (t == T.db_type || t == T.dhdb_type)) {
        bool with_h = false;
        if (P.flags & GAUDI_RINGS_USE_H) {  // a B atom of the ring with an H in bonding distance
          for (int i = 0; i < sz; ++i) {
            const int u = s.sring[r][i];
            if (s.he[u] != T.b_elem) continue;
            const double cutoff = (T.radius[T.b_elem] + T.radius[T.h_elem]) * P.factor;
            for (int a = 0; a < n; ++a) {
              if (eb[a] != T.h_elem) continue;
              const double d0 = s.hx[u][0] - xb[3 * a], d1 = s.hx[u][1] - xb[3 * a + 1], d2 = s.hx[u][2] - xb[3 * a + 2];
              with_h = with_h || sqrt(d0 * d0 + d1 * d1 + d2 * d2) <= cutoff;
            }
          }
        }
        t = with_h ? T.dhdb_type : T.db_type;
      }
      my_type[it] = t;
      bad = bad || t < 0;
    }
    if (rw_any(bad)) { status = GAUDI_RINGS_BAD_TYPE; break; }

    // ---- outputs
    for (int r = lane, it = 0; r < R; r += kRwLanes, ++it) {
      const size_t o = (size_t)b * MR + r;
      const int sz = s.ssize[r], t = my_type[it];
      double c0 = 0.0, c1 = 0.0, c2 = 0.0;
      for (int i = 0; i < sz; ++i) {
        const int u = s.sring[r][i];
        P.ring_atoms[o * 6 + i] = s.hv[u];
        c0 += s.hx[u][0];
        c1 += s.hx[u][1];
        c2 += s.hx[u][2];
      }
      c0 = c0 / sz;
      c1 = c1 / sz;
      c2 = c2 / sz;
      P.ring_size[o] = sz;
      P.ring_type[o] = t;
      P.centre[o * 3] = c0;
      P.centre[o * 3 + 1] = c1;
      P.centre[o * 3 + 2] = c2;
      int no = 0;
      if (T.no_orient[t]) {
        P.orient[o * 6] = c0;
        P.orient[o * 6 + 1] = c1;
        P.orient[o * 6 + 2] = c2;
        no = 1;
      } else {
        for (int i = 0; i < sz && no < 2; ++i) {
          const int u = s.sring[r][i];
          if (s.he[u] == T.c_elem) continue;
          P.orient[o * 6 + 3 * no] = s.hx[u][0];
          P.orient[o * 6 + 3 * no + 1] = s.hx[u][1];
          P.orient[o * 6 + 3 * no + 2] = s.hx[u][2];
          ++no;
        }
      }
      P.n_orient[o] = no;
      for (int q = 0; q < R; ++q) {  // get_rings_adj: a shared atom
        bool share = false;
        for (int k = 0; k < kRingWords; ++k) share = share || (s.amask[r][k] & s.amask[q][k]);
        P.adj[o * MR + q] = (unsigned char)(share && q != r);
      }
    }
  } while (false);

  if (lane == 0) {
    P.status[b] = status;
    P.n_rings[b] = status ? 0 : R;
  }
}

__global__ __launch_bounds__(64 * kRingWaves) void rings_kernel(const RingParams P, const RingPerceiveTables* __restrict__ Tp) {
  __shared__ RingSmem smem[kRingWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * kRingWaves + w;
  if (b >= P.B) return;
  perceive_rings(P, *Tp, smem[w], b, lane);
}

// the arguments both entry points share, checked and turned into the kernel's tables
static int rings_prepare(const gaudi_perception_tables* pt, int B, int A, const double* xyz, const int32_t* elem, const int32_t* n_atoms,
                         int flags, double factor, int max_rings, RingPerceiveTables& T, const char** why) {
  *why = "invalid argument";
  if (!pt || !xyz || !elem || !n_atoms || B < 0 || A < 1) return GAUDI_E_INVALID;
  if (flags & ~GAUDI_RINGS_USE_H) { *why = "unknown flag"; return GAUDI_E_INVALID; }
  if (!(factor > 0.0)) { *why = "covalency_factor must be positive"; return GAUDI_E_INVALID; }
  if (max_rings < 1 || max_rings > kRingMaxRings) { *why = "max_rings must be in 1..32"; return GAUDI_E_INVALID; }
  if (pt->n_elems < 1 || pt->n_elems > kRingMaxElems || pt->n_types < 1 || pt->n_types > kStabMaxTypes) {
    *why = "n_elems must be in 1..8 and n_types in 1..16";
    return GAUDI_E_INVALID;
  }
  auto elem_ok = [&](int e, bool optional) { return (optional && e == -1) || (e >= 0 && e < pt->n_elems); };
  if (!elem_ok(pt->h_elem, false) || !elem_ok(pt->c_elem, false) || !elem_ok(pt->b_elem, true)) { *why = "h_elem / c_elem / b_elem outside the element list"; return GAUDI_E_INVALID; }
  auto type_ok = [&](int t) { return t == -1 || (t >= 0 && t < pt->n_types); };
  if (!type_ok(pt->db_type) || !type_ok(pt->dhdb_type) || (pt->db_type < 0) != (pt->dhdb_type < 0)) { *why = "db_type / dhdb_type: both or neither, inside the type list"; return GAUDI_E_INVALID; }
  T = RingPerceiveTables{};
  T.n_elems = pt->n_elems;
  T.n_types = pt->n_types;
  T.h_elem = pt->h_elem;
  T.c_elem = pt->c_elem;
  T.b_elem = pt->b_elem;
  T.db_type = pt->db_type;
  T.dhdb_type = pt->dhdb_type;
  if (T.db_type >= 0 && T.b_elem < 0) { *why = "db_type without b_elem"; return GAUDI_E_INVALID; }
  for (int e = 0; e < pt->n_elems; ++e) {
    if (!(pt->cov_radius[e] > 0.0)) { *why = "cov_radius must be positive"; return GAUDI_E_INVALID; }
    T.radius[e] = pt->cov_radius[e];
  }
  for (int t = 0; t < pt->n_types; ++t) {
    const int sz = pt->ring_size[t];
    if (sz != 0 && (sz < 4 || sz > 6)) { *why = "ring_size must be 0 or 4..6"; return GAUDI_E_INVALID; }
    unsigned sig = 0u;
    for (int k = 0; k < sz; ++k) {
      if (pt->ring_elem[t][k] < 0 || pt->ring_elem[t][k] >= pt->n_elems) { *why = "ring_elem outside the element list"; return GAUDI_E_INVALID; }
      sig += 1u << (4 * pt->ring_elem[t][k]);
    }
    T.sig[t] = sig;
    T.no_orient[t] = pt->no_orientation[t] != 0;
  }
  for (int b = 0; b < B; ++b) {
    const int n = n_atoms[b];
    if (n < 0 || n > A) { *why = "n_atoms must be in 0..A"; return GAUDI_E_INVALID; }
    for (int a = 0; a < n; ++a)
      if (elem[(size_t)b * A + a] < 0 || elem[(size_t)b * A + a] >= pt->n_elems) { *why = "element index outside the element list"; return GAUDI_E_INVALID; }
  }
  return GAUDI_OK;
}

// bytes of the nine outputs for B molecules, in the order status, n_rings, ring_size, ring_atoms, ring_type, centre, n_orient, orient, adj
static void rings_out_sizes(size_t nB, int MR, size_t out[9]) {
  const size_t m = (size_t)MR;
  out[0] = sizeof(int) * nB;
  out[1] = sizeof(int) * nB;
  out[2] = sizeof(int) * nB * m;
  out[3] = sizeof(int) * nB * m * 6;
  out[4] = sizeof(int) * nB * m;
  out[5] = sizeof(double) * nB * m * 3;
  out[6] = sizeof(int) * nB * m;
  out[7] = sizeof(double) * nB * m * 6;
  out[8] = nB * m * m;
}

}  // namespace gaudi

#define GAUDI_RINGS_OUT_ARGS                                                                                                      \
  int32_t *status_out, int32_t *n_rings_out, int32_t *ring_size_out, int32_t *ring_atoms_out, int32_t *ring_type_out,             \
      double *centre_out, int32_t *n_orient_out, double *orient_out, uint8_t *adj_out

extern "C" int gaudi_atoms_to_rings(gaudi_handle* h, const gaudi_perception_tables* pt, int B, int A, const double* xyz,
                                    const int32_t* elem, const int32_t* n_atoms, int flags, double covalency_factor, int max_rings,
                                    GAUDI_RINGS_OUT_ARGS) {
  if (!h || !status_out || !n_rings_out || !ring_size_out || !ring_atoms_out || !ring_type_out || !centre_out || !n_orient_out ||
      !orient_out || !adj_out)
    return GAUDI_E_INVALID;
  gaudi::RingPerceiveTables T;
  const char* why = "";
  if (int rc = gaudi::rings_prepare(pt, B, A, xyz, elem, n_atoms, flags, covalency_factor, max_rings, T, &why)) return fail(h, rc, why);
  if (B == 0) return GAUDI_OK;
  HIPCHECK(h, hipSetDevice(h->device));
  const size_t nB = (size_t)B;
  size_t osz[9];
  gaudi::rings_out_sizes(nB, max_rings, osz);
  const size_t isz[4] = {sizeof(double) * nB * A * 3, sizeof(int) * nB * A, sizeof(int) * nB, sizeof(gaudi::RingPerceiveTables)};
  const void* ins[4] = {xyz, elem, n_atoms, &T};
  for (int i = 0; i < 4; ++i) {
    HIPCHECK(h, h->d_rings[i].reserve(isz[i]));
    HIPCHECK(h, hipMemcpyAsync(h->d_rings[i].p, ins[i], isz[i], hipMemcpyHostToDevice, h->stream));
  }
  // entries beyond a molecule's rings are not written by the kernel: zero, and -1 for the atom lists
  for (int i = 0; i < 9; ++i) {
    HIPCHECK(h, h->d_rings[4 + i].reserve(osz[i]));
    HIPCHECK(h, hipMemsetAsync(h->d_rings[4 + i].p, i == 3 ? 0xff : 0, osz[i], h->stream));
  }
  HIPCHECK(h, hipStreamSynchronize(h->stream));  // T is a local object
  gaudi::RingParams P{};
  P.B = B;
  P.A = A;
  P.flags = flags;
  P.max_rings = max_rings;
  P.factor = covalency_factor;
  P.xyz = h->d_rings[0].as<double>();
  P.elem = h->d_rings[1].as<int>();
  P.n_atoms = h->d_rings[2].as<int>();
  P.status = h->d_rings[4].as<int>();
  P.n_rings = h->d_rings[5].as<int>();
  P.ring_size = h->d_rings[6].as<int>();
  P.ring_atoms = h->d_rings[7].as<int>();
  P.ring_type = h->d_rings[8].as<int>();
  P.centre = h->d_rings[9].as<double>();
  P.n_orient = h->d_rings[10].as<int>();
  P.orient = h->d_rings[11].as<double>();
  P.adj = h->d_rings[12].as<unsigned char>();
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (h->prof) HIPCHECK(h, h->rings_log.begin(h->stream, ev));
  hipLaunchKernelGGL(gaudi::rings_kernel, dim3((B + gaudi::kRingWaves - 1) / gaudi::kRingWaves), dim3(64 * gaudi::kRingWaves), 0,
                     h->stream, P, (const gaudi::RingPerceiveTables*)h->d_rings[3].p);
  HIPCHECK(h, hipGetLastError());
  if (h->prof) HIPCHECK(h, h->rings_log.end(h->stream, ev));
  void* outs[9] = {status_out, n_rings_out, ring_size_out, ring_atoms_out, ring_type_out, centre_out, n_orient_out, orient_out, adj_out};
  for (int i = 0; i < 9; ++i) HIPCHECK(h, hipMemcpyAsync(outs[i], h->d_rings[4 + i].p, osz[i], hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  return GAUDI_OK;
}

extern "C" int gaudi_rings_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms) {
  if (!h || !n_launches || !total_ms) return GAUDI_E_INVALID;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, h->rings_log.fold(0));
  *n_launches = (int32_t)h->rings_log.n;
  *total_ms = h->rings_log.ms;
  return GAUDI_OK;
}

extern "C" int gaudi_host_atoms_to_rings(const gaudi_perception_tables* pt, int B, int A, const double* xyz, const int32_t* elem,
                                         const int32_t* n_atoms, int flags, double covalency_factor, int max_rings,
                                         GAUDI_RINGS_OUT_ARGS) {
  if (!status_out || !n_rings_out || !ring_size_out || !ring_atoms_out || !ring_type_out || !centre_out || !n_orient_out ||
      !orient_out || !adj_out)
    return GAUDI_E_INVALID;
  std::vector<gaudi::RingPerceiveTables> Tv(1);
  const char* why = "";
  if (int rc = gaudi::rings_prepare(pt, B, A, xyz, elem, n_atoms, flags, covalency_factor, max_rings, Tv[0], &why)) return rc;
  if (B == 0) return GAUDI_OK;
  size_t osz[9];
  gaudi::rings_out_sizes((size_t)B, max_rings, osz);
  void* outs[9] = {status_out, n_rings_out, ring_size_out, ring_atoms_out, ring_type_out, centre_out, n_orient_out, orient_out, adj_out};
  for (int i = 0; i < 9; ++i) memset(outs[i], i == 3 ? 0xff : 0, osz[i]);
  gaudi::RingParams P{};
  P.B = B;
  P.A = A;
  P.flags = flags;
  P.max_rings = max_rings;
  P.factor = covalency_factor;
  P.xyz = xyz;
  P.elem = elem;
  P.n_atoms = n_atoms;
  P.status = status_out;
  P.n_rings = n_rings_out;
  P.ring_size = ring_size_out;
  P.ring_atoms = ring_atoms_out;
  P.ring_type = ring_type_out;
  P.centre = centre_out;
  P.n_orient = n_orient_out;
  P.orient = orient_out;
  P.adj = adj_out;
  std::vector<gaudi::RingSmem> S(1);
  for (int b = 0; b < B; ++b) gaudi::perceive_rings(P, Tv[0], S[0], b, 0);
  return GAUDI_OK;
}
#undef GAUDI_RINGS_OUT_ARGS
