// stability.inc -- graph-of-rings stability check on the device (included at the end of gaudi_hip.hip).
//
// Replaces analyze/analyze.py:50-100 (check_stability) with its helpers positions2adj (utils/helpers.py:167-190),
// find_triplets_quads / angel3 / angel4 (analyze/analyze.py:234-319) and check_angels3/4 (:21-47): the step that
// follows sampling in eval_validity.py and sampling_edm.py:96.
//
// One 64-lane wave per molecule, four molecules per workgroup; everything lives in registers / 5 KB of LDS per wave:
//   1. orientation-node test (hetero), ring positions + types -> LDS;
//   2. lane i builds row i of the distance matrix, the 32-bit adjacency mask and the too-close flag;
//   3. breadth-first tree from ring 0 exactly as networkx yields it for from_numpy_array graphs (FIFO, neighbours in
//      ascending index) -- the reference only finds the 3-ring paths that touch a tree edge, so the tree is part of
//      the result; run redundantly by all lanes on wave-uniform data (no divergence, no synchronisation);
//   4. lanes = (side, k): for every tree edge the 2 x 32 candidate triplets are tested in parallel: 3-ring angle windows
//      of the centre ring type, then both quad extensions of every non-straight triplet with the dihedral rule.
// Arithmetic follows torch's CPU kernels operation by operation (unfused dot, fused norm -- see the oracle) with explicit
// individually rounded operations (contraction disabled) so that hipcc cannot fuse differently; thresholds arrive pre-multiplied by (1 -/+ tol)
// in double and rounded to fp32, which is what torch's scalar-tensor comparison does.

namespace gaudi {

constexpr int kStabMaxRings = 32;
constexpr int kStabMaxTypes = 16;

struct StabTables {
  int n_types, orientation, check_dihedrals, orient_type;
  float min_thr;                               // min_dist * (1 - tol)
  float lo[kStabMaxTypes][kStabMaxTypes];      // dist_lo * (1 - tol)
  float hi[kStabMaxTypes][kStabMaxTypes];      // dist_hi * (1 + tol); 0 = pair never bonds
  int a3_count[kStabMaxTypes];
  float a3_lo[kStabMaxTypes][4], a3_hi[kStabMaxTypes][4];
  float a4_180_thr, a4_0_thr;                  // a4["180"] * (1 - tol), a4["0"] * (1 + tol)
};

struct StabSmem {
  float x[kStabMaxRings][3];
  int type[kStabMaxRings];
  unsigned adj[kStabMaxRings];
  unsigned trip[kStabMaxRings][kStabMaxRings];  // [centre][a] bit b : de-duplicated triplets (a < b)
  int queue[kStabMaxRings], te_p[kStabMaxRings], te_c[kStabMaxRings];  // BFS state, written identically by all lanes
};

struct V3 { float x, y, z; };

// Individually rounded fp32 operations.  (HIP's __fmul_rn / __fadd_rn / __fsqrt_rn are NOT that on this toolchain: without
// OCML_BASIC_ROUNDED_OPERATIONS they are plain operators -- contractable into FMAs -- and the *native*, 1-ulp sqrt.)
// `#pragma clang fp contract(off)` forbids fusing; `/` and sqrtf are correctly rounded by hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }
__device__ __forceinline__ float sqrt_rn(float a) { return sqrtf(a); }
__device__ __forceinline__ float fma_rn(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

__device__ __forceinline__ V3 sub3(const float* a, const float* b) {
  return {sub_rn(a[0], b[0]), sub_rn(a[1], b[1]), sub_rn(a[2], b[2])};
}
// torch.dot (CPU, n = 3): unfused products summed in index order
__device__ __forceinline__ float dot3(V3 a, V3 b) {
  return add_rn(add_rn(mul_rn(a.x, b.x), mul_rn(a.y, b.y)), mul_rn(a.z, b.z));
}
// torch.norm (CPU, n = 3): fused multiply-add chain, then sqrt
__device__ __forceinline__ float norm3(V3 a) {
  return sqrt_rn(fma_rn(a.z, a.z, fma_rn(a.y, a.y, mul_rn(a.x, a.x))));
}
constexpr float kRad2Deg = 57.29577951308232f;

// coord2distances / positions2adj (utils/helpers.py:165-196) for one ring pair: shared with atoms.inc, so that both kernels agree
// bit for bit on which rings are fused
__device__ __forceinline__ float ring_dist(const float* a, const float* b) {
  const V3 d = sub3(a, b);
  return sqrt_rn(add_rn(add_rn(mul_rn(d.x, d.x), mul_rn(d.y, d.y)), mul_rn(d.z, d.z)));
}
__device__ __forceinline__ bool ring_bonded(const StabTables& T, int ti, int tj, float dist) {
  return T.hi[ti][tj] > 0.f && T.lo[ti][tj] < dist && dist < T.hi[ti][tj];
}

// analyze/analyze.py:234-240
__device__ __forceinline__ float angle3(const StabSmem& s, int a, int c, int b) {
  const V3 v1 = sub3(s.x[a], s.x[c]), v2 = sub3(s.x[b], s.x[c]);
  const float cosv = div_rn(dot3(v1, v2), mul_rn(norm3(v1), norm3(v2)));
  const float ang = mul_rn(acosf(cosv), kRad2Deg);
  return ang >= 0.f ? ang : ang + 360.f;
}

// analyze/analyze.py:243-270
__device__ __forceinline__ float angle4(const StabSmem& s, int i0, int i1, int i2, int i3) {
  const V3 d01 = sub3(s.x[i1], s.x[i0]);
  const V3 b0 = {mul_rn(-1.0f, d01.x), mul_rn(-1.0f, d01.y), mul_rn(-1.0f, d01.z)};
  V3 b1 = sub3(s.x[i2], s.x[i1]);
  const V3 b2 = sub3(s.x[i3], s.x[i2]);
  const float nb = norm3(b1);
  b1 = {div_rn(b1.x, nb), div_rn(b1.y, nb), div_rn(b1.z, nb)};
  const float p0 = dot3(b0, b1), p2 = dot3(b2, b1);
  const V3 v = {sub_rn(b0.x, mul_rn(p0, b1.x)), sub_rn(b0.y, mul_rn(p0, b1.y)), sub_rn(b0.z, mul_rn(p0, b1.z))};
  const V3 w = {sub_rn(b2.x, mul_rn(p2, b1.x)), sub_rn(b2.y, mul_rn(p2, b1.y)), sub_rn(b2.z, mul_rn(p2, b1.z))};
  const float xx = dot3(v, w);
  const V3 c = {sub_rn(mul_rn(b1.y, v.z), mul_rn(b1.z, v.y)), sub_rn(mul_rn(b1.z, v.x), mul_rn(b1.x, v.z)),
                sub_rn(mul_rn(b1.x, v.y), mul_rn(b1.y, v.x))};
  const float yy = dot3(c, w);
  return fabsf(mul_rn(atan2f(yy, xx), kRad2Deg));
}

struct StabParams {
  int B, N;
  const float* x;        // [B][N][3]
  const int* type;       // [B][N]
  const int* n_nodes;    // [B]
  unsigned char* flags;  // [B][5]
  float* dist;           // [B][N][N] or nullptr
  float* adj;            // [B][N][N] or nullptr
  gaudi_stability_aux* aux;  // [B] or nullptr
};

__global__ __launch_bounds__(256) void stability_kernel(const StabParams P, const StabTables* __restrict__ Tp) {
  const StabTables& T = *Tp;  // 2.7 KB of tables in global memory (L1/L2 resident), indexed per lane
  __shared__ StabSmem smem[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + w;
  if (b >= P.B) return;
  StabSmem& s = smem[w];
  const int N = P.N;
  const int n = P.n_nodes[b];
  const float* xb = P.x + (size_t)b * N * 3;
  const int* tb = P.type + (size_t)b * N;
  unsigned char* fl = P.flags + (size_t)b * 5;
  gaudi_stability_aux aux;
  aux.n_rings = 0; aux.n_edges = 0; aux.n_triplets = 0; aux.n_nan_angles = 0;
  aux.a3_min = INFINITY; aux.a3_max = -INFINITY; aux.a4_min = INFINITY; aux.a4_max = -INFINITY;
  bool f_or = true, f_dist = false, f_conn = false, f_a3 = false, f_a4 = false;

  int nr = n;
  if (T.orientation) {
    // analyze/analyze.py:66-78: second half = orientation nodes, all of the '.' type, none among the rings
    nr = n / 2;
    bool bad = false;
    for (int i = lane; i < n; i += 64) {
      const int t = tb[i];
      bad |= (i < nr) ? (t == T.orient_type) : (t != T.orient_type);
    }
    if (__ballot(bad) != 0ull || n - nr < 1) f_or = false;
  }
  aux.n_rings = nr;
  if (f_or) {
    for (int i = lane; i < nr * 3; i += 64) s.x[i / 3][i % 3] = xb[i];
    for (int i = lane; i < nr; i += 64) s.type[i] = tb[i];
    for (int i = lane; i < kStabMaxRings * kStabMaxRings; i += 64) (&s.trip[0][0])[i] = 0u;
    wave_lds_fence();

    // ---- rows of dist / adjacency (utils/helpers.py:159-190), too-close test (analyze/analyze.py:84-86)
    bool close = false;
    unsigned row = 0u;
    if (lane < nr) {
      const int ti = s.type[lane];
      for (int j = 0; j < nr; ++j) {
        const float dist = ring_dist(s.x[lane], s.x[j]);
        const int tj = s.type[j];
        const bool bonded = j != lane && ring_bonded(T, ti, tj, dist);
        row |= bonded ? (1u << j) : 0u;
        close |= j != lane && dist < T.min_thr;
        if (P.dist) P.dist[((size_t)b * N + lane) * N + j] = dist;
        if (P.adj) P.adj[((size_t)b * N + lane) * N + j] = bonded ? 1.f : 0.f;
      }
      s.adj[lane] = row;
    }
    wave_lds_fence();
    f_dist = __ballot(close) == 0ull;
    aux.n_edges = 0;
    {
      int deg = lane < nr ? __popc(row) : 0;
      for (int off = 32; off > 0; off >>= 1) deg += __shfl_xor(deg, off);
      aux.n_edges = deg / 2;
    }
  }

  if (f_or && f_dist && nr > 0) {
    // ---- BFS tree from ring 0 (nx.bfs_edges order), wave-uniform
    unsigned seen = 1u;
    int qh = 0, qt = 0, ne = 0;
    s.queue[qt++] = 0;
    while (qh < qt) {
      wave_lds_fence();
      const int u = s.queue[qh++];
      unsigned fresh = s.adj[u] & ~seen;
      seen |= fresh;
      while (fresh) {
        const int v = __ffs(fresh) - 1;
        fresh &= fresh - 1;
        s.te_p[ne] = u;
        s.te_c[ne] = v;
        ++ne;
        s.queue[qt++] = v;
      }
    }
    wave_lds_fence();
    f_conn = seen == (nr >= 32 ? 0xffffffffu : ((1u << nr) - 1u));

    if (f_conn) {
      // ---- triplets around every tree edge; lanes = (side, k)
      const int side = lane >> 5, k = lane & 31;
      bool bad3 = false, bad4 = false;
      float a3min = INFINITY, a3max = -INFINITY, a4min = INFINITY, a4max = -INFINITY;
      int nan_cnt = 0;
      for (int e = 0; e < ne; ++e) {
        const int c = side ? s.te_c[e] : s.te_p[e];  // centre ring
        const int o = side ? s.te_p[e] : s.te_c[e];  // the other end of the tree edge
        const unsigned nb_c = s.adj[c];
        if (k < nr && ((nb_c >> k) & 1u) && k != o) {
          const int a = o < k ? o : k, bb = o < k ? k : o;  // canonical orientation (analyze.py:287)
          const unsigned bit = 1u << bb;
          const unsigned old = atomicOr(&s.trip[c][a], bit);
          if ((old & bit) == 0u) {  // first time this triplet is seen (the reference de-duplicates with set())
            const float ang = angle3(s, a, c, bb);
            if (ang != ang) ++nan_cnt;
            a3min = fminf(a3min, ang);
            a3max = fmaxf(a3max, ang);
            // check_angels3 (analyze.py:21-36): inside any window of the centre ring type
            const int tc = s.type[c];
            bool ok = false;
            for (int q = 0; q < T.a3_count[tc]; ++q) ok |= T.a3_lo[tc][q] <= ang && ang <= T.a3_hi[tc][q];
            bad3 |= !ok;
            if (!(170.f < ang && ang < 190.f)) {
              // quads (analyze.py:293-309): extend both ends unless the new 3-ring angle is straight
              unsigned m = s.adj[a] & ~((1u << c) | (1u << bb));
              while (m) {
                const int n4 = __ffs(m) - 1;
                m &= m - 1;
                const float an = angle3(s, n4, a, c);
                if (!(175.f < an && an < 185.f)) {
                  const float d = n4 < bb ? angle4(s, n4, a, c, bb) : angle4(s, bb, c, a, n4);
                  a4min = fminf(a4min, d);
                  a4max = fmaxf(a4max, d);
                  bad4 |= !(T.a4_180_thr <= d || d <= T.a4_0_thr);
                }
              }
              m = s.adj[bb] & ~((1u << a) | (1u << c));
              while (m) {
                const int n4 = __ffs(m) - 1;
                m &= m - 1;
                const float an = angle3(s, c, bb, n4);
                if (!(175.f < an && an < 185.f)) {
                  const float d = a < n4 ? angle4(s, a, c, bb, n4) : angle4(s, n4, bb, c, a);
                  a4min = fminf(a4min, d);
                  a4max = fmaxf(a4max, d);
                  bad4 |= !(T.a4_180_thr <= d || d <= T.a4_0_thr);
                }
              }
            }
          }
        }
      }
      f_a3 = __ballot(bad3) == 0ull;
      f_a4 = T.check_dihedrals ? (__ballot(bad4) == 0ull) : true;
      for (int off = 32; off > 0; off >>= 1) {
        a3min = fminf(a3min, __shfl_xor(a3min, off));
        a3max = fmaxf(a3max, __shfl_xor(a3max, off));
        a4min = fminf(a4min, __shfl_xor(a4min, off));
        a4max = fmaxf(a4max, __shfl_xor(a4max, off));
        nan_cnt += __shfl_xor(nan_cnt, off);
      }
      wave_lds_fence();
      int cnt = 0;
      for (int i = lane; i < nr * nr; i += 64) cnt += __popc(s.trip[i / nr][i % nr]);
      for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
      aux.n_triplets = cnt;
      aux.n_nan_angles = nan_cnt;
      aux.a3_min = a3min; aux.a3_max = a3max; aux.a4_min = a4min; aux.a4_max = a4max;
    }
  }
  if (lane == 0) {
    fl[0] = f_or; fl[1] = f_dist; fl[2] = f_conn; fl[3] = f_a3; fl[4] = f_a4;
    if (P.aux) P.aux[b] = aux;
  }
}

}  // namespace gaudi

// The device image of gaudi_ring_tables: `tol` applied as the reference does, then fp32 (shared with atoms.inc).
static int stab_device_tables(gaudi_handle* h, const gaudi_ring_tables* tb, gaudi::StabTables& T) {
  const double tol = tb->tol;
  T.n_types = tb->n_types;
  T.orientation = tb->orientation;
  T.check_dihedrals = tb->check_dihedrals;
  T.orient_type = tb->n_types - 1;
  T.min_thr = (float)(tb->min_dist * (1 - tol));
  for (int i = 0; i < tb->n_types; ++i) {
    for (int j = 0; j < tb->n_types; ++j) {
      T.lo[i][j] = (float)(tb->dist_lo[i][j] * (1 - tol));
      T.hi[i][j] = tb->dist_hi[i][j] > 0 ? (float)(tb->dist_hi[i][j] * (1 + tol)) : 0.f;
    }
    if (tb->a3_count[i] < 0 || tb->a3_count[i] > 4) return fail(h, GAUDI_E_INVALID, "a3_count must be in 0..4");
    T.a3_count[i] = tb->a3_count[i];
    for (int q = 0; q < tb->a3_count[i]; ++q) {
      T.a3_lo[i][q] = (float)(tb->a3_lo[i][q] * (1 - tol));
      T.a3_hi[i][q] = (float)(tb->a3_hi[i][q] * (1 + tol));
    }
  }
  T.a4_180_thr = (float)(tb->a4_180 * (1 - tol));
  T.a4_0_thr = (float)(tb->a4_0 * (1 + tol));
  return GAUDI_OK;
}

extern "C" int gaudi_check_stability(gaudi_handle* h, const gaudi_ring_tables* tb, int B, int N, const float* x,
                                     const int32_t* ring_type, const int32_t* n_nodes, uint8_t* flags_out,
                                     float* dist_out, float* adj_out, gaudi_stability_aux* aux_out) {
  if (!h || !tb || !x || !ring_type || !n_nodes || !flags_out || B < 0 || N < 1) return GAUDI_E_INVALID;
  if (tb->n_types < 1 || tb->n_types > gaudi::kStabMaxTypes) return fail(h, GAUDI_E_INVALID, "n_types must be in 1..16");
  if (B == 0) return GAUDI_OK;
  const int max_rings = gaudi::kStabMaxRings;
  for (int b = 0; b < B; ++b) {
    const int n = n_nodes[b];
    if (n < 1 || n > N) return fail(h, GAUDI_E_INVALID, "n_nodes must be in 1..N (an empty molecule has no stability)");
    if ((tb->orientation ? n / 2 : n) > max_rings) return fail(h, GAUDI_E_CAPACITY, "more than 32 rings in one molecule");
    for (int i = 0; i < n; ++i) {
      const int t = ring_type[(size_t)b * N + i];
      if (t < 0 || t >= tb->n_types) return fail(h, GAUDI_E_INVALID, "ring type outside the table");
    }
  }
  HIPCHECK(h, hipSetDevice(h->device));
  gaudi::StabTables T{};
  if (int rc = stab_device_tables(h, tb, T)) return rc;

  const size_t xb = sizeof(float) * (size_t)B * N * 3, tbytes = sizeof(int) * (size_t)B * N, nn = (size_t)B * N * N;
  HIPCHECK(h, h->d_sx.reserve(xb));
  HIPCHECK(h, h->d_stype.reserve(tbytes));
  HIPCHECK(h, h->d_sn.reserve(sizeof(int) * B));
  HIPCHECK(h, h->d_sflags.reserve((size_t)B * 5));
  if (dist_out) HIPCHECK(h, h->d_sdist.reserve(sizeof(float) * nn));
  if (adj_out) HIPCHECK(h, h->d_sadj.reserve(sizeof(float) * nn));
  if (aux_out) HIPCHECK(h, h->d_saux.reserve(sizeof(gaudi_stability_aux) * B));
  HIPCHECK(h, hipMemcpyAsync(h->d_sx.p, x, xb, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(h->d_stype.p, ring_type, tbytes, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipMemcpyAsync(h->d_sn.p, n_nodes, sizeof(int) * B, hipMemcpyHostToDevice, h->stream));
  if (dist_out) HIPCHECK(h, hipMemsetAsync(h->d_sdist.p, 0, sizeof(float) * nn, h->stream));
  if (adj_out) HIPCHECK(h, hipMemsetAsync(h->d_sadj.p, 0, sizeof(float) * nn, h->stream));
  gaudi::StabParams P{};
  P.B = B;
  P.N = N;
  P.x = h->d_sx.as<float>();
  P.type = h->d_stype.as<int>();
  P.n_nodes = h->d_sn.as<int>();
  P.flags = h->d_sflags.as<unsigned char>();
  P.dist = dist_out ? h->d_sdist.as<float>() : nullptr;
  P.adj = adj_out ? h->d_sadj.as<float>() : nullptr;
  P.aux = aux_out ? h->d_saux.as<gaudi_stability_aux>() : nullptr;
  HIPCHECK(h, h->d_stab.reserve(sizeof(T)));
  HIPCHECK(h, hipMemcpyAsync(h->d_stab.p, &T, sizeof(T), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));  // T is a stack object
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (h->prof) HIPCHECK(h, h->stab_log.begin(h->stream, ev));
  hipLaunchKernelGGL(gaudi::stability_kernel, dim3((B + 3) / 4), dim3(256), 0, h->stream, P,
                     (const gaudi::StabTables*)h->d_stab.p);
  HIPCHECK(h, hipGetLastError());
  if (h->prof) HIPCHECK(h, h->stab_log.end(h->stream, ev));
  HIPCHECK(h, hipMemcpyAsync(flags_out, h->d_sflags.p, (size_t)B * 5, hipMemcpyDeviceToHost, h->stream));
  if (dist_out) HIPCHECK(h, hipMemcpyAsync(dist_out, h->d_sdist.p, sizeof(float) * nn, hipMemcpyDeviceToHost, h->stream));
  if (adj_out) HIPCHECK(h, hipMemcpyAsync(adj_out, h->d_sadj.p, sizeof(float) * nn, hipMemcpyDeviceToHost, h->stream));
  if (aux_out)
    HIPCHECK(h, hipMemcpyAsync(aux_out, h->d_saux.p, sizeof(gaudi_stability_aux) * B, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  // nx.is_connected raises on the null graph (a hetero "molecule" made of one orientation node): same here
  for (int b = 0; b < B; ++b)
    if (tb->orientation && n_nodes[b] / 2 == 0 && flags_out[(size_t)b * 5 + 0])
      return fail(h, GAUDI_E_INVALID, "molecule without rings: connectivity is undefined for the null graph");
  return GAUDI_OK;
}

extern "C" int gaudi_stability_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms) {
  if (!h || !n_launches || !total_ms) return GAUDI_E_INVALID;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, h->stab_log.fold(0));
  *n_launches = (int32_t)h->stab_log.n;
  *total_ms = h->stab_log.ms;
  return GAUDI_OK;
}
