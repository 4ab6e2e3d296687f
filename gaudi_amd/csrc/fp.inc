// fp.inc -- circular count fingerprints of graphs of atoms and their min/max (Tanimoto) similarity (included after canon.inc at the
// end of gaudi_hip.hip; DESIGN.md section 8j).
//
// The fingerprint.  The graph is canon.inc's (canon_graph reads and checks it): vertices = the non-hydrogen atoms, label =
// element * 8 + H count, deg = heavy neighbours.  All arithmetic is uint32_t and wraps:
//
//   mix(x):  x ^= x >> 16;  x *= 0x85ebca6b;  x ^= x >> 13;  x *= 0xc2b2ae35;  x ^= x >> 16
//   id_0(v) = mix(0x9e3779b9 + label(v) * 16 + deg(v))
//   id_r(v) = h after:  h = mix(r);  h = mix(h ^ id_{r-1}(v));  for the neighbours' id_{r-1} ascending:  h = mix(h ^ id)
//   fp[bin] = min(255, #{(v, r), r = 0..R : (id_r(v) & (n_bins - 1)) == bin}),  total = the sum of the stored bytes
//
// ONE text, two builds, as canon.inc: a 64-lane wave per molecule on the device (lanes are vertices, then bins), one lane that
// walks every index on the host.  The histogram is counted with integer adds in LDS, whose order does not matter.
//
// The similarity of rows a, b: common = sum min(a_i, b_i), union = total_a + total_b - common, similarity = common / union (0 when
// union = 0).  The kernels return the two integers.  fp_ahead is THE total order (device, host twin): larger similarity first by
// cross-multiplication in 64 bits, a union of 0 counting as similarity 0, equal similarity to the smaller library index.
//
// fp_nearest_kernel: a one-wave workgroup takes 64 * QPL queries (QPL per lane, register blocking: a library dword read from LDS
// serves QPL v_sad_u8) and one split of the library.  Per tile of 32 library rows and per slice of 64 bins the lane holds its
// queries' 16 dwords each, the tile's slice (2 KB) sits in LDS and is read with wave-uniform 16-byte reads, and 32 * QPL
// accumulators take sum |q_i - l_i|; common = (total_q + total_l - sad) / 2.  The next slice's global loads are issued before the
// current slice is computed.  A lane's running top-k lives in LDS (sorted, the
// k-th also in registers, so most candidates cost one comparison).  Per-split lists go to scratch and fp_merge_kernel (a wave per
// query) merges them by the same order: no atomics, and the result does not depend on the number of splits or the tile sizes.

namespace gaudi {

constexpr int kFpWaves = 2;
constexpr int kFpMaxBins = 1024;
constexpr int kFpMaxK = 16;
constexpr int kFpTile = 32;    // library rows per tile
constexpr int kFpSlice = 64;   // bins per slice: 16 dwords of a query in registers
constexpr int kFpPad = 0x7fffffff;  // the index of a list entry that holds no row: behind every row

struct FpSmem {
  CanonSmem g;
  unsigned int id[2][kCanonMaxHeavy];
  unsigned int hist[kFpMaxBins];
};

struct FpParams {
  CanonParams in;  // the input fields only
  int radius, n_bins;
  unsigned char* fp;
  int* total;
  int* status;
};

__host__ __device__ __forceinline__ unsigned int fp_mix(unsigned int x) {
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  x ^= x >> 16;
  return x;
}

__host__ __device__ __forceinline__ void fp_count(unsigned int* bin) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(bin, 1u);  // an LDS integer add: the sum does not depend on the order
#else
  ++*bin;
#endif
}

// x is ahead of y in the total order
__host__ __device__ __forceinline__ bool fp_ahead(int cx, int ux, int ix, int cy, int uy, int iy) {
  const long long l = (long long)cx * (uy > 0 ? uy : 1), r = (long long)cy * (ux > 0 ? ux : 1);
  return l != r ? l > r : ix < iy;
}

// One molecule.  Every branch around a fence is lane-uniform.
__host__ __device__ inline void circular_fingerprint(const FpParams& P, FpSmem& s, int b, int lane) {
  int H = 0, E = 0;
  const int status = canon_graph(P.in, s.g, b, lane, H, E);
  if (status == GAUDI_CANON_OK) {
    const unsigned int mask = (unsigned int)P.n_bins - 1u;
    for (int k = lane; k < P.n_bins; k += kRwLanes) s.hist[k] = 0u;
    rw_fence();
    for (int v = lane; v < H; v += kRwLanes) {
      int deg = 0;
      for (int k = 0; k < 8; ++k) deg += s.g.adj[v][k] != kCanonNone;
      const unsigned int id = fp_mix(0x9e3779b9u + (unsigned int)s.g.label[v] * 16u + (unsigned int)deg);
      s.id[0][v] = id;
      fp_count(&s.hist[id & mask]);
    }
    rw_fence();
    for (int r = 1; r <= P.radius; ++r) {
      const unsigned int* prev = s.id[(r - 1) & 1];
      unsigned int* next = s.id[r & 1];
      for (int v = lane; v < H; v += kRwLanes) {
        // signed order of (id ^ 2^31) = unsigned order of id; the padding is the largest value, so the first deg entries of
        // the sorted row are the neighbours' ids whatever they are
        int c[8];
        int deg = 0;
        for (int k = 0; k < 8; ++k) {
          const int o = s.g.adj[v][k];
          const bool there = o != kCanonNone;
          c[k] = there ? (int)(prev[there ? o : 0] ^ 0x80000000u) : 0x7fffffff;
          deg += there;
        }
        canon_sort8(c);
        unsigned int h = fp_mix((unsigned int)r);
        h = fp_mix(h ^ prev[v]);
        for (int k = 0; k < 8; ++k)
          if (k < deg) h = fp_mix(h ^ ((unsigned int)c[k] ^ 0x80000000u));
        next[v] = h;
        fp_count(&s.hist[h & mask]);
      }
      rw_fence();
    }
    int sum = 0;
    for (int k = lane; k < P.n_bins; k += kRwLanes) {
      const unsigned int c = s.hist[k] < 255u ? s.hist[k] : 255u;
      P.fp[(size_t)b * P.n_bins + k] = (unsigned char)c;
      sum += (int)c;
    }
    int total;
    (void)rw_scan(sum, lane, total);
    if (lane == 0) P.total[b] = total;
  }
  if (lane == 0) P.status[b] = status;
}

__global__ __launch_bounds__(64 * kFpWaves) void fp_kernel(const FpParams P) {
  __shared__ FpSmem smem[kFpWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * kFpWaves + w;
  if (b >= P.in.B) return;
  circular_fingerprint(P, smem[w], b, lane);
}

// ---- similarity ----------------------------------------------------------------------------------------------------------------

// total[row] = the sum of the row's bytes; one thread per row
__global__ __launch_bounds__(256) void fp_totals_kernel(const unsigned char* __restrict__ rows, int n_rows, int n_bins, int* __restrict__ total) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  const uint4* p = reinterpret_cast<const uint4*>(rows + (size_t)r * n_bins);
  unsigned int acc = 0u;
  for (int k = 0; k < n_bins / 16; ++k) {
    const uint4 v = p[k];
    acc = __builtin_amdgcn_sad_u8(v.x, 0u, acc);
    acc = __builtin_amdgcn_sad_u8(v.y, 0u, acc);
    acc = __builtin_amdgcn_sad_u8(v.z, 0u, acc);
    acc = __builtin_amdgcn_sad_u8(v.w, 0u, acc);
  }
  total[r] = (int)acc;
}

// A lane's sorted lists in LDS: entry j of query slot q of lane l at (j * QPL + q) * 64 + l (consecutive lanes, consecutive banks).
// Three arrays of k * QPL * 64 words in the launch's dynamic LDS: sized by the call's k, so k = 1 costs 768 * QPL bytes and not the
// 12 KB * QPL of k = 16, which alone would hold a CU to five workgroups.
struct FpLists {
  int *c, *u, *i;
};
__device__ __forceinline__ FpLists fp_lists(int* base, int words) { return FpLists{base, base + words, base + 2 * words}; }
static size_t fp_lists_bytes(int k, int qpl) { return sizeof(int) * 3 * (size_t)k * qpl * 64; }

// (cc, cu, ci) is ahead of the list's k-th entry: it takes its place in the order, and the new k-th comes back in (wc, wu, wi)
template <int QPL>
__device__ __forceinline__ void fp_insert(const FpLists& L, int q, int lane, int k, int cc, int cu, int ci, int& wc, int& wu, int& wi) {
  int j = k - 1;
  while (j > 0) {
    const int at = ((j - 1) * QPL + q) * 64 + lane;
    const int pc = L.c[at], pu = L.u[at], pi = L.i[at];
    if (!fp_ahead(cc, cu, ci, pc, pu, pi)) break;
    const int to = (j * QPL + q) * 64 + lane;
    L.c[to] = pc;
    L.u[to] = pu;
    L.i[to] = pi;
    --j;
  }
  const int to = (j * QPL + q) * 64 + lane;
  L.c[to] = cc;
  L.u[to] = cu;
  L.i[to] = ci;
  const int last = ((k - 1) * QPL + q) * 64 + lane;
  wc = L.c[last];
  wu = L.u[last];
  wi = L.i[last];
}

// sum |q - l| over all bins for the tile of kFpTile library rows from row0 (rows from `end` on read as zero) against the lane's QPL
// queries.  One wave; `tile` is its 2 KB of LDS.
template <int QPL>
__device__ __forceinline__ void fp_tile_sad(const unsigned char* __restrict__ lib, int row0, int end, int n_bins,
                                            const unsigned char* (&qrow)[QPL], uint4 (&tile)[kFpTile][4], int lane,
                                            unsigned int (&acc)[QPL][kFpTile]) {
#pragma unroll
  for (int q = 0; q < QPL; ++q)
#pragma unroll
    for (int r = 0; r < kFpTile; ++r) acc[q][r] = 0u;
  // the loads of slice sl + 1 are issued before slice sl is computed, so their latency hides behind its v_sad_u8
  const int n_slices = n_bins / kFpSlice, part = lane & 3;
  const unsigned char* lrow[2];
  bool there[2];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int row = row0 + (lane >> 2) + 16 * half;
    there[half] = row < end;
    lrow[half] = lib + (size_t)(there[half] ? row : row0) * n_bins + part * 16;
  }
  uint4 tnext[2], qnext[QPL][4];
#pragma unroll
  for (int half = 0; half < 2; ++half) tnext[half] = *reinterpret_cast<const uint4*>(lrow[half]);
#pragma unroll
  for (int q = 0; q < QPL; ++q)
#pragma unroll
    for (int p = 0; p < 4; ++p) qnext[q][p] = *reinterpret_cast<const uint4*>(qrow[q] + p * 16);
  for (int sl = 0; sl < n_slices; ++sl) {
    __syncthreads();  // the previous slice's reads before this slice's writes
#pragma unroll
    for (int half = 0; half < 2; ++half)
      tile[(lane >> 2) + 16 * half][part] = there[half] ? tnext[half] : make_uint4(0u, 0u, 0u, 0u);
    uint4 qv[QPL][4];
#pragma unroll
    for (int q = 0; q < QPL; ++q)
#pragma unroll
      for (int p = 0; p < 4; ++p) qv[q][p] = qnext[q][p];
    if (sl + 1 < n_slices) {
      const int off = (sl + 1) * kFpSlice;
#pragma unroll
      for (int half = 0; half < 2; ++half) tnext[half] = *reinterpret_cast<const uint4*>(lrow[half] + off);
#pragma unroll
      for (int q = 0; q < QPL; ++q)
#pragma unroll
        for (int p = 0; p < 4; ++p) qnext[q][p] = *reinterpret_cast<const uint4*>(qrow[q] + off + p * 16);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kFpTile; ++r)
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const uint4 l = tile[r][p];  // the same address in every lane: a broadcast read
#pragma unroll
        for (int q = 0; q < QPL; ++q) {
          unsigned int a = acc[q][r];
          a = __builtin_amdgcn_sad_u8(qv[q][p].x, l.x, a);
          a = __builtin_amdgcn_sad_u8(qv[q][p].y, l.y, a);
          a = __builtin_amdgcn_sad_u8(qv[q][p].z, l.z, a);
          a = __builtin_amdgcn_sad_u8(qv[q][p].w, l.w, a);
          acc[q][r] = a;
        }
      }
  }
}

struct FpNearestParams {
  const unsigned char* q;    // [B][n_bins]
  const int* qtot;           // [B]
  const unsigned char* lib;  // [M][n_bins]
  const int* ltot;           // [M]
  int B, M, n_bins, k, S, rows_per_split;  // rows_per_split: a multiple of kFpTile
  int* part;                 // [S][B][k][3]: common, union, index (kFpPad: no row)
};

template <int QPL>
__global__ __launch_bounds__(64) void fp_nearest_kernel(const FpNearestParams P) {
  __shared__ uint4 tile[kFpTile][4];
  __shared__ int ltot[kFpTile];
  extern __shared__ int fp_dyn[];
  const FpLists L = fp_lists(fp_dyn, P.k * QPL * 64);
  const int lane = threadIdx.x, k = P.k, split = blockIdx.y;
  int qi[QPL], tq[QPL], wc[QPL], wu[QPL], wi[QPL];
  const unsigned char* qrow[QPL];
#pragma unroll
  for (int q = 0; q < QPL; ++q) {
    qi[q] = (blockIdx.x * QPL + q) * 64 + lane;
    const int at = qi[q] < P.B ? qi[q] : P.B - 1;  // a lane past the batch computes on the last query and writes nothing
    qrow[q] = P.q + (size_t)at * P.n_bins;
    tq[q] = P.qtot[at];
    wc[q] = 0;
    wu[q] = 0;
    wi[q] = kFpPad;
    for (int j = 0; j < k; ++j) {
      const int to = (j * QPL + q) * 64 + lane;
      L.c[to] = 0;
      L.u[to] = 0;
      L.i[to] = kFpPad;
    }
  }
  const long long first = (long long)split * P.rows_per_split;
  const int begin = first < P.M ? (int)first : P.M;
  const int end = first + P.rows_per_split < P.M ? (int)(first + P.rows_per_split) : P.M;
  for (int row0 = begin; row0 < end; row0 += kFpTile) {
    unsigned int acc[QPL][kFpTile];
    fp_tile_sad<QPL>(P.lib, row0, end, P.n_bins, qrow, tile, lane, acc);
    if (lane < kFpTile) ltot[lane] = row0 + lane < end ? P.ltot[row0 + lane] : 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kFpTile; ++r) {
      const int idx = row0 + r, tl = ltot[r];
      if (idx < end) {  // (wave-uniform)
#pragma unroll
        for (int q = 0; q < QPL; ++q) {
          const int common = (tq[q] + tl - (int)acc[q][r]) >> 1, uni = tq[q] + tl - common;
          if (fp_ahead(common, uni, idx, wc[q], wu[q], wi[q])) fp_insert<QPL>(L, q, lane, k, common, uni, idx, wc[q], wu[q], wi[q]);
        }
      }
    }
    // (the next tile's first barrier stands between these reads of ltot and its next writes)
  }
#pragma unroll
  for (int q = 0; q < QPL; ++q) {
    if (qi[q] >= P.B) continue;
    int* out = P.part + ((size_t)split * P.B + qi[q]) * k * 3;
    for (int j = 0; j < k; ++j) {
      const int at = (j * QPL + q) * 64 + lane;
      out[3 * j] = L.c[at];
      out[3 * j + 1] = L.u[at];
      out[3 * j + 2] = L.i[at];
    }
  }
}

// One wave per query: lane l pushes the lists of splits l, l + 64, ... through the same insertion into a list of its own, then
// lane 0 does the same with the 64 lists and writes idx / common / union
__global__ __launch_bounds__(64) void fp_merge_kernel(const int* __restrict__ part, int B, int k, int S, int* __restrict__ idx_out,
                                                      int* __restrict__ common_out, int* __restrict__ union_out) {
  extern __shared__ int fp_dyn[];
  const FpLists L = fp_lists(fp_dyn, k * 64);
  const int lane = threadIdx.x, b = blockIdx.x;  // (the grid is B workgroups)
  for (int j = 0; j < k; ++j) {
    L.c[j * 64 + lane] = 0;
    L.u[j * 64 + lane] = 0;
    L.i[j * 64 + lane] = kFpPad;
  }
  int wc = 0, wu = 0, wi = kFpPad;
  for (int s = lane; s < S; s += 64) {
    const int* in = part + ((size_t)s * B + b) * k * 3;
    for (int j = 0; j < k; ++j) {
      const int c = in[3 * j], u = in[3 * j + 1], i = in[3 * j + 2];
      if (i == kFpPad) break;  // a list's rows come first
      if (fp_ahead(c, u, i, wc, wu, wi)) fp_insert<1>(L, 0, lane, k, c, u, i, wc, wu, wi);
    }
  }
  __syncthreads();
  if (lane != 0) return;
  for (int l = 1; l < 64; ++l)
    for (int j = 0; j < k; ++j) {
      const int c = L.c[j * 64 + l], u = L.u[j * 64 + l], i = L.i[j * 64 + l];
      if (i == kFpPad) break;
      if (fp_ahead(c, u, i, wc, wu, wi)) fp_insert<1>(L, 0, 0, k, c, u, i, wc, wu, wi);
    }
  for (int j = 0; j < k; ++j) {
    const int i = L.i[j * 64];
    idx_out[(size_t)b * k + j] = i == kFpPad ? -1 : i;
    common_out[(size_t)b * k + j] = L.c[j * 64];
    union_out[(size_t)b * k + j] = L.u[j * 64];
  }
}

// common_out [B][M]: grid (tiles of the library, blocks of 64 queries)
__global__ __launch_bounds__(64) void fp_common_kernel(const unsigned char* __restrict__ qs, const int* __restrict__ qtot,
                                                       const unsigned char* __restrict__ lib, const int* __restrict__ ltot_g, int B,
                                                       int M, int n_bins, int* __restrict__ common_out) {
  __shared__ uint4 tile[kFpTile][4];
  __shared__ int ltot[kFpTile];
  const int lane = threadIdx.x, row0 = blockIdx.x * kFpTile, qi = blockIdx.y * 64 + lane;
  const int at = qi < B ? qi : B - 1;
  const unsigned char* qrow[1] = {qs + (size_t)at * n_bins};
  const int tq = qtot[at];
  unsigned int acc[1][kFpTile];
  fp_tile_sad<1>(lib, row0, M, n_bins, qrow, tile, lane, acc);
  if (lane < kFpTile) ltot[lane] = row0 + lane < M ? ltot_g[row0 + lane] : 0;
  __syncthreads();
  if (qi >= B) return;
#pragma unroll
  for (int r = 0; r < kFpTile; ++r)
    if (row0 + r < M) common_out[(size_t)qi * M + row0 + r] = (tq + ltot[r] - (int)acc[0][r]) >> 1;
}

static bool fp_bins_ok(int n_bins) { return n_bins == 256 || n_bins == 512 || n_bins == 1024; }

// d_fp slots
enum FpBuf : int {
  kFpIn0 = 0,  // .. 3: the fingerprint's four inputs
  kFpRows = 4, kFpTotal, kFpStatus,
  kFpQ, kFpQTot, kFpTmpLib, kFpTmpTot, kFpResLib, kFpResTot, kFpPart, kFpOut, kFpMatrix,
  kFpBufs
};
static_assert(kFpBufs == 16, "gaudi_handle::d_fp");

// rows [n][n_bins] from the host into the buffer `rows`, their totals into `tot` (on the handle's stream)
static int fp_upload(gaudi_handle* h, DevBuf& rows, DevBuf& tot, const uint8_t* src, int n, int n_bins) {
  const size_t bytes = (size_t)n * n_bins;
  HIPCHECK(h, rows.reserve(bytes));
  HIPCHECK(h, tot.reserve(sizeof(int) * (size_t)n));
  HIPCHECK(h, hipMemcpyAsync(rows.p, src, bytes, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(fp_totals_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, rows.as<unsigned char>(), n, n_bins, tot.as<int>());
  HIPCHECK(h, hipGetLastError());
  return GAUDI_OK;
}
// ... into the d_fp slots `rows` and `tot` (fp_select.inc passes slots of its own)
static int fp_upload(gaudi_handle* h, int rows, int tot, const uint8_t* src, int n, int n_bins) {
  return fp_upload(h, h->d_fp[rows], h->d_fp[tot], src, n, n_bins);
}

// the library a call compares against: the one passed in (uploaded to the temporary slots) or the resident one
static int fp_library(gaudi_handle* h, int n_bins, int M, const uint8_t* lib, const unsigned char** rows, const int** tot) {
  if (lib) {
    if (int rc = fp_upload(h, kFpTmpLib, kFpTmpTot, lib, M, n_bins)) return rc;
    *rows = h->d_fp[kFpTmpLib].as<unsigned char>();
    *tot = h->d_fp[kFpTmpTot].as<int>();
    return GAUDI_OK;
  }
  if (h->fp_lib_rows == 0) return fail(h, GAUDI_E_STATE, "no resident fingerprint library: call gaudi_fp_library_set first");
  if (h->fp_lib_rows != M || h->fp_lib_bins != n_bins)
    return fail(h, GAUDI_E_INVALID, "M / n_bins differ from the resident fingerprint library's");
  *rows = h->d_fp[kFpResLib].as<unsigned char>();
  *tot = h->d_fp[kFpResTot].as<int>();
  return GAUDI_OK;
}

}  // namespace gaudi

#define GAUDI_FP_ARGS                                                                                                          \
  int n_elems, int h_elem, int c_elem, int B, int A, int M, const int32_t *elem, const int32_t *n_atoms, const int32_t *bonds, \
      const int32_t *n_bonds, int radius, int n_bins, uint8_t *fp_out, int32_t *total_out, int32_t *status_out

extern "C" int gaudi_circular_fingerprint(gaudi_handle* h, GAUDI_FP_ARGS) {
  if (!h || !fp_out || !total_out || !status_out) return GAUDI_E_INVALID;
  const char* why = "";
  if (int rc = gaudi::canon_prepare(n_elems, h_elem, c_elem, B, A, M, elem, n_atoms, bonds, n_bonds, &why)) return fail(h, rc, why);
  if (radius < 0 || radius > 3 || !gaudi::fp_bins_ok(n_bins)) return fail(h, GAUDI_E_INVALID, "radius must be 0..3 and n_bins 256, 512 or 1024");
  if (B == 0) return GAUDI_OK;
  HIPCHECK(h, hipSetDevice(h->device));
  const size_t nB = (size_t)B;
  const size_t isz[4] = {sizeof(int) * nB * A, sizeof(int) * nB, sizeof(int) * nB * M * 2, sizeof(int) * nB};
  const size_t osz[3] = {nB * n_bins, sizeof(int) * nB, sizeof(int) * nB};
  const void* ins[4] = {elem, n_atoms, bonds, n_bonds};
  for (int i = 0; i < 4; ++i) {
    HIPCHECK(h, h->d_fp[gaudi::kFpIn0 + i].reserve(isz[i]));
    HIPCHECK(h, hipMemcpyAsync(h->d_fp[gaudi::kFpIn0 + i].p, ins[i], isz[i], hipMemcpyHostToDevice, h->stream));
  }
  // a molecule without a fingerprint writes its status only: a zero row and total 0
  for (int i = 0; i < 3; ++i) {
    HIPCHECK(h, h->d_fp[gaudi::kFpRows + i].reserve(osz[i]));
    HIPCHECK(h, hipMemsetAsync(h->d_fp[gaudi::kFpRows + i].p, 0, osz[i], h->stream));
  }
  gaudi::FpParams P{};
  P.in.B = B;
  P.in.A = A;
  P.in.M = M;
  P.in.n_elems = n_elems;
  P.in.h_elem = h_elem;
  P.in.c_elem = c_elem;
  P.in.elem = h->d_fp[gaudi::kFpIn0].as<int>();
  P.in.n_atoms = h->d_fp[gaudi::kFpIn0 + 1].as<int>();
  P.in.bonds = h->d_fp[gaudi::kFpIn0 + 2].as<int>();
  P.in.n_bonds = h->d_fp[gaudi::kFpIn0 + 3].as<int>();
  P.radius = radius;
  P.n_bins = n_bins;
  P.fp = h->d_fp[gaudi::kFpRows].as<unsigned char>();
  P.total = h->d_fp[gaudi::kFpTotal].as<int>();
  P.status = h->d_fp[gaudi::kFpStatus].as<int>();
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (h->prof) HIPCHECK(h, h->fp_log.begin(h->stream, ev));
  hipLaunchKernelGGL(gaudi::fp_kernel, dim3((B + gaudi::kFpWaves - 1) / gaudi::kFpWaves), dim3(64 * gaudi::kFpWaves), 0, h->stream, P);
  HIPCHECK(h, hipGetLastError());
  if (h->prof) HIPCHECK(h, h->fp_log.end(h->stream, ev));
  void* outs[3] = {fp_out, total_out, status_out};
  for (int i = 0; i < 3; ++i) HIPCHECK(h, hipMemcpyAsync(outs[i], h->d_fp[gaudi::kFpRows + i].p, osz[i], hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  return GAUDI_OK;
}

extern "C" int gaudi_host_circular_fingerprint(GAUDI_FP_ARGS) {
  if (!fp_out || !total_out || !status_out) return GAUDI_E_INVALID;
  const char* why = "";
  if (int rc = gaudi::canon_prepare(n_elems, h_elem, c_elem, B, A, M, elem, n_atoms, bonds, n_bonds, &why)) return rc;
  if (radius < 0 || radius > 3 || !gaudi::fp_bins_ok(n_bins)) return GAUDI_E_INVALID;
  if (B == 0) return GAUDI_OK;
  const size_t nB = (size_t)B;
  memset(fp_out, 0, nB * n_bins);
  memset(total_out, 0, sizeof(int) * nB);
  memset(status_out, 0, sizeof(int) * nB);
  gaudi::FpParams P{};
  P.in.B = B;
  P.in.A = A;
  P.in.M = M;
  P.in.n_elems = n_elems;
  P.in.h_elem = h_elem;
  P.in.c_elem = c_elem;
  P.in.elem = elem;
  P.in.n_atoms = n_atoms;
  P.in.bonds = bonds;
  P.in.n_bonds = n_bonds;
  P.radius = radius;
  P.n_bins = n_bins;
  P.fp = fp_out;
  P.total = total_out;
  P.status = status_out;
  std::vector<gaudi::FpSmem> S(1);
  for (int b = 0; b < B; ++b) gaudi::circular_fingerprint(P, S[0], b, 0);
  return GAUDI_OK;
}
#undef GAUDI_FP_ARGS

extern "C" int gaudi_fp_library_set(gaudi_handle* h, int n_bins, int M, const uint8_t* lib) {
  if (!h || M < 0) return GAUDI_E_INVALID;
  HIPCHECK(h, hipSetDevice(h->device));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  h->fp_lib_rows = 0;
  h->fp_lib_bins = 0;
  if (M == 0) {
    h->d_fp[gaudi::kFpResLib].release();
    h->d_fp[gaudi::kFpResTot].release();
    return GAUDI_OK;
  }
  if (!lib || !gaudi::fp_bins_ok(n_bins)) return fail(h, GAUDI_E_INVALID, "n_bins must be 256, 512 or 1024 and lib given");
  if (int rc = gaudi::fp_upload(h, gaudi::kFpResLib, gaudi::kFpResTot, lib, M, n_bins)) return rc;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  h->fp_lib_rows = M;
  h->fp_lib_bins = n_bins;
  return GAUDI_OK;
}

extern "C" int gaudi_fp_nearest(gaudi_handle* h, int n_bins, int B, const uint8_t* q, int M, const uint8_t* lib, int k,
                                int32_t* idx_out, int32_t* common_out, int32_t* union_out) {
  if (!h || !q || !idx_out || !common_out || !union_out || B < 0 || M < 1) return GAUDI_E_INVALID;
  if (!gaudi::fp_bins_ok(n_bins) || k < 1 || k > gaudi::kFpMaxK) return fail(h, GAUDI_E_INVALID, "n_bins must be 256, 512 or 1024 and k in 1..16");
  if (B == 0) return GAUDI_OK;
  HIPCHECK(h, hipSetDevice(h->device));
  const unsigned char* d_lib = nullptr;
  const int* d_ltot = nullptr;
  if (int rc = gaudi::fp_library(h, n_bins, M, lib, &d_lib, &d_ltot)) return rc;
  if (int rc = gaudi::fp_upload(h, gaudi::kFpQ, gaudi::kFpQTot, q, B, n_bins)) return rc;
  // the splits: enough one-wave workgroups for every CU to hold several, each with at least eight tiles of the library
  const int qpl = B > 64 ? 2 : 1;
  const int qblocks = (B + 64 * qpl - 1) / (64 * qpl), tiles = (M + gaudi::kFpTile - 1) / gaudi::kFpTile;
  int S = (8 * h->num_cus + qblocks - 1) / qblocks;
  S = std::min(S, (tiles + 7) / 8);
  if (const char* v = getenv("GAUDI_FP_SPLITS")) S = atoi(v);
  S = std::max(1, std::min(S, 1024));
  const int tiles_per_split = (tiles + S - 1) / S;
  const size_t out_ints = (size_t)B * k, part_bytes = sizeof(int) * 3 * out_ints * S;
  HIPCHECK(h, h->d_fp[gaudi::kFpPart].reserve(part_bytes));
  HIPCHECK(h, h->d_fp[gaudi::kFpOut].reserve(sizeof(int) * 3 * out_ints));
  gaudi::FpNearestParams P{};
  P.q = h->d_fp[gaudi::kFpQ].as<unsigned char>();
  P.qtot = h->d_fp[gaudi::kFpQTot].as<int>();
  P.lib = d_lib;
  P.ltot = d_ltot;
  P.B = B;
  P.M = M;
  P.n_bins = n_bins;
  P.k = k;
  P.S = S;
  P.rows_per_split = tiles_per_split * gaudi::kFpTile;
  P.part = h->d_fp[gaudi::kFpPart].as<int>();
  int* out = h->d_fp[gaudi::kFpOut].as<int>();
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (h->prof) HIPCHECK(h, h->fp_log.begin(h->stream, ev));
  if (qpl == 2)
    hipLaunchKernelGGL(gaudi::fp_nearest_kernel<2>, dim3(qblocks, S), dim3(64), gaudi::fp_lists_bytes(k, 2), h->stream, P);
  else
    hipLaunchKernelGGL(gaudi::fp_nearest_kernel<1>, dim3(qblocks, S), dim3(64), gaudi::fp_lists_bytes(k, 1), h->stream, P);
  HIPCHECK(h, hipGetLastError());
  hipLaunchKernelGGL(gaudi::fp_merge_kernel, dim3(B), dim3(64), gaudi::fp_lists_bytes(k, 1), h->stream, P.part, B, k, S, out, out + out_ints,
                     out + 2 * out_ints);
  HIPCHECK(h, hipGetLastError());
  if (h->prof) HIPCHECK(h, h->fp_log.end(h->stream, ev));
  int32_t* outs[3] = {idx_out, common_out, union_out};
  for (int i = 0; i < 3; ++i)
    HIPCHECK(h, hipMemcpyAsync(outs[i], out + i * out_ints, sizeof(int) * out_ints, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  return GAUDI_OK;
}

extern "C" int gaudi_fp_common(gaudi_handle* h, int n_bins, int B, const uint8_t* q, int M, const uint8_t* lib, int32_t* common_out) {
  if (!h || !q || !common_out || B < 0 || M < 1) return GAUDI_E_INVALID;
  if (!gaudi::fp_bins_ok(n_bins)) return fail(h, GAUDI_E_INVALID, "n_bins must be 256, 512 or 1024");
  if ((long long)B * M > (1ll << 28)) return fail(h, GAUDI_E_CAPACITY, "gaudi_fp_common: B * M beyond 2^28");
  if (B == 0) return GAUDI_OK;
  HIPCHECK(h, hipSetDevice(h->device));
  const unsigned char* d_lib = nullptr;
  const int* d_ltot = nullptr;
  if (int rc = gaudi::fp_library(h, n_bins, M, lib, &d_lib, &d_ltot)) return rc;
  if (int rc = gaudi::fp_upload(h, gaudi::kFpQ, gaudi::kFpQTot, q, B, n_bins)) return rc;
  const size_t bytes = sizeof(int) * (size_t)B * M;
  HIPCHECK(h, h->d_fp[gaudi::kFpMatrix].reserve(bytes));
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (h->prof) HIPCHECK(h, h->fp_log.begin(h->stream, ev));
  hipLaunchKernelGGL(gaudi::fp_common_kernel, dim3((M + gaudi::kFpTile - 1) / gaudi::kFpTile, (B + 63) / 64), dim3(64), 0, h->stream,
                     h->d_fp[gaudi::kFpQ].as<unsigned char>(), h->d_fp[gaudi::kFpQTot].as<int>(), d_lib, d_ltot, B, M, n_bins,
                     h->d_fp[gaudi::kFpMatrix].as<int>());
  HIPCHECK(h, hipGetLastError());
  if (h->prof) HIPCHECK(h, h->fp_log.end(h->stream, ev));
  HIPCHECK(h, hipMemcpyAsync(common_out, h->d_fp[gaudi::kFpMatrix].p, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  return GAUDI_OK;
}

extern "C" int gaudi_host_fp_nearest(int n_bins, int B, const uint8_t* q, int M, const uint8_t* lib, int k, int32_t* idx_out,
                                     int32_t* common_out, int32_t* union_out) {
  if (!q || !lib || !idx_out || !common_out || !union_out || B < 0 || M < 1) return GAUDI_E_INVALID;
  if (!gaudi::fp_bins_ok(n_bins) || k < 1 || k > gaudi::kFpMaxK) return GAUDI_E_INVALID;
  std::vector<int> ltot(M);
  for (int m = 0; m < M; ++m) {
    int t = 0;
    for (int i = 0; i < n_bins; ++i) t += lib[(size_t)m * n_bins + i];
    ltot[m] = t;
  }
  for (int b = 0; b < B; ++b) {
    const uint8_t* qr = q + (size_t)b * n_bins;
    int32_t *ix = idx_out + (size_t)b * k, *cm = common_out + (size_t)b * k, *un = union_out + (size_t)b * k;
    int tq = 0;
    for (int i = 0; i < n_bins; ++i) tq += qr[i];
    for (int j = 0; j < k; ++j) {
      ix[j] = gaudi::kFpPad;
      cm[j] = 0;
      un[j] = 0;
    }
    for (int m = 0; m < M; ++m) {
      const uint8_t* lr = lib + (size_t)m * n_bins;
      int c = 0;
      for (int i = 0; i < n_bins; ++i) c += qr[i] < lr[i] ? qr[i] : lr[i];
      const int u = tq + ltot[m] - c;
      if (!gaudi::fp_ahead(c, u, m, cm[k - 1], un[k - 1], ix[k - 1])) continue;
      int j = k - 1;
      while (j > 0 && gaudi::fp_ahead(c, u, m, cm[j - 1], un[j - 1], ix[j - 1])) {
        cm[j] = cm[j - 1];
        un[j] = un[j - 1];
        ix[j] = ix[j - 1];
        --j;
      }
      cm[j] = c;
      un[j] = u;
      ix[j] = m;
    }
    for (int j = 0; j < k; ++j)
      if (ix[j] == gaudi::kFpPad) ix[j] = -1;
  }
  return GAUDI_OK;
}

extern "C" int gaudi_fp_profile_get(gaudi_handle* h, int32_t* n_launches, double* total_ms) {
  if (!h || !n_launches || !total_ms) return GAUDI_E_INVALID;
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, h->fp_log.fold(0));
  *n_launches = (int32_t)h->fp_log.n;
  *total_ms = h->fp_log.ms;
  return GAUDI_OK;
}
