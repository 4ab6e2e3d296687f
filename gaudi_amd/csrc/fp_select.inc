// fp_select.inc -- which rows of a fingerprint batch to take on: neighbour lists at a similarity threshold, Butina clusters on
// those lists and MaxMin (diverse subset) picking (included after fp.inc at the end of gaudi_hip.hip; DESIGN.md section 8q).
//
// Everything is exact integer arithmetic on fp.inc's common / union: a threshold is a rational thr_num / thr_den, the pair i, j is
// "at least thr" when union > 0 and common * thr_den >= thr_num * union in 64 bits, and two similarities are compared by fp_ahead's
// cross product.  A row is LIVE when its total is > 0; rows that are not live are never picked, never clustered, have no
// neighbours and are nobody's neighbour.
//
// fp_neighbours_kernel: fp_nearest_kernel's frame (a one-wave workgroup, 64 * QPL rows of the batch as queries against one split
// of the SAME batch through fp_tile_sad) with a cheaper epilogue: a multiply-compare and an add per pair.  COUNT writes per
// (split, row) counts, fp_offsets_kernel turns them into CSR offsets, FILL repeats the comparison and writes the indices at the
// (row, split) offset.  A lane walks its split's tiles in ascending row order and the splits are ascending ranges, so every list
// is ascending without a sort and without atomics, and no output depends on the number of splits.
//
// fp_order_kernel (one workgroup): a stable LSD radix sort of the row indices by N - count, four bits a pass.
// fp_walk_kernel (one workgroup): the Butina walk along that order with the assigned set as a bitset in LDS.
// fp_pick_kernel: one launch per MaxMin round; stream order is the only dependency between rounds (no grid barrier, no spin-wait,
// no communication between workgroups inside a launch).

namespace gaudi {

constexpr int kFsMaxRows = 1 << 20;
constexpr long long kFsMaxEntries = 1ll << 28;
constexpr int kFsMaxThr = 65536;
constexpr int kFsScanThreads = 1024;
constexpr int kFsSortThreads = 512;
constexpr int kFsWalkThreads = 256;
constexpr int kFsPickThreads = 256;
constexpr int kFsChunk = 256;  // pick rounds enqueued between two reads of the stop flag

// d_fps slots
enum FsBuf : int {
  kFsRows = 0, kFsTot, kFsPart, kFsOff, kFsCount, kFsOffsets, kFsList, kFsTotal, kFsOrdA, kFsOrdB, kFsOrder, kFsCluster, kFsNear,
  kFsCand, kFsPicks, kFsState,
  kFsBufs
};
static_assert(kFsBufs == 16, "gaudi_handle::d_fps");

__host__ __device__ __forceinline__ bool fp_at_least(int c, int u, int num, int den) {
  return u > 0 && (long long)c * den >= (long long)num * u;
}

// x is ahead of y in MaxMin's candidate order: the LESS similar first, equal similarity to the smaller row index; an index of
// kFpPad holds no row and is behind every row
__host__ __device__ __forceinline__ bool fp_least(int cx, int ux, int ix, int cy, int uy, int iy) {
  if (ix == kFpPad) return false;
  if (iy == kFpPad) return true;
  const long long l = (long long)cx * (uy > 0 ? uy : 1), r = (long long)cy * (ux > 0 ? ux : 1);
  return l != r ? l < r : ix < iy;
}

// similarity x strictly greater than similarity y
__host__ __device__ __forceinline__ bool fp_closer(int cx, int ux, int cy, int uy) {
  return (long long)cx * (uy > 0 ? uy : 1) > (long long)cy * (ux > 0 ? ux : 1);
}

// ---- neighbour lists -------------------------------------------------------------------------------------------------------------

struct FsNbParams {
  const unsigned char* rows;  // [N][n_bins]: queries and library alike
  const int* tot;             // [N]
  int N, n_bins, S, rows_per_split, thr_num, thr_den;
  int* part;        // COUNT: [S][N] counts out
  const int* off;   // FILL: [S][N] where (split, row) writes
  int* list;        // FILL: [total]
  long long total;  // FILL: no write at or beyond it
};

template <int QPL, bool FILL>
__global__ __launch_bounds__(64) void fp_neighbours_kernel(const FsNbParams P) {
  __shared__ uint4 tile[kFpTile][4];
  __shared__ int ltot[kFpTile];
  const int lane = threadIdx.x, split = blockIdx.y;
  int qi[QPL], tq[QPL], n[QPL];
  long long at[QPL];
  const unsigned char* qrow[QPL];
#pragma unroll
  for (int q = 0; q < QPL; ++q) {
    qi[q] = (blockIdx.x * QPL + q) * 64 + lane;
    const int row = qi[q] < P.N ? qi[q] : P.N - 1;  // a lane past the batch computes on the last row and writes nothing
    qrow[q] = P.rows + (size_t)row * P.n_bins;
    tq[q] = qi[q] < P.N ? P.tot[row] : 0;  // (a total of 0: not live, no hit)
    n[q] = 0;
    at[q] = FILL ? (long long)P.off[(size_t)split * P.N + row] : 0ll;
  }
  const long long first = (long long)split * P.rows_per_split;
  const int begin = first < P.N ? (int)first : P.N;
  const int end = first + P.rows_per_split < P.N ? (int)(first + P.rows_per_split) : P.N;
  for (int row0 = begin; row0 < end; row0 += kFpTile) {
    unsigned int acc[QPL][kFpTile];
    fp_tile_sad<QPL>(P.rows, row0, end, P.n_bins, qrow, tile, lane, acc);
    if (lane < kFpTile) ltot[lane] = row0 + lane < end ? P.tot[row0 + lane] : 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kFpTile; ++r) {
      const int idx = row0 + r, tl = ltot[r];
      if (idx < end && tl > 0) {  // (wave-uniform)
#pragma unroll
        for (int q = 0; q < QPL; ++q) {
          const int common = (tq[q] + tl - (int)acc[q][r]) >> 1, uni = tq[q] + tl - common;
          if (tq[q] > 0 && (long long)common * P.thr_den >= (long long)P.thr_num * uni) {
            if (FILL) {
              if (at[q] + n[q] < P.total) P.list[at[q] + n[q]] = idx;
            }
            ++n[q];
          }
        }
      }
    }
    // (the next tile's first barrier stands between these reads of ltot and its next writes)
  }
  if (!FILL) {
#pragma unroll
    for (int q = 0; q < QPL; ++q)
      if (qi[q] < P.N) P.part[(size_t)split * P.N + qi[q]] = n[q];
  }
}

// One workgroup: thread t owns rows [t * chunk, (t + 1) * chunk).  count[i] = the sum over the splits, offsets = its exclusive
// prefix (64-bit sums: the grand total may pass 2^31 before the host refuses it), off[s][i] = where split s of row i writes.
__global__ __launch_bounds__(kFsScanThreads) void fp_offsets_kernel(const int* __restrict__ part, int N, int S, int* __restrict__ count,
                                                                   int* __restrict__ offsets, int* __restrict__ off,
                                                                   long long* __restrict__ total) {
  __shared__ long long sh[kFsScanThreads];
  const int tid = threadIdx.x, chunk = (N + kFsScanThreads - 1) / kFsScanThreads;
  const long long b0 = (long long)tid * chunk;
  const int b = b0 < N ? (int)b0 : N, e = b0 + chunk < N ? (int)(b0 + chunk) : N;
  long long mine = 0;
  for (int i = b; i < e; ++i)
    for (int s = 0; s < S; ++s) mine += part[(size_t)s * N + i];
  sh[tid] = mine;
  __syncthreads();
  for (int d = 1; d < kFsScanThreads; d <<= 1) {
    const long long v = tid >= d ? sh[tid - d] : 0ll;
    __syncthreads();
    sh[tid] += v;
    __syncthreads();
  }
  long long run = sh[tid] - mine;
  for (int i = b; i < e; ++i) {
    offsets[i] = (int)run;
    int c = 0;
    for (int s = 0; s < S; ++s) {
      off[(size_t)s * N + i] = (int)(run + c);
      c += part[(size_t)s * N + i];
    }
    count[i] = c;
    run += c;
  }
  if (tid == kFsScanThreads - 1) {
    offsets[N] = (int)sh[tid];
    *total = sh[tid];
  }
}

// ---- Butina clusters -----------------------------------------------------------------------------------------------------------

// order = the row indices by count descending, then index ascending: a stable LSD radix sort by key = N - count, four bits a
// pass.  One workgroup; thread t owns positions [t * chunk, (t + 1) * chunk) of the current sequence, hist[digit][t] is its
// count, and the exclusive scan over (digit, thread) gives every thread its first output place for every digit.
__global__ __launch_bounds__(kFsSortThreads) void fp_order_kernel(const int* __restrict__ count, int N, int passes, int* a, int* b,
                                                                 int* __restrict__ order) {
  __shared__ int hist[16 * kFsSortThreads];
  __shared__ int sums[kFsSortThreads];
  const int tid = threadIdx.x, chunk = (N + kFsSortThreads - 1) / kFsSortThreads;
  const long long b0 = (long long)tid * chunk;
  const int lo = b0 < N ? (int)b0 : N, hi = b0 + chunk < N ? (int)(b0 + chunk) : N;
  int *src = a, *dst = b;
  for (int i = lo; i < hi; ++i) src[i] = i;
  for (int pass = 0; pass < passes; ++pass) {
    const int shift = 4 * pass;
    for (int d = 0; d < 16; ++d) hist[d * kFsSortThreads + tid] = 0;
    for (int i = lo; i < hi; ++i) ++hist[(((N - count[src[i]]) >> shift) & 15) * kFsSortThreads + tid];
    __syncthreads();
    // flattened entries [tid * 16, tid * 16 + 16) of hist: their sum, the scan of the sums, their exclusive prefixes written back
    int mine = 0;
    for (int f = 0; f < 16; ++f) mine += hist[tid * 16 + f];
    sums[tid] = mine;
    __syncthreads();
    for (int d = 1; d < kFsSortThreads; d <<= 1) {
      const int v = tid >= d ? sums[tid - d] : 0;
      __syncthreads();
      sums[tid] += v;
      __syncthreads();
    }
    int run = sums[tid] - mine;
    for (int f = 0; f < 16; ++f) {
      const int c = hist[tid * 16 + f];
      hist[tid * 16 + f] = run;
      run += c;
    }
    __syncthreads();
    for (int i = lo; i < hi; ++i) {
      const int v = src[i];
      dst[hist[(((N - count[v]) >> shift) & 15) * kFsSortThreads + tid]++] = v;
    }
    __syncthreads();  // (a workgroup's global writes are visible to it behind the barrier)
    int* t = src;
    src = dst;
    dst = t;
  }
  for (int i = lo; i < hi; ++i) order[i] = src[i];
}

// The walk, one workgroup.  The assigned set is a bitset in the launch's dynamic LDS ((N + 31) / 32 words: 128 KiB at 2^20 rows).
// The order is read in blocks of 64 with each row's count and list bounds, so a step that meets an assigned row costs one LDS
// read; a centroid's list is spread over the threads, which claim with an LDS atomic OR and write cluster[j].
__global__ __launch_bounds__(kFsWalkThreads) void fp_walk_kernel(const int* __restrict__ order, const int* __restrict__ count,
                                                                const int* __restrict__ offsets, const int* __restrict__ list, int N,
                                                                int* __restrict__ cluster, int* __restrict__ centroid,
                                                                int* __restrict__ size, int* __restrict__ n_clusters) {
  extern __shared__ unsigned int fs_bits[];
  __shared__ int o_row[64], o_cnt[64], o_lo[64], o_hi[64];
  __shared__ int sz[2];
  const int tid = threadIdx.x, words = (N + 31) / 32;
  for (int w = tid; w < words; w += kFsWalkThreads) fs_bits[w] = 0u;
  if (tid < 2) sz[tid] = 0;
  int nc = 0;
  bool done = false;
  for (int blk = 0; blk < N && !done; blk += 64) {
    __syncthreads();  // the previous block's reads (and the zeroing) before these writes
    if (tid < 64) {
      const int at = blk + tid;
      const int row = at < N ? order[at] : -1;
      o_row[tid] = row;
      o_cnt[tid] = row >= 0 ? count[row] : 0;
      o_lo[tid] = row >= 0 ? offsets[row] : 0;
      o_hi[tid] = row >= 0 ? offsets[row + 1] : 0;
    }
    __syncthreads();
    for (int e = 0; e < 64; ++e) {  // (every branch here is uniform over the workgroup)
      const int i = o_row[e];
      if (i < 0 || o_cnt[e] == 0) {  // past the batch, or the rows that are not live: they close the order
        done = true;
        break;
      }
      if ((fs_bits[i >> 5] >> (i & 31)) & 1u) continue;
      // Every wave must have read row i's bit before any wave claims: i is in its own list, and a wave that came late would
      // find it assigned, skip the centroid and miss its barriers.  Between two centroids the bits do not change, so the
      // waves' decisions agree wherever they are in the order.
      __syncthreads();
      int mine = 0;
      for (int p = o_lo[e] + tid; p < o_hi[e]; p += kFsWalkThreads) {
        const int j = list[p];
        const unsigned int m = 1u << (j & 31);
        if (!(atomicOr(&fs_bits[j >> 5], m) & m)) {
          cluster[j] = nc;
          ++mine;
        }
      }
      if (mine) atomicAdd(&sz[nc & 1], mine);
      __syncthreads();
      if (tid == 0) {
        centroid[nc] = i;
        size[nc] = sz[nc & 1];
        sz[nc & 1] = 0;  // (the next centroid adds to the other counter, the one after that finds this one zero behind its barrier)
      }
      ++nc;
    }
  }
  if (tid == 0) *n_clusters = nc;
}

// ---- MaxMin picking ------------------------------------------------------------------------------------------------------------

struct FsPickParams {
  const unsigned char* rows;  // [N][n_bins]
  const int* tot;             // [N]
  int N, n_bins, G, rows_per_wg;
  int *near_c, *near_u, *owner;  // [N]: the most similar chosen element; owner -1: none (or the row is not live), i itself: picked
  int* cand;                     // [2][G][3]: common, union, index (kFpPad: no row)
  int *picked, *pick_c, *pick_u;  // [k]
  int* state;                    // [0]: picking has stopped, [1]: picks made
  const int *seed_idx, *seed_c, *seed_u;  // [N] from the nearest search over the seeds, or null (round -1 reads them)
  int t;                         // the pick this round makes; -1: no pick, the state is set up and the first candidates found
  int forced_first;              // t = -1 without seeds: the only candidate (-1: every live row)
  int thr_num, thr_den;          // thr_den 0: no threshold
};

__device__ __forceinline__ void fp_least_wave(int& c, int& u, int& i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int oc = __shfl_xor(c, off), ou = __shfl_xor(u, off), oi = __shfl_xor(i, off);
    if (fp_least(oc, ou, oi, c, u, i)) {
      c = oc;
      u = ou;
      i = oi;
    }
  }
}

// Round t.  Every WAVE reduces the previous round's G candidates by itself (the order is total, so all of them arrive at the same
// pick), loads the pick's bytes, updates near for the workgroup's slice of rows and finds the slice's next candidate.  A row is
// read by n_bins / 64 neighbouring lanes, 16 bytes a lane and four loads each, and their partial sums meet in a butterfly inside
// the group.
__global__ __launch_bounds__(kFsPickThreads) void fp_pick_kernel(const FsPickParams P) {
  __shared__ int wbest[kFsPickThreads / 64][3];
  if (P.state[0]) return;  // (stopped in an earlier launch)
  const int tid = threadIdx.x, lane = tid & 63, g = blockIdx.x;
  const int lg = P.n_bins == 256 ? 2 : P.n_bins == 512 ? 3 : 4, L = 1 << lg, sub = tid & (L - 1);
  int pc = 0, pu = 0, pi = kFpPad, tp = 0;
  uint4 pv[4] = {};
  if (P.t >= 0) {
    const int* cd = P.cand + (size_t)(P.t & 1) * P.G * 3;
    for (int j = lane; j < P.G; j += 64) {
      const int c = cd[3 * j], u = cd[3 * j + 1], i = cd[3 * j + 2];
      if (fp_least(c, u, i, pc, pu, pi)) {
        pc = c;
        pu = u;
        pi = i;
      }
    }
    fp_least_wave(pc, pu, pi);
    if (pi == kFpPad || (P.thr_den > 0 && fp_at_least(pc, pu, P.thr_num, P.thr_den))) {  // (the same in every workgroup)
      if (g == 0 && tid == 0) P.state[0] = 1;
      return;
    }
    if (g == 0 && tid == 0) {
      P.picked[P.t] = pi;
      P.pick_c[P.t] = pc;
      P.pick_u[P.t] = pu;
      P.state[1] = P.t + 1;
    }
    tp = P.tot[pi];
    const unsigned char* prow = P.rows + (size_t)pi * P.n_bins;
#pragma unroll
    for (int s = 0; s < 4; ++s) pv[s] = *reinterpret_cast<const uint4*>(prow + (size_t)(s * L + sub) * 16);
  }
  int bc = 0, bu = 0, bi = kFpPad;
  const long long first = (long long)g * P.rows_per_wg;
  const int begin = first < P.N ? (int)first : P.N;
  const int end = first + P.rows_per_wg < P.N ? (int)(first + P.rows_per_wg) : P.N;
  const int rpp = kFsPickThreads >> lg;
  for (int base = begin; base < end; base += rpp) {
    const int i = base + (tid >> lg);
    const bool there = i < end;
    const int row = there ? i : begin;
    const int ti = P.tot[row];
    int common = 0, uni = 0;
    if (P.t >= 0) {
      const unsigned char* r = P.rows + (size_t)row * P.n_bins;
      unsigned int sad = 0u;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const uint4 v = *reinterpret_cast<const uint4*>(r + (size_t)(s * L + sub) * 16);
        sad = __builtin_amdgcn_sad_u8(v.x, pv[s].x, sad);
        sad = __builtin_amdgcn_sad_u8(v.y, pv[s].y, sad);
        sad = __builtin_amdgcn_sad_u8(v.z, pv[s].z, sad);
        sad = __builtin_amdgcn_sad_u8(v.w, pv[s].w, sad);
      }
      for (int off = 1; off < L; off <<= 1) sad += __shfl_xor(sad, off);
      common = (ti + tp - (int)sad) >> 1;
      uni = ti + tp - common;
    }
    if (there && sub == 0 && ti > 0) {
      int nc, nu, ow;
      if (P.t < 0) {
        nc = P.seed_idx ? P.seed_c[i] : 0;
        nu = P.seed_idx ? P.seed_u[i] : 0;
        ow = P.seed_idx ? -2 - P.seed_idx[i] : -1;
        P.near_c[i] = nc;
        P.near_u[i] = nu;
        P.owner[i] = ow;
      } else {
        nc = P.near_c[i];
        nu = P.near_u[i];
        ow = P.owner[i];
        const bool self = i == pi;
        if (self || ow == -1 || fp_closer(common, uni, nc, nu)) {
          nc = self ? ti : common;
          nu = self ? ti : uni;
          ow = pi;
          P.near_c[i] = nc;
          P.near_u[i] = nu;
          P.owner[i] = ow;
        }
      }
      const bool may = ow != i && (P.t >= 0 || P.forced_first < 0 || i == P.forced_first);
      if (may && fp_least(nc, nu, i, bc, bu, bi)) {
        bc = nc;
        bu = nu;
        bi = i;
      }
    }
  }
  fp_least_wave(bc, bu, bi);
  if (lane == 0) {
    wbest[tid >> 6][0] = bc;
    wbest[tid >> 6][1] = bu;
    wbest[tid >> 6][2] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kFsPickThreads / 64; ++w)
      if (fp_least(wbest[w][0], wbest[w][1], wbest[w][2], bc, bu, bi)) {
        bc = wbest[w][0];
        bu = wbest[w][1];
        bi = wbest[w][2];
      }
    int* out = P.cand + ((size_t)((P.t + 1) & 1) * P.G + g) * 3;
    out[0] = bc;
    out[1] = bu;
    out[2] = bi;
  }
}

// rows that are not live: near 0, 0 and owner -1 (one thread per row; the pick kernel writes the live rows only)
__global__ __launch_bounds__(256) void fp_pick_clear_kernel(int N, int* __restrict__ near_c, int* __restrict__ near_u, int* __restrict__ owner) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  near_c[i] = 0;
  near_u[i] = 0;
  owner[i] = -1;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

static const char* fs_check(int n_bins, int N, const void* rows, int thr_num, int thr_den, bool thr_optional, int* rc) {
  *rc = GAUDI_E_INVALID;
  if (!fp_bins_ok(n_bins)) return "n_bins must be 256, 512 or 1024";
  if (N < 0 || (N > 0 && !rows)) return "N must be >= 0 and rows given";
  if (!(thr_optional && thr_den == 0) && !(thr_den >= 1 && thr_den <= kFsMaxThr && thr_num >= 0 && thr_num <= thr_den))
    return "the threshold must be thr_num / thr_den with 0 <= thr_num <= thr_den <= 65536, thr_den >= 1";
  *rc = GAUDI_E_CAPACITY;
  if (N > kFsMaxRows) return "more than 2^20 rows";
  *rc = GAUDI_OK;
  return nullptr;
}

static int fs_splits(gaudi_handle* h, int qblocks, int tiles) {
  int S = (8 * h->num_cus + qblocks - 1) / qblocks;
  S = std::min(S, (tiles + 7) / 8);
  if (const char* v = getenv("GAUDI_FP_SPLITS")) S = atoi(v);
  return std::max(1, std::min(S, 1024));
}

static void fs_launch_neighbours(gaudi_handle* h, const FsNbParams& P, int qpl, int qblocks, bool fill) {
  const dim3 grid(qblocks, P.S), block(64);
  if (qpl == 2) {
    if (fill)
      hipLaunchKernelGGL((fp_neighbours_kernel<2, true>), grid, block, 0, h->stream, P);
    else
      hipLaunchKernelGGL((fp_neighbours_kernel<2, false>), grid, block, 0, h->stream, P);
  } else {
    if (fill)
      hipLaunchKernelGGL((fp_neighbours_kernel<1, true>), grid, block, 0, h->stream, P);
    else
      hipLaunchKernelGGL((fp_neighbours_kernel<1, false>), grid, block, 0, h->stream, P);
  }
}

// h->fs_ms: the stages of the most recent call made with profiling on (gaudi_fp_select_stages_get)
enum FsStage : int { kFsMsCount = 0, kFsMsOffsets, kFsMsFill, kFsMsSort, kFsMsWalk, kFsMsPickSetup, kFsMsPickRounds, kFsMsTotals, kFsStages };
static_assert(kFsStages == 8, "gaudi_handle::fs_ms");

// one entry of the profile log around `launches` launches
struct FsProf {
  gaudi_handle* h;
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  hipError_t begin() { return h->prof ? h->fp_log.begin(h->stream, ev) : hipSuccess; }
  hipError_t end(int launches) {
    if (!h->prof) return hipSuccess;
    h->fp_log.n += launches - 1;  // (folding the pair counts the one)
    return h->fp_log.end(h->stream, ev);
  }
  // behind a synchronisation of the stream, and before the log hands the pair out again: the bracketed time into a stage
  hipError_t read(int stage, bool add = false) {
    if (!h->prof) return hipSuccess;
    float t = 0.f;
    const hipError_t e = hipEventElapsedTime(&t, ev.first, ev.second);
    if (e == hipSuccess) h->fs_ms[stage] = (add ? h->fs_ms[stage] : 0.0) + t;
    return e;
  }
};

static void fs_stages_clear(gaudi_handle* h) {
  if (h->prof)
    for (double& v : h->fs_ms) v = 0.0;
}

// The batch's counts, offsets and (with_list) lists, left on the device in the slots kFsCount, kFsOffsets, kFsList; *total = the
// number of entries.  The rows are uploaded to kFsRows / kFsTot.  Beyond 2^28 entries: GAUDI_E_CAPACITY with the counts in place.
// The FILL pass runs when 0 < total <= fill_up_to (the caller's capacity).
static int fs_neighbours(gaudi_handle* h, int n_bins, int N, const uint8_t* rows, int thr_num, int thr_den, long long fill_up_to,
                         long long* total) {
  if (int rc = fp_upload(h, h->d_fps[kFsRows], h->d_fps[kFsTot], rows, N, n_bins)) return rc;
  const int qpl = N > 64 ? 2 : 1;
  const int qblocks = (N + 64 * qpl - 1) / (64 * qpl), tiles = (N + kFpTile - 1) / kFpTile;
  const int S = fs_splits(h, qblocks, tiles);
  const int tiles_per_split = (tiles + S - 1) / S;
  const size_t sn = sizeof(int) * (size_t)S * N;
  HIPCHECK(h, h->d_fps[kFsPart].reserve(sn));
  HIPCHECK(h, h->d_fps[kFsOff].reserve(sn));
  HIPCHECK(h, h->d_fps[kFsCount].reserve(sizeof(int) * (size_t)N));
  HIPCHECK(h, h->d_fps[kFsOffsets].reserve(sizeof(int) * ((size_t)N + 1)));
  HIPCHECK(h, h->d_fps[kFsTotal].reserve(sizeof(long long)));
  FsNbParams P{};
  P.rows = h->d_fps[kFsRows].as<unsigned char>();
  P.tot = h->d_fps[kFsTot].as<int>();
  P.N = N;
  P.n_bins = n_bins;
  P.S = S;
  P.rows_per_split = tiles_per_split * kFpTile;
  P.thr_num = thr_num;
  P.thr_den = thr_den;
  P.part = h->d_fps[kFsPart].as<int>();
  FsProf prof{h}, prof1{h};
  HIPCHECK(h, prof.begin());
  fs_launch_neighbours(h, P, qpl, qblocks, false);
  HIPCHECK(h, hipGetLastError());
  HIPCHECK(h, prof.end(1));
  HIPCHECK(h, prof1.begin());
  hipLaunchKernelGGL(fp_offsets_kernel, dim3(1), dim3(kFsScanThreads), 0, h->stream, P.part, N, S, h->d_fps[kFsCount].as<int>(),
                     h->d_fps[kFsOffsets].as<int>(), h->d_fps[kFsOff].as<int>(), h->d_fps[kFsTotal].as<long long>());
  HIPCHECK(h, hipGetLastError());
  HIPCHECK(h, prof1.end(1));
  HIPCHECK(h, hipMemcpyAsync(total, h->d_fps[kFsTotal].p, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, prof.read(kFsMsCount));
  HIPCHECK(h, prof1.read(kFsMsOffsets));
  if (*total > kFsMaxEntries) return fail(h, GAUDI_E_CAPACITY, "more than 2^28 neighbour entries: raise the threshold or cut the batch");
  if (*total > fill_up_to || *total == 0) return GAUDI_OK;
  HIPCHECK(h, h->d_fps[kFsList].reserve(sizeof(int) * (size_t)*total));
  P.off = h->d_fps[kFsOff].as<int>();
  P.list = h->d_fps[kFsList].as<int>();
  P.total = *total;
  FsProf prof2{h};
  HIPCHECK(h, prof2.begin());
  fs_launch_neighbours(h, P, qpl, qblocks, true);
  HIPCHECK(h, hipGetLastError());
  HIPCHECK(h, prof2.end(1));
  if (h->prof) {
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    HIPCHECK(h, prof2.read(kFsMsFill));
  }
  return GAUDI_OK;
}

// host twins' pieces
static void fs_host_totals(int n_bins, int n, const uint8_t* rows, std::vector<int>& tot) {
  tot.assign((size_t)n, 0);
  for (int i = 0; i < n; ++i) {
    int t = 0;
    for (int b = 0; b < n_bins; ++b) t += rows[(size_t)i * n_bins + b];
    tot[i] = t;
  }
}

static int fs_host_common(int n_bins, const uint8_t* a, const uint8_t* b) {
  int c = 0;
  for (int i = 0; i < n_bins; ++i) c += a[i] < b[i] ? a[i] : b[i];
  return c;
}

// every row's ascending list of neighbours, by plain loops over every pair
static void fs_host_lists(int n_bins, int N, const uint8_t* rows, int thr_num, int thr_den, std::vector<int>& tot,
                          std::vector<std::vector<int>>& lists) {
  fs_host_totals(n_bins, N, rows, tot);
  lists.assign((size_t)N, {});
  for (int i = 0; i < N; ++i) {
    if (tot[i] == 0) continue;
    for (int j = 0; j < N; ++j) {
      if (tot[j] == 0) continue;
      const int c = fs_host_common(n_bins, rows + (size_t)i * n_bins, rows + (size_t)j * n_bins);
      if (fp_at_least(c, tot[i] + tot[j] - c, thr_num, thr_den)) lists[i].push_back(j);
    }
  }
}

}  // namespace gaudi

extern "C" int gaudi_fp_neighbours(gaudi_handle* h, int n_bins, int N, const uint8_t* rows, int thr_num, int thr_den,
                                   int32_t* count_out, int64_t capacity, int64_t* offsets_out, int32_t* list_out) {
  if (!h) return GAUDI_E_INVALID;
  int rc = 0;
  if (const char* why = gaudi::fs_check(n_bins, N, rows, thr_num, thr_den, false, &rc)) return fail(h, rc, why);
  if (capacity < 0 || (capacity > 0 && !list_out) || (!list_out && capacity != 0)) return fail(h, GAUDI_E_INVALID, "list_out NULL goes with capacity 0");
  if (N == 0) return GAUDI_OK;
  if (!count_out || !offsets_out) return fail(h, GAUDI_E_INVALID, "count_out and offsets_out must be given");
  HIPCHECK(h, hipSetDevice(h->device));
  gaudi::fs_stages_clear(h);
  long long total = 0;
  rc = gaudi::fs_neighbours(h, n_bins, N, rows, thr_num, thr_den, list_out ? (long long)capacity : -1ll, &total);
  if (rc != GAUDI_OK && rc != GAUDI_E_CAPACITY) return rc;
  // the counts always; the offsets as 64-bit integers from them (beyond 2^28 entries the device's 32-bit ones may have wrapped)
  HIPCHECK(h, hipMemcpyAsync(count_out, h->d_fps[gaudi::kFsCount].p, sizeof(int) * (size_t)N, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  offsets_out[0] = 0;
  for (int i = 0; i < N; ++i) offsets_out[i + 1] = offsets_out[i] + count_out[i];
  if (rc != GAUDI_OK) return rc;
  if (!list_out) return GAUDI_OK;
  if (total > capacity) return fail(h, GAUDI_E_CAPACITY, "list_out holds " + std::to_string(capacity) + " entries, the lists have " + std::to_string(total));
  if (total > 0) {
    HIPCHECK(h, hipMemcpyAsync(list_out, h->d_fps[gaudi::kFsList].p, sizeof(int) * (size_t)total, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
  }
  return GAUDI_OK;
}

extern "C" int gaudi_host_fp_neighbours(int n_bins, int N, const uint8_t* rows, int thr_num, int thr_den, int32_t* count_out,
                                        int64_t capacity, int64_t* offsets_out, int32_t* list_out) {
  int rc = 0;
  if (gaudi::fs_check(n_bins, N, rows, thr_num, thr_den, false, &rc)) return rc;
  if (capacity < 0 || (capacity > 0 && !list_out) || (!list_out && capacity != 0)) return GAUDI_E_INVALID;
  if (N == 0) return GAUDI_OK;
  if (!count_out || !offsets_out) return GAUDI_E_INVALID;
  std::vector<int> tot;
  std::vector<std::vector<int>> lists;
  gaudi::fs_host_lists(n_bins, N, rows, thr_num, thr_den, tot, lists);
  offsets_out[0] = 0;
  for (int i = 0; i < N; ++i) {
    count_out[i] = (int32_t)lists[i].size();
    offsets_out[i + 1] = offsets_out[i] + count_out[i];
  }
  if (offsets_out[N] > gaudi::kFsMaxEntries) return GAUDI_E_CAPACITY;
  if (!list_out) return GAUDI_OK;
  if (offsets_out[N] > capacity) return GAUDI_E_CAPACITY;
  for (int i = 0; i < N; ++i) std::copy(lists[i].begin(), lists[i].end(), list_out + offsets_out[i]);
  return GAUDI_OK;
}

extern "C" int gaudi_fp_cluster(gaudi_handle* h, int n_bins, int N, const uint8_t* rows, int thr_num, int thr_den,
                                int32_t* cluster_out, int32_t* centroid_out, int32_t* size_out, int32_t* count_out,
                                int32_t* n_clusters_out) {
  if (!h) return GAUDI_E_INVALID;
  int rc = 0;
  if (const char* why = gaudi::fs_check(n_bins, N, rows, thr_num, thr_den, false, &rc)) return fail(h, rc, why);
  if (N == 0) return GAUDI_OK;
  if (!cluster_out || !centroid_out || !size_out || !count_out || !n_clusters_out) return fail(h, GAUDI_E_INVALID, "every output must be given");
  HIPCHECK(h, hipSetDevice(h->device));
  gaudi::fs_stages_clear(h);
  long long total = 0;
  if ((rc = gaudi::fs_neighbours(h, n_bins, N, rows, thr_num, thr_den, gaudi::kFsMaxEntries, &total))) return rc;
  const size_t nb = sizeof(int) * (size_t)N;
  HIPCHECK(h, h->d_fps[gaudi::kFsOrdA].reserve(nb));
  HIPCHECK(h, h->d_fps[gaudi::kFsOrdB].reserve(nb));
  HIPCHECK(h, h->d_fps[gaudi::kFsOrder].reserve(nb));
  HIPCHECK(h, h->d_fps[gaudi::kFsCluster].reserve(3 * nb + sizeof(int)));
  HIPCHECK(h, h->d_fps[gaudi::kFsList].reserve(sizeof(int)));  // (no entry at all: the walk still takes a pointer)
  int* cl = h->d_fps[gaudi::kFsCluster].as<int>();
  HIPCHECK(h, hipMemsetAsync(cl, 0xff, 2 * nb, h->stream));        // cluster, centroid: -1
  HIPCHECK(h, hipMemsetAsync(cl + 2 * (size_t)N, 0, nb + sizeof(int), h->stream));  // size, n_clusters: 0
  int passes = 0;
  while (passes < 6 && (N >> (4 * passes)) != 0) ++passes;  // the keys are 0..N
  const size_t lds = sizeof(unsigned int) * (((size_t)N + 31) / 32);
  if (lds > 48 * 1024)
    HIPCHECK(h, hipFuncSetAttribute((const void*)gaudi::fp_walk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  gaudi::FsProf prof{h};
  HIPCHECK(h, prof.begin());
  hipLaunchKernelGGL(gaudi::fp_order_kernel, dim3(1), dim3(gaudi::kFsSortThreads), 0, h->stream, h->d_fps[gaudi::kFsCount].as<int>(), N,
                     passes, h->d_fps[gaudi::kFsOrdA].as<int>(), h->d_fps[gaudi::kFsOrdB].as<int>(), h->d_fps[gaudi::kFsOrder].as<int>());
  HIPCHECK(h, hipGetLastError());
  HIPCHECK(h, prof.end(1));
  gaudi::FsProf prof2{h};
  HIPCHECK(h, prof2.begin());
  hipLaunchKernelGGL(gaudi::fp_walk_kernel, dim3(1), dim3(gaudi::kFsWalkThreads), lds, h->stream, h->d_fps[gaudi::kFsOrder].as<int>(),
                     h->d_fps[gaudi::kFsCount].as<int>(), h->d_fps[gaudi::kFsOffsets].as<int>(), h->d_fps[gaudi::kFsList].as<int>(), N, cl,
                     cl + N, cl + 2 * (size_t)N, cl + 3 * (size_t)N);
  HIPCHECK(h, hipGetLastError());
  HIPCHECK(h, prof2.end(1));
  HIPCHECK(h, hipMemcpyAsync(cluster_out, cl, nb, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipMemcpyAsync(centroid_out, cl + N, nb, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipMemcpyAsync(size_out, cl + 2 * (size_t)N, nb, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipMemcpyAsync(n_clusters_out, cl + 3 * (size_t)N, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipMemcpyAsync(count_out, h->d_fps[gaudi::kFsCount].p, nb, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  HIPCHECK(h, prof.read(gaudi::kFsMsSort));
  HIPCHECK(h, prof2.read(gaudi::kFsMsWalk));
  return GAUDI_OK;
}

extern "C" int gaudi_host_fp_cluster(int n_bins, int N, const uint8_t* rows, int thr_num, int thr_den, int32_t* cluster_out,
                                     int32_t* centroid_out, int32_t* size_out, int32_t* count_out, int32_t* n_clusters_out) {
  int rc = 0;
  if (gaudi::fs_check(n_bins, N, rows, thr_num, thr_den, false, &rc)) return rc;
  if (N == 0) return GAUDI_OK;
  if (!cluster_out || !centroid_out || !size_out || !count_out || !n_clusters_out) return GAUDI_E_INVALID;
  std::vector<int> tot;
  std::vector<std::vector<int>> lists;
  gaudi::fs_host_lists(n_bins, N, rows, thr_num, thr_den, tot, lists);
  long long total = 0;
  std::vector<int> order((size_t)N);
  for (int i = 0; i < N; ++i) {
    count_out[i] = (int32_t)lists[i].size();
    total += count_out[i];
    cluster_out[i] = -1;
    centroid_out[i] = -1;
    size_out[i] = 0;
    order[i] = i;
  }
  if (total > gaudi::kFsMaxEntries) return GAUDI_E_CAPACITY;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return count_out[a] > count_out[b]; });
  int nc = 0;
  for (int at = 0; at < N; ++at) {
    const int i = order[at];
    if (tot[i] == 0 || cluster_out[i] >= 0) continue;
    centroid_out[nc] = i;
    for (int j : lists[i])
      if (cluster_out[j] < 0) {
        cluster_out[j] = nc;
        ++size_out[nc];
      }
    ++nc;
  }
  *n_clusters_out = nc;
  return GAUDI_OK;
}

#define GAUDI_PICK_OUTS                                                                                                          \
  int32_t *picked_out, int32_t *pick_common_out, int32_t *pick_union_out, int32_t *n_picked_out, int32_t *owner_out,             \
      int32_t *owner_common_out, int32_t *owner_union_out

namespace gaudi {
// what both builds refuse; *first_row = the row a first pick without seeds takes (-1: none is forced, or no live row)
static const char* fs_pick_check(int n_bins, int N, const uint8_t* rows, int S, int first, int k, int thr_num, int thr_den,
                                 bool outs, int* rc) {
  if (const char* why = fs_check(n_bins, N, rows, thr_num, thr_den, true, rc)) return why;
  *rc = GAUDI_E_INVALID;
  if (S < 0 || k < 0) return "S and k must be >= 0";
  if (N > 0 && !outs) return "every output must be given";
  if (S == 0 && first != -1) {
    if (first < 0 || first >= N) return "first is out of range";
    bool live = false;
    for (int b = 0; b < n_bins; ++b) live |= rows[(size_t)first * n_bins + b] != 0;
    if (!live) return "first is not a live row";
  }
  *rc = GAUDI_OK;
  return nullptr;
}
}  // namespace gaudi

extern "C" int gaudi_fp_pick_diverse(gaudi_handle* h, int n_bins, int N, const uint8_t* rows, int S, const uint8_t* seeds, int first,
                                     int k, int thr_num, int thr_den, GAUDI_PICK_OUTS) {
  if (!h) return GAUDI_E_INVALID;
  int rc = 0;
  const bool outs = (k == 0 || (picked_out && pick_common_out && pick_union_out)) && n_picked_out && owner_out && owner_common_out && owner_union_out;
  if (const char* why = gaudi::fs_pick_check(n_bins, N, rows, S, first, k, thr_num, thr_den, outs, &rc)) return fail(h, rc, why);
  if (N == 0) return GAUDI_OK;
  HIPCHECK(h, hipSetDevice(h->device));
  using namespace gaudi;
  fs_stages_clear(h);
  if (int r = fp_upload(h, h->d_fps[kFsRows], h->d_fps[kFsTot], rows, N, n_bins)) return r;
  const size_t nb = sizeof(int) * (size_t)N;
  // the slices: a workgroup per 128 rows, 1024 at the most (a slice is walked 256 / (n_bins / 64) rows at a time, each step a
  // dependent trip to memory, so short slices on many workgroups: with 1024 rows a slice a round took 57 - 100 us whatever N)
  int G = std::max(1, std::min(1024, (N + 127) / 128));
  if (const char* v = getenv("GAUDI_FP_SPLITS")) G = atoi(v);
  G = std::max(1, std::min(G, 1024));
  const int rows_per_wg = (N + G - 1) / G;
  HIPCHECK(h, h->d_fps[kFsNear].reserve(3 * nb));
  HIPCHECK(h, h->d_fps[kFsCand].reserve(sizeof(int) * 6 * (size_t)G));
  HIPCHECK(h, h->d_fps[kFsPicks].reserve(sizeof(int) * 3 * (size_t)std::max(k, 1)));
  HIPCHECK(h, h->d_fps[kFsState].reserve(sizeof(int) * 2));
  FsPickParams P{};
  P.rows = h->d_fps[kFsRows].as<unsigned char>();
  P.tot = h->d_fps[kFsTot].as<int>();
  P.N = N;
  P.n_bins = n_bins;
  P.G = G;
  P.rows_per_wg = rows_per_wg;
  P.near_c = h->d_fps[kFsNear].as<int>();
  P.near_u = P.near_c + N;
  P.owner = P.near_u + N;
  P.cand = h->d_fps[kFsCand].as<int>();
  P.picked = h->d_fps[kFsPicks].as<int>();
  P.pick_c = P.picked + k;
  P.pick_u = P.pick_c + k;
  P.state = h->d_fps[kFsState].as<int>();
  P.t = -1;
  P.forced_first = S == 0 ? first : -1;
  P.thr_num = thr_num;
  P.thr_den = thr_den;
  HIPCHECK(h, hipMemsetAsync(P.state, 0, sizeof(int) * 2, h->stream));
  if (k > 0) {
    HIPCHECK(h, hipMemsetAsync(P.picked, 0xff, sizeof(int) * (size_t)k, h->stream));
    HIPCHECK(h, hipMemsetAsync(P.pick_c, 0, sizeof(int) * 2 * (size_t)k, h->stream));
  }
  int launches = 2;
  FsProf prof{h};
  if (S > 0) {
    // near from the seeds: ONE pass of the nearest search at k = 1 (fp_nearest_kernel + fp_merge_kernel), whose order -- the most
    // similar first, equal similarity to the smaller seed index -- is the rule "the earliest chosen wins"
    const unsigned char* d_lib = nullptr;
    const int* d_ltot = nullptr;
    if (int r = fp_library(h, n_bins, S, seeds, &d_lib, &d_ltot)) return r;
    const int qpl = N > 64 ? 2 : 1;
    const int qblocks = (N + 64 * qpl - 1) / (64 * qpl), tiles = (S + kFpTile - 1) / kFpTile;
    const int SP = fs_splits(h, qblocks, tiles);
    HIPCHECK(h, h->d_fp[kFpPart].reserve(sizeof(int) * 3 * (size_t)N * SP));
    HIPCHECK(h, h->d_fp[kFpOut].reserve(3 * nb));
    FpNearestParams Q{};
    Q.q = P.rows;
    Q.qtot = P.tot;
    Q.lib = d_lib;
    Q.ltot = d_ltot;
    Q.B = N;
    Q.M = S;
    Q.n_bins = n_bins;
    Q.k = 1;
    Q.S = SP;
    Q.rows_per_split = (tiles + SP - 1) / SP * kFpTile;
    Q.part = h->d_fp[kFpPart].as<int>();
    int* out = h->d_fp[kFpOut].as<int>();
    HIPCHECK(h, prof.begin());
    if (qpl == 2)
      hipLaunchKernelGGL(fp_nearest_kernel<2>, dim3(qblocks, SP), dim3(64), fp_lists_bytes(1, 2), h->stream, Q);
    else
      hipLaunchKernelGGL(fp_nearest_kernel<1>, dim3(qblocks, SP), dim3(64), fp_lists_bytes(1, 1), h->stream, Q);
    HIPCHECK(h, hipGetLastError());
    hipLaunchKernelGGL(fp_merge_kernel, dim3(N), dim3(64), fp_lists_bytes(1, 1), h->stream, Q.part, N, 1, SP, out, out + N, out + 2 * (size_t)N);
    HIPCHECK(h, hipGetLastError());
    P.seed_idx = out;
    P.seed_c = out + N;
    P.seed_u = out + 2 * (size_t)N;
    launches += 2;
  } else {
    HIPCHECK(h, prof.begin());
  }
  hipLaunchKernelGGL(fp_pick_clear_kernel, dim3((N + 255) / 256), dim3(256), 0, h->stream, N, P.near_c, P.near_u, P.owner);
  HIPCHECK(h, hipGetLastError());
  hipLaunchKernelGGL(fp_pick_kernel, dim3(G), dim3(kFsPickThreads), 0, h->stream, P);
  HIPCHECK(h, hipGetLastError());
  HIPCHECK(h, prof.end(launches));
  if (h->prof) {
    // the yardstick of a round: fp_totals_kernel once more over the same rows (it reads every byte once and writes the same totals)
    FsProf again{h};
    HIPCHECK(h, again.begin());
    hipLaunchKernelGGL(fp_totals_kernel, dim3((N + 255) / 256), dim3(256), 0, h->stream, P.rows, N, n_bins, h->d_fps[kFsTot].as<int>());
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, again.end(1));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    HIPCHECK(h, prof.read(kFsMsPickSetup));
    HIPCHECK(h, again.read(kFsMsTotals));
  }
  int state[2] = {0, 0};
  for (int t0 = 0; t0 < k && !state[0]; t0 += kFsChunk) {
    const int t1 = std::min(k, t0 + kFsChunk);
    FsProf chunk{h};
    HIPCHECK(h, chunk.begin());
    for (int t = t0; t < t1; ++t) {
      P.t = t;
      hipLaunchKernelGGL(fp_pick_kernel, dim3(G), dim3(kFsPickThreads), 0, h->stream, P);
      HIPCHECK(h, hipGetLastError());
    }
    HIPCHECK(h, chunk.end(t1 - t0));
    HIPCHECK(h, hipMemcpyAsync(state, P.state, sizeof(state), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    HIPCHECK(h, chunk.read(kFsMsPickRounds, true));
  }
  HIPCHECK(h, hipMemcpyAsync(state, P.state, sizeof(state), hipMemcpyDeviceToHost, h->stream));
  if (k > 0) {
    HIPCHECK(h, hipMemcpyAsync(picked_out, P.picked, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipMemcpyAsync(pick_common_out, P.pick_c, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipMemcpyAsync(pick_union_out, P.pick_u, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHECK(h, hipMemcpyAsync(owner_common_out, P.near_c, nb, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipMemcpyAsync(owner_union_out, P.near_u, nb, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipMemcpyAsync(owner_out, P.owner, nb, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(h, hipStreamSynchronize(h->stream));
  *n_picked_out = state[1];
  return GAUDI_OK;
}

extern "C" int gaudi_host_fp_pick_diverse(int n_bins, int N, const uint8_t* rows, int S, const uint8_t* seeds, int first, int k,
                                          int thr_num, int thr_den, GAUDI_PICK_OUTS) {
  int rc = 0;
  const bool outs = (k == 0 || (picked_out && pick_common_out && pick_union_out)) && n_picked_out && owner_out && owner_common_out && owner_union_out;
  if (gaudi::fs_pick_check(n_bins, N, rows, S, first, k, thr_num, thr_den, outs, &rc)) return rc;
  if (S > 0 && !seeds) return GAUDI_E_INVALID;  // (no resident library without a handle)
  if (N == 0) return GAUDI_OK;
  std::vector<int> tot, stot;
  gaudi::fs_host_totals(n_bins, N, rows, tot);
  gaudi::fs_host_totals(n_bins, S, seeds, stot);
  for (int t = 0; t < k; ++t) {
    picked_out[t] = -1;
    pick_common_out[t] = 0;
    pick_union_out[t] = 0;
  }
  int32_t *nc = owner_common_out, *nu = owner_union_out, *ow = owner_out;
  for (int i = 0; i < N; ++i) {
    nc[i] = 0;
    nu[i] = 0;
    ow[i] = -1;
    if (tot[i] == 0) continue;
    for (int s = 0; s < S; ++s) {
      const int c = gaudi::fs_host_common(n_bins, rows + (size_t)i * n_bins, seeds + (size_t)s * n_bins), u = tot[i] + stot[s] - c;
      if (ow[i] == -1 || gaudi::fp_closer(c, u, nc[i], nu[i])) {
        nc[i] = c;
        nu[i] = u;
        ow[i] = -2 - s;
      }
    }
  }
  int n = 0;
  for (int t = 0; t < k; ++t) {
    int bc = 0, bu = 0, bi = gaudi::kFpPad;
    for (int i = 0; i < N; ++i) {
      if (tot[i] == 0 || ow[i] == i) continue;
      if (t == 0 && S == 0 && first >= 0 && i != first) continue;
      if (gaudi::fp_least(nc[i], nu[i], i, bc, bu, bi)) {
        bc = nc[i];
        bu = nu[i];
        bi = i;
      }
    }
    if (bi == gaudi::kFpPad || (thr_den > 0 && gaudi::fp_at_least(bc, bu, thr_num, thr_den))) break;
    picked_out[t] = bi;
    pick_common_out[t] = bc;
    pick_union_out[t] = bu;
    ++n;
    for (int i = 0; i < N; ++i) {
      if (tot[i] == 0) continue;
      const int c = gaudi::fs_host_common(n_bins, rows + (size_t)i * n_bins, rows + (size_t)bi * n_bins), u = tot[i] + tot[bi] - c;
      if (i == bi) {
        nc[i] = tot[i];
        nu[i] = tot[i];
        ow[i] = bi;
      } else if (ow[i] == -1 || gaudi::fp_closer(c, u, nc[i], nu[i])) {
        nc[i] = c;
        nu[i] = u;
        ow[i] = bi;
      }
    }
  }
  *n_picked_out = n;
  return GAUDI_OK;
}
#undef GAUDI_PICK_OUTS

extern "C" int gaudi_fp_select_stages_get(gaudi_handle* h, double* ms_out) {
  if (!h || !ms_out) return GAUDI_E_INVALID;
  for (int i = 0; i < gaudi::kFsStages; ++i) ms_out[i] = h->fs_ms[i];
  return GAUDI_OK;
}
