// device_common.h -- shared device helpers for the gfx950 GaUDI sampler kernels.
//
// Execution model: ONE workgroup (4 waves, 256 threads) owns ONE molecule for the
// whole launch.  All dense contractions run on the fp32 matrix cores
// (v_mfma_f32_16x16x4_f32: exact fp32 fma chains, same peak as the vector ALUs) in the
// orientation   D[feature][col] += W[feature][k] * act[k][col]
// i.e. weights are the MFMA A operand (streamed from L2 in a tile-packed layout, 1 KiB
// contiguous per wave-instruction) and activations are the B operand with graph NODES or EDGES
// on the 16 MFMA columns (= lanes & 15).  In this orientation the C/D layout of one GEMM
// (lane = column, 4 regs = 4 consecutive features 16t+4g..) is exactly the B layout the next
// GEMM needs, so per-edge MLP chains never leave registers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gaudi {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kWaves = 4;
constexpr int kThreads = 256;
#ifndef GAUDI_PIN_SCHED
#define GAUDI_PIN_SCHED 1
#endif
#ifndef GAUDI_PF_REGS_NE1
#define GAUDI_PF_REGS_NE1 12
#endif
#ifndef GAUDI_PIN_SCHED_UNROLLED
#define GAUDI_PIN_SCHED_UNROLLED 1
#endif
// weight-tile prefetch depth (float4 per lane each) of the rolled edge GEMM: the largest divisor of T up to 13, so that
// the rotating register queue maps onto itself from one K chunk to the next (no copies, no waits)
__host__ __device__ constexpr int pick_pf(int T) {
  int best = 1;
  for (int d = 1; d <= 13; ++d)
    if (T % d == 0) best = d;
  return best;
}
#ifndef GAUDI_SEG_BATCH
#define GAUDI_SEG_BATCH 8  // rows of a 16-edge tile fetched per batch by the segmented sum
#endif
#ifndef GAUDI_KPF
#define GAUDI_KPF 6
#endif
constexpr int kPF = GAUDI_KPF;  // prefetch depth of the fully unrolled (chained) edge GEMM

// ---- diagnostic build only (-DGAUDI_STAMPS): per-phase cycle accounting by lane 0 of wave 0.
// Never compiled into the shipped library; numbers from a stamped build are shares, not run times.
#ifdef GAUDI_STAMPS
enum { ST_NODE = 0, ST_EDGE = 1, ST_EDGE_EPI = 2, ST_BARRIER = 3, ST_MISC = 4, ST_BWD_NODE = 5, ST_BWD_EDGE = 6,
       ST_BWD_COL = 7, ST_BWD_BARRIER = 8, ST_STASH = 9, ST_B_V = 10, ST_B_EV = 11, ST_B_CP = 12, ST_B_DCP = 13,
       ST_B_DE = 14, ST_B_DV = 15, ST_B_DT1 = 16, ST_B_DU = 17, ST_STAGE = 18, ST_GEO = 19,
       ST_EDM_IO = 20, ST_UPDATE = 21, ST_PRED_IO = 22, ST_GUIDE = 23, ST_X0 = 24, ST_X1 = 25, ST_X2 = 26, ST_X3 = 27,
       ST_B_DX = 28, ST_F_COORD = 29,  // the reverse pass's dx sum, the predictor's forward coord_update (w8_pred.h)
       ST_N = 30 };                    // (the host's buffer has 32 entries; 30 and 31 carry the launch's clock counters)
struct Stamps {
  unsigned long long acc[ST_N];
  unsigned long long last;
  __device__ void init() { for (int i = 0; i < ST_N; ++i) acc[i] = 0; last = __builtin_amdgcn_s_memtime(); }
  __device__ __forceinline__ void mark(int id) {
    const unsigned long long t = __builtin_amdgcn_s_memtime();
    acc[id] += t - last;
    last = t;
  }
};
#define STAMP(id) do { if (stamps_on) g_stamps.mark(id); } while (0)
#define STAMP_DECL , Stamps& g_stamps, bool stamps_on
#define STAMP_ARGS , g_stamps, stamps_on
#else
#define STAMP(id) do { } while (0)
#define STAMP_DECL
#define STAMP_ARGS
#endif

__host__ __device__ constexpr int align16(int n) { return (n + 15) & ~15; }
__host__ __device__ constexpr int align4(int n) { return (n + 3) & ~3; }
__host__ __device__ constexpr int pad_hidden(int h) { return (h + 15) & ~15; }

// v_exp_f32 + v_rcp_f32 (1 ulp each): ~2e-7 relative, well inside the 1e-4 parity budget
__device__ __forceinline__ float sigmoid_f(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

__device__ __forceinline__ float silu_f(float x) { return x * sigmoid_f(x); }
// d/dx silu(x) = s * (1 + x * (1 - s))
__device__ __forceinline__ float dsilu_f(float x) {
  float s = sigmoid_f(x);
  return s * (1.0f + x * (1.0f - s));
}
// silu(x) and silu'(x) from one sigmoid
__device__ __forceinline__ float silu_dsilu_f(float x, float& d) {
  const float s = sigmoid_f(x);
  d = s * (1.0f + x * (1.0f - s));
  return x * s;
}
__device__ __forceinline__ f4 silu4(f4 u) {
  f4 r;
  r[0] = silu_f(u[0]); r[1] = silu_f(u[1]); r[2] = silu_f(u[2]); r[3] = silu_f(u[3]);
  return r;
}
__device__ __forceinline__ f4 dsilu4(f4 u) { return (f4){dsilu_f(u[0]), dsilu_f(u[1]), dsilu_f(u[2]), dsilu_f(u[3])}; }
__device__ __forceinline__ f4 splat(float v) { return (f4){v, v, v, v}; }
// The same, four values at once, for the 8-wave kernels (round 6).  The multiplies and adds are written on the VECTOR so that hipcc
// selects the packed fp32 instructions (v_pk_mul_f32 / v_pk_add_f32: two values per issue slot); only the transcendentals stay one per
// value.  Same operations on the same operands as the scalar forms above: bit-identical results (__expf(-x) = v_exp_f32(x * -log2(e)),
// the constant below).  The 4-wave kernels keep the scalar forms: with these, the V4G predictor at the default widths (kerng_pred.hip,
// <0, 208>: the instantiation on the register cliff, sampler_kernel.h) returned a wrong input gradient (2.6 %) -- found by
// test_global_node_buffer_kernels_agree_with_the_lds_kernels.
__device__ __forceinline__ f4 sigmoid4v(f4 x) {
  const f4 e = x * splat(-1.4426950408889634f);
  const f4 d = (f4){__builtin_amdgcn_exp2f(e[0]), __builtin_amdgcn_exp2f(e[1]), __builtin_amdgcn_exp2f(e[2]), __builtin_amdgcn_exp2f(e[3])} +
               splat(1.0f);
  return (f4){__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1]), __builtin_amdgcn_rcpf(d[2]), __builtin_amdgcn_rcpf(d[3])};
}
__device__ __forceinline__ f4 silu4v(f4 u) { return u * sigmoid4v(u); }
// silu'(x) = s * (1 + x * (1 - s))
__device__ __forceinline__ f4 dsilu4v(f4 x) {
  const f4 s = sigmoid4v(x);
  return s * (splat(1.0f) + x * (splat(1.0f) - s));
}

// One MFMA k-step: the A fragment holds W[row = lane&15][k = 4*(lane>>4) + q], the B fragment the activation of
// column lane&15 at the same k (the k order inside a 16-chunk is permuted consistently on both operands, which only
// changes the summation order).
__device__ __forceinline__ f4 mfma1(float w, float b, f4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(w, b, acc, 0, 0, 0);
}
// NOTE on issue order: v_mfma_f32_16x16x4_f32 issues every 32 cycles but a dependent accumulate needs 40, so
// the k-step loop (q) is always the OUTER loop over >= 2 independent accumulators.

// sum over the 4 lane groups g = lane>>4 (same column), result in every lane
__device__ __forceinline__ float reduce_groups(float v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

// bitwise OR of `mask` (bits 0 .. nbits-1) over the workgroup.  __syncthreads_or returns a truth value, not the OR of the
// arguments: one reduction tells whether anything is set (the common case: nothing), then one per bit.
__device__ __forceinline__ int block_or_bits(int mask, int nbits) {
  if (!__syncthreads_or(mask)) return 0;
  int out = 0;
  for (int k = 0; k < nbits; ++k)
    if (__syncthreads_or(mask & (1 << k))) out |= 1 << k;
  return out;
}
__device__ __forceinline__ void wave_lds_fence() {
  // LDS operations of one wave execute in order; this only stops the compiler from moving
  // LDS accesses across and drains the LDS queue.
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------------------------------------
// Weight access.  All hot-path weight/bias loads go through ONE buffer descriptor per network
// (base + size in SGPRs) with a wave-uniform float offset (scalar soffset, folded by the compiler)
// and a per-lane float4 index (32-bit voffset): `buffer_load_dwordx4 v, voff, s[rsrc], soff offen`.
// Plain pointer arithmetic made hipcc build a 64-bit per-lane address for every 16x16 tile, hoist
// them out of the loops and spill them.
// ---------------------------------------------------------------------------------------------
typedef unsigned int u4 __attribute__((ext_vector_type(4)));
struct WBuf {
  __amdgpu_buffer_rsrc_t r;
};
__device__ __forceinline__ WBuf make_wbuf(const float* p, unsigned bytes) {
  WBuf w;
  w.r = __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, bytes, 0x00020000);
  return w;
}
__device__ __forceinline__ f4 ldw4(const WBuf& w, int off_floats, int lane_f4) {
  return __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(w.r, lane_f4 * 16, off_floats * 4, 0));
}
// node-GEMM weight tiles are read once per CU (no reuse in L1): cache-policy bits for those loads (experiment knob)
#ifndef GAUDI_NODE_LOAD_AUX
#define GAUDI_NODE_LOAD_AUX 0
#endif
__device__ __forceinline__ f4 ldw4n(const WBuf& w, int off_floats, int lane_f4) {
  return __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(w.r, lane_f4 * 16, off_floats * 4, GAUDI_NODE_LOAD_AUX));
}
__device__ __forceinline__ float ldw1(const WBuf& w, int off_floats) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(w.r, 0, off_floats * 4, 0));
}

// The activation stash of the predictor's reverse pass is written once and read once, 2.9 MB per molecule-step = 1.5 GB of
// traffic per C3 step: with the default cache policy it sweeps the XCD L2s and the 256 MiB Infinity Cache and evicts the
// 58 MB weight set every CU re-reads each step.  Non-temporal loads AND stores keep the stream out of the caches' working
// set: C3 46.06 -> 41.45 ms per 25-step launch (+11 %; non-temporal stores alone +1.3 %).
#ifndef GAUDI_STASH_NT
#define GAUDI_STASH_NT 2  // 0 = default cache policy, 1 = non-temporal stores of the activation stash, 2 = non-temporal loads too
#endif
// The stash lives in global memory and its pointers reach the out-of-line phases as kernel-argument values: typed generic they
// compile to flat_load / flat_store -- 64-bit address pairs plus an aperture check per access, and on gfx9 a FLAT operation
// ticks BOTH vmcnt and lgkmcnt, so every s_waitcnt lgkmcnt(0) in front of a ds_read also waits for stash traffic in flight
// (VERDICT r4 weak #3).  The accessors cast to the global address space: global_load / global_store, vmcnt only.
#define GAUDI_GLOBAL __attribute__((address_space(1)))
__device__ __forceinline__ void stash_store(f4* p, f4 v) {
#ifdef GAUDI_DIAG_NO_STASH_STORE  // (timing experiment only: wrong results)
  asm volatile("" ::"v"(p), "v"(v));
  return;
#endif
#if GAUDI_STASH_NT == 1 || GAUDI_STASH_NT == 2
  __builtin_nontemporal_store(v, (GAUDI_GLOBAL f4*)p);
#else
  *(GAUDI_GLOBAL f4*)p = v;
#endif
}
__device__ __forceinline__ f4 stash_load(const f4* p) {
#if GAUDI_STASH_NT >= 2
  return __builtin_nontemporal_load((const GAUDI_GLOBAL f4*)p);
#else
  return *(const GAUDI_GLOBAL f4*)p;
#endif
}
// The node rows of the stash (P, Q, npre: an eighth of its bytes) have their own policy switch: their reload opens every
// layer of the reverse pass with all eight waves waiting on it.
#ifndef GAUDI_NODE_STASH_NT
#define GAUDI_NODE_STASH_NT GAUDI_STASH_NT
#endif
__device__ __forceinline__ void nstash_store(f4* p, f4 v) {
#ifdef GAUDI_DIAG_NO_STASH_STORE
  asm volatile("" ::"v"(p), "v"(v));
  return;
#endif
#if GAUDI_NODE_STASH_NT == 1 || GAUDI_NODE_STASH_NT == 2
  __builtin_nontemporal_store(v, (GAUDI_GLOBAL f4*)p);
#else
  *(GAUDI_GLOBAL f4*)p = v;
#endif
}
__device__ __forceinline__ f4 nstash_load(const f4* p) {
#if GAUDI_NODE_STASH_NT >= 2
  return __builtin_nontemporal_load((const GAUDI_GLOBAL f4*)p);
#else
  return *(const GAUDI_GLOBAL f4*)p;
#endif
}
// scalar words of the stash (attention gates, phi) and other per-molecule global arrays touched from the phases
// A generic pointer that is known to address global memory, marked so that LLVM's address-space inference can see it: the
// round trip through the global address space is what the pass keys on, and every pointer DERIVED from the result (the node
// buffers of the V8G kernels: hundreds of access sites behind force-inlined helpers) compiles to global_* instead of flat_*.
template <class T>
__device__ __forceinline__ T* assume_global(T* p) {
  // through an integer: a generic -> global -> generic pair of casts is folded away before the inference pass runs
  GAUDI_GLOBAL T* g = (GAUDI_GLOBAL T*)(unsigned long long)p;
  return (T*)g;
}
// The same value, but new to the optimizer at this point.  Index arithmetic that only depends on the thread id is loop invariant:
// LLVM hoists it out of the layer loops and keeps the results -- dozens of LDS addresses -- alive across every GEMM of the pass, i.e.
// in scratch, and each phase then starts with scratch reads behind `s_waitcnt vmcnt(0)` (a trip to L2 each, one after the other:
// 17 per reverse layer before this existed).  A phase that derives its addresses from fresh(tid) recomputes them (a handful of
// integer instructions) and keeps nothing alive past its end.
__device__ __forceinline__ int fresh(int v) {
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ void gstore(float* p, float v) { *(GAUDI_GLOBAL float*)p = v; }
__device__ __forceinline__ float gload(const float* p) { return *(const GAUDI_GLOBAL float*)p; }
__device__ __forceinline__ void gstore4(f4* p, f4 v) { *(GAUDI_GLOBAL f4*)p = v; }
__device__ __forceinline__ f4 gload4(const f4* p) { return *(const GAUDI_GLOBAL f4*)p; }

// Small dense dot products  out(p) = sum_{k < K} a(p, k) * b(p, k)  for p < P  (embedding heads, readout, their reverse):
// with few pairs (cata: N*F = 11) one thread per pair walks K = 192..256 elements alone, 11 busy lanes and K dependent
// steps; then 16 lanes share a pair and fold with 4 shuffles.  With many pairs (hetero: N*F = 240) a thread per pair is the
// better shape.  Summation order differs between the two shapes, both are fixed (no atomics).
template <int NTHR = kThreads, class FA, class FB, class ST>
__device__ __forceinline__ void small_dots(int P, int K, int tid, FA a, FB b, ST store) {
  if (P * 16 > 2 * NTHR) {
    for (int p = tid; p < P; p += NTHR) {
      float acc = 0.f;
      for (int k = 0; k < K; ++k) acc += a(p, k) * b(p, k);
      store(p, acc);
    }
  } else {
    const int sub = tid & 15;
    for (int p0 = 0; p0 < P; p0 += NTHR / 16) {
      const int p = p0 + (tid >> 4);
      float acc = 0.f;
      if (p < P)
        for (int k = sub; k < K; k += 16) acc += a(p, k) * b(p, k);
      acc += __shfl_xor(acc, 8);
      acc += __shfl_xor(acc, 4);
      acc += __shfl_xor(acc, 2);
      acc += __shfl_xor(acc, 1);
      if (p < P && sub == 0) store(p, acc);
    }
  }
}

// Per-layer vectors (biases, attention / radial columns): weight buffer -> registers -> LDS in two halves.
// vec_prefetch issues all loads at once, one phase early (before the last node GEMM of the previous layer), so that
// the layer starts with LDS stores only; vec_commit writes them.  History: the obvious `for (idx...) s[idx] = w[idx]`
// loop compiled into 8 dependent load->store round trips (4.5 us per layer, 6 % of a guided step).  Dword loads / stores
// on purpose: a float4 version made the fused sampler_kernel<48,48> produce wrong, run-to-run varying results (either
// network alone was fine with it; hipcc also aborted with "Operand has incorrect register class" on a close variant),
// so the shape that is verified stays (tests/test_gpu_parity.py::test_guided_steps_are_reproducible).
template <int MAXLOADS>
struct VecPF {
  float r[MAXLOADS];
};
// count: floats of the vector block.  Lanes past it do not load: the descriptor's range check looks at the lane offset
// only (not at the scalar base), so an unguarded tail would read past the end of the weight allocation.
template <int MAXLOADS, int NTHR = kThreads>
__device__ __forceinline__ void vec_prefetch(VecPF<MAXLOADS>& pf, const WBuf& wb, int off, int count, int tid) {
#pragma unroll
  for (int k = 0; k < MAXLOADS; ++k) {
    const int idx = tid + k * NTHR;
    pf.r[k] = idx < count
                  ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wb.r, idx * 4, off * 4, 0))
                  : 0.f;
  }
}
template <int MAXLOADS, int NTHR = kThreads>
__device__ __forceinline__ void vec_commit(const VecPF<MAXLOADS>& pf, float* sVec, int count, int tid) {
#pragma unroll
  for (int k = 0; k < MAXLOADS; ++k) {
    const int idx = tid + k * NTHR;
    if (idx < count) sVec[idx] = pf.r[k];
  }
}

// ---------------------------------------------------------------------------------------------
// Node-level GEMM:  Y[n][o] = epi( sum_k Wa[o][k] Xa[n][k] (+ sum_k Wb[o][k] Xb[n][k]) + bias[o] )
// X*, Y live in LDS ([N][LD] row major, LD = HP+4).  W* are tile-packed [HP/16][HP/16][16][16]
// (float offsets into the weight buffer; -1 = absent).  Wave w produces output-feature tiles
// t = w, w+4, ... for every node tile, so every weight element is fetched by exactly one wave.
// ---------------------------------------------------------------------------------------------
enum NodeEpi { EPI_NONE = 0, EPI_SILU = 1, EPI_RESIDUAL_MASK = 2, EPI_MUL_DSILU = 3, EPI_ACCUM = 4 };

// First two K chunks of a node GEMM's weight tiles, loaded ahead of the call (typically before the previous
// GEMM's epilogue and the barrier in between) so the call does not start with an exposed L2 round trip.
template <int HP>
struct NodePF {
  static constexpr int UT = (HP / 16 + kWaves - 1) / kWaves;
  f4 a0[UT], a1[UT];
};

template <int HP>
__device__ __forceinline__ void node_prefetch(NodePF<HP>& pf, const WBuf& wb, int W, int wave, int lane) {
  constexpr int T = HP / 16;
  constexpr int UT = NodePF<HP>::UT;
  const int lo = (lane & 15) * 4 + (lane >> 4);
#pragma unroll
  for (int u = 0; u < UT; ++u) {
    const int t = wave + kWaves * u;
    const int toff = (t < T ? t : wave) * 256;  // same dummy-tile rule as node_gemm_impl
    pf.a0[u] = ldw4n(wb, W + toff, lo);
    pf.a1[u] = ldw4n(wb, W + (T > 1 ? T : 0) * 256 + toff, lo);
  }
}

// PRE: the first two chunks of Wa are already in `pf`.  nextW >= 0: before the epilogue, load the first two chunks
// of the NEXT node GEMM (weight offset nextW) into `pf`.  NT = 16-node column tiles served per weight load (the GEMM
// is bound by the per-CU L2 stream of its weights, so N > 16 must not stream them once per column tile).
template <int HP, int EPI, bool PRE, int NT>
__device__ __forceinline__ void node_gemm_impl(const WBuf& wb, int Wa, const float* sXa, int Wb, const float* sXb,
                                               const float* sBias, float* sY, const float* sRes, const float* sMask,
                                               int N, int wave, int lane, NodePF<HP>* pf, int nextW, float* gPre) {
  constexpr int T = HP / 16;
  constexpr int LD = HP + 4;
  constexpr int UT = (T + kWaves - 1) / kWaves;
  const int c = lane & 15, g = lane >> 4;
  const int lo = c * 4 + g;  // lane's float4 inside a 16x16 tile
  const int n_tiles = (N + 15) >> 4;
  // Branch-free inner loops: every wave runs UT output tiles; a wave without a UT-th tile recomputes its OWN first
  // tile and drops the result (wave-uniform test in the epilogue only).  Re-reading a tile this wave has just
  // requested hits L1; streaming some other tile would add L2 traffic to a loop that is bound by exactly that.
  int toff[UT];  // float offset of the wave's tiles inside one K chunk of a packed matrix
#pragma unroll
  for (int u = 0; u < UT; ++u) {
    const int t = wave + kWaves * u;
    toff[u] = (t < T ? t : wave) * 256;
  }
  // Two sources (Y = Wa Xa + Wb Xb) run as ONE K loop of 2T chunks so the load pipeline never restarts.
  const int KT = Wb >= 0 ? 2 * T : T;
  auto chunk = [&](int cc) {  // float offset of K chunk cc (clamped past the end: surplus loads are unused)
    const int k = cc < KT ? cc : KT - 1;
    return k < T ? Wa + k * (T * 256) : Wb + (k - T) * (T * 256);
  };
  for (int nt0 = 0; nt0 < n_tiles; nt0 += NT) {
    const float* xa[NT];
    const float* xb[NT];
    int node[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      node[j] = (nt0 + j) * 16 + c;
      const int nclamp = node[j] < N ? node[j] : N - 1;
      xa[j] = sXa + nclamp * LD + 4 * g;
      xb[j] = Wb >= 0 ? sXb + nclamp * LD + 4 * g - 16 * T : xa[j];  // indexed by the global chunk number
    }
    auto xin = [&](int j, int cc) { return *(const f4*)((cc < T ? xa[j] : xb[j]) + 16 * cc); };
    f4 acc[NT][UT];
#pragma unroll
    for (int u = 0; u < UT; ++u) {
      const f4 b = sBias != nullptr ? *(const f4*)(sBias + (toff[u] >> 4) + 4 * g) : splat(0.f);
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j][u] = b;
    }
    // Weight tiles are double-buffered in registers as two ping-pong sets (A, B) of two K chunks each: while
    // the MFMAs consume one set, the loads of the other set (4 chunks ahead) are in flight.  Roles are swapped by
    // unrolling, never by copying registers (a copy of an in-flight load forces vmcnt(0)).
    f4 a0[UT], a1[UT], b0[UT], b1[UT];
    if (PRE && nt0 == 0) {
#pragma unroll
      for (int u = 0; u < UT; ++u) { a0[u] = pf->a0[u]; a1[u] = pf->a1[u]; }
    } else {
#pragma unroll
      for (int u = 0; u < UT; ++u) {
        a0[u] = ldw4n(wb, chunk(0) + toff[u], lo);
        a1[u] = ldw4n(wb, chunk(1) + toff[u], lo);
      }
    }
    // k-step (q) outermost over NT*UT independent accumulators
    auto mmx = [&](const f4 (&w)[UT], const f4 (&x)[NT]) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int u = 0; u < UT; ++u) acc[j][u] = mfma1(w[u][q], x[j][q], acc[j][u]);
    };
    auto mm = [&](const f4 (&w)[UT], int cc) {
      f4 x[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) x[j] = xin(j, cc);
      mmx(w, x);
    };
    const int main_end = KT / 4 * 4;
#pragma unroll 1
    for (int cc = 0; cc < main_end; cc += 4) {
      f4 x0[NT], x1[NT], x2[NT], x3[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        x0[j] = xin(j, cc);
        x1[j] = xin(j, cc + 1);
        x2[j] = xin(j, cc + 2);
        x3[j] = xin(j, cc + 3);
      }
#pragma unroll
      for (int u = 0; u < UT; ++u) {
        b0[u] = ldw4n(wb, chunk(cc + 2) + toff[u], lo);
        b1[u] = ldw4n(wb, chunk(cc + 3) + toff[u], lo);
      }
#if GAUDI_PIN_SCHED
      // plain fences in source order: LDS reads + set B loads | MFMAs on set A | set A loads | MFMAs on set B
      __builtin_amdgcn_sched_barrier(0);
#endif
      mmx(a0, x0);
      mmx(a1, x1);
#if GAUDI_PIN_SCHED
      __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
      for (int u = 0; u < UT; ++u) {
        a0[u] = ldw4n(wb, chunk(cc + 4) + toff[u], lo);
        a1[u] = ldw4n(wb, chunk(cc + 5) + toff[u], lo);
      }
#if GAUDI_PIN_SCHED
      __builtin_amdgcn_sched_barrier(0);
#endif
      mmx(b0, x2);
      mmx(b1, x3);
#if GAUDI_PIN_SCHED
      __builtin_amdgcn_sched_barrier(0);
#endif
    }
    // tail: KT % 4 chunks (0..3), the first two already in a0 / a1
    const int rem = KT - main_end;
    if (rem >= 3) {
#pragma unroll
      for (int u = 0; u < UT; ++u) b0[u] = ldw4n(wb, chunk(main_end + 2) + toff[u], lo);
    }
    if (rem >= 1) mm(a0, main_end);
    if (rem >= 2) mm(a1, main_end + 1);
    // software pipelining ACROSS calls: the next node GEMM's first tiles travel while this one drains
    if (nextW >= 0 && nt0 + NT >= n_tiles) node_prefetch<HP>(*pf, wb, nextW, wave, lane);
    if (rem >= 3) mm(b0, main_end + 2);
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int u = 0; u < UT; ++u) {
        const int t = wave + kWaves * u;
        const int nd = node[j];
        if (t < T && nd < N) {
          f4 y = acc[j][u];
          float* dst = sY + nd * LD + 16 * t + 4 * g;
          if (gPre != nullptr) *(f4*)(gPre + nd * HP + 16 * t + 4 * g) = y;
          if (EPI == EPI_SILU) y = silu4(y);
          if (EPI == EPI_RESIDUAL_MASK) {
            const f4 r = *(const f4*)(sRes + nd * LD + 16 * t + 4 * g);
            y = (r + y) * sMask[nd];
          }
          if (EPI == EPI_MUL_DSILU) {  // y * silu'(pre-activation stored in sRes); in place is safe
            const f4 r = *(const f4*)(sRes + nd * LD + 16 * t + 4 * g);
            y = (f4){y[0] * dsilu_f(r[0]), y[1] * dsilu_f(r[1]), y[2] * dsilu_f(r[2]), y[3] * dsilu_f(r[3])};
          }
          if (EPI == EPI_ACCUM) y = *(const f4*)(sRes + nd * LD + 16 * t + 4 * g) + y;
          *(f4*)dst = y;
        }
      }
  }
}

template <int HP, int EPI, bool PRE = false>
__device__ __forceinline__ void node_gemm(const WBuf& wb, int Wa, const float* sXa, int Wb, const float* sXb,
                                          const float* sBias /* LDS [HP] or null */, float* sY, const float* sRes,
                                          const float* sMask, int N, int wave, int lane, NodePF<HP>* pf = nullptr,
                                          int nextW = -1, float* gPre = nullptr /* global [N][HP]: pre-epilogue value */) {
  if (N <= 16)
    node_gemm_impl<HP, EPI, PRE, 1>(wb, Wa, sXa, Wb, sXb, sBias, sY, sRes, sMask, N, wave, lane, pf, nextW, gPre);
  else
    node_gemm_impl<HP, EPI, PRE, 2>(wb, Wa, sXa, Wb, sXb, sBias, sY, sRes, sMask, N, wave, lane, pf, nextW, gPre);
}

// ---------------------------------------------------------------------------------------------
// Edge-level GEMM core for NE 16-edge tiles owned by one wave:
//   acc[e][t] (features 16t+4g+q of edge column c) = b2 + W2 . silu(u_e)
//   u_e[f] = P[i_e][f] + Q[j_e][f] + cr[f] * r_e + cd[f] * d0_e        (b1 is folded into P)
// which is Linear(2H+2 -> H) of [h_i | h_j | r | d0] factorised per node (exact algebra; only the
// fp32 summation order differs from the reference's concat+Linear: egnn_new.py:42-47,119-129;
// egnn_predictor/gcl.py:225-231).
// ---------------------------------------------------------------------------------------------
struct EdgeCol {
  int i, j;      // receiving / sending node of the lane's edge column
  float r, d0;   // radial (current x) and d0 (input x) of that edge
  const float* ft = nullptr;  // sin_embedding checkpoints (EF = 24): the edge's 24 sinusoid features in LDS (edm_device.h)
};

// u[f] for f = 16cc+4g+q of one edge column
// cr / cd (and every other per-layer vector) are staged in LDS once per layer: a VMEM load consumed inside a
// pipelined GEMM loop would force vmcnt(0) (in-order counter) and drain the weight prefetch queue.
__device__ __forceinline__ f4 edge_u(const float* p, const float* q, const float* sCr, const float* sCd, int g, int cc,
                                     float r, float d0) {
  const f4 crv = *(const f4*)(sCr + 16 * cc + 4 * g);
  const f4 cdv = *(const f4*)(sCd + 16 * cc + 4 * g);
  return *(const f4*)(p + 16 * cc) + *(const f4*)(q + 16 * cc) + crv * r + cdv * d0;
}

// The same with EF edge features instead of (r, d0): `sin_embedding=True` (edm/egnn/egnn_new.py:269-273,378-391) replaces the two
// scalar inputs of the first Linear by 2 x 12 sinusoids of sqrt(r), sqrt(d0); the factorised W1 = [A | B | C] then has EF = 24
// columns C_k (staged in LDS like cr / cd: sC + k HP) and u = P_i + Q_j + sum_k C_k feat_k.  Only the 4-wave kernels carry this
// form (a K = 24 contraction per value in the stage that generates the edge GEMM's input).
template <int EF>
__device__ __forceinline__ f4 edge_u_ef(const float* p, const float* q, const float* sC, int HPv, int g, int cc, const float* ft) {
  f4 u = *(const f4*)(p + 16 * cc) + *(const f4*)(q + 16 * cc);
#pragma unroll
  for (int k4 = 0; k4 < EF / 4; ++k4) {
    const f4 fv = *(const f4*)(ft + 4 * k4);
#pragma unroll
    for (int k = 0; k < 4; ++k) u = u + *(const f4*)(sC + (4 * k4 + k) * HPv + 16 * cc + 4 * g) * fv[k];
  }
  return u;
}

// "K tail" (8-wave kernels): a hidden size with H % 16 == 4 (196, 36) leaves 4 valid inputs in the last K chunk -- exactly
// one MFMA k-step.  That chunk is packed with input 16(T-1)+g on lane group g, element 0 (both operands), and costs one
// MFMA per tile instead of four.  u of the tail chunk for the lane's edge column; p / q point at the row + 4g.
__device__ __forceinline__ f4 edge_u_tail(const float* p, const float* q, const float* sCr, const float* sCd, int g, int T,
                                          float r, float d0) {
  const int f = 16 * (T - 1) + g;
  return (f4){p[f - 4 * g] + q[f - 4 * g] + sCr[f] * r + sCd[f] * d0, 0.f, 0.f, 0.f};
}

// EF: edge features of the first Linear -- 2: (r, d0) with their columns sCr, sCd; 24 (sin_embedding): sCr = the EF columns [EF][HP],
// sCd unused, the features come from ec[e].ft
template <int HP, int NE, int EF = 2>
__device__ __forceinline__ void edge_gemm_from_pq(f4 (&acc)[NE][HP / 16], const WBuf& wb, int W2, const float* sB2,
                                                  const float* sCr, const float* sCd,
                                                  const float* sP, const float* sQ, const EdgeCol (&ec)[NE], int lane) {
  constexpr int T = HP / 16;
  constexpr int LD = HP + 4;
  constexpr int PF = pick_pf(T);
  static_assert(T % PF == 0, "queue rotation must be the identity");
  const int c = lane & 15, g = lane >> 4;
  const int lo = c * 4 + g;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const f4 b = *(const f4*)(sB2 + 16 * t + 4 * g);
#pragma unroll
    for (int e = 0; e < NE; ++e) acc[e][t] = b;
  }
  const float* pp[NE];
  const float* qq[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    pp[e] = sP + ec[e].i * LD + 4 * g;
    qq[e] = sQ + ec[e].j * LD + 4 * g;
  }
  f4 wq[PF];
#pragma unroll
  for (int p = 0; p < PF; ++p) wq[p] = ldw4(wb, W2 + 256 * p, lo);
  f4 bin[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    if constexpr (EF == 2) bin[e] = silu4(edge_u(pp[e], qq[e], sCr, sCd, g, 0, ec[e].r, ec[e].d0));
    else bin[e] = silu4(edge_u_ef<EF>(pp[e], qq[e], sCr, HP, g, 0, ec[e].ft));
  }
  // K loop stays rolled (one 16-feature chunk per trip): the weight tiles of the next chunk are
  // prefetched by the tail of this one (rotating queue) and the next chunk's activations are
  // generated under this chunk's MFMAs.
#pragma unroll 1
  for (int cc = 0; cc < T; ++cc) {
    f4 nb[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) nb[e] = bin[e];
    const int Wc = W2 + cc * (T * 256);
    constexpr int TG = NE >= 2 ? 1 : 2;  // output tiles issued together: NE*TG >= 2 independent chains
#pragma unroll
    for (int t0 = 0; t0 < T; t0 += TG) {
      // T % PF == 0: tile (cc, t) always lives in queue slot t % PF.  The MFMAs read the slot, THEN the slot is
      // refilled in place with tile t + PF (issuing the refill first would need a second register and a copy at
      // the loop back-edge, i.e. a full vmcnt(0) drain per K chunk).
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < TG; ++k)
          if (t0 + k < T) {
#pragma unroll
            for (int e = 0; e < NE; ++e) acc[e][t0 + k] = mfma1(wq[(t0 + k) % PF][q], bin[e][q], acc[e][t0 + k]);
          }
      if (t0 == 0) {  // next chunk's activations (clamped on the last trip: no branch), interleaved with group 0
        const int ncc = cc + 1 < T ? cc + 1 : T - 1;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
          if constexpr (EF == 2) nb[e] = silu4(edge_u(pp[e], qq[e], sCr, sCd, g, ncc, ec[e].r, ec[e].d0));
          else nb[e] = silu4(edge_u_ef<EF>(pp[e], qq[e], sCr, HP, g, ncc, ec[e].ft));
        }
      }
#if GAUDI_PIN_SCHED
      // Plain scheduling fences in source order: MFMA group | refills of the slots it read | next group ...
      // Left alone, hipcc sinks the refill loads next to their consumers.  (The group-solver pins used earlier were
      // a few percent faster but miscompiled some instantiations -- DESIGN.md section 7.)
      __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
      for (int k = 0; k < TG; ++k) {
        const int t = t0 + k;
        if (t < T) {
          // tile index cc*T + t + PF (clamped at the end of the matrix; the surplus loads are unused)
          const int nxt = (cc * T + t + PF < T * T) ? (t + PF) : t;
          wq[t % PF] = ldw4(wb, Wc + 256 * nxt, lo);
        }
      }
#if GAUDI_PIN_SCHED
      __builtin_amdgcn_sched_barrier(0);
#endif
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) bin[e] = nb[e];
  }
}

// Edge-level GEMM whose input already sits in registers in C/B layout (chained MLP layer):
//   out[e][t] = init + W . in[e]      in[e][cc] = features 16cc+4g+q of edge column c
// init = bias (LDS vector or null) + per-column LDS rows rowinit[e] (may be null).
// Output-tile-outer order: only NE*TB accumulator quads are live while the K loop of an output tile
// runs (NE*TB >= 2 independent MFMA chains), each finished tile is retired once; the inputs stay in
// VGPRs.  (Input-chunk-outer order made hipcc shuttle every accumulator between AGPRs and VGPRs around
// each MFMA.)
template <int HP, int NE>
__device__ __forceinline__ void edge_gemm_from_regs(f4 (&out)[NE][HP / 16], const f4 (&in)[NE][HP / 16], const WBuf& wb,
                                                    int W, const float* sBias, const float* const (&rowinit)[NE], int lane) {
  constexpr int T = HP / 16;
  constexpr int TB = NE >= 2 ? 1 : 2;  // output tiles in flight
  // queue depth in tiles: a tile feeds 4*NE MFMAs (128*NE cycles), so single-tile calls need a deeper queue to
  // look the same ~1.5k cycles ahead
  constexpr int PFW = GAUDI_PF_REGS_NE1 > 0 && NE == 1 ? GAUDI_PF_REGS_NE1 : kPF;
  constexpr int PF = PFW < T ? PFW : T;
  constexpr int TT = (T + TB - 1) / TB * TB;  // tile count rounded up to TB (surplus tiles skipped)
  const int c = lane & 15, g = lane >> 4;
  const int lo = c * 4 + g;
  // flattened tile sequence: for t0 (step TB) { for cc { for tb } } ; tile (cc, t) sits at (cc*T + t)*256 floats
  auto tile_off = [](int seq) {
    const int per = T * TB;
    const int t0 = seq / per * TB, r = seq % per, cc = r / TB, tb = r % TB;
    const int t = t0 + tb < T ? t0 + tb : T - 1;
    return (cc * T + t) * 256;
  };
  constexpr int NSEQ = TT * T;
  f4 wq[PF];
#pragma unroll
  for (int p = 0; p < PF; ++p) wq[p] = ldw4(wb, W + tile_off(p), lo);
#pragma unroll
  for (int t0 = 0; t0 < T; t0 += TB) {
    f4 acc[NE][TB];
#pragma unroll
    for (int tb = 0; tb < TB; ++tb) {
      const int t = t0 + tb < T ? t0 + tb : T - 1;
      const f4 b = sBias != nullptr ? *(const f4*)(sBias + 16 * t + 4 * g) : splat(0.f);
#pragma unroll
      for (int e = 0; e < NE; ++e)
        acc[e][tb] = rowinit[e] != nullptr ? b + *(const f4*)(rowinit[e] + 16 * t + 4 * g) : b;
    }
#pragma unroll
    for (int cc = 0; cc < T; ++cc) {
      f4 w[TB];
#pragma unroll
      for (int tb = 0; tb < TB; ++tb) {
        const int seq = (t0 / TB) * (T * TB) + cc * TB + tb;
        w[tb] = wq[seq % PF];
        if (seq + PF < NSEQ) wq[seq % PF] = ldw4(wb, W + tile_off(seq + PF), lo);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int tb = 0; tb < TB; ++tb)
          if (t0 + tb < T) {
#pragma unroll
            for (int e = 0; e < NE; ++e) acc[e][tb] = mfma1(w[tb][q], in[e][cc][q], acc[e][tb]);
          }
#if GAUDI_PIN_SCHED_UNROLLED
      // Hard fence per tile group: nothing may cross, so the refill loads stay PF tiles ahead of their use exactly
      // as written (left alone, hipcc sinks them next to their consumers: vmcnt(1) waits, ~45 % MFMA efficiency).
      __builtin_amdgcn_sched_barrier(0);
#endif
    }
#pragma unroll
    for (int tb = 0; tb < TB; ++tb)
      if (t0 + tb < T) {
#pragma unroll
        for (int e = 0; e < NE; ++e) out[e][t0 + tb] = acc[e][tb];
      }
  }
}

// ---------------------------------------------------------------------------------------------
// Segmented edge->node sum ("scatter_add over row", egnn_new.py:403-414): the wave owns every
// edge of the nodes it serves and its edge list is sorted by receiving node, so the sum is a
// run-length reduction: the 16x HP tile is bounced through the wave's private LDS scratch and
// lanes 0..HP/4-1 accumulate 4 features each down the 16 edge slots, flushing a node's sum
// when the (wave-uniform) node id changes.  No atomics, fixed order (ascending j like the
// reference's CPU scatter).
// ---------------------------------------------------------------------------------------------
template <int HP>
struct SegSum {
  f4 run;
  int cur;
  __device__ __forceinline__ void init() { run = splat(0.f); cur = -1; }
  __device__ __forceinline__ void flush(float* sOut, float div, int lane) {
    constexpr int LD = HP + 4;
    if (cur >= 0 && lane < HP / 4) *(f4*)(sOut + cur * LD + 4 * lane) = run / div;
  }
  // scr: [16][LD] tile written as scr[col][feature]; node_of_col: value held by lane k = node of column k
  __device__ __forceinline__ void add_tile(const float* scr, int node_of_col, float* sOut, float div, int lane) {
    constexpr int LD = HP + 4;
    // all 16 rows are fetched first (independent LDS reads, one latency), then folded in slot order; reading them one
    // by one behind the wave-uniform "node changed" branches serialised 16 LDS round trips per tile
#pragma unroll
    for (int h = 0; h < 16 / GAUDI_SEG_BATCH; ++h) {  // batches of rows: fewer live registers than one batch of 16, one latency each
      f4 row[GAUDI_SEG_BATCH];
      if (lane < HP / 4) {
#pragma unroll
        for (int k = 0; k < GAUDI_SEG_BATCH; ++k) row[k] = *(const f4*)(scr + (GAUDI_SEG_BATCH * h + k) * LD + 4 * lane);
      }
#pragma unroll
      for (int k = 0; k < GAUDI_SEG_BATCH; ++k) {
        const int nk = __builtin_amdgcn_readlane(node_of_col, GAUDI_SEG_BATCH * h + k);
        if (nk != cur) {
          flush(sOut, div, lane);
          run = splat(0.f);
          cur = nk;
        }
        if (lane < HP / 4) run += row[k];
      }
    }
  }
};

// ---------------------------------------------------------------------------------------------
// Philox4x32-10 counter RNG + Box-Muller.  One call -> 4 standard normals.
// key = seed, counter = (quad index inside the sample's [N*D] draw, draw index, global sample lo/hi)
// so the stream is independent of batch sharding.
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t out[4]) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ inline f4 philox_normal4(uint64_t seed, uint64_t sample, uint32_t draw, uint32_t quad) {
  uint32_t r[4];
  philox4x32_10(quad, draw, (uint32_t)sample, (uint32_t)(sample >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
  const float k2m32 = 2.3283064365386963e-10f;  // 2^-32
  const float u1 = ((float)(r[0] >> 8) + 1.0f) * (1.0f / 16777216.0f);  // (0,1]
  const float u2 = (float)(r[1] >> 8) * (1.0f / 16777216.0f);
  const float u3 = ((float)(r[2] >> 8) + 1.0f) * (1.0f / 16777216.0f);
  const float u4 = (float)(r[3] >> 8) * (1.0f / 16777216.0f);
  (void)k2m32;
  const float ra = sqrtf(-2.0f * logf(u1)), rb = sqrtf(-2.0f * logf(u3));
  float sa, ca, sb, cb;
  sincosf(6.283185307179586f * u2, &sa, &ca);
  sincosf(6.283185307179586f * u4, &sb, &cb);
  return (f4){ra * ca, ra * sa, rb * cb, rb * sb};
}

// ---------------------------------------------------------------------------------------------
// Value targets (gaudi_sample_target): T(p) = sum_k w[k] p[k] + q[k] a(p[k] - c[k], side[k])^2 with a(d, 0) = d,
// a(d, +1) = max(d, 0) (upper bound), a(d, -1) = min(d, 0) (lower bound; a NaN d gives 0 on both hinges).
// One molecule's parameters are a row of 4 K + 1 floats: w [K] | q [K] | c [K] | side [K] | scale.
// Seed of the reverse pass, d(scale * T)/dp[k] = (w + (q + q) * a) * scale: every operation rounded on its own, in this order
// (no contraction), so the kernels, gaudi_host_target_seed and a numpy float32 expression agree bit for bit.
// ---------------------------------------------------------------------------------------------
__host__ __device__ constexpr int target_row_floats(int K) { return 4 * K + 1; }
__host__ __device__ inline float target_seed(const float* row, int K, int k, float p) {
#pragma clang fp contract(off)
  const float w = row[k], q = row[K + k], c = row[2 * K + k], side = row[3 * K + k], scale = row[4 * K];
  const float d = p - c;
  const float a = side == 0.f ? d : (side > 0.f ? (d > 0.f ? d : 0.f) : (d < 0.f ? d : 0.f));
  const float q2 = q + q;
  const float qa = q2 * a;
  const float g = w + qa;
  return g * scale;
}

}  // namespace gaudi
