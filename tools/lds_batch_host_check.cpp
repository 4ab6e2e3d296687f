// tools/lds_batch_host_check.cpp -- the host side of csrc/lds_fold.h against the plain one-row-per-iteration loops it replaces
// (w8_pred.h: pred_backward, w8_edm.h: coord_update), bit for bit: run lengths 0 .. 16, batch sizes 5 and 8, consecutive rows and
// rows through an index list, sums and differences, float and float4 values, the joint two-chain batch of the du gather; data
// with +-0, denormals, infinities and NaNs.  Stand-alone (tests/test_lds_batch_cpu.py builds and runs it, also under
// -fsanitize=address,undefined): the tables are sized exactly, so a load that was not clamped into the table is a finding.
//
// Two results are equal when their bits are, or when both are NaN: which payload a sum of two NaNs carries depends on the
// operand order of the add instruction, which a compiler may pick either way for the same expression.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lds_fold.h"

#if defined(__clang__)
typedef float f4 __attribute__((ext_vector_type(4)));
#else
typedef float f4 __attribute__((vector_size(16)));
#endif

static uint32_t g_state = 0x2545F491u;
static uint32_t rnd() {
  g_state ^= g_state << 13;
  g_state ^= g_state >> 17;
  g_state ^= g_state << 5;
  return g_state;
}
static float bits(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static float value() {
  switch (rnd() % 16) {
    case 0: return 0.0f;
    case 1: return -0.0f;
    case 2: return bits(0x7f800000u);  // +inf
    case 3: return bits(0xff800000u);  // -inf
    case 4: return bits(0x7fc00000u);  // NaN
    case 5: return bits(0x00000001u + rnd() % 1000);  // denormal
    case 6: return bits(0x7f7fffffu);  // the largest finite value: sums overflow
    default: return ((int)(rnd() % 2000001) - 1000000) * (1.0f / 4096.0f) * (float)(1u << (rnd() % 12));
  }
}
static bool same(float a, float b) {
  if (a != a && b != b) return true;
  return memcmp(&a, &b, 4) == 0;
}
static bool same(f4 a, f4 b) { return same(a[0], b[0]) && same(a[1], b[1]) && same(a[2], b[2]) && same(a[3], b[3]); }
static float init(float*) { return value(); }
static f4 init(f4*) { return (f4){value(), value(), value(), value()}; }

template <int B, class V>
static int check(int rows, int stride, int col) {
  int bad = 0;
  // heap tables of the exact size: the sanitizer sees a read one float outside either
  std::vector<float> table((size_t)(rows - 1) * stride + col + sizeof(V) / 4);
  std::vector<uint16_t> list(rows);
  for (int n = 0; n <= 16 && n <= rows; ++n) {
    for (int trial = 0; trial < 64; ++trial) {
      for (float& x : table) x = value();
      for (uint16_t& x : list) x = (uint16_t)(rnd() % rows);
      const int first = (int)(rnd() % (rows - n + 1));
      const float* base = table.data() + col;
      const V s0 = init((V*)nullptr);
      V pa = s0, ps = s0, qa = s0, qs = s0;
      for (int k = 0; k < n; ++k) pa += *(const V*)(base + (first + k) * stride);
      for (int k = 0; k < n; ++k) ps -= *(const V*)(base + (first + k) * stride);
      for (int k = first; k < first + n; ++k) qa += *(const V*)(base + (int)list[k] * stride);
      for (int k = first; k < first + n; ++k) qs -= *(const V*)(base + (int)list[k] * stride);
      bad += !same(pa, gaudi::fold_run<B, V>(s0, base, stride, first, n));
      bad += !same(ps, gaudi::fold_run<B, V, true>(s0, base, stride, first, n));
      bad += !same(qa, gaudi::fold_list<B, V>(s0, base, stride, list.data(), first, n));
      bad += !same(qs, gaudi::fold_list<B, V, true>(s0, base, stride, list.data(), first, n));
      // the du gather's form: two chains of different lengths share the batch loop (a run of n rows and a list of m)
      const int m = (int)(rnd() % ((rows - first < 16 ? rows - first : 16) + 1));
      V la = s0;
      for (int k = first; k < first + m; ++k) la += *(const V*)(base + (int)list[k] * stride);
      V sp = s0, sq = s0;
      for (int k0 = 0; k0 < (n > m ? n : m); k0 += B) {
        gaudi::FoldBatch<B, V> bp, bq;
        int rp[B], rq[B];
        bq.rows_of_list(rq, list.data(), first, k0, m);
        bp.rows_of_run(rp, first, k0, n);
        bp.load(base, stride, rp);
        bq.load(base, stride, rq);
        sp = bp.add(sp, k0, n);
        sq = bq.add(sq, k0, m);
      }
      bad += !same(pa, sp);
      bad += !same(la, sq);
    }
  }
  return bad;
}

int main() {
  int bad = 0, forms = 0;
  const int shapes[][3] = {{16, 4, 0}, {16, 4, 3}, {17, 20, 4}, {33, 212, 8}, {1, 4, 1}};  // rows, floats per row, column
  for (const auto& s : shapes) {
    bad += check<5, float>(s[0], s[1], s[2]);
    bad += check<8, float>(s[0], s[1], s[2]);
    forms += 2;
    if (s[2] % 4 == 0 && s[1] % 4 == 0) {  // (float4 rows are 16-byte aligned in the kernels)
      bad += check<5, f4>(s[0], s[1], s[2]);
      bad += check<8, f4>(s[0], s[1], s[2]);
      forms += 2;
    }
  }
  printf("lds_batch_host_check: %d table forms, run lengths 0..16, %d mismatches\n", forms, bad);
  return bad != 0;
}
