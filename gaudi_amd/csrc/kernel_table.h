// kernel_table.h -- how the host finds an instantiation of sampler_kernel_v<V, HPE, HPP, VT>.  Every kern*_*.hip holds one array
// of entries and registers it at load time; gaudi_hip.hip searches the registered arrays by key (find_kernel).  A key is never
// written down: entry<V, HPE, HPP, VT>() takes it from the same template arguments the function pointer is made of.
#pragma once
#include "sampler_kernel.h"

namespace gaudi {

typedef void (*kernel_fn)(const KParams);

// the arguments of the template, as values (sampler_kernel.h: V4T / V8T say what they select)
struct KernelKey {
  int waves;  // 4 or 8: the kernel family
  int sp;     // 8 waves: edge-GEMM arithmetic / weight ring (0 fp32 instructions, 1 full ring, 2 half ring)
  bool mr;
  int gn;     // node buffers in global memory: 0 none, 1 all of them, 2 all but P / Q (8 waves only)
  bool fr, pg;
  bool n1;    // 8 waves: node GEMMs compiled for one column tile and one tail k-step (at most 16 node slots)
  int ef;     // edge features of the denoiser's first Linears: 2, or 24 (sin_embedding)
  int hpe, hpp;
  bool vt;
};
inline bool operator==(const KernelKey& a, const KernelKey& b) {
  return a.waves == b.waves && a.sp == b.sp && a.mr == b.mr && a.gn == b.gn && a.fr == b.fr && a.pg == b.pg && a.n1 == b.n1 && a.ef == b.ef &&
         a.hpe == b.hpe && a.hpp == b.hpp && a.vt == b.vt;
}

struct KernelEntry {
  KernelKey key;
  kernel_fn fn;
  int side;  // not part of the key: stages of the side job the kernel has compiled in (sampler_kernel.h: V8T, SD); a launch asks for
             // the job through KParams::side_off, and a kernel without it ignores that
};
template <class V, int HPE, int HPP, bool VT = false>
constexpr KernelEntry entry() {
  KernelEntry e{};  // (fields by name: the order of KernelKey's members carries no meaning)
  e.key.waves = V::kWaveCount;
  e.key.sp = V::kSplit;
  e.key.mr = V::kMR;
  e.key.gn = V::kGN;
  e.key.fr = V::kFR;
  e.key.pg = V::kPG;
  e.key.n1 = V::kN1;
  e.key.ef = V::kEF;
  e.key.hpe = HPE;
  e.key.hpp = HPP;
  e.key.vt = VT;
  e.fn = &sampler_kernel_v<V, HPE, HPP, VT>;
  e.side = HPP != 0 ? V::kSD : 0;  // (the job is the predictor's)
  return e;
}

// one translation unit's entries, linked into the list gaudi_hip.hip owns (a zero-initialised pointer: ready before any
// translation unit's registration runs, whatever their order)
struct KernelTable {
  const KernelEntry* entries;
  int n;
  KernelTable* next;
  template <int N>
  explicit KernelTable(const KernelEntry (&e)[N]);
};
extern KernelTable* g_kernel_tables;
template <int N>
KernelTable::KernelTable(const KernelEntry (&e)[N]) : entries(e), n(N), next(g_kernel_tables) {
  g_kernel_tables = this;
}

}  // namespace gaudi
