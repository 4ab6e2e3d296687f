// kern8s2_edm_192.hip -- sampler_kernel_v<V8T<1, false, 0, true>, ...>: the resident full-ring split-operand kernel (kern8s_edm_192.hip) with FR set -- node-GEMM
// split passes and epilogues recompute their lane addresses per call (w8_nodes_f16.h: FL); the host runs it when a workgroup has
// more than 16 node slots (two column tiles per node GEMM: C4, packed workgroups).  Instantiations [(192, 0)];
// registered in the kernel table (kernel_table.h).
#include "kernel_table.h"

namespace {
using namespace gaudi;
using V = V8T<1, false, 0, true>;
const KernelEntry kEntries[] = {
    entry<V, 192, 0>(),
};
KernelTable kTable(kEntries);
}  // namespace
