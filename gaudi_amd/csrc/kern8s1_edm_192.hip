// kern8s1_edm_192.hip -- sampler_kernel_v<V8T<1, false, 0, false, false, true>, ...>: the resident full-ring split-operand kernel
// (kern8s_edm_192.hip) with N1 set -- node GEMMs compiled for ONE column tile (w8_nodes_f16.h: kNodeOneTile); the host runs it
// when a workgroup has at most 16 node slots (unguided chains of C2 / C3-sized molecules).  Instantiations [(192, 0)];
// registered in the kernel table (kernel_table.h).
#include "kernel_table.h"

namespace {
using namespace gaudi;
using V = V8T<1, false, 0, false, false, true>;
const KernelEntry kEntries[] = {
    entry<V, 192, 0>(),
};
KernelTable kTable(kEntries);
}  // namespace
