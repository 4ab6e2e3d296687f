// kern8s1_fused_192_208.hip -- sampler_kernel_v<V8T<1, false, 0, false, false, true>, ...>: the resident full-ring split-operand kernel
// (kern8s_fused_192_208.hip) with N1 set -- node GEMMs compiled for ONE column tile and ONE tail k-step (w8_nodes_f16.h:
// kNodeOneTile); the host runs it when a workgroup has at most 16 node slots and the 208-wide network has H % 16 == 4 (C2, C3).
// Value-target launches keep the plain kernel.  SD (GAUDI_SIDE_STAGES, build switch): the predictor's forward pass can give the last
// wave a side job where the host asks for it (sampler_kernel.h: V8T, SD; w8_pred.h: pred_forward) -- bit 0 = stage A, 0 = the
// kernel without the job.  Instantiations [(192, 208)]; registered in the kernel table (kernel_table.h).
#include "kernel_table.h"

#ifndef GAUDI_SIDE_STAGES
#define GAUDI_SIDE_STAGES 1
#endif

namespace {
using namespace gaudi;
using V = V8T<1, false, 0, false, false, true, GAUDI_SIDE_STAGES>;
const KernelEntry kEntries[] = {
    entry<V, 192, 208>(),
};
KernelTable kTable(kEntries);
}  // namespace
