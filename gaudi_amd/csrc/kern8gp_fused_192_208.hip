// kern8gp_fused_192_208.hip -- 8-wave sampler kernels with three of the five node buffers in global memory and P / Q in LDS
// (sampler_kernel.h: V8T<1, true, 2>; w8_edm.h: gn_lds_buffers -- round 6): what a molecule beyond the resident kernels' LDS limit
// runs on where that plan fits (gaudi_hip.hip: stage_graph8), kern8g_* otherwise.  Own translation unit;
// registered in the kernel table (kernel_table.h).
#include "kernel_table.h"

namespace {
using namespace gaudi;
using V = V8T<1, true, 2>;
const KernelEntry kEntries[] = {
    entry<V, 192, 208, true>(), entry<V, 192, 208>(),
};
KernelTable kTable(kEntries);
}  // namespace
