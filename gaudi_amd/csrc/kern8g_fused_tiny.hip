// kern8g_fused_tiny.hip -- 8-wave sampler kernels with the node buffers in global memory (sampler_kernel.h: V8T<1, true, 1> = V8G, round 4):
// molecules whose node buffers do not fit 160 KiB of LDS beside the weight ring; split edge GEMMs with the full ring, several
// rounds of edge tiles in the predictor [the test widths].  Own translation unit (the instantiations compile in parallel);
// registered in the kernel table (kernel_table.h).
#include "kernel_table.h"

namespace {
using namespace gaudi;
using V = V8T<1, true, 1>;
const KernelEntry kEntries[] = {
    entry<V, 32, 48, true>(), entry<V, 32, 48>(),
    entry<V, 32, 32, true>(), entry<V, 32, 32>(),
    entry<V, 48, 48, true>(), entry<V, 48, 48>(),
    entry<V, 64, 64, true>(), entry<V, 64, 64>(),
};
KernelTable kTable(kEntries);
}  // namespace
