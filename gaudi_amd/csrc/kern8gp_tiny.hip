// kern8gp_tiny.hip -- 8-wave sampler kernels with three of the five node buffers in global memory and P / Q in LDS
// (sampler_kernel.h: V8T<1, true, 2>; w8_edm.h: gn_lds_buffers -- round 6) [the test widths: fused, EDM only, predictor only].
// Own translation unit; registered in the kernel table (kernel_table.h).
#include "kernel_table.h"

namespace {
using namespace gaudi;
using V = V8T<1, true, 2>;
const KernelEntry kEntries[] = {
    entry<V, 32, 48, true>(), entry<V, 32, 48>(),
    entry<V, 32, 0>(),
    entry<V, 0, 48, true>(), entry<V, 0, 48>(),
};
KernelTable kTable(kEntries);
}  // namespace
