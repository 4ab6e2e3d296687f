// kern8s_fused_tiny.hip -- sampler_kernel_v<V8S, ...> (8 waves, edge and node GEMMs on fp16-pair operands: w8_split.h, w8_nodes_f16.h) instantiations [(32, 48), (32, 32), (48, 48), (64, 64)] (own translation unit so the
// instantiations compile in parallel; registered in the kernel table (kernel_table.h)).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V8S, 32, 48, true>(), entry<V8S, 32, 48>(),
    entry<V8S, 32, 32, true>(), entry<V8S, 32, 32>(),
    entry<V8S, 48, 48, true>(), entry<V8S, 48, 48>(),
    entry<V8S, 64, 64, true>(), entry<V8S, 64, 64>(),
};
KernelTable kTable(kEntries);
}  // namespace
