// kern8h_fused_tiny.hip -- sampler_kernel_v<V8H, ...> (8 waves, edge and node GEMMs on fp16-pair operands with the half-size weight ring: w8_split.h, SplitGeo MODE 2) instantiations [(32, 48), (32, 32), (48, 48), (64, 64)] (own translation unit so the
// instantiations compile in parallel; registered in the kernel table (kernel_table.h)).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V8H, 32, 48, true>(), entry<V8H, 32, 48>(),
    entry<V8H, 32, 32, true>(), entry<V8H, 32, 32>(),
    entry<V8H, 48, 48, true>(), entry<V8H, 48, 48>(),
    entry<V8H, 64, 64, true>(), entry<V8H, 64, 64>(),
};
KernelTable kTable(kEntries);
}  // namespace
