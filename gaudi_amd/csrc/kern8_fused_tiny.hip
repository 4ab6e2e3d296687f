// kern8_fused_tiny.hip -- sampler_kernel_v<V8, ...> (8 waves, two per SIMD) instantiations [(32, 48), (32, 32), (48, 48), (64, 64)] (own translation unit so the
// instantiations compile in parallel; registered in the kernel table (kernel_table.h)).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V8, 32, 48, true>(), entry<V8, 32, 48>(),
    entry<V8, 32, 32, true>(), entry<V8, 32, 32>(),
    entry<V8, 48, 48, true>(), entry<V8, 48, 48>(),
    entry<V8, 64, 64, true>(), entry<V8, 64, 64>(),
};
KernelTable kTable(kEntries);
}  // namespace
