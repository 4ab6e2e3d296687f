// kern8_pred_256.hip -- sampler_kernel_v<V8, ...> (8 waves, two per SIMD) instantiations [(0, 256)] (own translation unit so the
// instantiations compile in parallel; registered in the kernel table (kernel_table.h)).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V8, 0, 256, true>(), entry<V8, 0, 256>(),
};
KernelTable kTable(kEntries);
}  // namespace
