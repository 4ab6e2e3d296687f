// kern8_pred_208.hip -- sampler_kernel_v<V8, ...> (8 waves, two per SIMD) instantiations [(0, 208)] (own translation unit so the
// instantiations compile in parallel; registered in the kernel table (kernel_table.h)).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V8, 0, 208, true>(), entry<V8, 0, 208>(),
};
KernelTable kTable(kEntries);
}  // namespace
