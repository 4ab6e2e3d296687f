// kern_pred_208.hip -- sampler_kernel_v<V4, ...> instantiations [(0, 208)] (own translation unit so the
// instantiations compile in parallel; registered in the kernel table (kernel_table.h)).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V4, 0, 208, true>(), entry<V4, 0, 208>(),
};
KernelTable kTable(kEntries);
}  // namespace
