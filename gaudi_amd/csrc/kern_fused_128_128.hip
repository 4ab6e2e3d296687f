// kern_fused_128_128.hip -- sampler_kernel_v<V4, ...> instantiations [(128, 128)] (own translation unit so the
// instantiations compile in parallel; registered in the kernel table (kernel_table.h)).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V4, 128, 128, true>(), entry<V4, 128, 128>(),
};
KernelTable kTable(kEntries);
}  // namespace
