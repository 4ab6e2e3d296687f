// kern_fused_192_192.hip -- sampler_kernel_v<V4, ...> instantiations [(192, 192)] (own translation unit so the
// instantiations compile in parallel; registered in the kernel table (kernel_table.h)).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V4, 192, 192, true>(), entry<V4, 192, 192>(),
};
KernelTable kTable(kEntries);
}  // namespace
