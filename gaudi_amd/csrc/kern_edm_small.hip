// kern_edm_small.hip -- sampler_kernel_v<V4, ...> instantiations [(32, 0), (48, 0), (64, 0), (128, 0)] (own translation unit so the
// instantiations compile in parallel; registered in the kernel table (kernel_table.h)).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V4, 32, 0>(),
    entry<V4, 48, 0>(),
    entry<V4, 64, 0>(),
    entry<V4, 128, 0>(),
};
KernelTable kTable(kEntries);
}  // namespace
