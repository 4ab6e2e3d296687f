// kern8s2_fused_tiny.hip -- sampler_kernel_v<V8T<1, false, 0, true>, ...> (see kern8s2_fused_192_208.hip) for the test-sized networks [(32, 48), (64, 64)];
// registered in the kernel table (kernel_table.h).
#include "kernel_table.h"

namespace {
using namespace gaudi;
using V = V8T<1, false, 0, true>;
const KernelEntry kEntries[] = {
    entry<V, 32, 48, true>(), entry<V, 32, 48>(),
    entry<V, 64, 64, true>(), entry<V, 64, 64>(),
};
KernelTable kTable(kEntries);
}  // namespace
