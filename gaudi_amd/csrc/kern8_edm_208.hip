// kern8_edm_208.hip -- sampler_kernel_v<V8, ...> (8 waves, two per SIMD) instantiations [(208, 0)] (own translation unit so the
// instantiations compile in parallel; registered in the kernel table (kernel_table.h)).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V8, 208, 0>(),
};
KernelTable kTable(kEntries);
}  // namespace
