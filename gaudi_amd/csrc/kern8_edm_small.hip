// kern8_edm_small.hip -- sampler_kernel_v<V8, ...> (8 waves, two per SIMD) instantiations [(32, 0), (48, 0), (64, 0), (128, 0)] (own translation unit so the
// instantiations compile in parallel; registered in the kernel table (kernel_table.h)).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V8, 32, 0>(),
    entry<V8, 48, 0>(),
    entry<V8, 64, 0>(),
    entry<V8, 128, 0>(),
};
KernelTable kTable(kEntries);
}  // namespace
