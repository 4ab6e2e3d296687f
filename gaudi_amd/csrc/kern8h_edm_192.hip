// kern8h_edm_192.hip -- sampler_kernel_v<V8H, ...> (8 waves, edge and node GEMMs on fp16-pair operands with the half-size weight ring: w8_split.h, SplitGeo MODE 2) instantiations [(192, 0)] (own translation unit so the
// instantiations compile in parallel; registered in the kernel table (kernel_table.h)).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V8H, 192, 0>(),
};
KernelTable kTable(kEntries);
}  // namespace
