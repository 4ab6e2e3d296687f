// kern8s_edm_small.hip -- sampler_kernel_v<V8S, ...> (8 waves, edge and node GEMMs on fp16-pair operands: w8_split.h, w8_nodes_f16.h) instantiations [(32, 0), (48, 0), (64, 0), (128, 0)] (own translation unit so the
// instantiations compile in parallel; registered in the kernel table (kernel_table.h)).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V8S, 32, 0>(),
    entry<V8S, 48, 0>(),
    entry<V8S, 64, 0>(),
    entry<V8S, 128, 0>(),
};
KernelTable kTable(kEntries);
}  // namespace
