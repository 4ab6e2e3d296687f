// kern8s_pred_208.hip -- sampler_kernel_v<V8S, ...> (8 waves, edge and node GEMMs on fp16-pair operands: w8_split.h, w8_nodes_f16.h) instantiations [(0, 208)] (own translation unit so the
// instantiations compile in parallel; registered in the kernel table (kernel_table.h)).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V8S, 0, 208, true>(), entry<V8S, 0, 208>(),
};
KernelTable kTable(kEntries);
}  // namespace
