// kern8m_pred_small.hip -- 8-wave kernels whose predictor runs SEVERAL rounds of eight edge tiles (graphs of more than 128 live-edge slots:
// fully connected molecules of 12+ nodes; w8_pred.h, template flag MR) [the test widths, predictor only, SP = 0, 1, 2]; own translation unit so the
// instantiations compile in parallel; registered in the kernel table (kernel_table.h).  SP: 0 = fp32 matrix instructions,
// 1 / 2 = split operands with the full / half weight ring.
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V8T<0, true>, 0, 32, true>(), entry<V8T<0, true>, 0, 32>(),
    entry<V8T<0, true>, 0, 48, true>(), entry<V8T<0, true>, 0, 48>(),
    entry<V8T<0, true>, 0, 64, true>(), entry<V8T<0, true>, 0, 64>(),
    entry<V8T<1, true>, 0, 32, true>(), entry<V8T<1, true>, 0, 32>(),
    entry<V8T<1, true>, 0, 48, true>(), entry<V8T<1, true>, 0, 48>(),
    entry<V8T<1, true>, 0, 64, true>(), entry<V8T<1, true>, 0, 64>(),
    entry<V8T<2, true>, 0, 32, true>(), entry<V8T<2, true>, 0, 32>(),
    entry<V8T<2, true>, 0, 48, true>(), entry<V8T<2, true>, 0, 48>(),
    entry<V8T<2, true>, 0, 64, true>(), entry<V8T<2, true>, 0, 64>(),
};
KernelTable kTable(kEntries);
}  // namespace
