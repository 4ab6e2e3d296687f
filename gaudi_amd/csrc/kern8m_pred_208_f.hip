// kern8m_pred_208_f.hip -- 8-wave kernels whose predictor runs SEVERAL rounds of eight edge tiles (graphs of more than 128 live-edge slots:
// fully connected molecules of 12+ nodes; w8_pred.h, template flag MR) [(0, 208), SP = 0]; own translation unit so the
// instantiations compile in parallel; registered in the kernel table (kernel_table.h).  SP: 0 = fp32 matrix instructions,
// 1 / 2 = split operands with the full / half weight ring.
#include "kernel_table.h"

namespace {
using namespace gaudi;
using V = V8T<0, true>;
const KernelEntry kEntries[] = {
    entry<V, 0, 208, true>(), entry<V, 0, 208>(),
};
KernelTable kTable(kEntries);
}  // namespace
