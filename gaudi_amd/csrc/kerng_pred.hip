// kerng_pred.hip -- V4G kernels (node buffers in global memory), predictor only (the unit-test entry points).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V4G, 0, 48, true>(), entry<V4G, 0, 48>(),
    entry<V4G, 0, 208, true>(), entry<V4G, 0, 208>(),
};
KernelTable kTable(kEntries);
}  // namespace
