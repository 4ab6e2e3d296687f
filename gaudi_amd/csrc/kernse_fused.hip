// kernse_fused.hip -- 4-wave sampler kernels for sin_embedding denoisers (sampler_kernel.h: V4S; edm_device.h: EF = 24) with the
// guidance predictor fused: the tiny and the default width pairs (own translation unit; registered in the kernel table (kernel_table.h)).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V4S, 32, 48, true>(), entry<V4S, 32, 48>(),
    entry<V4S, 192, 208, true>(), entry<V4S, 192, 208>(),
};
KernelTable kTable(kEntries);
}  // namespace
