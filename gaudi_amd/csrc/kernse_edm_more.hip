// kernse_edm_more.hip -- 4-wave sampler kernels for sin_embedding denoisers (sampler_kernel.h: V4S; edm_device.h: EF = 24), EDM only,
// the remaining hidden sizes of the 4-wave family: an unguided chain runs on these alone, a guided one as two launches per step with
// the ordinary predictor-only kernel (gaudi_hip.hip: LaunchPlan::two).  Own translation unit; registered in the kernel table (kernel_table.h).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V4S, 48, 0>(),
    entry<V4S, 64, 0>(),
    entry<V4S, 128, 0>(),
    entry<V4S, 208, 0>(),
    entry<V4S, 256, 0>(),
};
KernelTable kTable(kEntries);
}  // namespace
