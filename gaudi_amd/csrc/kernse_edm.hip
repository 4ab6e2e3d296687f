// kernse_edm.hip -- 4-wave sampler kernels for sin_embedding denoisers (sampler_kernel.h: V4S / V4GS; edm_device.h: EF = 24), EDM
// only: resident node buffers at the tiny and the default width (the other widths: kernse_edm_more.hip), node buffers in global
// memory for molecules beyond the LDS limit (own translation unit; registered in the kernel table (kernel_table.h)).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V4S, 32, 0>(),
    entry<V4S, 192, 0>(),
    entry<V4GS, 32, 0>(),
    entry<V4GS, 192, 0>(),
};
KernelTable kTable(kEntries);
}  // namespace
