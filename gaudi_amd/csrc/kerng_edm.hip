// kerng_edm.hip -- 4-wave sampler kernels with the node buffers in global memory (sampler_kernel.h: V4G), EDM only:
// molecules whose working set exceeds 160 KiB of LDS (own translation unit; registered in the kernel table (kernel_table.h)).
#include "kernel_table.h"

namespace {
using namespace gaudi;
const KernelEntry kEntries[] = {
    entry<V4G, 32, 0>(),
    entry<V4G, 192, 0>(),
};
KernelTable kTable(kEntries);
}  // namespace
