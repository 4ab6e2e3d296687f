// kern8mp_fused.hip -- 8-wave kernels for WIDE groups on the FULL weight ring (round 6): several rounds of eight edge tiles, split
// operands, the predictor's fifth node buffer in the workgroup's global scratch (sampler_kernel.h: V8T<1, true, 0, false, true>;
// w8_pred.h: PredSmem, PG) -- two cata-11 molecules per workgroup do not fit five resident buffers beside the full ring at the
// default widths [(192, 208) and the test widths (32, 48)].  Own translation unit; registered in the kernel table (kernel_table.h).
#include "kernel_table.h"

namespace {
using namespace gaudi;
using V = V8T<1, true, 0, false, true>;
const KernelEntry kEntries[] = {
    entry<V, 192, 208>(),
    entry<V, 32, 48>(),
};
KernelTable kTable(kEntries);
}  // namespace
