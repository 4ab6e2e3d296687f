// kern8gp_pred_208.hip -- 8-wave sampler kernels with three of the five node buffers in global memory and P / Q in LDS
// (sampler_kernel.h: V8T<1, true, 2>; w8_edm.h: gn_lds_buffers -- round 6): what a molecule beyond the resident kernels' LDS limit
// runs on where that plan fits (gaudi_hip.hip: stage_graph8), kern8g_* otherwise.  Own translation unit; looked up through
// gaudi_kern8gp_pred_208.
#include "sampler_kernel.h"

typedef void (*kernel_fn)(const gaudi::KParams);

kernel_fn gaudi_kern8gp_pred_208(int hpe, int hpp) {
  const bool vt = (hpp & gaudi::kVtKernel) != 0;  // the value-target instantiation (sampler_kernel.h: VT)
  hpp &= ~gaudi::kVtKernel;
  if (hpe == 0 && hpp == 208) return vt ? gaudi::sampler_kernel8gp<0, 208, true> : gaudi::sampler_kernel8gp<0, 208>;
  return nullptr;
}
