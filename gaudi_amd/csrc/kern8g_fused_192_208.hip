// kern8g_fused_192_208.hip -- 8-wave sampler kernels with the node buffers in global memory (sampler_kernel.h: V8T<1, true, 1> = V8G, round 4):
// molecules whose node buffers do not fit 160 KiB of LDS beside the weight ring; split edge GEMMs with the full ring, several
// rounds of edge tiles in the predictor [(192, 208): the default architectures].  Own translation unit (the instantiations compile in parallel); looked up by
// gaudi_hip.hip through gaudi_kern8g_fused_192_208.
#include "sampler_kernel.h"

typedef void (*kernel_fn)(const gaudi::KParams);

kernel_fn gaudi_kern8g_fused_192_208(int hpe, int hpp) {
  const bool vt = (hpp & gaudi::kVtKernel) != 0;  // the value-target instantiation (sampler_kernel.h: VT)
  hpp &= ~gaudi::kVtKernel;
  if (hpe == 192 && hpp == 208) return vt ? gaudi::sampler_kernel8g<192, 208, true> : gaudi::sampler_kernel8g<192, 208>;
  return nullptr;
}
