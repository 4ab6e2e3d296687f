// kern_fused_208_208.hip -- sampler_kernel instantiations [(208, 208)] (own translation unit so the
// instantiations compile in parallel; looked up by gaudi_hip.hip through gaudi_kern_fused_208_208).
#include "sampler_kernel.h"

typedef void (*kernel_fn)(const gaudi::KParams);

kernel_fn gaudi_kern_fused_208_208(int hpe, int hpp) {
  const bool vt = (hpp & gaudi::kVtKernel) != 0;  // the value-target instantiation (sampler_kernel.h: VT)
  hpp &= ~gaudi::kVtKernel;
  if (hpe == 208 && hpp == 208) return vt ? gaudi::sampler_kernel<208, 208, true> : gaudi::sampler_kernel<208, 208>;
  return nullptr;
}
