// kern_pred_192.hip -- sampler_kernel instantiations [(0, 192)] (own translation unit so the
// instantiations compile in parallel; looked up by gaudi_hip.hip through gaudi_kern_pred_192).
#include "sampler_kernel.h"

typedef void (*kernel_fn)(const gaudi::KParams);

kernel_fn gaudi_kern_pred_192(int hpe, int hpp) {
  const bool vt = (hpp & gaudi::kVtKernel) != 0;  // the value-target instantiation (sampler_kernel.h: VT)
  hpp &= ~gaudi::kVtKernel;
  if (hpe == 0 && hpp == 192) return vt ? gaudi::sampler_kernel<0, 192, true> : gaudi::sampler_kernel<0, 192>;
  return nullptr;
}
