// kern_pred_small.hip -- sampler_kernel instantiations [(0, 32), (0, 48), (0, 64), (0, 128)] (own translation unit so the
// instantiations compile in parallel; looked up by gaudi_hip.hip through gaudi_kern_pred_small).
#include "sampler_kernel.h"

typedef void (*kernel_fn)(const gaudi::KParams);

kernel_fn gaudi_kern_pred_small(int hpe, int hpp) {
  const bool vt = (hpp & gaudi::kVtKernel) != 0;  // the value-target instantiation (sampler_kernel.h: VT)
  hpp &= ~gaudi::kVtKernel;
  if (hpe == 0 && hpp == 32) return vt ? gaudi::sampler_kernel<0, 32, true> : gaudi::sampler_kernel<0, 32>;
  if (hpe == 0 && hpp == 48) return vt ? gaudi::sampler_kernel<0, 48, true> : gaudi::sampler_kernel<0, 48>;
  if (hpe == 0 && hpp == 64) return vt ? gaudi::sampler_kernel<0, 64, true> : gaudi::sampler_kernel<0, 64>;
  if (hpe == 0 && hpp == 128) return vt ? gaudi::sampler_kernel<0, 128, true> : gaudi::sampler_kernel<0, 128>;
  return nullptr;
}
