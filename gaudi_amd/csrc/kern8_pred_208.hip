// kern8_pred_208.hip -- sampler_kernel8 (8 waves, two per SIMD) instantiations [(0, 208)] (own translation unit so the
// instantiations compile in parallel; looked up by gaudi_hip.hip through gaudi_kern8_pred_208).
#include "sampler_kernel.h"

typedef void (*kernel_fn)(const gaudi::KParams);

kernel_fn gaudi_kern8_pred_208(int hpe, int hpp) {
  const bool vt = (hpp & gaudi::kVtKernel) != 0;  // the value-target instantiation (sampler_kernel.h: VT)
  hpp &= ~gaudi::kVtKernel;
  if (hpe == 0 && hpp == 208) return vt ? gaudi::sampler_kernel8<0, 208, true> : gaudi::sampler_kernel8<0, 208>;
  return nullptr;
}
