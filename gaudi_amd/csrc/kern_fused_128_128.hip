// kern_fused_128_128.hip -- sampler_kernel instantiations [(128, 128)] (own translation unit so the
// instantiations compile in parallel; looked up by gaudi_hip.hip through gaudi_kern_fused_128_128).
#include "sampler_kernel.h"

typedef void (*kernel_fn)(const gaudi::KParams);

kernel_fn gaudi_kern_fused_128_128(int hpe, int hpp) {
  const bool vt = (hpp & gaudi::kVtKernel) != 0;  // the value-target instantiation (sampler_kernel.h: VT)
  hpp &= ~gaudi::kVtKernel;
  if (hpe == 128 && hpp == 128) return vt ? gaudi::sampler_kernel<128, 128, true> : gaudi::sampler_kernel<128, 128>;
  return nullptr;
}
