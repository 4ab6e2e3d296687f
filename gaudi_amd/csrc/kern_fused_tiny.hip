// kern_fused_tiny.hip -- sampler_kernel instantiations [(32, 48), (32, 32), (48, 48), (64, 64)] (own translation unit so the
// instantiations compile in parallel; looked up by gaudi_hip.hip through gaudi_kern_fused_tiny).
#include "sampler_kernel.h"

typedef void (*kernel_fn)(const gaudi::KParams);

kernel_fn gaudi_kern_fused_tiny(int hpe, int hpp) {
  const bool vt = (hpp & gaudi::kVtKernel) != 0;  // the value-target instantiation (sampler_kernel.h: VT)
  hpp &= ~gaudi::kVtKernel;
  if (hpe == 32 && hpp == 48) return vt ? gaudi::sampler_kernel<32, 48, true> : gaudi::sampler_kernel<32, 48>;
  if (hpe == 32 && hpp == 32) return vt ? gaudi::sampler_kernel<32, 32, true> : gaudi::sampler_kernel<32, 32>;
  if (hpe == 48 && hpp == 48) return vt ? gaudi::sampler_kernel<48, 48, true> : gaudi::sampler_kernel<48, 48>;
  if (hpe == 64 && hpp == 64) return vt ? gaudi::sampler_kernel<64, 64, true> : gaudi::sampler_kernel<64, 64>;
  return nullptr;
}
