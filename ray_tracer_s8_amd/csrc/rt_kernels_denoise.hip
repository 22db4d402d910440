// Device code of the a-trous denoiser (rt_denoise.hip.h): the entry, iteration and output kernels.  Its own translation unit: the
// tile, query, trace and feature-buffer kernels' code objects are untouched by it.
#define RT_DENOISE_KERNELS
#include "rt_denoise.hip.h"

namespace rtk {
DnFn dn_entry_kernel() { return rt_dn_entry_kernel; }
DnFn dn_step_kernel(bool lds, bool final_step) {
    if (lds) return final_step ? rt_dn_step_kernel<true, true> : rt_dn_step_kernel<true, false>;
    return final_step ? rt_dn_step_kernel<false, true> : rt_dn_step_kernel<false, false>;
}
DnFn dn_output_kernel() { return rt_dn_output_kernel; }
}  // namespace rtk
