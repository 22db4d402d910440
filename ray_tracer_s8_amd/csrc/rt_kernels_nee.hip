// Device code of the next-event-estimation integrator for caller rays (rt_nee.hip.h): path segments and shadow rays of one lane
// through one closest-hit site, over the query path's exact-node walk (engine 2) or its scan in primitive order (engine 1, plain or
// BVH semantics).  Its own translation unit: the tile, query, trace, path-step and direct-lighting kernels' code objects are untouched
// by it.
#include "rt_nee.hip.h"

namespace rtk {
template <int PICK>
static NeeFn nee_kernel_of(int engine, int scan_mode) {
    if (engine == 2) return rt_nee_kernel<2, 2, PICK>;
    if (engine == 1 && scan_mode == 0) return rt_nee_kernel<1, 0, PICK>;
    if (engine == 1 && scan_mode == 2) return rt_nee_kernel<1, 2, PICK>;
    return nullptr;
}

// by_power: the instances of RT_FLAG_LIGHTS_BY_POWER; the others are the code they were before the flag existed
NeeFn nee_kernel(int engine, int scan_mode, bool by_power) {
    return by_power ? nee_kernel_of<PICK_POWER>(engine, scan_mode) : nee_kernel_of<PICK_UNIFORM>(engine, scan_mode);
}
}  // namespace rtk
