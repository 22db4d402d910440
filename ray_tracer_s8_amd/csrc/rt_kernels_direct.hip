// Device code of the direct lighting of caller rays (rt_direct.hip.h): one light sample per active hit record, its shadow ray over the
// query path's exact-node walk (engine 2) or its scan in primitive order (engine 1, plain or BVH semantics).  Its own translation
// unit: the tile, query, trace and path-step kernels' code objects are untouched by it.
#include "rt_direct.hip.h"

namespace rtk {
template <int PICK>
static DirectFn direct_kernel_of(int engine, int scan_mode) {
    if (engine == 2) return rt_direct_kernel<2, 2, PICK>;
    if (engine == 1 && scan_mode == 0) return rt_direct_kernel<1, 0, PICK>;
    if (engine == 1 && scan_mode == 2) return rt_direct_kernel<1, 2, PICK>;
    return nullptr;
}

// by_power: the instances of RT_FLAG_LIGHTS_BY_POWER; the others are the code they were before the flag existed
DirectFn direct_kernel(int engine, int scan_mode, bool by_power) {
    return by_power ? direct_kernel_of<PICK_POWER>(engine, scan_mode) : direct_kernel_of<PICK_UNIFORM>(engine, scan_mode);
}
}  // namespace rtk
