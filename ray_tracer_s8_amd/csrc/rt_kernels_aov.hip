// Device code of the feature buffers of a strip (rt_aov.hip.h): the tile's camera rays, their first hits over the query path's
// exact-node walk (engine 2) or its scan in primitive order (engine 1, plain or BVH semantics).  Its own translation unit: the tile,
// query and trace kernels' code objects are untouched by it.
#include "rt_aov.hip.h"

namespace rtk {
AovFn aov_kernel(int engine, int scan_mode) {
    if (engine == 2) return rt_aov_kernel<2, 2>;
    if (engine == 1 && scan_mode == 0) return rt_aov_kernel<1, 0>;
    if (engine == 1 && scan_mode == 2) return rt_aov_kernel<1, 2>;
    return nullptr;
}
}  // namespace rtk
