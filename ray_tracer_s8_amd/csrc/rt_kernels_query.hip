// Device code of the ray-query engines (rt_query.hip.h): the exact-node walk (engine 2) and the scan in primitive order (engine 1,
// plain or BVH semantics), each in a closest-hit and an any-hit form.  Its own translation unit: the tile kernels' code objects are
// untouched by it.
#include "rt_query.hip.h"

namespace rtk {
QueryFn query_kernel(int engine, int scan_mode, bool any) {
    if (engine == 2) return any ? rt_query_kernel<2, 2, true> : rt_query_kernel<2, 2, false>;
    if (engine == 1 && scan_mode == 0) return any ? rt_query_kernel<1, 0, true> : rt_query_kernel<1, 0, false>;
    if (engine == 1 && scan_mode == 2) return any ? rt_query_kernel<1, 2, true> : rt_query_kernel<1, 2, false>;
    return nullptr;
}
}  // namespace rtk

// the unit kernel of the closest-hit arithmetic as THIS unit compiles it (test library only; tests/test_gpu_operands.py)
#ifdef RT_DEBUG_HOOKS
#define RT_UNIT_ID 2
#include "rt_unit.hip.h"
#endif
