// Device code of path tracing of caller rays (rt_trace.hip.h): ray_color over the query path's exact-node walk (engine 2) or its scan in
// primitive order (engine 1, plain or BVH semantics).  Its own translation unit: the tile and query kernels' code objects are untouched
// by it.
#include "rt_trace.hip.h"

namespace rtk {
TraceFn trace_kernel(int engine, int scan_mode) {
    if (engine == 2) return rt_trace_kernel<2, 2>;
    if (engine == 1 && scan_mode == 0) return rt_trace_kernel<1, 0>;
    if (engine == 1 && scan_mode == 2) return rt_trace_kernel<1, 2>;
    return nullptr;
}
}  // namespace rtk

// the unit kernel of the light-sampling and scatter arithmetic as THIS unit compiles it (test library only;
// tests/test_gpu_sampling_operands.py)
#ifdef RT_DEBUG_HOOKS
#define RT_UNIT_ID 6
#include "rt_unit_sampling.hip.h"
#endif
