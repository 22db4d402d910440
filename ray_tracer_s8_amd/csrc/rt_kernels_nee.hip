// Device code of the next-event-estimation integrator for caller rays (rt_nee.hip.h): path segments and shadow rays of one lane
// through one closest-hit site, over the query path's exact-node walk (engine 2) or its scan in primitive order (engine 1, plain or
// BVH semantics).  Its own translation unit: the tile, query, trace, path-step and direct-lighting kernels' code objects are untouched
// by it.
#include "rt_nee.hip.h"

namespace rtk {
template <int PICK, int SHAPE, int LOBE>
static NeeFn nee_kernel_of(int engine, int scan_mode) {
    if (engine == 2) return rt_nee_kernel<2, 2, PICK, SHAPE, LOBE>;
    if (engine == 1 && scan_mode == 0) return rt_nee_kernel<1, 0, PICK, SHAPE, LOBE>;
    if (engine == 1 && scan_mode == 2) return rt_nee_kernel<1, 2, PICK, SHAPE, LOBE>;
    return nullptr;
}
template <int LOBE>
static NeeFn nee_kernel_lobe(int engine, int scan_mode, bool by_power, bool cone) {
    if (cone) return by_power ? nee_kernel_of<PICK_POWER, SHAPE_CONE, LOBE>(engine, scan_mode) : nee_kernel_of<PICK_UNIFORM, SHAPE_CONE, LOBE>(engine, scan_mode);
    return by_power ? nee_kernel_of<PICK_POWER, SHAPE_AREA, LOBE>(engine, scan_mode) : nee_kernel_of<PICK_UNIFORM, SHAPE_AREA, LOBE>(engine, scan_mode);
}

// by_power: the instances of RT_FLAG_LIGHTS_BY_POWER; cone: those of RT_LIGHTS_CONE; lobe: those of RT_GLOSSY_MIS; the others are the
// code they were before the flag and the settings existed
NeeFn nee_kernel(int engine, int scan_mode, bool by_power, bool cone, bool lobe) {
    return lobe ? nee_kernel_lobe<1>(engine, scan_mode, by_power, cone) : nee_kernel_lobe<0>(engine, scan_mode, by_power, cone);
}
}  // namespace rtk

// the unit kernel of the light-sampling and scatter arithmetic as THIS unit compiles it (test library only;
// tests/test_gpu_sampling_operands.py)
#ifdef RT_DEBUG_HOOKS
#define RT_UNIT_ID 4
#include "rt_unit_sampling.hip.h"
#endif
