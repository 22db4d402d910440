// Device code of the BVH-traversal engines (ISECT 2: exact 64-byte nodes, 3: quantised 32-byte nodes, 4: the same
// with a capped LDS stack, 5: the exact tree resident in LDS, 6: the same walked nearer child first with distance culling,
// 7: quantised nodes walked nearer child first with distance culling, 8: the same with a capped LDS stack, 9: the exact nodes
// walked nearer child first with distance culling).  Its own
// translation unit: compiled with -fno-slp-vectorize (build.py) — packed FP32 pairs made by the SLP vectoriser in the
// ray-generation / shading code cost these kernels 1.5 % (register pairs, v_pk_mov), while the linear kernels gain 3 %.
#include "rt_kernel.hip.h"

namespace rtk {
template <bool STATS>
KernelFn traverse_kernel(int isect, bool tris) {           // (the order of the cases is the kernels' order in the code object)
    switch (isect) {
        case 5: return tris ? rt_tile_kernel<5, false, LTREE_BLOCK, STATS, true> : rt_tile_kernel<5, false, LTREE_BLOCK, STATS, false>;
        case 6: return tris ? rt_tile_kernel<6, false, LTREE_BLOCK, STATS, true> : rt_tile_kernel<6, false, LTREE_BLOCK, STATS, false>;
        case 7: return rt_tile_kernel<7, false, BLOCK, STATS>;
        case 8: return rt_tile_kernel<8, false, BLOCK, STATS>;
        case 9: return rt_tile_kernel<9, false, BLOCK, STATS>;
        case 3: return rt_tile_kernel<3, false, BLOCK, STATS>;
        case 2: return rt_tile_kernel<2, false, BLOCK, STATS>;
        case 4: return rt_tile_kernel<4, false, BLOCK, STATS>;
        default: return nullptr;
    }
}
KernelFn kernel_traverse(int isect, bool stats, bool tris) { return stats ? traverse_kernel<true>(isect, tris) : traverse_kernel<false>(isect, tris); }

// Self-test of sqrt_rn as the traversal kernels use it (tests/test_gpu_parity.py, rt_debug_sqrt_selftest): every f32 bit pattern in
// [from, from + n) through sqrt_rn and through the compiler's IEEE sequence; counts the patterns whose results differ in any bit
// (NaN results count as equal when both are NaN: their payloads are never stored).
__global__ void sqrt_selftest_kernel(uint32_t from, unsigned long long n, unsigned long long* bad) {
    unsigned long long mine = 0;
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
        float x = __uint_as_float(from + (uint32_t)i);
        asm volatile("" : "+v"(x));
        const float ref = __builtin_sqrtf(x);
        const float a = sqrt_rn(x), b = sqrt_rn<true>(x);
        const bool both_nan_a = (a != a) && (ref != ref), both_nan_b = (b != b) && (ref != ref);
        if (__float_as_uint(a) != __float_as_uint(ref) && !both_nan_a) mine++;
        if (__float_as_uint(b) != __float_as_uint(ref) && !both_nan_b) mine++;
    }
    if (mine) atomicAdd(bad, mine);
}
void sqrt_selftest_launch(uint32_t from, unsigned long long n, unsigned long long* d_bad, hipStream_t st) {
    hipLaunchKernelGGL(sqrt_selftest_kernel, dim3(4096), dim3(256), 0, st, from, n, d_bad);
}
}  // namespace rtk

// the unit kernel of the closest-hit arithmetic as THIS unit compiles it (test library only; tests/test_gpu_operands.py)
#ifdef RT_DEBUG_HOOKS
#define RT_UNIT_ID 1
#include "rt_unit.hip.h"
#endif
