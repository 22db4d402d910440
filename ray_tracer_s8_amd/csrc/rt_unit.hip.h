// Device unit kernel of the closest-hit arithmetic (test library only: every includer wraps this file in #ifdef RT_DEBUG_HOOKS).
// One lane per record calls ONE device function of rt_kernel.hip.h on the record's operands and stores what it returns, so that
// tests/test_gpu_operands.py can hold exact_sphere, exact_triangle, the two slab tests, the normalisations, f32_as_u8 and the RNG to
// the oracle operand by operand.  The functions are __forceinline__, and the translation units differ in flags (build.py UNITS) and in
// the square root they choose (RT_IEEE_SQRT_PLAIN), so each unit that wants checking instantiates the kernel for itself:
//     #define RT_UNIT_ID <n>      (0 lin, 1 trav, 2 query: rt_debug_unit's `unit` argument)
//     #include "rt_unit.hip.h"
// (rt_api.hip includes it without RT_UNIT_ID: the record sizes and the launchers' declarations only, and the sibling header.)
// Records are 32-bit words, plain loads and stores.  Words in / out per family (tests/_operand_cases.py holds the same table):
//   0 SPHERE       in 12: o d cen r t_min t_max                 out 2: hit, t              exact_sphere(o, 2*d, cen, r*r, ...)
//   1 SPHERE_NORM  in 12: the same                              out 5: hit, t, normalize(d)           the same after Ray::new
//   2 TRIANGLE     in 17: o d A B C t_min t_max                 out 2: hit, t              exact_triangle
//   3 AABB         in 12: o d lo hi                             out 3: intersects_aabb, intersects_aabb_finite, RayAux::finite
//   4 CHAIN        in 18: o d leaf lo hi outer lo hi            out 3: intersects_aabb(leaf), intersects_aabb(outer), finite
//   5 NORMALIZE    in  3: v                                     out 7: normalize(v), try_normalize's boolean, normalize_or_zero(v)
//   6 AS_U8        in  1: v                                     out 1: the byte
//   7 RNG          in  2: st (low word, high word)              out 28: seed_state's 4 words (low, high each), 4 next_u32, 4 u01,
//                                                                       4 uniform_m1_1 (drawn in that order), the final 4 words
// t is stored as the function leaves it (zero-initialised before the call): it means something only where hit is set.
// Families 8 .. 16 (units 3 .. 6), the light-sampling and scatter arithmetic, are rt_unit_sampling.hip.h's.
#pragma once
#include "rt_kernel.hip.h"

namespace rtk {
constexpr int UNIT_FAMILIES = 8;
constexpr int UNIT_RNG_DRAWS = 4;
__host__ __device__ constexpr int unit_words_in(int family) {
    return family == 0 || family == 1 ? 12 : family == 2 ? 17 : family == 3 ? 12 : family == 4 ? 18 : family == 5 ? 3 : family == 6 ? 1 : 2;
}
__host__ __device__ constexpr int unit_words_out(int family) {
    return family == 0 ? 2 : family == 1 ? 5 : family == 2 ? 2 : family == 3 ? 3 : family == 4 ? 3 : family == 5 ? 7 : family == 6 ? 1 : 28;
}

// one launch over n records on stream st; d_in / d_out hold n * unit_words_in / _out(family) words
void unit_launch_lin(int family, unsigned long long n, const uint32_t* d_in, uint32_t* d_out, hipStream_t st);      // rt_kernels_lin.hip
void unit_launch_trav(int family, unsigned long long n, const uint32_t* d_in, uint32_t* d_out, hipStream_t st);     // rt_kernels_trav.hip
void unit_launch_query(int family, unsigned long long n, const uint32_t* d_in, uint32_t* d_out, hipStream_t st);    // rt_kernels_query.hip

#ifdef RT_UNIT_ID
template <int UNIT>
__global__ void __launch_bounds__(256) rt_unit_kernel(int family, unsigned long long n, const uint32_t* __restrict__ in,
                                                      uint32_t* __restrict__ out) {
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= n) return;
    const uint32_t* r = in + i * (unsigned long long)unit_words_in(family);
    uint32_t* w = out + i * (unsigned long long)unit_words_out(family);
    auto F = [&](int k) { return __uint_as_float(r[k]); };
    auto V = [&](int k) { return mk(F(k), F(k + 1), F(k + 2)); };
    auto put3 = [&](int k, V3 v) {
        w[k] = __float_as_uint(v.x);
        w[k + 1] = __float_as_uint(v.y);
        w[k + 2] = __float_as_uint(v.z);
    };
    switch (family) {
        case 0:
        case 1: {
            const V3 o = V(0), cen = V(6);
            V3 d = V(3);
            if (family == 1) d = normalize(d);                       // Ray::new (ray.rs:133-143)
            const float rad = F(9);
            const float rr = rad * rad;
            float t = 0.0f;
            const bool hit = exact_sphere(o, 2.0f * d, cen, rr, F(10), F(11), t);
            w[0] = hit ? 1u : 0u;
            w[1] = __float_as_uint(t);
            if (family == 1) put3(2, d);
            break;
        }
        case 2: {
            float tv[9];
            for (int k = 0; k < 9; k++) tv[k] = F(6 + k);
            float t = 0.0f;
            const bool hit = exact_triangle(V(0), V(3), tv, F(15), F(16), t);
            w[0] = hit ? 1u : 0u;
            w[1] = __float_as_uint(t);
            break;
        }
        case 3: {
            const V3 o = V(0);
            const RayAux a = ray_aux(V(3), false);
            const float4 lo = make_float4(F(6), F(7), F(8), 0.f), hi = make_float4(F(9), F(10), F(11), 0.f);
            w[0] = intersects_aabb(o, a, lo, hi) ? 1u : 0u;
            w[1] = intersects_aabb_finite(o, a, lo, hi) ? 1u : 0u;
            w[2] = a.finite ? 1u : 0u;
            break;
        }
        case 4: {
            const V3 o = V(0);
            const RayAux a = ray_aux(V(3), false);
            w[0] = intersects_aabb(o, a, make_float4(F(6), F(7), F(8), 0.f), make_float4(F(9), F(10), F(11), 0.f)) ? 1u : 0u;
            w[1] = intersects_aabb(o, a, make_float4(F(12), F(13), F(14), 0.f), make_float4(F(15), F(16), F(17), 0.f)) ? 1u : 0u;
            w[2] = a.finite ? 1u : 0u;
            break;
        }
        case 5: {
            const V3 v = V(0);
            V3 tn = mk(0.f, 0.f, 0.f);
            put3(0, normalize(v));
            w[3] = try_normalize(v, tn) ? 1u : 0u;
            put3(4, normalize_or_zero(v));
            break;
        }
        case 6:
            w[0] = f32_as_u8(F(0));
            break;
        case 7: {
            Rng g = seed_state((uint64_t)r[0] | ((uint64_t)r[1] << 32));
            auto put_state = [&](int k) {
                const uint64_t s[4] = {g.s0, g.s1, g.s2, g.s3};
                for (int j = 0; j < 4; j++) {
                    w[k + 2 * j] = (uint32_t)s[j];
                    w[k + 2 * j + 1] = (uint32_t)(s[j] >> 32);
                }
            };
            put_state(0);
            for (int j = 0; j < UNIT_RNG_DRAWS; j++) w[8 + j] = next_u32(g);
            for (int j = 0; j < UNIT_RNG_DRAWS; j++) w[12 + j] = __float_as_uint(u01(g));
            for (int j = 0; j < UNIT_RNG_DRAWS; j++) w[16 + j] = __float_as_uint(uniform_m1_1(g));
            put_state(20);
            break;
        }
        default:
            break;
    }
}

#if RT_UNIT_ID == 0
void unit_launch_lin
#elif RT_UNIT_ID == 1
void unit_launch_trav
#else
void unit_launch_query
#endif
    (int family, unsigned long long n, const uint32_t* d_in, uint32_t* d_out, hipStream_t st) {
    hipLaunchKernelGGL(rt_unit_kernel<RT_UNIT_ID>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, family, n, d_in, d_out);
}
#endif  // RT_UNIT_ID
}  // namespace rtk

// rt_api.hip (no RT_UNIT_ID) takes both unit headers through this one: the sibling's record sizes and launchers, and what
// rt_debug_unit asks of the two together.
#ifndef RT_UNIT_ID
#include "rt_unit_sampling.hip.h"
namespace rtk {
// units 0 .. 2 carry families 0 .. 7, units 3 .. 6 the families unit_carries names
inline bool unit_instantiated(int unit, int family) {
    return (unit >= 0 && unit <= 2 && family >= 0 && family < UNIT_FAMILIES) ||
           (family >= UNIT_SAMPLING_FIRST && family < UNIT_SAMPLING_END && unit_carries(unit, family));
}
inline int unit_record_in(int family) { return family < UNIT_FAMILIES ? unit_words_in(family) : sampling_words_in(family); }
inline int unit_record_out(int family) { return family < UNIT_FAMILIES ? unit_words_out(family) : sampling_words_out(family); }
inline void unit_launch(int unit, int family, unsigned long long n, const uint32_t* d_in, uint32_t* d_out, hipStream_t st) {
    (unit == 0 ? unit_launch_lin : unit == 1 ? unit_launch_trav : unit == 2 ? unit_launch_query : unit == 3 ? unit_launch_direct :
     unit == 4 ? unit_launch_nee : unit == 5 ? unit_launch_bounce : unit_launch_trace)(family, n, d_in, d_out, st);
}
}  // namespace rtk
#endif
