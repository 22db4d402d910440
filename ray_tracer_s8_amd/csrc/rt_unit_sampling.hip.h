// Device unit kernel of the light-sampling and scatter arithmetic (test library only: every includer wraps this file in
// #ifdef RT_DEBUG_HOOKS).  The sibling of rt_unit.hip.h for everything that samples a light or scatters a ray: one lane per record
// calls the functions of rt_direct_math.h, rt_nee_math.h and the device-only shade lines of rt_path_steps.hip.h on the record's
// operands and stores what they return, so that tests/test_gpu_sampling_operands.py can hold them to the numpy restatements
// (tests/_sampling_cases.py) operand by operand; family 16 calls rt_lobe_math.h for tests/test_gpu_lobe_operands.py
// (tests/_lobe_cases.py).  The translation units whose product kernels inline these lines instantiate the
// kernel for themselves, with the families their kernels use:
//     #define RT_UNIT_ID <n>      (3 direct, 4 nee, 5 bounce, 6 trace: rt_debug_unit's `unit` argument)
//     #include "rt_unit_sampling.hip.h"
// (rt_api.hip takes it through rt_unit.hip.h, without RT_UNIT_ID: the record sizes, unit_carries and the launchers' declarations only.)
// Records are 32-bit words, plain loads and stores; the output is zero-filled before the launch, and a word a family does not write
// stays 0.  The layouts of families 8, 9, 11, 12 and 13 are those of the g++ harnesses under tests/host/ (named below), so one corpus
// feeds g++, numpy and the device.  Words in / out per family (tests/_sampling_cases.py holds the same table), and the units that carry it:
//    8 DIRECT      in 28: direct_host.cpp direct_math               out 16: k, L, d2, cs, cl, facing, W, rgb, w, area      3 4
//                         pick_light, sphere_point | fold_pair, triangle_point, triangle_area; light_geometry, sphere_weight |
//                         triangle_weight, radiance
//    9 WEIGHT_IP   in  6: lightpick_host.cpp lightpick_weights      out  2: sphere_weight_ip | triangle_weight_ip, and         3 4
//                                                                           rtnee::view_weight_ip of the same view
//   10 PICK_POWER  in 20: u, M (1 .. 16), total, M_big (1 .. 2^23), out  2: pick_light_power(u, M, c, total),                  3 4
//                         c[16] (the running sums, read in the record)      pick_light(u, M_big); an M outside 1 .. 16 or an
//                                                                           M_big outside 1 .. 2^23 writes nothing
//   11 CONE        in 16: cone_host.cpp cone_samples                out 20: q, in the regime, and in the regime only v, omc,    3 4
//                                                                           dc2, dc, ct, st, wn, cs, facing, W, L, v.v
//   12 CONE_VIEW   in 14: cone_host.cpp cone_views                  out  5: cs', omc', in_regime, samplable, W'                  4
//   13 NEE_VIEW    in 14: nee_host.cpp nee_view, then [13] a W      out  8: cs', cl', d2', samplable, W', bounce_weight(W'),     4
//                                                                           light_weight(W), bounce_weight(W)
//   14 SCATTER     in 10: d, n, roughness, x1, x2, sm               out  7: unit_sphere_vec, scattered_dir, try_normalize fell  5 6
//                                                                           back to n
//   15 SKY         in  3: d                                         out  3: sky_colour                                        5 6
//   16 LOBE        in 16: lobe_host.cpp lobe_records: n, d, rho,    out 20: sampled_class, g, gn, c, r, kappa, b, D, in the      4
//                         w, W, us, unused                                  lobe, cg, lobe_sample_taken(W); lobe_factor_scatter(us):
//                                                                           m, t, cg, in the lobe; 0
#pragma once
#include "rt_lobe_math.h"
#include "rt_nee_math.h"
#include "rt_path_steps.hip.h"

namespace rtk {
constexpr int UNIT_SAMPLING_FIRST = 8, UNIT_SAMPLING_END = 17;     // families [FIRST, END)
constexpr int UNIT_PICK_TABLE = 16;                                // running sums a PICK_POWER record holds
__host__ __device__ constexpr int sampling_words_in(int family) {
    return family == 8 ? 28 : family == 9 ? 6 : family == 10 ? 4 + UNIT_PICK_TABLE : family == 11 ? 16 : family == 12 ? 14 :
           family == 13 ? 14 : family == 14 ? 10 : family == 16 ? 16 : 3;
}
__host__ __device__ constexpr int sampling_words_out(int family) {
    return family == 8 ? 16 : family == 9 ? 2 : family == 10 ? 2 : family == 11 ? 20 : family == 12 ? 5 : family == 13 ? 8 :
           family == 14 ? 7 : family == 16 ? 20 : 3;
}
// the (unit, family) pairs that are instantiated: rt_debug_unit refuses every other pair before any device work
__host__ __device__ constexpr bool unit_carries(int unit, int family) {
    return unit == 3 ? family >= 8 && family <= 11 : unit == 4 ? (family >= 8 && family <= 13) || family == 16 :
           unit == 5 || unit == 6 ? family == 14 || family == 15 : false;
}

// one launch over n records on stream st; d_in / d_out hold n * sampling_words_in / _out(family) words
void unit_launch_direct(int family, unsigned long long n, const uint32_t* d_in, uint32_t* d_out, hipStream_t st);   // rt_kernels_direct.hip
void unit_launch_nee(int family, unsigned long long n, const uint32_t* d_in, uint32_t* d_out, hipStream_t st);      // rt_kernels_nee.hip
void unit_launch_bounce(int family, unsigned long long n, const uint32_t* d_in, uint32_t* d_out, hipStream_t st);   // rt_kernels_bounce.hip
void unit_launch_trace(int family, unsigned long long n, const uint32_t* d_in, uint32_t* d_out, hipStream_t st);    // rt_kernels_trace.hip

#ifdef RT_UNIT_ID
template <int UNIT>
__global__ void __launch_bounds__(256) rt_unit_sampling_kernel(int family, unsigned long long n, const uint32_t* __restrict__ in,
                                                               uint32_t* __restrict__ out) {
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= n || !unit_carries(UNIT, family)) return;
    const uint32_t* r = in + i * (unsigned long long)sampling_words_in(family);
    uint32_t* w = out + i * (unsigned long long)sampling_words_out(family);
    auto F = [&](int k) { return __uint_as_float(r[k]); };
    auto V = [&](int k) { return rtdl::Vec{F(k), F(k + 1), F(k + 2)}; };
    auto put = [&](int k, float v) { w[k] = __float_as_uint(v); };
    auto put3 = [&](int k, rtdl::Vec v) {
        w[k] = __float_as_uint(v.x);
        w[k + 1] = __float_as_uint(v.y);
        w[k + 2] = __float_as_uint(v.z);
    };
    if constexpr (unit_carries(UNIT, 8)) {
        if (family == 8) {
            const bool sphere = r[0] == 0;
            const uint32_t M = r[1];
            w[0] = rtdl::pick_light(F(2), M);
            rtdl::Vec L, nl;
            float size, area = 0.0f;
            if (sphere) {
                nl = V(13);
                size = F(12);
                L = rtdl::sphere_point(V(9), size, nl);
            } else {
                float u1 = F(18), u2 = F(19);
                rtdl::fold_pair(u1, u2);
                L = rtdl::triangle_point(V(9), V(12), V(15), u1, u2);
                nl = V(20);
                size = area = rtdl::triangle_area(V(9), V(12), V(15));
            }
            const rtdl::Geometry g = rtdl::light_geometry(V(3), V(6), L, nl, sphere);
            const float W = sphere ? rtdl::sphere_weight(g.cs, g.cl, size, M, g.d2) : rtdl::triangle_weight(g.cs, g.cl, size, M, g.d2);
            put3(1, L);
            put(4, g.d2), put(5, g.cs), put(6, g.cl);
            w[7] = g.facing ? 1u : 0u;
            put(8, W);
            put3(9, rtdl::radiance(V(23), F(26), W));
            put3(12, g.w);
            put(15, area);
        } else if (family == 9) {
            const bool sphere = r[0] == 0;
            const float cs = F(1), cl = F(2), size = F(3), ip = F(4), d2 = F(5);
            put(0, sphere ? rtdl::sphere_weight_ip(cs, cl, size, ip, d2) : rtdl::triangle_weight_ip(cs, cl, size, ip, d2));
            rtnee::View v;
            v.cs = cs, v.cl = cl, v.d2 = d2, v.samplable = true;
            put(1, rtnee::view_weight_ip(v, sphere, size, ip));
        } else if (family == 10) {
            const uint32_t M = r[1], M_big = r[3];
            if (M >= 1u && M <= (uint32_t)UNIT_PICK_TABLE && M_big >= 1u && M_big <= rtdl::MAX_LIGHTS) {
                w[0] = rtdl::pick_light_power(F(0), M, reinterpret_cast<const float*>(r + 4), F(2));
                w[1] = rtdl::pick_light(F(0), M_big);
            }
        } else if (family == 11) {
            const rtdl::Vec P = V(0), c = V(3);
            const float rad = F(6);
            const rtdl::ConeAxis ax = rtdl::cone_axis(P, c, rad);
            put(0, ax.q);
            if (rtdl::cone_regime(ax.q)) {
                w[1] = 1u;
                const rtdl::Cone k = rtdl::cone_sample(P, c, rad, F(7), F(8), F(9));
                const rtdl::Geometry g = rtdl::cone_geometry(V(10), k.v);
                put3(2, k.v);
                put(5, k.omc), put(6, k.dc2), put(7, k.dc), put(8, k.ct), put(9, k.st);
                put3(10, g.w);
                put(13, g.cs);
                w[14] = g.facing ? 1u : 0u;
                put(15, rtdl::cone_weight(g.cs, k.omc, F(13)));
                put3(16, rtdl::cone_point(P, g.w, rad, k));
                put(19, g.d2);
            }
        }
    }
    if constexpr (unit_carries(UNIT, 12)) {
        if (family == 12) {
            const rtnee::ConeView v = rtnee::emitter_view_cone(V(0), V(3), V(6), V(9), F(12));
            put(0, v.cs), put(1, v.omc);
            w[2] = v.in_regime ? 1u : 0u;
            w[3] = v.samplable ? 1u : 0u;
            put(4, rtnee::cone_view_weight(v, F(13)));
        } else if (family == 13) {
            const bool sphere = r[0] == 0;
            const rtnee::View v = rtnee::emitter_view(V(2), V(5), V(8), F(11), sphere);
            const float W = rtnee::view_weight(v, sphere, F(12), r[1]);
            put(0, v.cs), put(1, v.cl), put(2, v.d2);
            w[3] = v.samplable ? 1u : 0u;
            put(4, W);
            put(5, rtnee::bounce_weight(W));
            put(6, rtnee::light_weight(F(13)));
            put(7, rtnee::bounce_weight(F(13)));
        }
    }
    if constexpr (unit_carries(UNIT, 16)) {
        if (family == 16) {
            const rtdl::Vec nrm = V(0), g = rtlobe::glossy_dir(V(3), nrm);
            const float rho = F(6), gn = rtdl::dot3(nrm, g);
            const rtlobe::Lobe l = rtlobe::lobe_of(nrm, g, rho);
            const rtlobe::LobeFactor f = rtlobe::lobe_factor(l, V(7));
            w[0] = rtlobe::sampled_class(rho, gn);
            put3(1, g);
            put(4, gn);
            put3(5, l.c);
            put(8, l.r), put(9, l.kappa), put(10, f.b), put(11, f.D);
            w[12] = f.in_lobe ? 1u : 0u;
            put(13, f.cg);
            w[14] = rtlobe::lobe_sample_taken(f, F(10)) ? 1u : 0u;
            const rtlobe::ScatterFactor s = rtlobe::lobe_factor_scatter(l, V(11));
            put(15, s.m), put(16, s.t), put(17, s.cg);
            w[18] = s.in_lobe ? 1u : 0u;
        }
    }
    if constexpr (unit_carries(UNIT, 14)) {
        if (family == 14) {
            const V3 d = mk(F(0), F(1), F(2)), nrm = mk(F(3), F(4), F(5));
            const float rough = F(6), x1 = F(7), x2 = F(8), sm = F(9);
            const V3 us = unit_sphere_vec(x1, x2, sm);
            put3(0, dvec(us));
            put3(3, dvec(scattered_dir(d, nrm, rough, x1, x2, sm)));
            // The flag is scattered_dir's try_normalize on scattered_dir's own operand `pre`, which the function does not return:
            // the three lines below are a copy of its first three (rt_path_steps.hip.h) and change with them.  A copy that drifts
            // shows: the flag is held to the restatement, whose direction (words 3 .. 5) is the product's own.
            const V3 diffuse_dir = us + nrm;
            const V3 glossy_dir = d - (2.0f * dot(d, nrm)) * nrm;
            V3 xdir;
            w[6] = try_normalize(diffuse_dir + rough * (glossy_dir - diffuse_dir), xdir) ? 0u : 1u;
        } else if (family == 15) {
            put3(0, dvec(sky_colour(mk(F(0), F(1), F(2)))));
        }
    }
}

#if RT_UNIT_ID == 3
void unit_launch_direct
#elif RT_UNIT_ID == 4
void unit_launch_nee
#elif RT_UNIT_ID == 5
void unit_launch_bounce
#else
void unit_launch_trace
#endif
    (int family, unsigned long long n, const uint32_t* d_in, uint32_t* d_out, hipStream_t st) {
    hipLaunchKernelGGL(rt_unit_sampling_kernel<RT_UNIT_ID>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, family, n, d_in, d_out);
}
#endif  // RT_UNIT_ID
}  // namespace rtk
