/* nee_trace.c — the next-event-estimation integrator through the C-ABI alone: the scene and the camera of nee_rays.c (a diffuse sphere
 * on a diffuse floor triangle under a small light, a 32 x 32 pinhole at (0, 1, 2)) through rt_scene_trace_nee in both modes and
 * through rt_scene_trace, max_bounces = 3 each, one launch per estimator and pass.  What nee_rays.c composes from K host-form steps
 * and K - 1 light-sample calls per pass is ONE call here, and RT_NEE_MIS adds what that recipe cannot: the balance heuristic between
 * the light sample and the bounce.  S passes with fresh RNG states give N * S samples of each.  Build from the repository root (after
 * `python -m ray_tracer_s8_amd.build`):
 *
 *     gcc -std=c99 -O2 -Iinclude examples/nee_trace.c -Lray_tracer_s8_amd/lib -lrt_s8 \
 *         -Wl,-rpath,ray_tracer_s8_amd/lib -Wl,-rpath-link,/opt/rocm/lib -lm -o nee_trace && ./nee_trace
 *
 * Prints the mean and the variance of the samples' luminance for the three estimators and NEE_TRACE_OK when the means of both modes
 * agree with rt_scene_trace's within five standard errors; exits 2 when rt_init finds no HIP device. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "rt_tile.h"

#define W 32
#define H 32
#define N (W * H)
#define S 16
#define BOUNCES 3

static float luminance(const float* c) { return (c[0] + c[1] + c[2]) / 3.0f; }

/* SplitMix64: well-mixed xoshiro256++ states from a counter */
static uint64_t splitmix(uint64_t* x) {
    uint64_t z = (*x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main(void) {
    int n_dev = 0;
    int rc = rt_init(&n_dev);
    if (rc != RT_OK) {
        fprintf(stderr, "rt_init: %s (%s): no HIP device\n", rt_strerror(rc), rt_last_error());
        return 2;
    }
    rt_sphere sph[2];
    memset(sph, 0, sizeof sph);
    sph[0].cz = -3.0f; sph[0].radius = 1.0f; sph[0].albedo_r = 0.8f; sph[0].albedo_g = 0.3f; sph[0].albedo_b = 0.3f;
    sph[1].cx = 1.0f; sph[1].cy = 3.0f; sph[1].cz = -2.0f; sph[1].radius = 0.3f;
    sph[1].albedo_r = sph[1].albedo_g = sph[1].albedo_b = 1.0f; sph[1].emission = 20.0f;
    rt_triangle tri;
    memset(&tri, 0, sizeof tri);
    const float a[3] = {-10.f, -1.f, 0.f}, b[3] = {10.f, -1.f, 0.f}, c[3] = {0.f, -1.f, -20.f};
    memcpy(tri.a, a, sizeof a); memcpy(tri.b, b, sizeof b); memcpy(tri.c, c, sizeof c);
    tri.albedo_r = tri.albedo_g = tri.albedo_b = 0.5f;
    rt_scene* scene = NULL;
    if ((rc = rt_scene_create(0, sph, 2, &tri, 1, NULL, &scene)) != RT_OK) {
        fprintf(stderr, "rt_scene_create: %s (%s)\n", rt_strerror(rc), rt_last_error());
        return 1;
    }
    /* a pinhole at (0, 1, 2) aimed at the sphere's centre: forward f, right r, up u; 60 degrees across */
    const float eye[3] = {0.f, 1.f, 2.f}, at[3] = {0.f, 0.f, -3.f};
    float f[3] = {at[0] - eye[0], at[1] - eye[1], at[2] - eye[2]};
    float fl = sqrtf(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    for (int k = 0; k < 3; k++) f[k] /= fl;
    float r[3] = {-f[2], 0.f, f[0]};                                   /* f x (0, 1, 0) */
    float rl = sqrtf(r[0] * r[0] + r[2] * r[2]);
    r[0] /= rl; r[2] /= rl;
    const float u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};
    const float half = tanf(0.5235988f);
    static rt_ray rays[N];
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const float sx = ((x + 0.5f) / W * 2.f - 1.f) * half, sy = (1.f - (y + 0.5f) / H * 2.f) * half;
            rt_ray* ry = &rays[y * W + x];
            ry->ox = eye[0]; ry->oy = eye[1]; ry->oz = eye[2];
            ry->dx = f[0] + sx * r[0] + sy * u[0];
            ry->dy = f[1] + sx * r[1] + sy * u[1];
            ry->dz = f[2] + sx * r[2] + sy * u[2];
            ry->t_min = 0.001f; ry->t_max = 1000.f;
        }
    static uint64_t state[4 * N];
    static float col[3 * N];
    static uint32_t segs[N], shadow[N];
    rt_nee_request nq;
    memset(&nq, 0, sizeof nq);
    nq.spp = 1; nq.max_bounces = BOUNCES; nq.ray_form = RT_TRACE_RAY_NEW;
    rt_trace_request tq;
    memset(&tq, 0, sizeof tq);
    tq.spp = 1; tq.max_bounces = BOUNCES; tq.ray_form = RT_TRACE_RAY_NEW;
    /* estimator 0: RT_NEE_LIGHT_ONLY, 1: RT_NEE_MIS, 2: rt_scene_trace */
    static const char* const names[3] = {"nee, light only", "nee, MIS       ", "rt_scene_trace "};
    double sum[3] = {0, 0, 0}, sq[3] = {0, 0, 0};
    uint64_t shadow_rays = 0, seed = 2024;
    int ok = 1;
    for (int s = 0; s < S && ok; s++)
        for (int e = 0; e < 3; e++) {
            for (int i = 0; i < 4 * N; i++) state[i] = splitmix(&seed);
            rt_tile_stats st;
            if (e < 2) {
                nq.mode = e == 0 ? RT_NEE_LIGHT_ONLY : RT_NEE_MIS;
                rc = rt_scene_trace_nee(scene, &nq, rays, N, state, col, segs, shadow, &st);
                uint64_t n_seg = 0, n_sh = 0;
                for (int i = 0; i < N; i++) { n_seg += segs[i]; n_sh += shadow[i]; }
                shadow_rays += n_sh;
                ok = ok && st.n_launches == 1 && st.primary_rays == N && st.ray_segments == n_seg + n_sh;
            } else {
                rc = rt_scene_trace(scene, &tq, rays, N, state, col, NULL, &st);
            }
            if (rc != RT_OK) {
                fprintf(stderr, "%s: %s (%s)\n", names[e], rt_strerror(rc), rt_last_error());
                return 1;
            }
            for (int i = 0; i < N; i++) {
                const double x = luminance(col + 3 * i);
                sum[e] += x; sq[e] += x * x;
            }
        }
    const double n = (double)N * S;
    double mean[3], var[3];
    for (int e = 0; e < 3; e++) {
        mean[e] = sum[e] / n;
        var[e] = (sq[e] - n * mean[e] * mean[e]) / (n - 1);
    }
    printf("samples %d of each; shadow rays %llu\n", N * S, (unsigned long long)shadow_rays);
    for (int e = 0; e < 3; e++) printf("%s: mean %.5f variance %.5f (variance of rt_scene_trace / this: %.1f)\n", names[e], mean[e], var[e], var[2] / var[e]);
    for (int e = 0; e < 2; e++) ok = ok && fabs(mean[e] - mean[2]) <= 5.0 * sqrt(var[e] / n + var[2] / n);
    ok = ok && shadow_rays > 0;
    /* a mode that does not exist is refused */
    nq.mode = 2;
    ok = ok && rt_scene_trace_nee(scene, &nq, rays, N, state, col, NULL, NULL, NULL) == RT_ERR_BAD_ARG;
    rt_scene_destroy(scene);
    rt_shutdown();
    if (!ok) {
        fprintf(stderr, "unexpected next-event-estimation results\n");
        return 1;
    }
    printf("NEE_TRACE_OK\n");
    return 0;
}
