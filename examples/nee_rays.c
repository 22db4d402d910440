/* nee_rays.c — next-event estimation through the C-ABI alone: a diffuse sphere on a diffuse floor triangle under a small light, a
 * 32 x 32 pinhole camera of the caller's own at (0, 1, 2), and K = 4 path steps (rt_scene_bounce, host form), each followed by one
 * light sample at every hit that scattered (rt_scene_direct on the step's hit records and its next list).  Per ray the caller keeps a
 * throughput T and a colour c:
 *     MISSED:    c += T * sky, the path ends;
 *     EMITTED:   c += T * light only at the first step (later the sample of the step before has counted that light), the path ends;
 *     SCATTERED: T *= albedo, then c += T * direct (not at the last step: a light sample stands for the NEXT segment's hit).
 * Every material has roughness 0, so the mean over many samples is the mean of rt_scene_trace (max_bounces = K - 1) of the same
 * rays — which finds the light only by hitting it — with far less variance.  S passes with fresh RNG states give N * S samples of
 * each.  Build from the repository root (after `python -m ray_tracer_s8_amd.build`):
 *
 *     gcc -std=c99 -O2 -Iinclude examples/nee_rays.c -Lray_tracer_s8_amd/lib -lrt_s8 \
 *         -Wl,-rpath,ray_tracer_s8_amd/lib -Wl,-rpath-link,/opt/rocm/lib -lm -o nee_rays && ./nee_rays
 *
 * Prints the mean and the variance of the samples' luminance for both estimators and NEE_OK when the means agree within five
 * standard errors and the variance is the lower one; exits 2 when rt_init finds no HIP device. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "rt_tile.h"

#define W 32
#define H 32
#define N (W * H)
#define K 4
#define S 16

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
    uint32_t n_lights = 0;
    int ok = rt_scene_light_count(scene, &n_lights) == RT_OK && n_lights == 1;
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
    static rt_ray first[N], rays[N];
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const float sx = ((x + 0.5f) / W * 2.f - 1.f) * half, sy = (1.f - (y + 0.5f) / H * 2.f) * half;
            rt_ray* ry = &first[y * W + x];
            ry->ox = eye[0]; ry->oy = eye[1]; ry->oz = eye[2];
            ry->dx = f[0] + sx * r[0] + sy * u[0];
            ry->dy = f[1] + sx * r[1] + sy * u[1];
            ry->dz = f[2] + sx * r[2] + sy * u[2];
            ry->t_min = 0.001f; ry->t_max = 1000.f;
        }
    static uint64_t state[4 * N];
    static rt_bounce step[N];
    static rt_hit hits[N];
    static rt_direct light[N];
    static uint32_t list[2][N];
    static float T[3 * N], col[3 * N], ref[3 * N];
    rt_bounce_request rq;
    memset(&rq, 0, sizeof rq);
    rt_direct_request dq;
    memset(&dq, 0, sizeof dq);
    dq.t_min = 0.001f; dq.t_max = 1000.f;
    rt_trace_request tq;
    memset(&tq, 0, sizeof tq);
    tq.spp = 1; tq.max_bounces = K - 1; tq.ray_form = RT_TRACE_RAY_NEW;
    double sum[2] = {0, 0}, sq[2] = {0, 0};
    uint64_t shadow_rays = 0, lit = 0, seed = 2024;
    for (int s = 0; s < S && ok; s++) {
        /* the caller's estimator */
        for (int i = 0; i < 4 * N; i++) state[i] = splitmix(&seed);
        memcpy(rays, first, sizeof rays);
        for (int i = 0; i < 3 * N; i++) { T[i] = 1.0f; col[i] = 0.0f; }
        uint32_t n_act = N;
        for (int k = 0; k < K && n_act; k++) {
            const uint32_t* active = k ? list[(k + 1) % 2] : NULL;     /* the first step takes every ray */
            uint32_t* next = list[k % 2];
            uint32_t n_next = 0;
            rt_tile_stats st;
            rq.ray_form = k ? RT_TRACE_RAY_AS_GIVEN : RT_TRACE_RAY_NEW;
            rc = rt_scene_bounce(scene, &rq, rays, N, state, active, k ? n_act : 0, step, hits, next, &n_next, &st);
            const int sample = k < K - 1;                              /* (the trace's last segment has no bounce after it) */
            if (rc == RT_OK && n_next && sample) {
                rc = rt_scene_direct(scene, &dq, hits, N, state, next, n_next, light, &st);
                shadow_rays += st.ray_segments;
                ok = ok && st.primary_rays == 0 && st.n_launches == 1 && st.ray_segments <= n_next;
            }
            if (rc != RT_OK) {
                fprintf(stderr, "step %d: %s (%s)\n", k, rt_strerror(rc), rt_last_error());
                return 1;
            }
            for (uint32_t j = 0; j < n_act; j++) {
                const uint32_t i = active ? active[j] : j;
                const rt_bounce* b_ = &step[i];
                const float rgb[3] = {b_->r, b_->g, b_->b};
                if (b_->status == RT_BOUNCE_SCATTERED && sample) {
                    const float d[3] = {light[i].r, light[i].g, light[i].b};
                    lit += light[i].status == RT_DIRECT_LIT;
                    for (int ch = 0; ch < 3; ch++) {
                        T[3 * i + ch] *= rgb[ch];
                        col[3 * i + ch] += T[3 * i + ch] * d[ch];
                    }
                } else if (b_->status == RT_BOUNCE_MISSED || (b_->status == RT_BOUNCE_EMITTED && k == 0)) {
                    for (int ch = 0; ch < 3; ch++) col[3 * i + ch] += T[3 * i + ch] * rgb[ch];
                }
            }
            n_act = n_next;
        }
        /* the library's own integrator on the same rays, other states */
        for (int i = 0; i < 4 * N; i++) state[i] = splitmix(&seed);
        if ((rc = rt_scene_trace(scene, &tq, first, N, state, ref, NULL, NULL)) != RT_OK) {
            fprintf(stderr, "rt_scene_trace: %s (%s)\n", rt_strerror(rc), rt_last_error());
            return 1;
        }
        for (int i = 0; i < N; i++) {
            const double x0 = luminance(col + 3 * i), x1 = luminance(ref + 3 * i);
            sum[0] += x0; sq[0] += x0 * x0;
            sum[1] += x1; sq[1] += x1 * x1;
        }
    }
    const double n = (double)N * S;
    const double mean0 = sum[0] / n, mean1 = sum[1] / n;
    const double var0 = (sq[0] - n * mean0 * mean0) / (n - 1), var1 = (sq[1] - n * mean1 * mean1) / (n - 1);
    printf("samples %d; shadow rays %llu, lit %llu\n", N * S, (unsigned long long)shadow_rays, (unsigned long long)lit);
    printf("bounce + direct: mean %.5f variance %.5f\n", mean0, var0);
    printf("rt_scene_trace:  mean %.5f variance %.5f (variance ratio %.1f)\n", mean1, var1, var1 / var0);
    ok = ok && lit > 0 && fabs(mean0 - mean1) <= 5.0 * sqrt(var0 / n + var1 / n) && var0 < var1;
    /* an index beyond the batch is refused */
    list[0][0] = N;
    ok = ok && rt_scene_direct(scene, &dq, hits, N, state, list[0], 1, light, NULL) == RT_ERR_BAD_ARG;
    rt_scene_destroy(scene);
    rt_shutdown();
    if (!ok) {
        fprintf(stderr, "unexpected direct-lighting results\n");
        return 1;
    }
    printf("NEE_OK\n");
    return 0;
}
