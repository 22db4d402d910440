/* glossy_lights.c — light samples at glossy hits through the C-ABI alone: a room whose ground has roughness 0.5 and whose three
 * spheres have roughness 0, 0.5 and 1, under one sphere light and one triangle light, seen by a narrow pinhole camera pitched down
 * onto them, through rt_scene_trace and through rt_scene_trace_nee in mode RT_NEE_MIS under both settings of
 * rt_scene_set_glossy_sampling, max_bounces = 3.  Under RT_GLOSSY_BOUNCE a hit of roughness > 0 takes no light sample, so on most of
 * this room RT_NEE_MIS is the blind bounce; under RT_GLOSSY_MIS such a hit takes one, weighted by the density of the reference's
 * scatter lobe.  Build from the repository root (after `python -m ray_tracer_s8_amd.build`):
 *
 *     gcc -std=c99 -O2 -Iinclude examples/glossy_lights.c -Lray_tracer_s8_amd/lib -lrt_s8 \
 *         -Wl,-rpath,ray_tracer_s8_amd/lib -Wl,-rpath-link,/opt/rocm/lib -lm -o glossy_lights && ./glossy_lights
 *
 * Prints the mean and the variance of the samples' luminance of each estimator next to rt_scene_trace's, and GLOSSY_LIGHTS_OK when the
 * setting reads back, both means agree with rt_scene_trace's within five standard errors, RT_GLOSSY_MIS traces more shadow rays and
 * its variance is the lower one; exits 2 when rt_init finds no HIP device. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rt_tile.h"

#define W 64
#define H 32
#define SPP 32
#define N (W * H * SPP)
#define BOUNCES 3
#define N_SPH 5

static float luminance(const float* c) { return (c[0] + c[1] + c[2]) / 3.0f; }

/* SplitMix64: well-mixed xoshiro256++ states from a counter */
static uint64_t splitmix(uint64_t* x) {
    uint64_t z = (*x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static rt_sphere sphere(double x, double y, double z, double r, double ar, double ag, double ab, double rough, double emission) {
    rt_sphere s;
    memset(&s, 0, sizeof s);
    s.cx = (float)x; s.cy = (float)y; s.cz = (float)z; s.radius = (float)r;
    s.albedo_r = (float)ar; s.albedo_g = (float)ag; s.albedo_b = (float)ab;
    s.roughness = (float)rough;
    s.emission = (float)emission;
    return s;
}

int main(void) {
    int n_dev = 0;
    int rc = rt_init(&n_dev);
    if (rc != RT_OK) {
        fprintf(stderr, "rt_init: %s (%s): no HIP device\n", rt_strerror(rc), rt_last_error());
        return 2;
    }
    rt_sphere sph[N_SPH];
    sph[0] = sphere(0.0, -100.5, -3.0, 100.0, 0.5, 0.6, 0.4, 0.5, 0);                  /* the ground, roughness 0.5 */
    sph[1] = sphere(-1.2, 0.0, -3.2, 0.5, 0.8, 0.3, 0.3, 0.0, 0);
    sph[2] = sphere(0.0, 0.0, -3.0, 0.5, 0.3, 0.7, 0.4, 0.5, 0);
    sph[3] = sphere(1.2, 0.0, -2.8, 0.5, 0.7, 0.7, 0.2, 1.0, 0);
    sph[4] = sphere(0.2, 2.3, -3.0, 0.5, 1.0, 0.9, 0.7, 0.0, 6.0);                     /* the sphere light */
    rt_triangle tri;
    memset(&tri, 0, sizeof tri);
    tri.a[0] = -2.5f; tri.a[1] = 0.2f; tri.a[2] = -4.5f;
    tri.b[0] = -1.5f; tri.b[1] = 1.8f; tri.b[2] = -4.8f;
    tri.c[0] = -2.8f; tri.c[1] = 1.5f; tri.c[2] = -3.6f;
    tri.albedo_r = 0.6f; tri.albedo_g = 0.8f; tri.albedo_b = 1.0f; tri.emission = 3.0f; /* the triangle light */
    rt_scene* scene = NULL;
    if ((rc = rt_scene_create(0, sph, N_SPH, &tri, 1, NULL, &scene)) != RT_OK) {
        fprintf(stderr, "rt_scene_create: %s (%s)\n", rt_strerror(rc), rt_last_error());
        return 1;
    }
    uint32_t m = 0, setting = 99;
    int ok = rt_scene_light_count(scene, &m) == RT_OK && m == 2;
    ok = ok && rt_scene_glossy_sampling(scene, &setting) == RT_OK && setting == RT_GLOSSY_BOUNCE;          /* the default */
    ok = ok && rt_scene_set_glossy_sampling(scene, 2u) == RT_ERR_BAD_ARG;                                   /* no such setting */
    rt_ray* rays = malloc(sizeof(rt_ray) * N);
    uint64_t* state = malloc(sizeof(uint64_t) * 4 * N);
    float* col = malloc(sizeof(float) * 3 * N);
    uint32_t* shadow = malloc(sizeof(uint32_t) * N);
    if (!rays || !state || !col || !shadow) return 1;
    /* a pinhole at the origin looking down -z, pitched down onto the spheres; SPP records of every pixel's ray */
    for (int i = 0; i < N; i++) {
        const int p = i % (W * H), x = p % W, y = p / W;
        memset(&rays[i], 0, sizeof rays[i]);
        rays[i].dx = (float)((((x + 0.5) / W) * 2 - 1) * 0.3 * W / H);
        rays[i].dy = (float)((1 - ((y + 0.5) / H) * 2) * 0.3 - 0.1);
        rays[i].dz = -1.0f;
        rays[i].t_min = 0.001f; rays[i].t_max = 1000.0f;
    }
    /* estimator 0: rt_scene_trace; 1, 2: rt_scene_trace_nee in mode RT_NEE_MIS under RT_GLOSSY_BOUNCE and RT_GLOSSY_MIS */
    static const char* const names[3] = {"rt_scene_trace            ", "RT_NEE_MIS, glossy: bounce", "RT_NEE_MIS, glossy: MIS   "};
    double mean[3], var[3];
    unsigned long long shadow_sum[3] = {0, 0, 0};
    for (int e = 0; e < 3; e++) {
        uint64_t seed = e == 0 ? 2026 : 77;                                /* the same states under either setting */
        for (int i = 0; i < 4 * N; i++) state[i] = splitmix(&seed);
        rt_tile_stats st;
        if (e == 0) {
            rt_trace_request tq;
            memset(&tq, 0, sizeof tq);
            tq.spp = 1; tq.max_bounces = BOUNCES;
            rc = rt_scene_trace(scene, &tq, rays, N, state, col, NULL, &st);
            memset(shadow, 0, sizeof(uint32_t) * N);
        } else {
            rt_nee_request nq;
            memset(&nq, 0, sizeof nq);
            nq.spp = 1; nq.max_bounces = BOUNCES; nq.mode = RT_NEE_MIS;
            const uint32_t want = e == 2 ? RT_GLOSSY_MIS : RT_GLOSSY_BOUNCE;
            ok = ok && rt_scene_set_glossy_sampling(scene, want) == RT_OK && rt_scene_glossy_sampling(scene, &setting) == RT_OK && setting == want;
            rc = rt_scene_trace_nee(scene, &nq, rays, N, state, col, NULL, shadow, &st);
        }
        if (rc != RT_OK) {
            fprintf(stderr, "%s: %s (%s)\n", names[e], rt_strerror(rc), rt_last_error());
            return 1;
        }
        ok = ok && st.n_launches == 1;
        double sum = 0, sq = 0;
        for (int i = 0; i < N; i++) {
            const double x = luminance(col + 3 * i);
            sum += x; sq += x * x;
            shadow_sum[e] += shadow[i];
        }
        mean[e] = sum / N;
        var[e] = (sq - (double)N * mean[e] * mean[e]) / (N - 1);
    }
    printf("samples %d of each\n", N);
    for (int e = 0; e < 3; e++)
        printf("%s: mean %.5f variance %.5f  variance of rt_scene_trace / this %.3f  shadow rays %llu\n", names[e], mean[e], var[e], var[0] / var[e],
               shadow_sum[e]);
    printf("variance RT_GLOSSY_BOUNCE / RT_GLOSSY_MIS: %.2f\n", var[1] / var[2]);
    for (int e = 1; e < 3; e++) ok = ok && fabs(mean[0] - mean[e]) <= 5.0 * sqrt(var[0] / N + var[e] / N);
    ok = ok && shadow_sum[2] > shadow_sum[1] && var[2] < var[1];
    free(rays); free(state); free(col); free(shadow);
    rt_scene_destroy(scene);
    rt_shutdown();
    if (!ok) {
        fprintf(stderr, "unexpected glossy-sampling results\n");
        return 1;
    }
    printf("GLOSSY_LIGHTS_OK\n");
    return 0;
}
