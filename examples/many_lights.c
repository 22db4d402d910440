/* many_lights.c — light selection by power through the C-ABI alone: a room of four diffuse spheres under one lamp (emission 6, radius
 * 0.5) and 32 dim spheres (emission 0.05, radius 0.05) on a ring around it, M = 33 emitters, through rt_scene_trace_nee with and
 * without RT_FLAG_LIGHTS_BY_POWER, max_bounces = 3, RT_NEE_MIS.  Picked uniformly the lamp gets one light sample in 33, weighted by
 * 33; with the flag it gets about every second one (rt_scene_light_table prints the probabilities).  S passes with fresh RNG states
 * give N * S samples of each.  Build from the repository root (after `python -m ray_tracer_s8_amd.build`):
 *
 *     gcc -std=c99 -O2 -Iinclude examples/many_lights.c -Lray_tracer_s8_amd/lib -lrt_s8 \
 *         -Wl,-rpath,ray_tracer_s8_amd/lib -Wl,-rpath-link,/opt/rocm/lib -lm -o many_lights && ./many_lights
 *
 * Prints the mean and the variance of the samples' luminance for both picks and MANY_LIGHTS_OK when the two means agree within five
 * standard errors and the probabilities add up to 1; exits 2 when rt_init finds no HIP device. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "rt_tile.h"

#define W 64
#define H 32
#define N (W * H)
#define S 16
#define BOUNCES 3
#define N_DIM 32
#define N_SPH (5 + N_DIM)

static float luminance(const float* c) { return (c[0] + c[1] + c[2]) / 3.0f; }

/* SplitMix64: well-mixed xoshiro256++ states from a counter */
static uint64_t splitmix(uint64_t* x) {
    uint64_t z = (*x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static rt_sphere sphere(float x, float y, float z, float r, float ar, float ag, float ab, float emission) {
    rt_sphere s;
    memset(&s, 0, sizeof s);
    s.cx = x; s.cy = y; s.cz = z; s.radius = r;
    s.albedo_r = ar; s.albedo_g = ag; s.albedo_b = ab;
    s.emission = emission;
    return s;
}

int main(void) {
    int n_dev = 0;
    int rc = rt_init(&n_dev);
    if (rc != RT_OK) {
        fprintf(stderr, "rt_init: %s (%s): no HIP device\n", rt_strerror(rc), rt_last_error());
        return 2;
    }
    static rt_sphere sph[N_SPH];
    sph[0] = sphere(0.0f, -100.5f, -3.0f, 100.0f, 0.5f, 0.6f, 0.4f, 0.0f);
    sph[1] = sphere(-1.2f, 0.0f, -3.2f, 0.5f, 0.8f, 0.3f, 0.3f, 0.0f);
    sph[2] = sphere(0.0f, 0.0f, -3.0f, 0.5f, 0.3f, 0.7f, 0.4f, 0.0f);
    sph[3] = sphere(1.2f, 0.0f, -2.8f, 0.5f, 0.7f, 0.7f, 0.2f, 0.0f);
    sph[4] = sphere(0.2f, 2.3f, -3.0f, 0.5f, 1.0f, 0.9f, 0.7f, 6.0f);                  /* the lamp */
    for (int i = 0; i < N_DIM; i++) {
        const float a = (float)i * (6.2831853f / N_DIM);
        sph[5 + i] = sphere(0.2f + 1.6f * cosf(a), 1.6f + 0.3f * sinf(3.0f * a), -3.0f + 1.6f * sinf(a), 0.05f, 1.0f, 0.9f, 0.7f, 0.05f);
    }
    rt_scene* scene = NULL;
    if ((rc = rt_scene_create(0, sph, N_SPH, NULL, 0, NULL, &scene)) != RT_OK) {
        fprintf(stderr, "rt_scene_create: %s (%s)\n", rt_strerror(rc), rt_last_error());
        return 1;
    }
    /* the table: which emitter, and how likely under either pick */
    uint32_t m = 0, world[N_SPH];
    float p[N_SPH], p_uniform[N_SPH];
    int ok = rt_scene_light_count(scene, &m) == RT_OK && m == 1 + N_DIM;
    ok = ok && rt_scene_light_table(scene, RT_FLAG_LIGHTS_BY_POWER, world, p, N_SPH) == RT_OK;
    ok = ok && rt_scene_light_table(scene, RT_FLAG_NONE, NULL, p_uniform, N_SPH) == RT_OK;
    ok = ok && rt_scene_light_table(scene, RT_FLAG_LIGHTS_BY_POWER, world, p, m - 1) == RT_ERR_BAD_ARG;     /* too small a capacity */
    if (!ok) {
        fprintf(stderr, "rt_scene_light_table: %s\n", rt_last_error());
        return 1;
    }
    double p_sum = 0.0;
    for (uint32_t k = 0; k < m; k++) p_sum += p[k];
    printf("emitters %u; the lamp (world position %u): p = %.4f by power, %.4f uniformly; a dim sphere: p = %.4f\n", m, world[0], p[0],
           p_uniform[0], p[1]);
    /* a pinhole at the origin looking down -z, pitched down onto the spheres */
    static rt_ray rays[N];
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            rt_ray* ry = &rays[y * W + x];
            memset(ry, 0, sizeof *ry);
            ry->dx = ((x + 0.5f) / W * 2.f - 1.f) * 0.3f * W / H;
            ry->dy = (1.f - (y + 0.5f) / H * 2.f) * 0.3f - 0.1f;
            ry->dz = -1.f;
            ry->t_min = 0.001f; ry->t_max = 1000.f;
        }
    static uint64_t state[4 * N];
    static float col[3 * N];
    rt_nee_request nq;
    memset(&nq, 0, sizeof nq);
    nq.spp = 1; nq.max_bounces = BOUNCES; nq.ray_form = RT_TRACE_RAY_NEW; nq.mode = RT_NEE_MIS;
    static const char* const names[2] = {"picked uniformly", "picked by power "};
    double sum[2] = {0, 0}, sq[2] = {0, 0};
    uint64_t seed = 2025;
    for (int s = 0; s < S; s++)
        for (int e = 0; e < 2; e++) {
            for (int i = 0; i < 4 * N; i++) state[i] = splitmix(&seed);
            nq.flags = e ? RT_FLAG_LIGHTS_BY_POWER : RT_FLAG_NONE;
            rt_tile_stats st;
            if ((rc = rt_scene_trace_nee(scene, &nq, rays, N, state, col, NULL, NULL, &st)) != RT_OK) {
                fprintf(stderr, "%s: %s (%s)\n", names[e], rt_strerror(rc), rt_last_error());
                return 1;
            }
            ok = ok && st.n_launches == 1;
            for (int i = 0; i < N; i++) {
                const double x = luminance(col + 3 * i);
                sum[e] += x; sq[e] += x * x;
            }
        }
    const double n = (double)N * S;
    double mean[2], var[2];
    for (int e = 0; e < 2; e++) {
        mean[e] = sum[e] / n;
        var[e] = (sq[e] - n * mean[e] * mean[e]) / (n - 1);
    }
    printf("samples %d of each\n", N * S);
    for (int e = 0; e < 2; e++) printf("%s: mean %.5f variance %.5f\n", names[e], mean[e], var[e]);
    printf("variance picked uniformly / by power: %.2f\n", var[0] / var[1]);
    ok = ok && fabs(mean[0] - mean[1]) <= 5.0 * sqrt(var[0] / n + var[1] / n) && fabs(p_sum - 1.0) < 1e-4 && p[0] > 0.5f;
    rt_scene_destroy(scene);
    rt_shutdown();
    if (!ok) {
        fprintf(stderr, "unexpected many-light results\n");
        return 1;
    }
    printf("MANY_LIGHTS_OK\n");
    return 0;
}
