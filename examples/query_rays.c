/* query_rays.c — ray queries through the C-ABI alone: a resident scene of two spheres and a floor triangle, four rays, their
 * closest hits and an occlusion query.  Build from the repository root (after `python -m ray_tracer_s8_amd.build`):
 *
 *     gcc -std=c99 -O2 -Iinclude examples/query_rays.c -Lray_tracer_s8_amd/lib -lrt_s8 \
 *         -Wl,-rpath,ray_tracer_s8_amd/lib -Wl,-rpath-link,/opt/rocm/lib -o query_rays && ./query_rays
 *
 * Prints one line per ray and QUERY_OK; exits 2 when rt_init finds no HIP device. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "rt_tile.h"

int main(void) {
    int n_dev = 0;
    int rc = rt_init(&n_dev);
    if (rc != RT_OK) {
        fprintf(stderr, "rt_init: %s (%s): no HIP device\n", rt_strerror(rc), rt_last_error());
        return 2;
    }
    rt_sphere sph[2];
    memset(sph, 0, sizeof sph);
    sph[0].cz = -3.0f; sph[0].radius = 1.0f; sph[0].albedo_r = 0.8f;
    sph[1].cx = 2.5f; sph[1].cz = -4.0f; sph[1].radius = 0.5f; sph[1].albedo_g = 0.8f;
    rt_triangle tri;
    memset(&tri, 0, sizeof tri);
    const float a[3] = {-10.f, -1.f, 0.f}, b[3] = {10.f, -1.f, 0.f}, c[3] = {0.f, -1.f, -20.f};
    memcpy(tri.a, a, sizeof a); memcpy(tri.b, b, sizeof b); memcpy(tri.c, c, sizeof c);
    rt_scene* scene = NULL;
    if ((rc = rt_scene_create(0, sph, 2, &tri, 1, NULL, &scene)) != RT_OK) {
        fprintf(stderr, "rt_scene_create: %s (%s)\n", rt_strerror(rc), rt_last_error());
        return 1;
    }
    /* straight at sphere 0, at sphere 1, down onto the floor, up into the sky */
    rt_ray rays[4] = {{0.f, 0.f, 0.f, 0.001f, 0.f, 0.f, -1.f, 1000.f},
                      {0.f, 0.f, 0.f, 0.001f, 2.5f, 0.f, -4.f, 1000.f},
                      {0.f, 0.f, 0.f, 0.001f, 0.f, -1.f, -1.f, 1000.f},
                      {0.f, 0.f, 0.f, 0.001f, 0.f, 1.f, 0.f, 1000.f}};
    rt_hit hits[4];
    rt_tile_stats st;
    if ((rc = rt_scene_intersect(scene, rays, 4, RT_QUERY_CLOSEST, RT_FLAG_NONE, hits, &st)) != RT_OK) {
        fprintf(stderr, "rt_scene_intersect: %s (%s)\n", rt_strerror(rc), rt_last_error());
        return 1;
    }
    const uint32_t want[4] = {0u, 1u, 2u, RT_HIT_NONE};
    int ok = st.primary_rays == 4 && st.n_launches == 1;
    for (int i = 0; i < 4; i++) {
        printf("ray %d: index %d distance %g point (%g, %g, %g) normal (%g, %g, %g)\n", i, hits[i].index == RT_HIT_NONE ? -1 : (int)hits[i].index,
               hits[i].distance, hits[i].px, hits[i].py, hits[i].pz, hits[i].nx, hits[i].ny, hits[i].nz);
        ok = ok && hits[i].index == want[i];
    }
    ok = ok && hits[0].distance == 2.0f && hits[0].nz == 1.0f && isinf(hits[3].distance);
    rt_hit occ[4];
    if ((rc = rt_scene_intersect(scene, rays, 4, RT_QUERY_ANY, RT_FLAG_NONE, occ, NULL)) != RT_OK) {
        fprintf(stderr, "rt_scene_intersect (any): %s (%s)\n", rt_strerror(rc), rt_last_error());
        return 1;
    }
    for (int i = 0; i < 4; i++) ok = ok && ((occ[i].index == RT_HIT_NONE) == (want[i] == RT_HIT_NONE));
    ok = ok && rt_scene_intersect(scene, rays, 0, RT_QUERY_CLOSEST, RT_FLAG_NONE, hits, NULL) == RT_ERR_BAD_ARG;
    rt_scene_destroy(scene);
    rt_shutdown();
    if (!ok) {
        fprintf(stderr, "unexpected hits\n");
        return 1;
    }
    printf("QUERY_OK\n");
    return 0;
}
