/* Plain-C client of include/rt_tile.h's placed camera: a few frames of an orbit inside the c2-style box (five wall spheres, a light,
 * ten small spheres laid out on a ring here) through one persistent rt_frame_ctx.  Per frame: rt_frame_ctx_set_camera, then
 * rt_frame_ctx_render; the world stays resident, the frame buffer stays page-locked, and every new pose starts from the snake
 * strip assignment again.  Writes <prefix>_<k>.ppm.
 *   gcc -std=c11 -O2 -Iinclude examples/render_posed.c -Lray_tracer_s8_amd/lib -lrt_s8 -Wl,-rpath,... -lm -o render_posed
 *   ./render_posed [frames] [prefix]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "rt_tile.h"

#define N_SMALL 10

int main(int argc, char** argv) {
    const int n_frames = argc > 1 ? atoi(argv[1]) : 8;
    const char* prefix = argc > 2 ? argv[2] : "orbit";
    int n_dev = 0;
    int rc = rt_init(&n_dev);
    if (rc != RT_OK) {
        fprintf(stderr, "rt_init: %s (%s)\n", rt_strerror(rc), rt_last_error());
        return 2;                       /* no GPU: fail loudly, there is no CPU fallback */
    }
    rt_sphere world[6 + N_SMALL] = {
        {-102.0f, 0.0f, -4.0f, 100.0f, 0.75f, 0.15f, 0.15f, 0.0f, 0.0f},
        {102.0f, 0.0f, -4.0f, 100.0f, 0.15f, 0.75f, 0.15f, 0.0f, 0.0f},
        {0.0f, -102.0f, -4.0f, 100.0f, 0.73f, 0.73f, 0.73f, 0.0f, 0.0f},
        {0.0f, 102.0f, -4.0f, 100.0f, 0.73f, 0.73f, 0.73f, 0.0f, 0.0f},
        {0.0f, 0.0f, -108.0f, 100.0f, 0.73f, 0.73f, 0.73f, 0.0f, 0.0f},
        {0.0f, 1.6f, -4.0f, 0.5f, 1.0f, 1.0f, 1.0f, 0.0f, 8.0f},
    };
    const float two_pi = 6.2831853f;
    for (int i = 0; i < N_SMALL; i++) {
        const float a = two_pi * (float)i / N_SMALL, r = 0.25f + 0.02f * (float)i;
        rt_sphere s = {1.1f * cosf(a), -2.0f + r, -4.0f + 1.1f * sinf(a), r, 0.2f + 0.07f * (float)i, 0.5f, 0.9f - 0.07f * (float)i,
                       i >= 8 ? 1.0f : 0.0f, 0.0f};
        world[6 + i] = s;
    }
    rt_tile_request rq;
    rt_tile_request_defaults(&rq);
    rq.width = 256;
    rq.height = 144;
    rq.divisions = 8;
    rq.spp = 16;
    rq.seed = 42;
    const size_t frame_bytes = (size_t)rq.width * rq.height * 3;
    unsigned char* frame = (unsigned char*)malloc(frame_bytes);
    rt_frame_ctx* job = NULL;
    rc = rt_frame_ctx_create(NULL, 0, &job);
    if (rc == RT_OK) rc = rt_frame_ctx_set_world(job, world, 6 + N_SMALL, NULL, 0, NULL);
    for (int k = 0; k < n_frames && rc == RT_OK; k++) {
        /* the eye circles the middle of the box at radius 1.5, a little above the small spheres, and looks at the middle */
        const float a = two_pi * (float)k / (float)n_frames;
        rt_camera cam;
        rt_camera_defaults(&cam);
        cam.origin[0] = 1.5f * sinf(a);
        cam.origin[1] = -0.6f;
        cam.origin[2] = -4.0f + 1.5f * cosf(a);
        cam.target[0] = 0.0f;
        cam.target[1] = -1.2f;
        cam.target[2] = -4.0f;
        rc = rt_frame_ctx_set_camera(job, &cam);
        rt_frame_stats fs;
        if (rc == RT_OK) rc = rt_frame_ctx_render(job, &rq, frame, frame_bytes, &fs);
        if (rc != RT_OK) break;
        char path[512];
        snprintf(path, sizeof path, "%s_%02d.ppm", prefix, k);
        FILE* f = fopen(path, "wb");
        if (!f) {
            fprintf(stderr, "cannot write %s\n", path);
            rc = -100;
            break;
        }
        fprintf(f, "P6\n%u %u\n255\n", rq.width, rq.height);
        fwrite(frame, 1, frame_bytes, f);
        fclose(f);
        printf("frame %d: eye (%.2f, %.2f, %.2f)  assignment %u  segments %llu  wall %.2f ms -> %s\n", k, cam.origin[0], cam.origin[1],
               cam.origin[2], fs.assignment, (unsigned long long)fs.totals.ray_segments, fs.wall_ms, path);
    }
    if (rc != RT_OK) fprintf(stderr, "render_posed: rc=%d %s (%s)\n", rc, rt_strerror(rc), rt_last_error());
    rt_frame_ctx_destroy(job);              /* before the buffer it has page-locked is freed */
    free(frame);
    rt_shutdown();
    if (rc == RT_OK) printf("C_CLIENT_OK devices=%d frames=%d\n", n_dev, n_frames);
    return rc == RT_OK ? 0 : 1;
}
