// Test harness (CPU only, built by tests/test_history_host.py with g++ -ffp-contract=off): one frame of the film-history library
// (history_csrc/rt_history.h) run with the product's own per-pixel lines and camera setup (history_csrc/rt_history_math.h,
// csrc/rt_plan.h) over plain arrays, counting how often each branch of accumulate_pixel is taken.  With -DHISTORY_HOST_MAIN it is a
// stand-alone program (its own main) that runs a few frames, for a sanitizer build.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rt_history_math.h"

namespace {

struct Planes {
    float* accum;
    float* moments;
    float* length;
    float* depth;
    uint32_t* index;
    float* normal;
};

struct PrevState {
    const Planes& s;
    void guard(size_t i, float& N, uint32_t& index, float& z) const {
        N = s.length[i];
        index = s.index[i];
        z = s.depth[i];
    }
    void normal(size_t i, float n[3]) const {
        for (int k = 0; k < 3; k++) n[k] = s.normal[3 * i + k];
    }
    void values(size_t i, float C[3], float M[2]) const {
        for (int k = 0; k < 3; k++) C[k] = s.accum[3 * i + k];
        M[0] = s.moments[2 * i];
        M[1] = s.moments[2 * i + 1];
    }
};

struct Counter {
    uint64_t* c;
    void operator()(int b) const { c[b]++; }
};

}  // namespace

extern "C" {

int history_branch_count() { return rthm::BR_COUNT; }

// One frame.  fp: alpha, n_max, k_depth, k_normal.  rq, cam: the frame's first strip and camera (cam NULL: the reference camera);
// prq: NULL for a first frame.  normal NULL: a call without normals.  prev, next: six plane pointers each in rth_state's order.
// counts: BR_COUNT counters, added to.  Returns 0, or 1 for a pose make_pose refuses.
int history_frame_host(uint32_t W, uint32_t R, const float* fp, const rt_tile_request* rq, const rt_camera* cam,
                       const rt_tile_request* prq, const rt_camera* pcam, const float* C, const float* M, const float* depth,
                       const uint32_t* hits, const uint32_t* index, const float* normal, void* const* prev, void* const* next,
                       uint64_t* counts) {
    rthm::Frame f = {};
    f.W = W;
    f.R = R;
    f.normals = normal ? 1u : 0u;
    f.alpha = fp[0];
    f.n_max = fp[1];
    f.kd = fp[2];
    f.kn2 = fp[3] * fp[3];
    if (!rthm::set_cameras(f, *rq, cam, prq, pcam)) return 1;
    Planes pv = {}, nx;
    if (prq) pv = {(float*)prev[0], (float*)prev[1], (float*)prev[2], (float*)prev[3], (uint32_t*)prev[4], (float*)prev[5]};
    nx = {(float*)next[0], (float*)next[1], (float*)next[2], (float*)next[3], (uint32_t*)next[4], (float*)next[5]};
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    for (uint32_t r = 0; r < R; r++)
        for (uint32_t x = 0; x < W; x++) {
            const size_t i = (size_t)r * W + x;
            float oN, oZ;
            rthm::accumulate_pixel(f, x, r, C + 3 * i, M + 2 * i, depth[i], hits[i], index[i], normal ? normal + 3 * i : zero,
                                   PrevState{pv}, Counter{counts}, nx.accum + 3 * i, nx.moments + 2 * i, oN, oZ);
            nx.length[i] = oN;
            nx.depth[i] = oZ;
            nx.index[i] = index[i];
            if (normal)
                for (int k = 0; k < 3; k++) nx.normal[3 * i + k] = normal[3 * i + k];
        }
    return 0;
}
}

#ifdef HISTORY_HOST_MAIN
// Four frames of a 37 x 11 band (strips 1 and 2 of 3 of a 37 x 33 frame) under a camera that drifts and turns, with normals, the
// state alternated between two sets: every branch that reads a plane runs under the sanitizer.
int main() {
    const uint32_t W = 37, H = 33, R = 22;
    rt_tile_request rq = {};
    rq.width = W;
    rq.height = H;
    rq.divisions = 3;
    rq.division_no = 1;
    rq.fov = 1.0f;
    rq.focal_length = 1.0f;
    const size_t np = (size_t)W * R;
    std::vector<float> C(np * 3), M(np * 2), D(np), N(np * 3);
    std::vector<uint32_t> hits(np), idx(np);
    struct Set {
        std::vector<float> a, m, l, d, n;
        std::vector<uint32_t> i;
    } sets[2];
    for (auto& s : sets) {
        s.a.resize(np * 3);
        s.m.resize(np * 2);
        s.l.resize(np);
        s.d.resize(np);
        s.n.resize(np * 3);
        s.i.resize(np);
    }
    std::vector<uint64_t> counts(rthm::BR_COUNT);
    const float fp[4] = {0.3f, 3.0f, 0.2f, 0.5f};
    rt_camera cams[4] = {};
    uint32_t lcg = 12345u;
    auto rnd = [&] { return (float)((lcg = lcg * 1664525u + 1013904223u) >> 8) / 16777216.0f; };
    for (int k = 0; k < 4; k++) {
        cams[k].origin[0] = 0.4f * k - 0.5f;
        cams[k].origin[1] = 0.1f * k;
        cams[k].target[0] = 0.3f * k - 0.4f;
        cams[k].target[2] = -1.0f;
        cams[k].up[1] = 1.0f;
        for (size_t i = 0; i < np; i++) {
            hits[i] = rnd() < 0.1f ? 0u : 2u;
            idx[i] = rnd() < 0.05f ? 0xffffffffu : (uint32_t)(i % W) / 8u;
            D[i] = hits[i] * (4.0f + rnd());
            for (int c = 0; c < 3; c++) {
                C[3 * i + c] = rnd();
                N[3 * i + c] = c == 2 ? (float)hits[i] : 0.2f * rnd();
            }
            M[2 * i] = rnd();
            M[2 * i + 1] = rnd();
        }
        // a few subnormal, huge and non-finite inputs at pixels of their own (the classes of tests/_extreme_planes.py), and the integer
        // planes' extremes: whatever a plane holds, no line reads or writes outside its buffer
        const float special[] = {1e-45f, -1e-45f, 5.9e-39f, 1.1754942e-38f, -0.0f, 1e-30f, 1.9e19f, 3e38f, -3.4028235e38f,
                                 __builtin_inff(), -__builtin_inff(), __builtin_nanf(""), -__builtin_nanf(""), -1.5f};
        for (size_t j = 0; j < sizeof special / sizeof *special; j++) {
            const size_t i = (53 * j + 11 * (size_t)k + 5) % np;
            const float v = special[j];
            switch ((j + (size_t)k) % 4) {
                case 0: C[3 * i + j % 3] = v; break;
                case 1: M[2 * i + j % 2] = v; break;
                case 2: D[i] = v; break;
                default: N[3 * i + j % 3] = v; break;
            }
        }
        hits[(29 * (size_t)k + 3) % np] = 0xffffffffu;
        hits[(29 * (size_t)k + 47) % np] = (1u << 24) + 1u;
        hits[(29 * (size_t)k + 91) % np] = 0u;                    // (under a depth and a normal that are not zero)
        idx[(29 * (size_t)k + 135) % np] = 0xffffffffu;
        Set &pv = sets[(k + 1) & 1], &nx = sets[k & 1];
        void* prev[6] = {pv.a.data(), pv.m.data(), pv.l.data(), pv.d.data(), pv.i.data(), pv.n.data()};
        void* next[6] = {nx.a.data(), nx.m.data(), nx.l.data(), nx.d.data(), nx.i.data(), nx.n.data()};
        if (history_frame_host(W, R, fp, &rq, &cams[k], k ? &rq : nullptr, k ? &cams[k - 1] : nullptr, C.data(), M.data(), D.data(),
                               hits.data(), idx.data(), N.data(), prev, next, counts.data()))
            return 1;
    }
    uint64_t blended = counts[rthm::BR_BLEND];
    std::printf("history_host: %llu pixels blended\n", (unsigned long long)blended);
    return blended ? 0 : 2;
}
#endif
