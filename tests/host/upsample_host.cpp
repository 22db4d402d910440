// Test harness (CPU only, built by tests/test_upsample_host.py with g++ -ffp-contract=off): one call of the film-upsampler library
// (upsample_csrc/rt_upsample.h) run with the product's own per-pixel lines (upsample_csrc/rt_upsample_math.h) over plain arrays,
// counting how often each admission test rejects a tap and how often each class occurs.  With -DUPSAMPLE_HOST_MAIN it is a
// stand-alone program (its own main) that runs every plane set at three scales, for a sanitizer build.
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "rt_upsample_math.h"

namespace {

struct Side {
    const float* albedo;
    const float* normal;
    const float* depth;
    const uint32_t* hits;
    const uint32_t* index;
};

struct LowFilm {
    const float* linear;
    const Side& s;
    void colour(size_t i, float L[3]) const {
        for (int k = 0; k < 3; k++) L[k] = linear[3 * i + k];
    }
    void albedo(size_t i, float A[3]) const {
        for (int k = 0; k < 3; k++) A[k] = s.albedo[3 * i + k];
    }
    void normal(size_t i, float n[3]) const {
        for (int k = 0; k < 3; k++) n[k] = s.normal[3 * i + k];
    }
    float depth(size_t i) const { return s.depth[i]; }
    uint32_t hits(size_t i) const { return s.hits[i]; }
    uint32_t index(size_t i) const { return s.index[i]; }
};

struct Counter {
    uint64_t* c;
    void operator()(int b) const { c[b]++; }
};

struct Call {
    rtum::Frame f;
    const float* linear;
    Side lo, hi;
    float* out_linear;
    float* out_f32;
    uint8_t* out_rgb;
    uint8_t* out_class;
    uint64_t* counts;
};

template <uint32_t PLANES>
void run(const Call& c) {
    if constexpr (rtum::planes_ok(PLANES)) {
        const rtum::Frame& f = c.f;
        for (uint32_t r = 0; r < f.Rh; r++)
            for (uint32_t x = 0; x < f.Wh; x++) {
                const size_t i = (size_t)r * f.Wh + x;
                rtum::Guide g = {};
                if (PLANES & rtum::P_ALBEDO)
                    for (int k = 0; k < 3; k++) g.A[k] = c.hi.albedo[3 * i + k];
                if (PLANES & rtum::P_NORMAL)
                    for (int k = 0; k < 3; k++) g.n[k] = c.hi.normal[3 * i + k];
                if (PLANES & rtum::P_DEPTH) g.D = c.hi.depth[i];
                if (PLANES & rtum::P_HITS) g.hits = c.hi.hits[i];
                if (PLANES & rtum::P_INDEX) g.index = c.hi.index[i];
                float V[3];
                uint32_t cls;
                rtum::gather_pixel<PLANES>(f, x, r, g, LowFilm{c.linear, c.lo}, Counter{c.counts}, V, cls);
                rtum::exit_pixel<PLANES>(f, g, V, c.out_linear + 3 * i, c.out_f32 + 3 * i, c.out_rgb + 3 * i);
                c.out_class[i] = (uint8_t)cls;
            }
    }
}

template <uint32_t... P>
void dispatch(uint32_t planes, const Call& c, std::integer_sequence<uint32_t, P...>) {
    using Fn = void (*)(const Call&);
    static const Fn table[] = {run<P>...};
    table[planes](c);
}

}  // namespace

extern "C" {

int upsample_branch_count() { return rtum::BR_COUNT; }

// One call.  dims: Wl, Rl, Hl, y0l, Wh, Rh, Hh, y0h, kl, kh.  fp: k_depth, k_normal, eps.  lo, hi: five plane pointers each in
// rtu_planes' order (albedo, normal, depth, hits, index), NULL for a plane the call has not.  The four outputs are all written.
// counts: BR_COUNT counters, added to.  Returns 0, or 1 for a plane set no call may have.
int upsample_host(const uint32_t* dims, const float* fp, const float* linear, void* const* lo, void* const* hi, float* out_linear,
                  float* out_f32, uint8_t* out_rgb, uint8_t* out_class, uint64_t* counts) {
    Call c = {};
    rtum::Frame& f = c.f;
    f.Wl = dims[0], f.Rl = dims[1], f.Hl = dims[2], f.y0l = dims[3];
    f.Wh = dims[4], f.Rh = dims[5], f.Hh = dims[6], f.y0h = dims[7];
    rtum::frame_dens(f.Wl, f.Hl, f.u_den_l, f.v_den_l);
    rtum::frame_dens(f.Wh, f.Hh, f.u_den_h, f.v_den_h);
    f.kl_f = (float)dims[8];
    f.kh_f = (float)dims[9];
    f.kd = fp[0];
    f.kn2 = fp[1] * fp[1];
    f.eps = fp[2];
    c.linear = linear;
    c.lo = {(const float*)lo[0], (const float*)lo[1], (const float*)lo[2], (const uint32_t*)lo[3], (const uint32_t*)lo[4]};
    c.hi = {(const float*)hi[0], (const float*)hi[1], (const float*)hi[2], (const uint32_t*)hi[3], (const uint32_t*)hi[4]};
    uint32_t planes = 0;
    for (int k = 0; k < 5; k++) {
        if ((lo[k] != nullptr) != (hi[k] != nullptr)) return 1;
        if (lo[k]) planes |= 1u << k;
    }
    if (!rtum::planes_ok(planes)) return 1;
    c.out_linear = out_linear;
    c.out_f32 = out_f32;
    c.out_rgb = out_rgb;
    c.out_class = out_class;
    c.counts = counts;
    dispatch(planes, c, std::make_integer_sequence<uint32_t, rtum::P_ALL + 1u>{});
    return 0;
}
}

#ifdef UPSAMPLE_HOST_MAIN
// A 13 x 5 band (strip 1 of 3 of a 13 x 15 frame) to 2, 3 and 4 times its size, on every plane set: every line that reads a plane
// runs under the sanitizer, with exactly sized buffers.
int main() {
    const uint32_t Wl = 13, Rl = 5, Hl = 15, y0l = 5;
    const size_t nl = (size_t)Wl * Rl;
    std::vector<float> L(nl * 3), Al(nl * 3), Nl(nl * 3), Dl(nl);
    std::vector<uint32_t> hl(nl), il(nl);
    uint32_t lcg = 2463534242u;
    auto rnd = [&] { return (float)((lcg = lcg * 1664525u + 1013904223u) >> 8) / 16777216.0f; };
    auto fill = [&](size_t n, uint32_t W, uint32_t cell, uint32_t k, float* A, float* N, float* D, uint32_t* h, uint32_t* ix) {
        for (size_t i = 0; i < n; i++) {
            h[i] = rnd() < 0.15f ? 0u : k;
            ix[i] = rnd() < 0.1f ? 0xffffffffu : (uint32_t)(i % W) / cell;
            D[i] = h[i] * (4.0f + (rnd() < 0.2f ? 3.0f : 0.1f) * rnd());
            for (int c = 0; c < 3; c++) {
                A[3 * i + c] = k * rnd();
                N[3 * i + c] = c == 2 ? (rnd() < 0.1f ? -1.0f : 1.0f) * (float)h[i] : 0.2f * rnd();
            }
        }
    };
    // a few subnormal, huge and non-finite values at pixels of their own (the classes of tests/_extreme_planes.py) and the integer
    // planes' extremes, on a side's planes: whatever a plane holds, no line reads or writes outside its buffer
    const float special[] = {1e-45f, -1e-45f, 5.9e-39f, 1.1754942e-38f, -0.0f, 1e-30f, 1.9e19f, 3e38f, -3.4028235e38f,
                             __builtin_inff(), -__builtin_inff(), __builtin_nanf(""), -__builtin_nanf(""), -1.5f};
    auto salt = [&](size_t n, float k, float* A, float* N, float* D, uint32_t* h, uint32_t* ix) {
        for (size_t j = 0; j < sizeof special / sizeof *special; j++) {
            const size_t i = (17 * j + 5) % n;
            switch (j % 3) {
                case 0: A[3 * i + j % 3] = special[j]; break;
                case 1: N[3 * i + j % 3] = special[j]; break;
                default: D[i] = special[j]; break;
            }
        }
        A[3 * (n / 2)] = -0.01f * k;                              // d = A / k + eps = 0 at the side's k
        h[3 % n] = 0xffffffffu;
        h[7 % n] = (1u << 24) + 1u;
        h[11 % n] = 0u;                                           // (under a depth and a normal that are not zero)
        ix[13 % n] = 0xffffffffu;
    };
    fill(nl, Wl, 4, 2, Al.data(), Nl.data(), Dl.data(), hl.data(), il.data());
    salt(nl, 2.0f, Al.data(), Nl.data(), Dl.data(), hl.data(), il.data());
    for (float& v : L) v = 2.0f * rnd();
    for (size_t j = 0; j < sizeof special / sizeof *special; j++) L[(7 * j + 2) % L.size()] = special[j];
    std::vector<uint64_t> counts(rtum::BR_COUNT);
    const float fp[3] = {0.1f, 0.9f, 0.01f};
    for (uint32_t s = 2; s <= 4; s++) {
        const uint32_t Wh = s * Wl, Rh = s * Rl;
        const size_t nh = (size_t)Wh * Rh;
        std::vector<float> Ah(nh * 3), Nh(nh * 3), Dh(nh), lin(nh * 3), f32(nh * 3);
        std::vector<uint32_t> hh(nh), ih(nh);
        std::vector<uint8_t> rgb(nh * 3), cls(nh);
        fill(nh, Wh, 4 * s, 1, Ah.data(), Nh.data(), Dh.data(), hh.data(), ih.data());
        salt(nh, 1.0f, Ah.data(), Nh.data(), Dh.data(), hh.data(), ih.data());
        const uint32_t dims[10] = {Wl, Rl, Hl, y0l, Wh, Rh, s * Hl, s * y0l, 2, 1};
        for (uint32_t planes = 0; planes <= rtum::P_ALL; planes++) {
            if (!rtum::planes_ok(planes)) continue;
            void* lo[5] = {Al.data(), Nl.data(), Dl.data(), hl.data(), il.data()};
            void* hi[5] = {Ah.data(), Nh.data(), Dh.data(), hh.data(), ih.data()};
            for (int k = 0; k < 5; k++)
                if (!(planes >> k & 1u)) lo[k] = hi[k] = nullptr;
            if (upsample_host(dims, fp, L.data(), lo, hi, lin.data(), f32.data(), rgb.data(), cls.data(), counts.data())) return 1;
        }
    }
    for (int b = 0; b < rtum::BR_COUNT; b++)
        if (!counts[b]) {
            std::printf("upsample_host: branch %d never taken\n", b);
            return 2;
        }
    std::printf("upsample_host: %llu pixels upsampled, %llu of them by the bilinear fall-back\n",
                (unsigned long long)(counts[rtum::BR_CLASS0] + counts[rtum::BR_CLASS1]), (unsigned long long)counts[rtum::BR_CLASS1]);
    return 0;
}
#endif
