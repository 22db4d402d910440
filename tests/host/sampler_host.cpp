// Test harness (CPU only, built by tests/test_sampler_host.py with g++ -ffp-contract=off): the calls of the film-sampler library
// (sampler_csrc/rt_sampler.h) run with the product's own per-pixel lines (sampler_csrc/rt_sampler_math.h) over plain arrays, the lists
// built serially in ascending order.  With -DSAMPLER_HOST_MAIN it is a stand-alone program (its own main) that runs a round on a small
// image, for a sanitizer build.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_sampler_math.h"

namespace {

struct Bytes {
    const uint8_t* b;
    uint8_t operator()(size_t i) const { return b[i]; }
};

}  // namespace

extern "C" {

// rts_select.  err [R W], active [R W] (strip i's list from i Hs W), strip_counts [R / Hs].
int sampler_select_host(uint32_t W, uint32_t R, uint32_t Hs, uint32_t dilate, float threshold, float eps, const float* moments,
                        const int32_t* counts, float* err, uint32_t* active, uint32_t* strip_counts) {
    if (W == 0 || R == 0 || Hs == 0 || R % Hs != 0 || dilate > 1) return 1;
    std::vector<uint8_t> flag((size_t)W * R);
    for (size_t i = 0; i < flag.size(); i++) {
        err[i] = rtsm::pixel_error(moments[2 * i], moments[2 * i + 1], counts[i], eps);
        flag[i] = rtsm::noisy(err[i], threshold) ? 1 : 0;
    }
    const uint32_t P = Hs * W;
    for (uint32_t s = 0; s < R / Hs; s++) {
        uint32_t n = 0;
        for (uint32_t q = 0; q < P; q++)
            if (rtsm::active_pixel(q % W, s * Hs + q / W, W, R, dilate, Bytes{flag.data()})) active[(size_t)s * P + n++] = q;
        strip_counts[s] = n;
    }
    return 0;
}

// rts_gather on one buffer of 32-byte records
int sampler_gather_host(uint32_t n_active, uint32_t k, uint32_t pixels, const uint32_t* active, const uint8_t* records, uint8_t* out) {
    for (uint32_t a = 0; a < n_active; a++) {
        if (active[a] >= pixels) continue;
        for (uint32_t j = 0; j < k; j++)
            std::memcpy(out + 32 * ((size_t)a * k + j), records + 32 * rtsm::record_index(active[a], k, j), 32);
    }
    return 0;
}

// rts_fold
int sampler_fold_host(uint32_t n_active, uint32_t k, uint32_t pixels, const uint32_t* active, const float* rgb, float* accum,
                      float* moments, int32_t* counts) {
    for (uint32_t a = 0; a < n_active; a++) {
        const size_t q = active[a];
        if (q >= pixels) continue;
        rtsm::fold_pixel(rgb + 3 * (size_t)a * k, k, accum + 3 * q, moments + 2 * q);
        counts[q] += (int32_t)k;
    }
    return 0;
}

// rts_normalise
int sampler_normalise_host(uint64_t pixels, uint32_t e0, const float* accum, const float* moments, const int32_t* counts,
                           float* out_accum, float* out_moments) {
    for (size_t i = 0; i < pixels; i++) {
        if (counts[i] == (int32_t)e0) {
            std::memcpy(out_accum + 3 * i, accum + 3 * i, 12);
            std::memcpy(out_moments + 2 * i, moments + 2 * i, 8);
        } else {
            rtsm::normalise_pixel(accum + 3 * i, moments + 2 * i, counts[i], (float)e0, out_accum + 3 * i, out_moments + 2 * i);
        }
    }
    return 0;
}

}  // extern "C"

#ifdef SAMPLER_HOST_MAIN
int main() {
    const uint32_t W = 37, R = 12, Hs = 4, k = 3, e0 = 4;
    const size_t n = (size_t)W * R;
    std::vector<float> acc(3 * n), mom(2 * n), err(n), oa(3 * n), om(2 * n);
    std::vector<int32_t> cnt(n, (int32_t)e0);
    std::vector<uint32_t> active(n), sc(R / Hs);
    uint32_t x = 12345u;
    auto rnd = [&] { x = x * 1664525u + 1013904223u; return (float)(x >> 8) / 16777216.0f; };
    for (size_t i = 0; i < n; i++) {
        const float y = rnd() * 3.0f, s = (i % 3) ? rnd() : 0.0f;
        acc[3 * i] = acc[3 * i + 1] = acc[3 * i + 2] = y * (float)e0 / 3.0f;
        mom[2 * i] = y * (float)e0;
        mom[2 * i + 1] = (y * y + s * s) * (float)e0;
    }
    // a few subnormal, huge and non-finite sums at pixels of their own (the classes of tests/_extreme_planes.py), and below some
    // such samples: whatever the planes hold, no line reads or writes outside its buffer
    const float special[] = {1e-45f, -1e-45f, 5.9e-39f, 1.1754942e-38f, -0.0f, 1e-30f, 1.9e19f, 3e38f, -3.4028235e38f,
                             __builtin_inff(), -__builtin_inff(), __builtin_nanf(""), -__builtin_nanf(""), -1.5f};
    const size_t n_special = sizeof special / sizeof *special;
    for (size_t j = 0; j < n_special; j++) {
        const size_t i = (31 * j + 7) % n;
        if (j % 3 == 2)
            acc[3 * i + j % 3] = special[j];
        else
            mom[2 * i + j % 3] = special[j];
    }
    uint64_t total = 0;
    for (uint32_t dilate = 0; dilate < 2; dilate++) {
        if (sampler_select_host(W, R, Hs, dilate, 0.05f, 0.015625f, mom.data(), cnt.data(), err.data(), active.data(), sc.data())) return 1;
        const uint32_t P = Hs * W;
        for (uint32_t s = 0; s < R / Hs; s++) {
            const uint32_t na = sc[s];
            std::vector<uint8_t> rays((size_t)P * k * 32, 7), out((size_t)na * k * 32 + 1);
            sampler_gather_host(na, k, P, active.data() + (size_t)s * P, rays.data(), out.data());
            std::vector<float> rgb((size_t)na * k * 3);
            for (float& v : rgb) v = rnd();
            for (size_t j = 0; j < n_special && !rgb.empty(); j++) rgb[(13 * j + s) % rgb.size()] = special[j];
            sampler_fold_host(na, k, P, active.data() + (size_t)s * P, rgb.data(), acc.data() + 3 * (size_t)s * P,
                              mom.data() + 2 * (size_t)s * P, cnt.data() + (size_t)s * P);
            total += na;
        }
        sampler_normalise_host(n, e0, acc.data(), mom.data(), cnt.data(), oa.data(), om.data());
    }
    std::printf("%llu pixels sampled\n", (unsigned long long)total);
    return total ? 0 : 1;
}
#endif
