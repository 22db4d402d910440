// Test harness (CPU only, built by tests/test_robust_host.py with g++ -ffp-contract=off): the two calls of the robust-film library
// (robust_csrc/rt_robust.h) run with the product's own per-pixel lines (robust_csrc/rt_robust_math.h) over plain arrays.  With
// -DROBUST_HOST_MAIN it is a stand-alone program (its own main) that folds a job in cuts and resolves every K at three counts in
// every mode, over buckets that hold extreme values too, for a sanitizer build.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rt_robust_math.h"

namespace {

struct PixelBuckets {
    const float* at;
    size_t stride;
    float operator()(int k, int c) const { return at[(size_t)k * stride + (size_t)c]; }
};

struct Outputs {
    float* linear;
    float* gini;
    int32_t* kept;
    float* variance;
    float* accum;
    float* moments;
};

template <int K>
void resolve(const float* B, uint32_t N, const rtrm::Call& call, const Outputs& o) {
    for (uint32_t i = 0; i < N; i++) {
        rtrm::Pixel p;
        rtrm::resolve_pixel<K>(call, PixelBuckets{B + 3 * (size_t)i, 3 * (size_t)N}, p);
        for (int c = 0; c < 3; c++) o.linear[3 * (size_t)i + c] = p.r[c], o.accum[3 * (size_t)i + c] = p.accum[c];
        o.gini[i] = p.G;
        o.kept[i] = p.kept;
        o.variance[i] = p.v;
        o.moments[2 * (size_t)i + 0] = p.S1;
        o.moments[2 * (size_t)i + 1] = p.S2;
    }
}

}  // namespace

extern "C" {

// rtr_fold over one strip: records [P][n][3], buckets the strip's part of bucket 0, stride in floats.  Returns 0, or 1 for a K or n
// the library refuses.
int robust_fold_host(const float* records, uint32_t P, uint32_t n, uint32_t first, uint32_t K, float* buckets, uint64_t stride) {
    if (!rtrm::buckets_ok(K) || n == 0 || stride < 3 * (uint64_t)P) return 1;
    for (uint32_t i = 0; i < P; i++)
        rtrm::fold_pixel(records + (size_t)i * n * 3, n, first % K, K, buckets + 3 * (size_t)i, (size_t)stride);
    return 0;
}

// rtr_resolve over N pixels: B [K][N][3].  Every output is written.  Returns 0, or 1 for arguments the library refuses.
int robust_resolve_host(const float* B, uint32_t N, uint32_t K, uint32_t e, uint32_t mode, uint32_t c, float* linear, float* gini,
                        int32_t* kept, float* variance, float* accum, float* moments) {
    if (!rtrm::buckets_ok(K) || e < K || mode > rtrm::MODE_TRIM || (mode == rtrm::MODE_TRIM ? c > (K - 1) / 2 : c != 0)) return 1;
    const rtrm::Call call = rtrm::make_call(K, e, mode, c);
    const Outputs o = {linear, gini, kept, variance, accum, moments};
    switch (K) {
        case 3: resolve<3>(B, N, call, o); break;
        case 5: resolve<5>(B, N, call, o); break;
        case 7: resolve<7>(B, N, call, o); break;
        case 9: resolve<9>(B, N, call, o); break;
        case 11: resolve<11>(B, N, call, o); break;
        case 13: resolve<13>(B, N, call, o); break;
        default: resolve<15>(B, N, call, o); break;
    }
    return 0;
}
}

#ifdef ROBUST_HOST_MAIN
// 37 pixels.  Per K: a job of 4 K + 3 samples folded in one call and in ragged cuts into exactly sized buffers (the two must agree
// byte for byte), resolved at three counts in every mode; then the same with subnormal, huge and non-finite values (the classes of
// tests/_extreme_planes.py) written over the sums: whatever a bucket holds, no line reads or writes outside its buffer, and no
// conversion is undefined.
int main() {
    const uint32_t P = 37;
    uint32_t lcg = 2463534242u;
    auto rnd = [&] { return (float)((lcg = lcg * 1664525u + 1013904223u) >> 8) / 16777216.0f; };
    const float special[] = {1e-45f, -1e-45f, 5.9e-39f, 1.1754942e-38f, -0.0f, 1e-30f, 1.9e19f, 3e38f, 3.4028235e38f, -3.4028235e38f,
                             __builtin_inff(), -__builtin_inff(), __builtin_nanf(""), -__builtin_nanf(""), -1.5f};
    const size_t n_special = sizeof special / sizeof *special;
    unsigned long long resolved = 0;
    for (uint32_t K = 3; K <= 15; K += 2) {
        const uint32_t e = 4 * K + 3;
        std::vector<float> rec((size_t)P * e * 3);
        for (float& v : rec) v = rnd() < 0.05f ? 400.0f * rnd() : rnd();
        std::vector<float> whole((size_t)K * P * 3, 0.0f), cut((size_t)K * P * 3, 0.0f);
        if (robust_fold_host(rec.data(), P, e, 0, K, whole.data(), 3 * P)) return 1;
        const uint32_t cuts[] = {1, 2, K + 5, 4, e};              // lengths; the last takes what is left
        uint32_t b = 0;
        for (uint32_t len : cuts) {
            const uint32_t n = b + len > e ? e - b : len;
            if (n == 0) break;
            std::vector<float> part((size_t)P * n * 3);           // exactly the sub-range's records, pixel major
            for (uint32_t i = 0; i < P; i++)
                for (uint32_t j = 0; j < 3 * n; j++) part[(size_t)i * n * 3 + j] = rec[(size_t)i * e * 3 + 3 * (size_t)b + j];
            if (robust_fold_host(part.data(), P, n, b, K, cut.data(), 3 * P)) return 1;
            b += n;
        }
        if (b != e) return 1;
        for (size_t i = 0; i < whole.size(); i++)
            if (__builtin_bit_cast(uint32_t, whole[i]) != __builtin_bit_cast(uint32_t, cut[i])) {
                std::printf("robust_host: K %u: the cut fold differs at %zu\n", K, i);
                return 2;
            }
        std::vector<float> lin(P * 3), gini(P), var(P), acc(P * 3), mom(P * 2);
        std::vector<int32_t> kept(P);
        for (int pass = 0; pass < 2; pass++) {
            if (pass == 1) {
                for (size_t j = 0; j < n_special; j++) whole[(11 * j + 3) % whole.size()] = special[j];
                for (size_t j = 0; j < n_special && j < P; j++)                               // and in every bucket of a pixel
                    for (uint32_t k = 0; k < K; k++)
                        for (int c = 0; c < 3; c++) whole[((size_t)k * P + (P - 1 - j)) * 3 + c] = special[j];
            }
            for (uint32_t count : {K, K + 1, e})
                for (uint32_t mode = 0; mode < 2; mode++)
                    for (uint32_t c = 0; c <= (mode ? (K - 1) / 2 : 0); c++) {
                        if (robust_resolve_host(whole.data(), P, K, count, mode, c, lin.data(), gini.data(), kept.data(), var.data(),
                                                acc.data(), mom.data()))
                            return 1;
                        for (uint32_t i = 0; i < P; i++) {
                            if (kept[i] < 1 || kept[i] > (int32_t)K || !(kept[i] & 1) || !(gini[i] >= 0.0f && gini[i] <= 1.0f)) {
                                std::printf("robust_host: K %u pixel %u: kept %d, gini %g\n", K, i, kept[i], (double)gini[i]);
                                return 3;
                            }
                            if (mode && kept[i] != (int32_t)(2 * c + 1)) return 3;
                        }
                        resolved += P;
                    }
        }
    }
    std::printf("robust_host: %llu pixels resolved\n", resolved);
    return 0;
}
#endif
