// rt_private_host.h — what the host files of the private libraries (<name>_csrc/rt_<name>.hip; build.PRIVATE) share: the exception
// boundary, the export macro and the pointer checks their refusals are written with.  Host code only, no state, nothing of any one
// library: a status is an int the caller names.
#pragma once

#include <cstddef>
#include <cstdint>

#define RT_PRIVATE_EXPORT extern "C" __attribute__((visibility("default")))

namespace rtpriv {

// the body's status, or INTERNAL (the library's <PREFIX>_ERR_INTERNAL) if it throws: nothing crosses the C boundary
template <int INTERNAL, class F>
int guarded(const F& body) {
    try {
        return body();
    } catch (...) {
        return INTERNAL;
    }
}

// after a launch: `ok` if it was accepted, `err` (the library's <PREFIX>_ERR_HIP) if not
inline int after_launch(int ok, int err) { return hipGetLastError() == hipSuccess ? ok : err; }

inline bool misaligned(const void* q, uintptr_t to = 4) { return ((uintptr_t)q & (to - 1)) != 0; }

struct Range {
    uintptr_t b, e;
};

// buffer q of n bytes (nothing for a NULL)
inline Range range(const void* q, uint64_t n) { return q ? Range{(uintptr_t)q, (uintptr_t)q + (uintptr_t)n} : Range{0, 0}; }
// two buffers share a byte (an empty one shares none)
inline bool overlap(const Range& a, const Range& b) { return a.b < a.e && b.b < b.e && a.b < b.e && b.b < a.e; }

// two of the buffers overlap
template <size_t N>
bool any_overlap(const Range (&r)[N]) {
    for (size_t i = 0; i < N; i++)
        for (size_t j = i + 1; j < N; j++)
            if (overlap(r[i], r[j])) return true;
    return false;
}

// a buffer of `a` overlaps one of `b`
template <size_t N, size_t M>
bool any_overlap(const Range (&a)[N], const Range (&b)[M]) {
    for (const Range& x : a)
        for (const Range& y : b)
            if (overlap(x, y)) return true;
    return false;
}

}  // namespace rtpriv
