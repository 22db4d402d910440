// CPU harness around the PRODUCT's device-resource owners (ray_tracer_s8_amd/csrc/rt_device.h), for tests/test_device_host.py.
// A link seam, not a mock layer: this file DEFINES the HIP functions the header calls, as counting fakes, so the header is compiled
// exactly as the library compiles it and the program links and runs without the runtime.  The fakes
//   - keep the sets of live allocations, events and streams; a double free or an unknown handle is a VIOLATION: the stand-alone
//     program aborts on it, the library form records it (dh_violation) and leaves the handle alone, so that the test fails
//     and the next one still runs;
//   - log every call as one letter (dh_log), in order;
//   - fail the k-th fallible call (dh_fail_at; allocation, creation, wait, copy, record: everything but the releases).
// With -DDEVICE_HOST_MAIN it is a stand-alone program (run under -fsanitize=address,undefined by the test).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "rt_device.h"

namespace {
std::map<void*, size_t> g_mem;      // live allocations and their sizes
std::set<void*> g_events, g_streams;
std::string g_log;
long g_calls = 0, g_fail_at = -1;

std::string g_violation;
void violation(const char* what) {
    fprintf(stderr, "device_host: %s\n", what);
    g_violation = what;
#ifdef DEVICE_HOST_MAIN
    abort();
#endif
}
// one fallible call: logged, counted, and failed when its number is up
bool refused(char letter) {
    g_log += letter;
    return g_calls++ == g_fail_at;
}
template <class H>
H new_handle(std::set<void*>& live) {
    void* h = malloc(1);
    live.insert(h);
    return (H)h;
}
void drop_handle(std::set<void*>& live, void* h, const char* what) {
    if (live.erase(h)) free(h);
    else violation(what);
}
}  // namespace

// ---- the HIP functions rt_device.h calls
hipError_t hipMalloc(void** p, size_t bytes) {                                   // M
    if (refused('M')) return hipErrorOutOfMemory;
    *p = bytes ? malloc(bytes) : nullptr;                                        // (the runtime gives no memory for no bytes)
    if (*p) g_mem[*p] = bytes;
    return hipSuccess;
}
hipError_t hipFree(void* p) {                                                    // F
    g_log += 'F';
    if (!p) return hipSuccess;
    if (g_mem.erase(p)) free(p);
    else violation("hipFree of a pointer that is not live");
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {      // C
    if (refused('C')) return hipErrorInvalidValue;
    if (kind != hipMemcpyHostToDevice) violation("hipMemcpyAsync: not an upload");
    if (bytes) {
        auto it = g_mem.find(dst);
        if (it != g_mem.end() && it->second >= bytes) memcpy(dst, src, bytes);
        else violation("hipMemcpyAsync beyond its allocation");
    }
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {                    // E
    if (refused('E')) return hipErrorOutOfMemory;
    *e = new_handle<hipEvent_t>(g_events);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {                                       // D
    g_log += 'D';
    drop_handle(g_events, e, "hipEventDestroy of an event that is not live");
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) {                                   // W
    if (refused('W')) return hipErrorInvalidValue;
    if (!g_events.count(e)) violation("hipEventSynchronize on an event that is not live");
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) {                           // R (the header never records: the sequences below do, as
    if (refused('R')) return hipErrorInvalidValue;                               //   the library does between the header's calls)
    if (!g_events.count(e)) violation("hipEventRecord on an event that is not live");
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {                  // S
    if (refused('S')) return hipErrorOutOfMemory;
    *s = new_handle<hipStream_t>(g_streams);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {                                     // X
    g_log += 'X';
    drop_handle(g_streams, s, "hipStreamDestroy of a stream that is not live");
    return hipSuccess;
}

namespace {
using namespace rtdev;
struct Rec16 {
    float v[4];
};
#define TRY(expr)                       \
    do {                                \
        if ((expr) != hipSuccess) return 1; \
    } while (0)

// A sequence shaped like the library's scene upload: the context's two streams, the scene behind a unique_ptr, two timing events,
// uploads of mixed sizes and record types (one empty), the counters; the scene is handed over only at the end.
struct SceneLike {
    DevArray<Rec16> geom, nodes;
    DevArray<float> emis;
    DevArray<uint32_t> big, rank;
    DevArray<unsigned long long> counters;
    GrowBuf ring, stage;
    EventPool events;
};
int upload_like(std::unique_ptr<SceneLike>& out, Stream& st, Stream& cs) {
    Stream a, b;
    TRY(a.create());
    TRY(b.create());
    cs = std::move(b);
    st = std::move(a);
    auto sc = std::make_unique<SceneLike>();
    Event e0, e1;
    TRY(e0.create());
    TRY(e1.create());
    const std::vector<Rec16> geom(37), nodes(5);
    const std::vector<float> emis(111, 1.f);
    const std::vector<uint32_t> none, rank(1, 7u);
    TRY(hipEventRecord(e0.get(), st.get()));
    TRY(sc->geom.upload(geom, st.get()));
    TRY(sc->emis.upload(emis, st.get()));
    TRY(sc->big.upload(none, st.get()));          // an empty array: both calls are made, nothing is held
    TRY(sc->nodes.upload(nodes, st.get()));
    TRY(sc->rank.upload(rank, st.get()));
    TRY(sc->counters.alloc(20));
    TRY(hipEventRecord(e1.get(), st.get()));
    TRY(hipEventSynchronize(e1.get()));
    if (sc->big || !sc->geom || !sc->rank || !sc->counters) return 2;
    out = std::move(sc);
    return 0;
}

// A sequence shaped like a host form on that scene: its staging grows, two leases bracket the copies, a launch takes a ring (grown,
// its event made on first use) and its own pair, which goes to the pending list; a second launch on a larger ring has to wait for the
// first; everything pending is collected.
int host_form_like(SceneLike& sc, hipStream_t st) {
    TRY(sc.stage.grow(4096));
    EventPool::Lease up, down;
    TRY(sc.events.lease(up));
    TRY(sc.events.lease(down));
    TRY(hipEventRecord(up.a(), st));
    for (size_t ring_bytes : {1024u, 8192u}) {
        EventPool::Lease ev;
        TRY(sc.events.lease(ev));
        TRY(sc.ring.grow(ring_bytes));
        if (!sc.ring.done) TRY(sc.ring.done.create(hipEventDisableTiming));
        TRY(hipEventRecord(ev.a(), st));
        TRY(hipEventRecord(ev.b(), st));
        ev.to_pending();
        TRY(hipEventRecord(sc.ring.done.get(), st));
    }
    TRY(hipEventRecord(down.b(), st));
    for (const EventPool::Pair& p : sc.events.pending()) TRY(hipEventSynchronize(p.b));
    sc.events.collected();
    return 0;
}

// both sequences, everything released at scope exit whichever step fails
int run_sequences() {
    Stream st, cs;
    std::unique_ptr<SceneLike> sc;
    int rc = upload_like(sc, st, cs);
    if (rc) return rc;
    if ((rc = host_form_like(*sc, st.get()))) return rc;
    return host_form_like(*sc, st.get());          // (a second call reuses: no creation, no growth)
}

// Moves: the moved-from owner holds nothing, the handle is released once (a second release is a violation).
int moves() {
    DevArray<float> a;
    TRY(a.alloc(8));
    float* pa = a.get();
    DevArray<float> b(std::move(a));
    if (a || a.get() || b.get() != pa) return 10;
    DevArray<float> c;
    TRY(c.alloc(4));
    c = std::move(b);                     // frees c's own, takes b's
    if (b || c.get() != pa || g_mem.size() != 1) return 11;
    c = std::move(c);                     // self-move: still held
    if (c.get() != pa) return 12;
    Event e;
    TRY(e.create());
    Event f(std::move(e));
    if (e || !f || g_events.size() != 1) return 13;
    Stream s;
    TRY(s.create());
    Stream t;
    t = std::move(s);
    if (s || !t || g_streams.size() != 1) return 14;
    GrowBuf g;
    TRY(g.grow(100));
    TRY(g.done.create());
    char* pg = g.data();
    GrowBuf h(std::move(g));
    if (g.data() || g.size() || g.done || h.data() != pg || h.size() != 100 || !h.done) return 15;
    TRY(g.grow(10));                      // the moved-from area is an empty one: it can grow again
    g = std::move(h);
    if (h.data() || h.size() || g.data() != pg || g.size() != 100 || g_mem.size() != 2) return 16;
    EventPool pool;
    {
        EventPool::Lease l1;
        TRY(pool.lease(l1));
        EventPool::Lease l2(std::move(l1));
        if (l1 || !l2) return 17;
        std::vector<EventPool::Lease> v;
        v.push_back(std::move(l2));       // as the tile host form keeps its leases
        if (l2 || !v[0]) return 18;
    }                                     // one return to the pool, not three
    EventPool::Lease again;
    const long before = g_calls;
    TRY(pool.lease(again));
    if (g_calls != before || g_events.size() != 4) return 19;      // (no create call; alive: f, g.done and the pool's one pair)
    return 0;
}
}  // namespace

extern "C" {

void dh_reset(long fail_at) {
    g_log.clear();
    g_calls = 0;
    g_fail_at = fail_at;
}
long dh_calls() { return g_calls; }
const char* dh_violation() { return g_violation.c_str(); }
// a test starts from nothing alive, whatever a failed one before it left behind (its owners are never destroyed)
void dh_forget() {
    for (auto& m : g_mem) free(m.first);
    for (auto* live : {&g_events, &g_streams})
        for (void* h : *live) free(h);
    g_mem.clear();
    g_events.clear();
    g_streams.clear();
    g_violation.clear();
}
const char* dh_log() { return g_log.c_str(); }
void dh_live(uint64_t* out3) {
    out3[0] = g_mem.size();
    out3[1] = g_events.size();
    out3[2] = g_streams.size();
}
int dh_run_sequences() { return run_sequences(); }
int dh_moves() { return moves(); }

// ---- GrowBuf behind a handle
void* dh_grow_new() { return new GrowBuf; }
void dh_grow_free(void* g) { delete (GrowBuf*)g; }
int dh_grow(void* g, uint64_t bytes) { return (int)((GrowBuf*)g)->grow(bytes); }
int dh_grow_make_done(void* g) { return (int)((GrowBuf*)g)->done.create(hipEventDisableTiming); }
uint64_t dh_grow_size(const void* g) { return ((const GrowBuf*)g)->size(); }
uint64_t dh_grow_data(const void* g) { return (uint64_t)(uintptr_t)((const GrowBuf*)g)->data(); }

// ---- EventPool and its leases behind handles
void* dh_pool_new() { return new EventPool; }
void dh_pool_free(void* p) { delete (EventPool*)p; }
void* dh_lease(void* p, int* status) {          // NULL when the pool could not make a pair
    auto* l = new EventPool::Lease;
    *status = (int)((EventPool*)p)->lease(*l);
    if (*status == 0) return l;
    const bool empty = !*l && !l->a() && !l->b();
    delete l;
    if (!empty) *status = -1;                   // (a failed lease holds nothing)
    return nullptr;
}
void dh_lease_events(const void* l, uint64_t* out2) {
    out2[0] = (uint64_t)(uintptr_t)((const EventPool::Lease*)l)->a();
    out2[1] = (uint64_t)(uintptr_t)((const EventPool::Lease*)l)->b();
}
void dh_lease_drop(void* l) { delete (EventPool::Lease*)l; }
void dh_lease_to_pending(void* l) { ((EventPool::Lease*)l)->to_pending(); }
uint64_t dh_pool_pending(const void* p, uint64_t* out, uint64_t room) {      // pairs as (a, b), at most `room` of them
    const auto& v = ((const EventPool*)p)->pending();
    for (size_t i = 0; i < v.size() && i < room; i++) {
        out[2 * i] = (uint64_t)(uintptr_t)v[i].a;
        out[2 * i + 1] = (uint64_t)(uintptr_t)v[i].b;
    }
    return v.size();
}
void dh_pool_collected(void* p) { ((EventPool*)p)->collected(); }

}  // extern "C"

#ifdef DEVICE_HOST_MAIN
// Every sequence, with every call of it failing in turn, in one process: for the sanitizers.
int main() {
    auto clean = [](const char* what) {
        if (!g_mem.empty() || !g_events.empty() || !g_streams.empty()) {
            printf("%s: %zu allocations, %zu events, %zu streams left\n", what, g_mem.size(), g_events.size(), g_streams.size());
            exit(1);
        }
    };
    dh_reset(-1);
    if (run_sequences() != 0) return printf("clean run failed\n"), 1;
    clean("clean run");
    const long n = g_calls;
    for (long k = 0; k < n; k++) {
        dh_reset(k);
        if (run_sequences() == 0) return printf("call %ld failed and the run did not\n", k), 1;
        clean("failed run");
    }
    dh_reset(-1);
    if (int rc = moves()) return printf("moves: %d\n", rc), 1;
    clean("moves");
    printf("DEVICE_HOST_OK %ld calls\n", n);
    return 0;
}
#endif
