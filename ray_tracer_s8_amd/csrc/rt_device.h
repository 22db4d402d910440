// rt_device.h — owners of the host layer's device resources (rt_api.hip): one hipMalloc, one event, one stream, an area that only
// grows, and the pool of event pairs that time a scene's launches.  Host-only: the runtime's API header and nothing of the kernels,
// so tests/host/device_host.cpp compiles it with g++ against counting fakes of the HIP functions named here.
// Every owner is move-only and releases in its destructor; a moved-from owner releases nothing.  Failure is the runtime's status
// code, never an exception.  THE DEVICE OF A RESOURCE MUST BE CURRENT ON THE THREAD THAT DESTROYS ITS OWNER.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>
#include <vector>

namespace rtdev {

// One handle and the call that releases it: what DevArray, Event and Stream share.
template <class H, class Free>
class Owner {
  protected:
    H h_ = nullptr;

  public:
    Owner() = default;
    Owner(Owner&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Owner& operator=(Owner&& o) noexcept {
        if (this != &o) {
            reset();
            h_ = std::exchange(o.h_, nullptr);
        }
        return *this;
    }
    ~Owner() { reset(); }
    void reset() {
        if (h_) (void)Free()(h_);
        h_ = nullptr;
    }
    H get() const { return h_; }
    H release() { return std::exchange(h_, nullptr); }      // the caller owns the handle now
    explicit operator bool() const { return h_ != nullptr; }
};
struct FreeMem { hipError_t operator()(void* p) const { return hipFree(p); } };
struct FreeEvent { hipError_t operator()(hipEvent_t e) const { return hipEventDestroy(e); } };
struct FreeStream { hipError_t operator()(hipStream_t s) const { return hipStreamDestroy(s); } };

// One hipMalloc of n records of T.  alloc and upload replace what was held; on failure nothing is held.
template <class T>
struct DevArray : Owner<T*, FreeMem> {
    hipError_t alloc(size_t n) {
        this->reset();
        hipError_t e = hipMalloc((void**)&this->h_, n * sizeof(T));
        if (e != hipSuccess) this->h_ = nullptr;
        return e;
    }
    // allocate for v and enqueue its copy on `stream` (v stays alive until the stream has passed it); an empty v makes both calls too
    template <class U>
    hipError_t upload(const std::vector<U>& v, hipStream_t stream) {
        static_assert(sizeof(U) % sizeof(T) == 0, "whole records of T");
        hipError_t e = alloc(v.size() * (sizeof(U) / sizeof(T)));
        return e != hipSuccess ? e : hipMemcpyAsync(this->h_, v.data(), v.size() * sizeof(U), hipMemcpyHostToDevice, stream);
    }
};

struct Event : Owner<hipEvent_t, FreeEvent> {
    // flags: hipEventDefault for a timing event, hipEventDisableTiming for one that only orders streams
    hipError_t create(unsigned flags = hipEventDefault) {
        reset();
        hipError_t e = hipEventCreateWithFlags(&h_, flags);
        if (e != hipSuccess) h_ = nullptr;
        return e;
    }
};

struct Stream : Owner<hipStream_t, FreeStream> {
    hipError_t create(unsigned flags = hipStreamNonBlocking) {
        reset();
        hipError_t e = hipStreamCreateWithFlags(&h_, flags);
        if (e != hipSuccess) h_ = nullptr;
        return e;
    }
};

// A device area that only grows.  `done` is the end of the last launch that used the area: its users create it when they first need it
// and record it after each launch; an area nobody launches on concurrently (a staging buffer) never has one.
class GrowBuf {
    DevArray<char> d_;
    size_t bytes_ = 0;

  public:
    Event done;
    GrowBuf() = default;
    GrowBuf(GrowBuf&& o) noexcept : d_(std::move(o.d_)), bytes_(std::exchange(o.bytes_, 0)), done(std::move(o.done)) {}
    GrowBuf& operator=(GrowBuf&& o) noexcept {
        d_ = std::move(o.d_);
        bytes_ = std::exchange(o.bytes_, 0);
        done = std::move(o.done);
        return *this;
    }
    char* data() const { return d_.get(); }
    size_t size() const { return bytes_; }
    // At least `bytes`: no call when large enough; else wait for `done` (a launch in flight may still use the old area), free, allocate.
    // data() and size() agree at every return: after a failed wait the old area, after a failed allocation none.
    hipError_t grow(size_t bytes) {
        if (bytes_ >= bytes) return hipSuccess;
        if (d_ && done) {
            hipError_t e = hipEventSynchronize(done.get());
            if (e != hipSuccess) return e;
        }
        bytes_ = 0;
        hipError_t e = d_.alloc(bytes);
        if (e == hipSuccess) bytes_ = bytes;
        return e;
    }
    void reset() {
        d_.reset();
        bytes_ = 0;
        done.reset();
    }
};

// The pairs of timing events around a scene's launches.  A pair is leased (reused, else created: both events or neither); the lease
// gives it back when it goes out of scope unless to_pending() handed it to the list of launches not yet collected, whose pairs
// collected() makes free again.  The pool outlives its leases and destroys every event it made.
class EventPool {
  public:
    struct Pair {
        hipEvent_t a = nullptr, b = nullptr;
    };
    class Lease {
        EventPool* pool_ = nullptr;
        Pair ev_;
        friend class EventPool;

      public:
        Lease() = default;
        Lease(Lease&& o) noexcept : pool_(std::exchange(o.pool_, nullptr)), ev_(o.ev_) {}
        ~Lease() { release(); }
        hipEvent_t a() const { return ev_.a; }
        hipEvent_t b() const { return ev_.b; }
        explicit operator bool() const { return pool_ != nullptr; }
        void release() {
            if (pool_) pool_->free_.push_back(ev_);      // (never allocates: lease() reserved a place for every pair made)
            pool_ = nullptr;
        }
        void to_pending() {
            pool_->pending_.push_back(ev_);
            pool_ = nullptr;
        }
    };

    EventPool() = default;
    EventPool(const EventPool&) = delete;
    EventPool& operator=(const EventPool&) = delete;
    ~EventPool() {
        for (auto* list : {&pending_, &free_})
            for (Pair& p : *list) {
                (void)hipEventDestroy(p.a);
                (void)hipEventDestroy(p.b);
            }
    }
    hipError_t lease(Lease& out) {
        out.release();
        if (free_.empty()) {
            Event a, b;
            hipError_t e = a.create();
            if (e != hipSuccess || (e = b.create()) != hipSuccess) return e;
            free_.reserve(made_ + 1);
            made_++;
            free_.push_back(Pair{a.release(), b.release()});
        }
        out.ev_ = free_.back();
        free_.pop_back();
        out.pool_ = this;
        return hipSuccess;
    }
    const std::vector<Pair>& pending() const { return pending_; }
    void collected() {
        free_.insert(free_.end(), pending_.begin(), pending_.end());
        pending_.clear();
    }

  private:
    std::vector<Pair> free_, pending_;
    size_t made_ = 0;
};

}  // namespace rtdev
