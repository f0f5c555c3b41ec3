// cg_own.h -- the four owners of HIP resources: a device buffer, a pinned host block, an event
// and a stream, each freed by its destructor.  All are movable, not copyable, and empty once
// moved from; leak() forgets the handle without freeing it (cg_dist's stuck abort).  Every
// acquisition and free moves one of four process-wide counts, read by cg_debug_live.
#pragma once

#include <atomic>
#include <cstddef>

#include <hip/hip_runtime.h>

namespace cg {

enum { kLiveDev, kLivePinned, kLiveEvents, kLiveStreams };
inline std::atomic<long long> own_live[4];

// Grow-only block of device (kLiveDev) or pinned host (kLivePinned) memory.
template <int kKind>
struct OwnedBuf {
    void *p = nullptr;
    size_t bytes = 0;
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.leak(); }
    OwnedBuf &operator=(OwnedBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p;
            bytes = o.bytes;
            o.leak();
        }
        return *this;
    }
    ~OwnedBuf() { release(); }
    hipError_t ensure(size_t n) { return n <= bytes ? hipSuccess : grow(n, false); }
    // device memory only: uncached fine-grained, where a stream's waits on memory poll
    hipError_t ensure_uncached(size_t n) { return n <= bytes ? hipSuccess : grow(n, true); }
    void release()
    {
        if (!p) return;
        (void)(kKind == kLiveDev ? hipFree(p) : hipHostFree(p));
        --own_live[kKind];
        leak();
    }
    void leak()
    {
        p = nullptr;
        bytes = 0;
    }

  private:
    hipError_t grow(size_t n, bool uncached)
    {
        release();
        hipError_t e = kKind != kLiveDev ? hipHostMalloc(&p, n, hipHostMallocDefault)
                       : uncached        ? hipExtMallocWithFlags(&p, n, hipDeviceMallocUncached)
                                         : hipMalloc(&p, n);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        bytes = n;
        ++own_live[kKind];
        return e;
    }
};
using DevBuf = OwnedBuf<kLiveDev>;
using PinnedBuf = OwnedBuf<kLivePinned>;

// An event, created on first use.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.leak(); }
    Event &operator=(Event &&o) noexcept
    {
        if (this != &o) {
            destroy();
            e = o.e;
            o.leak();
        }
        return *this;
    }
    ~Event() { destroy(); }
    hipError_t ensure(unsigned flags = hipEventDisableTiming)
    {
        if (e) return hipSuccess;
        hipError_t r = hipEventCreateWithFlags(&e, flags);
        if (r != hipSuccess) {
            e = nullptr;
            return r;
        }
        ++own_live[kLiveEvents];
        return r;
    }
    operator hipEvent_t() const { return e; }
    void leak() { e = nullptr; }

  private:
    void destroy()
    {
        if (!e) return;
        (void)hipEventDestroy(e);
        --own_live[kLiveEvents];
        e = nullptr;
    }
};

// A stream, created on first use; the destructor waits for its work.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : s(o.s) { o.leak(); }
    Stream &operator=(Stream &&o) noexcept
    {
        if (this != &o) {
            destroy();
            s = o.s;
            o.leak();
        }
        return *this;
    }
    ~Stream() { destroy(); }
    hipError_t ensure(unsigned flags) { return s ? hipSuccess : created(hipStreamCreateWithFlags(&s, flags)); }
    hipError_t ensure_priority(unsigned flags, int prio)
    {
        return s ? hipSuccess : created(hipStreamCreateWithPriority(&s, flags, prio));
    }
    operator hipStream_t() const { return s; }
    void leak() { s = nullptr; }

  private:
    hipError_t created(hipError_t r)
    {
        if (r != hipSuccess) s = nullptr;
        else ++own_live[kLiveStreams];
        return r;
    }
    void destroy()
    {
        if (!s) return;
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
        --own_live[kLiveStreams];
        s = nullptr;
    }
};

}  // namespace cg
