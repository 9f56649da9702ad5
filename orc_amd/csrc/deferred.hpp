// deferred.hpp — pinned host memory with an explicit lifetime (DevBuf's counterpart), and a record the device sends there behind a launch
// for the host to look at one step later.
#pragma once
#include "common.hpp"

namespace orc {

template <class T>
struct PinnedBuf {
    T *p = nullptr;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    PinnedBuf(PinnedBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; o.p = nullptr; }
        return *this;
    }
    ~PinnedBuf() { release(); }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
    }
    int alloc(size_t count) {
        release();
        ORC_HIP(hipHostMalloc((void **)&p, count * sizeof(T), hipHostMallocDefault));
        return ORC_OK;
    }
};

// copy() pieces of a record into `host` behind the launch that wrote them, mark() it, and wait() for it before reading: by then the
// step's last synchronisation has long completed the copies.
template <class T>
struct Deferred {
    PinnedBuf<T> host;
    hipEvent_t landed = nullptr;
    bool pending = false;  // host is on its way
    Deferred() = default;
    Deferred(const Deferred &) = delete;
    Deferred &operator=(const Deferred &) = delete;
    Deferred &operator=(Deferred &&o) noexcept {
        if (this != &o) { release(); host = std::move(o.host); landed = o.landed; pending = o.pending; o.landed = nullptr; o.pending = false; }
        return *this;
    }
    ~Deferred() { release(); }
    // the buffer of `len` elements and the event, or neither
    int create(size_t len, const char *what) {
        release();
        ORC_TRY(host.alloc(len));
        if (hipEventCreateWithFlags(&landed, hipEventDisableTiming) != hipSuccess) {
            host.release();
            return set_error(ORC_ERR_HIP, "%s: hipEventCreate failed", what);
        }
        return ORC_OK;
    }
    int copy(size_t at, const void *dev, size_t bytes) {
        ORC_HIP(hipMemcpyAsync(host.p + at, dev, bytes, hipMemcpyDeviceToHost, ctx().stream));
        return ORC_OK;
    }
    int mark() {
        ORC_HIP(hipEventRecord(landed, ctx().stream));
        pending = true;
        return ORC_OK;
    }
    // *had: a record was on its way and `host` now holds it
    int wait(bool *had) {
        *had = pending;
        if (!pending) return ORC_OK;
        ORC_HIP(hipEventSynchronize(landed));
        pending = false;
        return ORC_OK;
    }
    void release() {
        if (landed) { (void)hipEventSynchronize(landed); (void)hipEventDestroy(landed); }
        landed = nullptr; pending = false;
        host.release();
    }
};

}  // namespace orc
