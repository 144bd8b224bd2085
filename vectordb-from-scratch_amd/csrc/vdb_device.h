// vdb_device.h -- the owners of everything the host code gets from the HIP runtime: device memory, pinned host memory,
// streams and events.  Allocation and free live HERE and nowhere else in csrc/*.cpp: a handle declares its resources as
// members of these types (streams first, so that they are destroyed last) and frees nothing by hand; a function that builds
// several buffers builds them in locals and move-assigns them into the handle once all have succeeded.  Every type is
// move-only and has exactly one owner.  Also the one HIP_TRY and the one exception guard of the library.
// Depends on the runtime API, vdb_internal.h and the public status codes only (vdb_hnsw.cpp and vdb_shard.cpp include it
// without vdb_index.h).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <exception>
#include <new>

#include "../../include/vdb_flat.h"
#include "vdb_internal.h"

namespace vdbi {

inline int hip_fail(hipError_t e, const char* file, int line, const char* expr) {
    char buf[512];
    snprintf(buf, sizeof(buf), "HIP error %d (%s) at %s:%d: %s", (int)e, hipGetErrorString(e), file, line, expr);
    return vdb_internal::set_error(VDB_ERR_DEVICE, buf);
}

#define HIP_TRY(expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return ::vdbi::hip_fail(e_, __FILE__, __LINE__, #expr);           \
    } while (0)

inline int guard_fail(const char* what) {
    char buf[512];
    snprintf(buf, sizeof(buf), "internal error: %s", what);
    return vdb_internal::set_error(VDB_ERR_DEVICE, buf);
}

// No C++ exception may cross the C ABI (ctypes, a Rust FFI caller: undefined behaviour or abort).  Every extern "C" entry
// point that can allocate runs its body through this.
template <class F> int guarded(F&& body) noexcept {
    try { return body(); }
    catch (const std::bad_alloc&) { return guard_fail("out of host memory"); }
    catch (const std::exception& e) { return guard_fail(e.what()); }
    catch (...) { return guard_fail("unknown C++ exception"); }
}

// Device memory: n elements at p.  Reads as a T* wherever one is expected.
template <typename T> struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    operator T*() const { return p; }
    // Drops the old block and makes one of exactly `count` elements; on failure the buffer is empty.  The raw error: for
    // callers that tolerate a failure or grow by a rule of their own.
    hipError_t alloc(size_t count) {
        release();
        hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e != hipSuccess) p = nullptr;
        else n = count;
        return e;
    }
    // Grow-only; the old contents are NOT carried over.  A large-enough buffer costs a compare.
    int ensure(size_t want) {
        if (want <= n) return VDB_OK;
        HIP_TRY(alloc(std::max(want, n + n / 2)));
        return VDB_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

// Pinned host memory: n elements at h.  Mapped (the default): d is the device's view of the same bytes; else d is null.
// Reads as the HOST pointer wherever a T* is expected.
template <typename T> struct HostBuf {
    T* h = nullptr;
    T* d = nullptr;
    size_t n = 0;
    unsigned flags;
    explicit HostBuf(unsigned flags_ = hipHostMallocMapped) : flags(flags_) {}
    HostBuf(HostBuf&& o) noexcept : h(o.h), d(o.d), n(o.n), flags(o.flags) { o.h = o.d = nullptr; o.n = 0; }
    HostBuf& operator=(HostBuf&& o) noexcept {
        if (this != &o) { release(); h = o.h; d = o.d; n = o.n; flags = o.flags; o.h = o.d = nullptr; o.n = 0; }
        return *this;
    }
    ~HostBuf() { release(); }
    operator T*() const { return h; }
    hipError_t alloc(size_t count) {
        release();
        hipError_t e = hipHostMalloc((void**)&h, count * sizeof(T), flags);
        if (e != hipSuccess) { h = nullptr; return e; }
        if ((flags & hipHostMallocMapped) && (e = hipHostGetDevicePointer((void**)&d, h, 0)) != hipSuccess) { release(); return e; }
        n = count;
        return hipSuccess;
    }
    int ensure(size_t want) {
        if (want <= n) return VDB_OK;
        HIP_TRY(alloc(std::max(want, n + n / 2)));
        return VDB_OK;
    }
    void release() {
        if (h) (void)hipHostFree(h);
        h = d = nullptr;
        n = 0;
    }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
    Stream& operator=(Stream&& o) noexcept {
        if (this != &o) { destroy(); s = o.s; o.s = nullptr; }
        return *this;
    }
    ~Stream() { destroy(); }
    operator hipStream_t() const { return s; }
    int create(unsigned flags) {                    // no-op when already created
        if (s) return VDB_OK;
        HIP_TRY(hipStreamCreateWithFlags(&s, flags));
        return VDB_OK;
    }
    void destroy() {
        if (s) (void)hipStreamDestroy(s);
        s = nullptr;
    }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept {
        if (this != &o) { destroy(); e = o.e; o.e = nullptr; }
        return *this;
    }
    ~Event() { destroy(); }
    operator hipEvent_t() const { return e; }
    int create(unsigned flags) {                    // no-op when already created (the lazily made events)
        if (e) return VDB_OK;
        HIP_TRY(hipEventCreateWithFlags(&e, flags));
        return VDB_OK;
    }
    void destroy() {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
};

}  // namespace vdbi
