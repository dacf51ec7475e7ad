// hip_host.hpp — the host-side HIP plumbing of the C ABI, stated once for the handle (handle.hpp) and for the multi-GPU group
// (group.cpp, which sees no handle): error reporting, the device guard and the owning buffers.  Private to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>

#include "../../include/pdmpc.h"

extern "C" void pdmpc_set_last_error(const char* msg);  // api.cpp: the string pdmpc_last_error returns

inline int fail(int code, const std::string& msg) {
    pdmpc_set_last_error(msg.c_str());
    return code;
}
// what a host-only part returned, its message in err, as this library reports it
inline int failed(int rc, const std::string& err) { return rc ? fail(rc, err) : PDMPC_OK; }

#define HIPCHK(expr)                                                                                 \
    do {                                                                                             \
        hipError_t e__ = (expr);                                                                     \
        if (e__ != hipSuccess) {                                                                     \
            char buf__[512];                                                                         \
            snprintf(buf__, sizeof buf__, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return fail(PDMPC_ERR_HIP, buf__);                                                       \
        }                                                                                            \
    } while (0)

// The current device belongs to the caller (torch reads it with hipGetDevice: a collective issued after a call into this library
// must not find itself on another GPU).  Every entry point that works on the handle's device switches to it through this guard,
// which puts the caller's device back on every exit path.  Without a device it switches to none: the entry points of a group call
// hipSetDevice per rank themselves, and the caller's device comes back all the same.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    DeviceGuard() : switched(true) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    }
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) {
            err = hipSetDevice(dev);
            switched = err == hipSuccess;
        }
    }
    ~DeviceGuard() {
        if (switched && prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define ON_DEVICE(dev)                 \
    DeviceGuard device_guard__((dev)); \
    HIPCHK(device_guard__.err)

// Buffers own their memory: move-only (a vector of banks moves them when it grows), freed with their owner.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    ~DevBuf() { release(); }
    int ensure(size_t n) {
        const size_t want = std::max(n, (size_t)64);
        return n <= cap ? 0 : ensure_exact(want + want / 2);
    }
    int ensure_exact(size_t n) {  // no head room: the arenas are sized in gigabytes
        if (n <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc((void**)&p, std::max(n, (size_t)64) * sizeof(T));
        if (e != hipSuccess) return (int)e;
        cap = std::max(n, (size_t)64);
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// ... pinned host memory, allocated with the hipHostMalloc flags it was made with (a group's is portable: every rank's device copies
// from it, and mapped where the ranks' kernels write into it)
template <class T>
struct PinnedBuf {
    T* p = nullptr;
    size_t cap = 0;
    unsigned flags = hipHostMallocDefault;
    PinnedBuf() = default;
    explicit PinnedBuf(unsigned malloc_flags) : flags(malloc_flags) {}
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf(PinnedBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)), flags(o.flags) {}
    ~PinnedBuf() { release(); }
    int ensure(size_t n) { return ensure_keep(n, 0); }
    int ensure_keep(size_t n, size_t keep) {  // the first `keep` elements carried over
        if (n <= cap) return 0;
        size_t want = std::max(n, (size_t)64);
        want += want / 2;
        T* q = nullptr;
        hipError_t e = hipHostMalloc((void**)&q, want * sizeof(T), flags);
        if (e != hipSuccess) return (int)e;
        if (p && keep) std::memcpy(q, p, std::min(keep, cap) * sizeof(T));
        if (p) (void)hipHostFree(p);
        p = q;
        cap = want;
        return 0;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};
