// re_own.h -- the two owners of device and pinned host memory (host code only).  Whatever holds a DevBuf or a Pinned, as a member or as a local,
// frees it by going out of scope; nothing is released by hand.  live_allocations() counts the blocks the two types hold, for leak tests.
#pragma once
#include <hip/hip_runtime_api.h>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <utility>

namespace re {

inline std::atomic<uint64_t> g_live_allocations{ 0 };      // blocks (not bytes) held by DevBuf and Pinned objects of this process
inline uint64_t live_allocations() { return g_live_allocations.load(std::memory_order_relaxed); }

// n elements of device memory.  alloc() remembers the byte counter it booked into (or nullptr: unaccounted), so that release() and the destructor book out of the same one.
template <typename T> struct DevBuf {
    T *p = nullptr; size_t n = 0; uint64_t *acct = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n), acct(o.acct) { o.p = nullptr; o.n = 0; o.acct = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; n = o.n; acct = o.acct; o.p = nullptr; o.n = 0; o.acct = nullptr; }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t alloc(size_t count, uint64_t *account) {
        release();
        if (count == 0) count = 1;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), count * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return e; }
        n = count; acct = account; if (acct) *acct += count * sizeof(T);
        g_live_allocations.fetch_add(1, std::memory_order_relaxed);
        return e;
    }
    void release() {
        if (p) { (void)hipFree(p); if (acct) *acct -= n * sizeof(T); g_live_allocations.fetch_sub(1, std::memory_order_relaxed); }
        p = nullptr; n = 0; acct = nullptr;
    }
};

// One zeroed block of pinned host memory (hipHostMalloc with the given flags); d is the device's address of it when the block is mapped, nullptr otherwise.
struct Pinned {
    void *h = nullptr, *d = nullptr; size_t bytes = 0;
    Pinned() = default;
    Pinned(const Pinned &) = delete;
    Pinned &operator=(const Pinned &) = delete;
    Pinned(Pinned &&o) noexcept : h(o.h), d(o.d), bytes(o.bytes) { o.h = o.d = nullptr; o.bytes = 0; }
    Pinned &operator=(Pinned &&o) noexcept {
        if (this != &o) { release(); h = o.h; d = o.d; bytes = o.bytes; o.h = o.d = nullptr; o.bytes = 0; }
        return *this;
    }
    ~Pinned() { release(); }
    hipError_t alloc(size_t count, unsigned flags) {
        release();
        hipError_t e = hipHostMalloc(&h, count, flags);
        if (e != hipSuccess) { h = nullptr; return e; }
        bytes = count; memset(h, 0, count);
        g_live_allocations.fetch_add(1, std::memory_order_relaxed);
        if ((flags & hipHostMallocMapped) && (e = hipHostGetDevicePointer(&d, h, 0)) != hipSuccess) release();
        return e;
    }
    void release() {
        if (h) { (void)hipHostFree(h); g_live_allocations.fetch_sub(1, std::memory_order_relaxed); }
        h = d = nullptr; bytes = 0;
    }
    template <typename T> T *host(size_t off = 0) const { return reinterpret_cast<T *>(static_cast<char *>(h) + off); }
    template <typename T> T *dev(size_t off = 0) const { return reinterpret_cast<T *>(static_cast<char *>(d) + off); }
};

static_assert(!std::is_copy_constructible<DevBuf<int>>::value && !std::is_copy_assignable<DevBuf<int>>::value, "DevBuf is move-only");
static_assert(std::is_nothrow_move_constructible<DevBuf<int>>::value && std::is_nothrow_move_assignable<DevBuf<int>>::value, "DevBuf moves without throwing");
static_assert(!std::is_copy_constructible<Pinned>::value && !std::is_copy_assignable<Pinned>::value, "Pinned is move-only");
static_assert(std::is_nothrow_move_constructible<Pinned>::value && std::is_nothrow_move_assignable<Pinned>::value, "Pinned moves without throwing");

}  // namespace re
