// The two memory owners of csrc/re_own.h (DevBuf, Pinned) and their live-allocation counter, without a device and without the HIP runtime library: the five
// runtime functions they call are defined here over malloc, with a switch that makes the next allocation fail.  Prints "ok".
#include "re_own.h"
#include <cstdio>
#include <cstdlib>
#include <set>

static std::set<void *> g_dev, g_host;      // blocks handed out and not yet freed
static int g_frees = 0, g_double_frees = 0;
static bool g_fail_next = false;
static const size_t DEV_OFFSET = 1 << 20;   // "device address" of a mapped block: host address + this

extern "C" hipError_t hipMalloc(void **p, size_t bytes) {
    if (g_fail_next) { g_fail_next = false; *p = reinterpret_cast<void *>(0x1); return hipErrorOutOfMemory; }      // (a failed call may leave anything in *p)
    *p = malloc(bytes); g_dev.insert(*p); return hipSuccess;
}
extern "C" hipError_t hipFree(void *p) { g_frees++; if (!g_dev.erase(p)) { g_double_frees++; return hipErrorInvalidValue; } free(p); return hipSuccess; }
extern "C" hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) {
    if (g_fail_next) { g_fail_next = false; *p = reinterpret_cast<void *>(0x1); return hipErrorOutOfMemory; }
    *p = malloc(bytes); memset(*p, 0xAB, bytes); g_host.insert(*p); return hipSuccess;
}
extern "C" hipError_t hipHostFree(void *p) { g_frees++; if (!g_host.erase(p)) { g_double_frees++; return hipErrorInvalidValue; } free(p); return hipSuccess; }
extern "C" hipError_t hipHostGetDevicePointer(void **d, void *h, unsigned int) { *d = static_cast<char *>(h) + DEV_OFFSET; return hipSuccess; }

#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

using re::DevBuf; using re::Pinned; using re::live_allocations;

int main() {
    uint64_t acct = 0, other = 0;
    {   // alloc books bytes and count; alloc on a full buffer releases first; alloc(0) still gives one element
        DevBuf<uint32_t> a;
        CHECK(a.p == nullptr && a.n == 0 && live_allocations() == 0);
        CHECK(a.alloc(10, &acct) == hipSuccess && a.p && a.n == 10 && acct == 40 && live_allocations() == 1 && g_dev.size() == 1);
        void *first = a.p;
        CHECK(a.alloc(3, &acct) == hipSuccess && a.n == 3 && acct == 12 && live_allocations() == 1 && g_dev.size() == 1 && !g_dev.count(first) && g_frees == 1);
        CHECK(a.alloc(0, &acct) == hipSuccess && a.p && a.n == 1 && acct == 4 && live_allocations() == 1);
        a.release();
        CHECK(a.p == nullptr && a.n == 0 && acct == 0 && live_allocations() == 0 && g_dev.empty());
        a.release();                                                         // (an empty buffer: nothing happens)
        CHECK(acct == 0 && live_allocations() == 0 && g_double_frees == 0);
    }
    {   // a failing alloc leaves the buffer empty and both counters unchanged
        DevBuf<uint64_t> a; const int frees = g_frees;
        g_fail_next = true;
        CHECK(a.alloc(5, &acct) == hipErrorOutOfMemory && a.p == nullptr && a.n == 0 && acct == 0 && live_allocations() == 0);
        CHECK(a.alloc(5, nullptr) == hipSuccess && acct == 0 && live_allocations() == 1);      // unaccounted: counted as a block, booked nowhere
        a.release();
        CHECK(g_frees == frees + 1 && live_allocations() == 0);             // (nothing was freed for the failed call)
    }
    {   // the destructor books out of the counter alloc remembered, not of another one
        { DevBuf<uint8_t> a; CHECK(a.alloc(100, &acct) == hipSuccess); DevBuf<uint8_t> b; CHECK(b.alloc(7, &other) == hipSuccess); CHECK(acct == 100 && other == 7 && live_allocations() == 2); }
        CHECK(acct == 0 && other == 0 && live_allocations() == 0 && g_dev.empty());
    }
    {   // move construction, move assignment onto a full buffer, self-move, std::swap
        DevBuf<uint32_t> a; CHECK(a.alloc(4, &acct) == hipSuccess);
        uint32_t *pa = a.p;
        DevBuf<uint32_t> b(std::move(a));
        CHECK(a.p == nullptr && a.n == 0 && b.p == pa && b.n == 4 && acct == 16 && live_allocations() == 1);
        DevBuf<uint32_t> c; CHECK(c.alloc(8, &other) == hipSuccess && other == 32 && live_allocations() == 2);
        uint32_t *pc = c.p;
        c = std::move(b);                                                    // releases what c held, out of c's counter
        CHECK(c.p == pa && c.n == 4 && b.p == nullptr && other == 0 && acct == 16 && live_allocations() == 1 && !g_dev.count(pc) && g_dev.count(pa));
        DevBuf<uint32_t> &self = c;
        c = std::move(self);
        CHECK(c.p == pa && c.n == 4 && acct == 16 && live_allocations() == 1 && g_dev.count(pa));
        DevBuf<uint32_t> d; CHECK(d.alloc(2, &other) == hipSuccess);
        uint32_t *pd = d.p;
        std::swap(c, d);
        CHECK(c.p == pd && c.n == 2 && d.p == pa && d.n == 4 && acct == 16 && other == 8 && live_allocations() == 2 && g_dev.size() == 2);
        c.release();                                                         // each side still books out of its own counter
        CHECK(other == 0 && acct == 16);
    }
    CHECK(acct == 0 && other == 0 && live_allocations() == 0 && g_dev.empty() && g_double_frees == 0);
    {   // Pinned: mapped and unmapped, zeroed, freed once
        Pinned m; const int frees = g_frees;
        CHECK(m.alloc(64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess && m.h && m.bytes == 64 && m.d == static_cast<char *>(m.h) + DEV_OFFSET && live_allocations() == 1);
        for (size_t i = 0; i < 64; i++) CHECK(m.host<unsigned char>()[i] == 0);
        CHECK(m.host<uint32_t>(8) == reinterpret_cast<uint32_t *>(static_cast<char *>(m.h) + 8) && m.dev<uint32_t>(8) == reinterpret_cast<uint32_t *>(static_cast<char *>(m.d) + 8));
        Pinned u;
        CHECK(u.alloc(16, hipHostMallocDefault) == hipSuccess && u.h && u.d == nullptr && live_allocations() == 2);
        for (size_t i = 0; i < 16; i++) CHECK(u.host<unsigned char>()[i] == 0);
        void *hm = m.h;
        Pinned v(std::move(m));
        CHECK(m.h == nullptr && m.d == nullptr && m.bytes == 0 && v.h == hm && v.bytes == 64 && live_allocations() == 2);
        u = std::move(v);                                                    // frees u's block
        CHECK(u.h == hm && v.h == nullptr && live_allocations() == 1 && g_host.size() == 1 && g_frees == frees + 1);
        CHECK(u.alloc(8, hipHostMallocDefault) == hipSuccess && u.bytes == 8 && u.d == nullptr && live_allocations() == 1 && g_frees == frees + 2);      // alloc on a full block frees first
        g_fail_next = true;
        Pinned w;
        CHECK(w.alloc(8, hipHostMallocMapped) == hipErrorOutOfMemory && w.h == nullptr && w.d == nullptr && w.bytes == 0 && live_allocations() == 1);
    }
    CHECK(live_allocations() == 0 && g_host.empty() && g_dev.empty() && g_double_frees == 0);
    printf("ok\n");
    return 0;
}
