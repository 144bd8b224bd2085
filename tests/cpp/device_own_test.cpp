// The owning types of csrc/vdb_device.h against counting fakes of the HIP entry points they use: no HIP runtime is linked and
// no GPU touched (the fakes below ARE hipMalloc & co. of this program).  Built with -fsanitize=address,undefined by
// tests/test_device_own_cpu.py: a double free, a leak at exit or a use after free fails the run even where no check names it.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <utility>

#include "../../vectordb-from-scratch_amd/csrc/vdb_device.h"

namespace {

std::set<void*> g_dev, g_host, g_streams, g_events;      // what is live
long g_calls = 0;                                        // every runtime call made
long g_allocs = 0, g_fail_at = -1;                       // the g_fail_at-th allocation from now (0-based) fails
int g_bad_free = 0;
std::string g_error;
int g_failed = 0;

bool alloc_fails() { return g_allocs++ == g_fail_at; }
void fail_nth(long n) { g_allocs = 0; g_fail_at = n; }
size_t live() { return g_dev.size() + g_host.size(); }

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
    ++g_calls;
    if (alloc_fails()) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    g_dev.insert(*p);
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    ++g_calls;
    if (!g_dev.erase(p)) { ++g_bad_free; return hipErrorInvalidValue; }
    free(p);
    return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) {
    ++g_calls;
    if (alloc_fails()) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    g_host.insert(*p);
    return hipSuccess;
}
hipError_t hipHostFree(void* p) {
    ++g_calls;
    if (!g_host.erase(p)) { ++g_bad_free; return hipErrorInvalidValue; }
    free(p);
    return hipSuccess;
}
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned int) {
    ++g_calls;
    if (!g_host.count(h)) return hipErrorInvalidValue;
    *d = h;
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) {
    ++g_calls;
    if (alloc_fails()) return hipErrorOutOfMemory;
    *s = (hipStream_t)malloc(1);
    g_streams.insert(*s);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
    ++g_calls;
    if (!g_streams.erase(s)) { ++g_bad_free; return hipErrorInvalidValue; }
    free(s);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
    ++g_calls;
    if (alloc_fails()) return hipErrorOutOfMemory;
    *e = (hipEvent_t)malloc(1);
    g_events.insert(*e);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
    ++g_calls;
    if (!g_events.erase(e)) { ++g_bad_free; return hipErrorInvalidValue; }
    free(e);
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
}

namespace vdb_internal {
int set_error(int code, const char* msg) { g_error = msg; return code; }
}  // namespace vdb_internal

using vdbi::DevBuf;
using vdbi::Event;
using vdbi::HostBuf;
using vdbi::Stream;

static void test_scope_and_moves() {
    {
        DevBuf<float> a;
        CHECK(a.alloc(10) == hipSuccess && a.p && a.n == 10 && live() == 1);
        float* pa = a.p;
        DevBuf<float> b(std::move(a));                          // move construction: b owns, a is empty
        CHECK(b.p == pa && b.n == 10 && !a.p && a.n == 0 && live() == 1);
        DevBuf<float> c;
        CHECK(c.alloc(4) == hipSuccess && live() == 2);
        float* pc = c.p;
        c = std::move(b);                                       // move assignment: c's old block is freed exactly once
        CHECK(c.p == pa && c.n == 10 && !b.p && live() == 1 && !g_dev.count(pc) && g_bad_free == 0);
        float* as_ptr = c;                                      // reads as a T*
        CHECK(as_ptr == pa);
        CHECK(c.alloc(3) == hipSuccess && c.n == 3 && live() == 1 && !g_dev.count(pa));     // alloc drops the old block
        c.release(); c.release();
        CHECK(!c.p && c.n == 0 && live() == 0 && g_bad_free == 0);
        Stream s, s2; Event e, e2;
        CHECK(s.create(0) == VDB_OK && e.create(0) == VDB_OK && g_streams.size() == 1 && g_events.size() == 1);
        const hipStream_t hs = s; const hipEvent_t he = e;
        const long calls = g_calls;
        CHECK(s.create(0) == VDB_OK && e.create(0) == VDB_OK && g_calls == calls && (hipStream_t)s == hs && (hipEvent_t)e == he);   // already created: no-op
        CHECK(s2.create(0) == VDB_OK && e2.create(0) == VDB_OK);
        s2 = std::move(s); e2 = std::move(e);
        CHECK((hipStream_t)s2 == hs && !(hipStream_t)s && (hipEvent_t)e2 == he && g_streams.size() == 1 && g_events.size() == 1);
        HostBuf<int> h;
        CHECK(h.alloc(8) == hipSuccess);
        HostBuf<int> h2(std::move(h));
        CHECK(h2.h && h2.d == h2.h && h2.n == 8 && !h.h && !h.d && g_host.size() == 1);
        DevBuf<int> keep;
        CHECK(keep.ensure(5) == VDB_OK);                        // left to the scope's end
    }
    CHECK(live() == 0 && g_streams.empty() && g_events.empty() && g_bad_free == 0);
}

static void test_ensure() {
    {
        DevBuf<int> a;
        CHECK(a.ensure(100) == VDB_OK && a.n == 100);
        long calls = g_calls;
        int* p = a.p;
        CHECK(a.ensure(100) == VDB_OK && a.ensure(1) == VDB_OK && a.ensure(0) == VDB_OK && g_calls == calls && a.p == p);   // want <= n: no runtime call
        CHECK(a.ensure(101) == VDB_OK && a.n == 150 && live() == 1);                    // max(want, n + n / 2)
        CHECK(a.ensure(1000) == VDB_OK && a.n == 1000 && live() == 1);
        HostBuf<char> h;
        CHECK(h.ensure(64) == VDB_OK && h.n == 64);
        calls = g_calls;
        CHECK(h.ensure(64) == VDB_OK && g_calls == calls);
        CHECK(h.ensure(65) == VDB_OK && h.n == 96 && g_host.size() == 1);
    }
    CHECK(live() == 0);
}

static void test_failure_leaves_empty() {
    {
        DevBuf<int> a;
        CHECK(a.alloc(10) == hipSuccess);
        int* old = a.p;
        fail_nth(0);
        CHECK(a.alloc(20) == hipErrorOutOfMemory && !a.p && a.n == 0 && !g_dev.count(old) && live() == 0);
        CHECK(a.ensure(10) == VDB_OK);
        old = a.p;
        fail_nth(0);
        g_error.clear();
        CHECK(a.ensure(11) == VDB_ERR_DEVICE && !a.p && a.n == 0 && !g_dev.count(old) && live() == 0);
        CHECK(g_error.find("HIP error") == 0 && g_error.find("out of memory") != std::string::npos &&
              g_error.find("vdb_device.h:") != std::string::npos && g_error.find("alloc(") != std::string::npos);   // code, string, file:line, expression
        HostBuf<int> h;
        CHECK(h.alloc(4) == hipSuccess);
        fail_nth(0);
        CHECK(h.ensure(5) == VDB_ERR_DEVICE && !h.h && !h.d && h.n == 0 && live() == 0);
        Stream s; Event e;
        fail_nth(0);
        CHECK(s.create(0) == VDB_ERR_DEVICE && !(hipStream_t)s);
        fail_nth(0);
        CHECK(e.create(0) == VDB_ERR_DEVICE && !(hipEvent_t)e);
        fail_nth(-1);
    }
    CHECK(live() == 0 && g_streams.empty() && g_events.empty() && g_bad_free == 0);
}

// the pattern of resize_store and of sync_mirror's full rebuild: eight arrays built in locals, moved into the owner only when
// all eight exist
struct Owner { DevBuf<float> b[8]; size_t cap = 0; };
static int rebuild(Owner* o, size_t cap) {
    DevBuf<float> nb[8];
    for (int i = 0; i < 8; ++i) HIP_TRY(nb[i].alloc(cap));
    for (int i = 0; i < 8; ++i) o->b[i] = std::move(nb[i]);
    o->cap = cap;
    return VDB_OK;
}
static void test_all_or_nothing() {
    {
        Owner o;
        fail_nth(-1);
        CHECK(rebuild(&o, 16) == VDB_OK && live() == 8 && o.cap == 16);
        float* old[8];
        for (int i = 0; i < 8; ++i) old[i] = o.b[i].p;
        for (long k = 0; k < 8; ++k) {
            fail_nth(k);
            CHECK(rebuild(&o, 32) == VDB_ERR_DEVICE);
            CHECK(live() == 8 && o.cap == 16);                  // zero new blocks stay live
            for (int i = 0; i < 8; ++i) CHECK(o.b[i].p == old[i] && o.b[i].n == 16 && g_dev.count(old[i]));   // the old ones untouched
        }
        fail_nth(-1);
        CHECK(rebuild(&o, 32) == VDB_OK && live() == 8 && o.cap == 32);
        for (int i = 0; i < 8; ++i) CHECK(o.b[i].n == 32 && !g_dev.count(old[i]));
    }
    CHECK(live() == 0 && g_bad_free == 0);
}

static void test_host_mapped_and_default() {
    {
        HostBuf<int> m;                                         // mapped is the default
        HostBuf<int> d(hipHostMallocDefault);
        CHECK(m.alloc(4) == hipSuccess && d.alloc(4) == hipSuccess);
        CHECK(m.h && m.d == m.h && d.h && d.d == nullptr);
        int* as_ptr = d;                                        // reads as the host pointer
        CHECK(as_ptr == d.h);
        d = HostBuf<int>(hipHostMallocDefault);                 // assignment from an empty one frees
        CHECK(!d.h && g_host.size() == 1);
    }
    CHECK(live() == 0 && g_bad_free == 0);
}

static void test_guarded() {
    g_error.clear();
    CHECK(vdbi::guarded([]() -> int { throw std::bad_alloc(); }) == VDB_ERR_DEVICE && g_error == "internal error: out of host memory");
    CHECK(vdbi::guarded([]() -> int { return 7; }) == 7);
}

int main() {
    test_scope_and_moves();
    test_ensure();
    test_failure_leaves_empty();
    test_all_or_nothing();
    test_host_mapped_and_default();
    test_guarded();
    CHECK(live() == 0 && g_streams.empty() && g_events.empty() && g_bad_free == 0);
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("device ownership ok\n");
    return 0;
}
