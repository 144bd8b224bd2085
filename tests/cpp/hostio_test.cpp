// The shared steps of the host-pointer batch searches (csrc/vdb_hostio.h: batch_shape, stage_mask, emit_lists / copy_out) against
// fakes of the few runtime calls they make: "device" memory is host memory, hipMemcpyAsync is a memcpy that counts, the stream
// synchronisation and the event wait only count.  No HIP runtime is linked and no GPU touched.  Built with
// -fsanitize=address,undefined by tests/test_hostio_cpu.py: a read or write one element past a list fails the run by itself.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../vectordb-from-scratch_amd/csrc/vdb_hostio.h"

namespace {

std::set<void*> g_dev;
long g_copies = 0, g_syncs = 0, g_waits = 0, g_allocs = 0;
size_t g_last_copy_bytes = 0;
hipEvent_t g_last_event = nullptr;
std::string g_error;
int g_failed = 0;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
    ++g_allocs;
    *p = malloc(bytes ? bytes : 1);                                 // exactly the bytes asked for: ASan sees an overrun
    g_dev.insert(*p);
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    if (!g_dev.erase(p)) return hipErrorInvalidValue;
    free(p);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
    ++g_copies;
    g_last_copy_bytes = bytes;
    memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { ++g_syncs; return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t e, unsigned int) { ++g_waits; g_last_event = e; return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "error"; }
}

namespace vdb_internal {
int set_error(int code, const char* msg) { g_error = msg; return code; }
}  // namespace vdb_internal

using vdbi::Batch;
using vdbi::DevBuf;
using vdbi::Lists;
using vdbi::MaskSrc;

static void test_batch_shape() {
    uint64_t ids[8]; float ds[8]; size_t cnt[4];
    size_t kmax = 99;
    Batch b;
    b.nq = 3; b.k = 2; b.kstride = 2; b.ids = ids; b.dists = ds; b.counts = cnt;
    CHECK(vdbi::batch_shape(b, &kmax) == VDB_OK && kmax == 2);                     // ks null: k
    const size_t ks[3] = {1, 4, 0};
    b.ks = ks; b.k = 100; b.kstride = 4;
    CHECK(vdbi::batch_shape(b, &kmax) == VDB_OK && kmax == 4);                     // ks given: its largest, k ignored
    b.kstride = 3;
    g_error.clear();
    CHECK(vdbi::batch_shape(b, &kmax) == VDB_ERR_INVALID_ARGUMENT && g_error == "kstride 3 smaller than the largest k 4");
    b.ids = nullptr;                                                               // both wrong: the stride is named first
    CHECK(vdbi::batch_shape(b, &kmax) == VDB_ERR_INVALID_ARGUMENT && g_error == "kstride 3 smaller than the largest k 4");
    b.kstride = 4;
    CHECK(vdbi::batch_shape(b, &kmax) == VDB_ERR_INVALID_ARGUMENT && g_error == "null output");
    b.ids = ids; b.dists = nullptr;
    CHECK(vdbi::batch_shape(b, &kmax) == VDB_ERR_INVALID_ARGUMENT && g_error == "null output");
    const size_t zeros[3] = {0, 0, 0};
    b.ks = zeros; b.ids = nullptr; b.dists = nullptr; b.kstride = 0;
    CHECK(vdbi::batch_shape(b, &kmax) == VDB_OK && kmax == 0);                     // kmax == 0: no output array is needed
    b.ks = nullptr; b.k = 5; b.kstride = 5; b.nq = 0;
    CHECK(vdbi::batch_shape(b, &kmax) == VDB_OK && kmax == 5);                     // nq == 0: none either
    b.ks = ks;                                                                     // nq == 0 with ks: nothing of ks is read
    CHECK(vdbi::batch_shape(b, &kmax) == VDB_OK && kmax == 0);
    b.kstride = 4; b.ks = nullptr;
    CHECK(vdbi::batch_shape(b, &kmax) == VDB_ERR_INVALID_ARGUMENT && g_error == "kstride 4 smaller than the largest k 5");
}

static void test_stage_mask() {
    hipStream_t s = (hipStream_t)0x10;
    for (size_t bits : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65}) {
        const size_t words = (bits + 63) / 64;
        std::vector<uint64_t> host(words);                                         // exactly `words` long: a longer read is an overrun
        for (size_t i = 0; i < words; ++i) host[i] = 0x0123456789abcdefull + i;
        uint64_t dummy = 0;
        DevBuf<uint64_t> buf;
        const uint64_t* d = nullptr;
        const long copies = g_copies, syncs = g_syncs, waits = g_waits;
        MaskSrc m;
        m.host = words ? host.data() : &dummy; m.bits = bits;
        CHECK(vdbi::stage_mask(buf, m, s, &d) == VDB_OK);
        CHECK(d == buf.p && d != nullptr && buf.n >= 1 && buf.n >= words);         // never smaller than one word
        CHECK(g_copies - copies == (words ? 1 : 0) && g_syncs == syncs && g_waits == waits);
        if (words) CHECK(g_last_copy_bytes == words * 8 && memcmp(buf.p, host.data(), words * 8) == 0);
    }
    {   // grow-only: a smaller mask after a larger one reuses the buffer
        DevBuf<uint64_t> buf;
        std::vector<uint64_t> host(4, ~0ull);
        const uint64_t* d = nullptr;
        MaskSrc m;
        m.host = host.data(); m.bits = 256;
        CHECK(vdbi::stage_mask(buf, m, s, &d) == VDB_OK && buf.n == 4);
        uint64_t* p = buf.p;
        const long allocs = g_allocs;
        m.bits = 65;
        CHECK(vdbi::stage_mask(buf, m, s, &d) == VDB_OK && buf.p == p && g_allocs == allocs && g_last_copy_bytes == 16);
    }
    {   // a compiled mask: one event wait, no copy, no allocation
        DevBuf<uint64_t> buf;
        uint64_t words[2] = {1, 2};
        const uint64_t* d = nullptr;
        const long copies = g_copies, waits = g_waits, allocs = g_allocs, syncs = g_syncs;
        MaskSrc m;
        m.compiled = words; m.done = (hipEvent_t)0x20; m.bits = 128;
        CHECK(vdbi::stage_mask(buf, m, s, &d) == VDB_OK && d == words);
        CHECK(g_waits - waits == 1 && g_last_event == (hipEvent_t)0x20 && g_copies == copies && g_allocs == allocs && g_syncs == syncs && !buf.p);
    }
    {   // a raw device mask: nothing enqueued; no mask: null
        DevBuf<uint64_t> buf;
        uint64_t words[2] = {1, 2};
        const uint64_t* d = nullptr;
        const long copies = g_copies, waits = g_waits, allocs = g_allocs, syncs = g_syncs;
        MaskSrc m;
        m.device = words; m.bits = 100;
        CHECK(vdbi::stage_mask(buf, m, s, &d) == VDB_OK && d == words);
        d = words;
        CHECK(vdbi::stage_mask(buf, MaskSrc{}, s, &d) == VDB_OK && d == nullptr);
        CHECK(g_waits == waits && g_copies == copies && g_allocs == allocs && g_syncs == syncs && !buf.p);
    }
}

constexpr uint64_t ID_SENTINEL = 0xdeadbeefdeadbeefull;
constexpr float D_SENTINEL = -12345.0f;
constexpr int32_t C_SENTINEL = -77;
constexpr size_t N_SENTINEL = 0xabcdefu;

// One copy-out (through the fakes when `device`, else the pure loop alone) against the expectation written out independently.
static void run_copy_out(size_t nq, size_t stride, size_t kstride, const std::vector<size_t>* ks, size_t k, const std::vector<uint32_t>& counts,
                         bool dev_codes, bool want_codes, bool device) {
    // the "device" lists: exactly nq * stride elements each
    std::vector<uint64_t> li(nq * stride);
    std::vector<float> ld(nq * stride);
    std::vector<int32_t> lc(nq * stride);
    for (size_t i = 0; i < li.size(); ++i) { li[i] = 1000 + i; ld[i] = 0.5f * (float)i; lc[i] = (int32_t)i - 3; }
    std::vector<uint64_t> oi(nq * kstride, ID_SENTINEL);
    std::vector<float> od(nq * kstride, D_SENTINEL);
    std::vector<int32_t> oc(nq * kstride, C_SENTINEL);
    std::vector<size_t> on(nq, N_SENTINEL);
    Batch b;
    b.nq = nq; b.ks = ks ? ks->data() : nullptr; b.k = k; b.kstride = kstride;
    b.ids = oi.data(); b.dists = od.data(); b.codes = want_codes ? oc.data() : nullptr; b.counts = on.data();
    const Lists L{li.data(), ld.data(), counts.data(), dev_codes ? lc.data() : nullptr, stride};
    const long copies = g_copies, syncs = g_syncs;
    size_t total = N_SENTINEL;
    if (device) CHECK(vdbi::copy_out(L, b, (hipStream_t)0x10, &total) == VDB_OK);
    else total = vdbi::emit_lists(L, b);
    if (device) {
        CHECK(g_syncs - syncs == 1);                                               // exactly one synchronisation
        const long lists = nq * stride ? (dev_codes ? 3 : 2) : 0;                  // nothing is enqueued for an empty list
        CHECK(g_copies - copies == (nq ? 1 : 0) + lists);
    } else {
        CHECK(g_syncs == syncs && g_copies == copies);                             // the pure part makes no runtime call
    }
    size_t sum = 0;
    for (size_t q = 0; q < nq; ++q) {
        size_t want = counts[q];
        if (want > stride) want = stride;                                          // a count beyond the stride is clamped to it
        const size_t kq = ks ? (*ks)[q] : k;
        if (want > kq) want = kq;
        CHECK(on[q] == want);
        sum += want;
        for (size_t i = 0; i < kstride; ++i) {
            const size_t o = q * kstride + i;
            if (i < want) {
                CHECK(oi[o] == li[q * stride + i] && od[o] == ld[q * stride + i]);
                CHECK(oc[o] == (dev_codes && want_codes ? lc[q * stride + i] : C_SENTINEL));
            } else {
                CHECK(oi[o] == ID_SENTINEL && od[o] == D_SENTINEL && oc[o] == C_SENTINEL);   // beyond the count: untouched
            }
        }
    }
    CHECK(total == sum);
}

static void test_copy_out() {
    for (int device = 0; device < 2; ++device)
        for (size_t nq : {(size_t)0, (size_t)1, (size_t)3})
            for (size_t stride : {(size_t)0, (size_t)1, (size_t)5})
                for (size_t extra : {(size_t)0, (size_t)3})                           // kstride == the device stride, and larger
                    for (int codes = 0; codes < 4; ++codes) {
                        const size_t kstride = stride + extra;
                        // counts: 0, the full list, more than the stride
                        std::vector<uint32_t> counts(nq);
                        for (size_t q = 0; q < nq; ++q) counts[q] = q == 0 ? (uint32_t)stride : q == 1 ? 0u : (uint32_t)stride + 4;
                        run_copy_out(nq, stride, kstride, nullptr, kstride, counts, codes & 1, codes & 2, device);      // one k, never the limit
                        run_copy_out(nq, stride, kstride, nullptr, stride / 2, counts, codes & 1, codes & 2, device);   // one k below the counts
                        // per-query k: 0, below the count, above the count (as far as the caller's stride allows)
                        std::vector<size_t> ks(nq);
                        for (size_t q = 0; q < nq; ++q) ks[q] = q == 0 ? 0 : q == 1 ? kstride : (stride > 1 ? stride - 1 : 0);
                        for (size_t q = 0; q < nq; ++q) counts[q] = q == 1 ? (uint32_t)(stride / 2) : (uint32_t)stride;
                        run_copy_out(nq, stride, kstride, &ks, 999, counts, codes & 1, codes & 2, device);
                    }
}

// reads the caller enqueued on the stream beforehand are covered by the ONE synchronisation of the copy-out
static void test_copy_out_after_callers_reads() {
    const uint64_t totals_dev[2] = {7, 9};
    uint64_t totals[2] = {0, 0};
    const uint64_t li[2] = {5, 6}; const float ld[2] = {1.0f, 2.0f}; const uint32_t cnt[2] = {1, 1};
    uint64_t oi[2]; float od[2]; size_t on[2];
    hipStream_t s = (hipStream_t)0x10;
    const long syncs = g_syncs, copies = g_copies;
    CHECK(hipMemcpyAsync(totals, totals_dev, sizeof(totals), hipMemcpyDeviceToHost, s) == hipSuccess);
    Batch b;
    b.nq = 2; b.k = b.kstride = 1; b.ids = oi; b.dists = od; b.counts = on;
    CHECK(vdbi::copy_out(Lists{li, ld, cnt, nullptr, 1}, b, s) == VDB_OK);          // (no total asked for)
    CHECK(g_syncs - syncs == 1 && g_copies - copies == 4 && totals[1] == 9 && oi[1] == 6 && on[0] == 1);
}

int main() {
    test_batch_shape();
    test_stage_mask();
    test_copy_out();
    test_copy_out_after_callers_reads();
    CHECK(g_dev.empty());
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("host io ok\n");
    return 0;
}
