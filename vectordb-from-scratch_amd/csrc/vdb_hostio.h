// vdb_hostio.h -- the three steps that surround the device search of every host-pointer batch entry point of the flat index,
// each written ONCE: the check of the batch's shape, the staging of its id mask, and the copy of the device lists into the
// caller's strided arrays.  The plain handle (vdb_flat.cpp, vdb_search.cpp) and the sharded parent (vdb_multi.cpp) call the same
// code, so the two cannot drift apart.
// Depends on vdb_device.h and the public status codes only: no index, no kernel declarations (tests/cpp/hostio_test.cpp
// compiles it alone against fakes of the runtime).  Not part of the C ABI.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vdb_device.h"

namespace vdbi {

// A batch as the caller shaped it: nq queries, k results each (ks[b] where ks is given), and where the answers go -- list b at
// ids[b * kstride], dists[b * kstride] (and codes or scores, where the search has them and the caller wants them), its length in
// counts[b].
struct Batch {
    size_t nq = 0; const size_t* ks = nullptr; size_t k = 0, kstride = 0;
    uint64_t* ids = nullptr; float* dists = nullptr; int32_t* codes = nullptr; size_t* counts = nullptr;
    float* scores = nullptr;
};

// *kmax = the largest k of the batch; refuses a stride below it, then missing output arrays.
inline int batch_shape(const Batch& b, size_t* kmax) {
    size_t m = b.ks ? 0 : b.k;
    for (size_t i = 0; b.ks && i < b.nq; ++i) m = std::max(m, b.ks[i]);
    *kmax = m;
    if (m > b.kstride) {
        char buf[128];
        snprintf(buf, sizeof(buf), "kstride %zu smaller than the largest k %zu", b.kstride, m);
        return vdb_internal::set_error(VDB_ERR_INVALID_ARGUMENT, buf);
    }
    if (m && b.nq && (!b.ids || !b.dists)) return vdb_internal::set_error(VDB_ERR_INVALID_ARGUMENT, "null output");
    return VDB_OK;
}

// An id mask in the one form it came in (at most one pointer is set): `bits` bits in host memory; a compiled mask's words in
// HBM, complete behind `done`; or words already on the device, written on the searching stream.
struct MaskSrc {
    const uint64_t* host = nullptr; size_t bits = 0;
    const uint64_t* compiled = nullptr; hipEvent_t done = nullptr;
    const uint64_t* device = nullptr;
};

// *d_mask = the words to search under on stream s, null without a mask.  A host mask is uploaded into `buf` (grow-only, never
// empty); s waits for a compiled one's event; a device mask is used where it is.
inline int stage_mask(DevBuf<uint64_t>& buf, const MaskSrc& m, hipStream_t s, const uint64_t** d_mask) {
    *d_mask = nullptr;
    if (m.host) {
        const size_t words = (m.bits + 63) / 64;
        int rc = buf.ensure(std::max<size_t>(words, 1));
        if (rc) return rc;
        if (words) HIP_TRY(hipMemcpyAsync(buf.p, m.host, words * 8, hipMemcpyHostToDevice, s));
        *d_mask = buf.p;
    } else if (m.compiled) {
        HIP_TRY(hipStreamWaitEvent(s, m.done, 0));
        *d_mask = m.compiled;
    } else if (m.device) {
        *d_mask = m.device;
    }
    return VDB_OK;
}

// The lists of a finished search, in host-readable memory or on the device: list b at ids[b * stride], counts[b] entries of it
// valid (a count above the stride means the stride).  codes and scores may be null.
struct Lists {
    const uint64_t* ids = nullptr; const float* dists = nullptr; const uint32_t* counts = nullptr; const int32_t* codes = nullptr;
    size_t stride = 0;
    const float* scores = nullptr;
};

// Host arrays to the caller's arrays; no runtime call.  Returns the number of entries written.
inline size_t emit_lists(const Lists& h, const Batch& b) {
    size_t total = 0;
    for (size_t q = 0; q < b.nq; ++q) {
        const size_t kq = b.ks ? b.ks[q] : b.k;
        const size_t c = std::min(std::min<size_t>(h.counts[q], h.stride), kq);   // per-query k: a prefix of the batch-wide result
        b.counts[q] = c;
        total += c;
        for (size_t i = 0; i < c; ++i) {
            b.ids[q * b.kstride + i] = h.ids[q * h.stride + i];
            b.dists[q * b.kstride + i] = h.dists[q * h.stride + i];
            if (h.codes && b.codes) b.codes[q * b.kstride + i] = h.codes[q * h.stride + i];
            if (h.scores && b.scores) b.scores[q * b.kstride + i] = h.scores[q * h.stride + i];
        }
    }
    return total;
}

// Device lists to the caller's arrays: the reads are enqueued on s (none for an empty list), s is synchronised ONCE -- reads the
// caller enqueued on s before are complete then, too -- and emit_lists does the rest.  *total, if given: the entries written.
inline int copy_out(const Lists& d, const Batch& b, hipStream_t s, size_t* total = nullptr) {
    const size_t n = b.nq * d.stride;
    std::vector<uint32_t> cnt(b.nq);
    std::vector<uint64_t> ids(n);
    std::vector<float> ds(n);
    std::vector<int32_t> cs(d.codes ? n : 0);
    std::vector<float> sc(d.scores && b.scores ? n : 0);
    if (b.nq) HIP_TRY(hipMemcpyAsync(cnt.data(), d.counts, b.nq * 4, hipMemcpyDeviceToHost, s));
    if (n) {
        HIP_TRY(hipMemcpyAsync(ids.data(), d.ids, n * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(ds.data(), d.dists, n * 4, hipMemcpyDeviceToHost, s));
        if (!cs.empty()) HIP_TRY(hipMemcpyAsync(cs.data(), d.codes, n * 4, hipMemcpyDeviceToHost, s));
        if (!sc.empty()) HIP_TRY(hipMemcpyAsync(sc.data(), d.scores, n * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    const size_t t = emit_lists(Lists{ids.data(), ds.data(), cnt.data(), cs.empty() ? nullptr : cs.data(), d.stride, sc.empty() ? nullptr : sc.data()}, b);
    if (total) *total = t;
    return VDB_OK;
}

}  // namespace vdbi
