// vdb_bin.cpp -- the binary flat index (include/vdb_flat.h "Binary vectors"): packed rows in HBM at a stride of
// whole 64-byte chunks with their popcounts, ids, id ranks and live bitmap, the id -> row map on the host (which keeps NO copy of
// the rows), and the batch search that runs kernels_bin.hip: the queries widened once, one workgroup per (row segment, query
// tile) under a threshold all of them share, then one per query to merge.
//
// What the kernels may assume is checked HERE: dim is a multiple of 8 within the range; every row and query has the index's
// dimension and is zero-padded to ld bytes; the store is not empty when a search is launched; every k is at most 1024 and at most
// the stride of the device lists; a launch's (segment, query tile) pairs are fewer than 2^31, its partial lists fit their
// workspace and its shared thresholds are open when the score kernel starts.
#include "kernels_bin.h"
#include "vdb_index.h"
#include "vdb_meta.h"

using namespace vdbi;

struct vdb_bin_index {
    int metric = 0, device = 0;
    Stream stream;                                                  // declared first: destroyed after every buffer below
    std::mutex mu;                                                  // searches share the workspace: one at a time
    uint32_t dim = 0, ld = 0;                                       // bits; bytes between two rows.  Fixed by the first add
    // the rows, append order; an overwritten or removed row stays (dead): nothing reclaims it
    std::vector<uint64_t> ids;
    std::vector<uint32_t> live;
    std::unordered_map<uint64_t, uint32_t> row_of;                  // live ids only
    bool dirty = false;
    size_t up_rows = 0;                                             // what d_ids already holds
    DevBuf<uint8_t> d_rows;                                         // [cap_rows][ld]
    DevBuf<int32_t> d_nx;
    size_t cap_rows = 0;
    DevBuf<uint64_t> d_ids, d_sorted;
    DevBuf<uint32_t> d_live, d_rank, d_flags;                       // d_flags: [2..3] the 64-bit key counter
    // the workspace of a search
    DevBuf<uint8_t> d_q, d_qw;
    DevBuf<int32_t> d_nq;
    DevBuf<uint32_t> d_ks, d_out_counts, d_part_cnt, d_gthr;
    DevBuf<uint64_t> d_mask, d_out_ids, d_part;
    DevBuf<float> d_out_dists;
    uint64_t last_segs = 0, last_groups = 0, last_keys = 0;

    static constexpr size_t PART_CAP = 256u << 20;                  // bytes of partial lists of one launch (one query tile always runs)
};

namespace {

// `host` [0, n) on the device: the tail behind `have` when the buffer is large enough, everything into a larger one otherwise
template <typename T> int upload_tail(DevBuf<T>& d, const std::vector<T>& host, size_t have, hipStream_t s) {
    if (host.size() > d.n) {
        HIP_TRY(d.alloc(std::max<size_t>(host.size() + host.size() / 2, 1024)));
        have = 0;
    }
    if (host.size() > have) HIP_TRY(hipMemcpyAsync(d.p + have, host.data() + have, (host.size() - have) * sizeof(T), hipMemcpyHostToDevice, s));
    return VDB_OK;
}

// room for `need` rows of ld bytes: a larger block takes the stored rows and popcounts over, device to device
int grow(vdb_bin_index* h, size_t need, uint32_t ld, hipStream_t s) {
    if (need <= h->cap_rows) return VDB_OK;
    const size_t cap = std::max<size_t>(need + need / 2, 1024), have = h->ids.size();
    DevBuf<uint8_t> rows;
    DevBuf<int32_t> nx;
    HIP_TRY(rows.alloc(cap * ld));
    HIP_TRY(nx.alloc(cap));
    if (have) {
        HIP_TRY(hipMemcpyAsync(rows.p, h->d_rows.p, have * ld, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(nx.p, h->d_nx.p, have * 4, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    h->d_rows = std::move(rows);
    h->d_nx = std::move(nx);
    h->cap_rows = cap;
    return VDB_OK;
}

void kill_row(vdb_bin_index* h, uint32_t row) {
    h->live[row >> 5] &= ~(1u << (row & 31));
    h->dirty = true;
}

int check_dim(size_t dim) {
    if (dim < 8 || dim > vdb::BIN_MAX_DIM || dim % 8)
        return fail(VDB_ERR_INVALID_ARGUMENT, "dimension %zu: a binary row has 8 to %u bits, a multiple of 8", dim, vdb::BIN_MAX_DIM);
    return VDB_OK;
}

// The device sees ids, live bits and id ranks as the host has them.  The caller holds mu.
int flush_locked(vdb_bin_index* h) {
    if (!h->dirty) return VDB_OK;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const uint32_t n_rows = (uint32_t)h->ids.size();
    int rc;
    if (h->d_ids.n < h->ids.size()) h->up_rows = 0;
    if ((rc = upload_tail(h->d_ids, h->ids, h->up_rows, s)) || (rc = upload_tail(h->d_live, h->live, 0, s))) return rc;
    // (distance, id) order needs ids in 32 bits of the key: the rank of each live row's id among the live ids
    std::vector<std::pair<uint64_t, uint32_t>> by_id;
    by_id.reserve(h->row_of.size());
    for (const auto& kv : h->row_of) by_id.push_back(kv);
    std::sort(by_id.begin(), by_id.end());
    std::vector<uint32_t> rank(n_rows, 0);
    std::vector<uint64_t> sorted(by_id.size());
    for (size_t r = 0; r < by_id.size(); ++r) { sorted[r] = by_id[r].first; rank[by_id[r].second] = (uint32_t)r; }
    sorted.push_back(0);                                            // (never empty: upload_tail allocates)
    if ((rc = upload_tail(h->d_rank, rank, 0, s)) || (rc = upload_tail(h->d_sorted, sorted, 0, s))) return rc;
    HIP_TRY(hipStreamSynchronize(s));                               // (rank and sorted are read by the copies until here)
    h->up_rows = h->ids.size();
    h->dirty = false;
    return VDB_OK;
}

int search(vdb_bin_index* h, const uint8_t* queries, size_t nq, size_t dim, const size_t* ks, size_t k, const MaskSrc& mask, size_t kstride,
           uint64_t* out_ids, float* out_dists, size_t* out_counts) {
    if (!h) return fail(VDB_ERR_INVALID_ARGUMENT, "null handle");
    if (nq && (!queries || !out_counts)) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (nq >= (1ull << 31)) return fail(VDB_ERR_INVALID_ARGUMENT, "too many queries");
    Batch b;
    b.nq = nq; b.ks = ks; b.k = k; b.kstride = kstride; b.ids = out_ids; b.dists = out_dists; b.counts = out_counts;
    size_t kmax = 0;
    int rc;
    if ((rc = batch_shape(b, &kmax))) return rc;
    if (kmax > vdb::BIN_MAX_K) return fail(VDB_ERR_INVALID_ARGUMENT, "k = %zu: a binary search returns at most %u results", kmax, vdb::BIN_MAX_K);
    if (nq == 0) return VDB_OK;
    std::lock_guard<std::mutex> g(h->mu);
    if (h->dim && dim != h->dim) return fail_dim(h->dim, dim);
    if ((rc = flush_locked(h))) return rc;
    h->last_segs = h->last_groups = h->last_keys = 0;
    if (h->row_of.empty() || kmax == 0) {                           // nothing can be a candidate
        for (size_t i = 0; i < nq; ++i) out_counts[i] = 0;
        return VDB_OK;
    }
    // the padded packed image of the batch and its popcounts
    const uint32_t ld = h->ld;
    const size_t bytes = dim / 8;
    std::vector<uint8_t> img(nq * (size_t)ld, 0);
    std::vector<int32_t> qn(nq);
    std::vector<uint32_t> kq(nq);
    for (size_t i = 0; i < nq; ++i) {
        int32_t sum = 0;
        for (size_t j = 0; j < bytes; ++j) {
            const uint8_t e = queries[i * bytes + j];
            img[i * ld + j] = e;
            sum += __builtin_popcount(e);
        }
        qn[i] = sum;
        kq[i] = (uint32_t)(ks ? ks[i] : k);
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    Drain drain{s};                                                 // img, qn and kq are read by their copies
    const uint32_t n_rows = (uint32_t)h->ids.size();
    if ((rc = upload_tail(h->d_q, img, 0, s)) || (rc = upload_tail(h->d_nq, qn, 0, s)) || (rc = upload_tail(h->d_ks, kq, 0, s))) return rc;
    if ((rc = h->d_qw.ensure(nq * (size_t)ld * 8))) return rc;
    vdb::launch_bin_widen(h->d_q, ld, nq, h->d_qw, s);
    const uint64_t* d_mask = nullptr;
    if ((rc = stage_mask(h->d_mask, mask, s, &d_mask))) return rc;
    if ((rc = h->d_out_ids.ensure(nq * kmax)) || (rc = h->d_out_dists.ensure(nq * kmax)) || (rc = h->d_out_counts.ensure(nq)) ||
        (rc = h->d_flags.ensure(4)))
        return rc;
    vdb::BinSearchParams p{};
    p.rows = h->d_rows; p.ld = ld; p.n_rows = n_rows; p.nx = h->d_nx;
    p.live = h->d_live; p.row_ids = h->d_ids; p.rank = h->d_rank; p.sorted_ids = h->d_sorted;
    p.qw = h->d_qw; p.nq = h->d_nq; p.ks = h->d_ks; p.metric = h->metric;
    p.id_mask = d_mask; p.mask_bits = mask.bits;
    p.seg_rows = vdb::BIN_SEG_ROWS; p.segs = (n_rows + vdb::BIN_SEG_ROWS - 1) / vdb::BIN_SEG_ROWS;
    p.qt = vdb::bin_query_tile((uint32_t)kmax); p.cap = vdb::bin_select_cap((uint32_t)kmax);
    p.out_ids = h->d_out_ids; p.out_dists = h->d_out_dists; p.out_counts = h->d_out_counts; p.kout = (uint32_t)kmax;
    p.counters = reinterpret_cast<unsigned long long*>(h->d_flags.p + 2);
    // a launch: whole query tiles, as many as the partial lists' cap and the grid allow, at least one
    const size_t per_query = (size_t)p.segs * kmax;
    size_t step = std::max<size_t>(vdb_bin_index::PART_CAP / (8 * per_query) / p.qt, 1);
    step = std::min<size_t>(step, std::max<size_t>(((1ull << 31) - 1) / p.segs, 1)) * p.qt;
    step = std::min(step, (nq + p.qt - 1) / p.qt * p.qt);
    if ((rc = h->d_part.ensure(step * per_query)) || (rc = h->d_part_cnt.ensure(step * p.segs)) || (rc = h->d_gthr.ensure(step))) return rc;
    vdb::launch_bin_fill(h->d_flags, 4, 0, s);
    for (size_t a = 0; a < nq; a += step) {
        p.q0 = (uint32_t)a; p.n_q = (uint32_t)std::min(step, nq - a);
        p.part = h->d_part; p.part_cnt = h->d_part_cnt; p.gthr = h->d_gthr;
        vdb::launch_bin_fill(h->d_gthr, p.n_q, vdb::BIN_OPEN, s);   // the launch's thresholds: nothing proven yet
        vdb::launch_bin_score(p, s);
        vdb::launch_bin_merge(p, s);
        h->last_groups += (uint64_t)p.segs * ((p.n_q + p.qt - 1) / p.qt);
    }
    HIP_TRY(hipGetLastError());
    uint32_t flags[4] = {0};
    HIP_TRY(hipMemcpyAsync(flags, h->d_flags, sizeof(flags), hipMemcpyDeviceToHost, s));
    Lists d;
    d.ids = h->d_out_ids; d.dists = h->d_out_dists; d.counts = h->d_out_counts; d.stride = kmax;
    if ((rc = copy_out(d, b, s))) return rc;                        // synchronises s: flags are here, too
    h->last_segs = p.segs;
    memcpy(&h->last_keys, flags + 2, 8);
    return VDB_OK;
}

}  // namespace

extern "C" {

int vdb_bin_create(int metric, int device, vdb_bin_index** out) {
    return guarded([&]() -> int {
    if (!out) return fail(VDB_ERR_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
    if (metric != VDB_BIN_HAMMING && metric != VDB_BIN_JACCARD) return fail(VDB_ERR_INVALID_ARGUMENT, "metric %d is neither Hamming nor Jaccard", metric);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VDB_ERR_DEVICE, "no HIP device available: this engine has no CPU path");
    if (device < 0 || device >= ndev) return fail(VDB_ERR_INVALID_ARGUMENT, "device %d out of range (%d)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(VDB_ERR_DEVICE, "device %d is %s; the kernels are built for gfx950 only", device, prop.gcnArchName);
    auto h = std::make_unique<vdb_bin_index>();
    h->metric = metric;
    h->device = device;
    int rc;
    if ((rc = h->stream.create(hipStreamNonBlocking))) return rc;
    *out = h.release();
    return VDB_OK;
    });
}

void vdb_bin_destroy(vdb_bin_index* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    delete h;
}

int vdb_bin_add_bulk(vdb_bin_index* h, const uint64_t* ids, const uint8_t* rows, size_t n, size_t dim) {
    return guarded([&]() -> int {
    if (!h || (n && (!ids || !rows))) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return VDB_OK;
    int rc;
    if ((rc = check_dim(dim))) return rc;
    std::lock_guard<std::mutex> g(h->mu);
    if (h->dim && dim != h->dim) return fail_dim(h->dim, dim);
    const size_t have = h->ids.size();
    if (have + (uint64_t)n >= 0xffffffffull) return fail(VDB_ERR_INVALID_ARGUMENT, "the index holds fewer than 2^32 rows (dead rows included)");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t bytes = dim / 8;
    const uint32_t ld = vdbi::round_up((uint32_t)bytes, vdb::BIN_LD_ALIGN);
    if (!h->dim) h->cap_rows = 0;                                   // (a first add that failed may have left a block of another stride)
    if ((rc = grow(h, have + n, ld, s))) return rc;
    // the rows go up padded and are never kept here; their popcounts are computed where they now lie
    std::vector<uint8_t> padded;
    const uint8_t* src = rows;
    if (ld != bytes) {
        padded.assign(n * (size_t)ld, 0);
        for (size_t i = 0; i < n; ++i) memcpy(padded.data() + i * ld, rows + i * bytes, bytes);
        src = padded.data();
    }
    HIP_TRY(hipMemcpyAsync(h->d_rows.p + have * ld, src, n * (size_t)ld, hipMemcpyHostToDevice, s));
    vdb::launch_bin_row_popcounts(h->d_rows, ld, (uint32_t)have, (uint32_t)(have + n), h->d_nx, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));                               // (the caller's rows and `padded` are read until here)
    if (!h->dim) { h->dim = (uint32_t)dim; h->ld = ld; }            // the first rows are in place: only now is the dimension fixed
    for (size_t i = 0; i < n; ++i) {
        auto it = h->row_of.find(ids[i]);
        if (it != h->row_of.end()) kill_row(h, it->second);         // the last vector of an id wins
        const uint32_t row = (uint32_t)h->ids.size();
        h->ids.push_back(ids[i]);
        if ((row >> 5) >= h->live.size()) h->live.push_back(0);
        h->live[row >> 5] |= 1u << (row & 31);
        h->row_of[ids[i]] = row;
    }
    h->dirty = true;
    return VDB_OK;
    });
}

int vdb_bin_remove(vdb_bin_index* h, uint64_t id) {
    return guarded([&]() -> int {
    if (!h) return fail(VDB_ERR_INVALID_ARGUMENT, "null handle");
    std::lock_guard<std::mutex> g(h->mu);
    auto it = h->row_of.find(id);
    if (it == h->row_of.end()) return VDB_OK;
    kill_row(h, it->second);
    h->row_of.erase(it);
    return VDB_OK;
    });
}

size_t vdb_bin_len(const vdb_bin_index* h) { return h ? h->row_of.size() : 0; }

int vdb_bin_flush(vdb_bin_index* h) {
    return guarded([&]() -> int {
    if (!h) return fail(VDB_ERR_INVALID_ARGUMENT, "null handle");
    std::lock_guard<std::mutex> g(h->mu);
    return flush_locked(h);
    });
}

int vdb_bin_search_batch(vdb_bin_index* h, const uint8_t* queries, size_t nq, size_t dim, const size_t* ks, size_t k, const uint64_t* id_mask,
                         size_t mask_bits, size_t kstride, uint64_t* out_ids, float* out_dists, size_t* out_counts) {
    return guarded([&]() -> int {
    int rc;
    if (nq && (rc = check_dim(dim))) return rc;
    MaskSrc m;
    m.host = id_mask; m.bits = id_mask ? mask_bits : 0;
    return search(h, queries, nq, dim, ks, k, m, kstride, out_ids, out_dists, out_counts);
    });
}

int vdb_bin_search_batch_filtered(vdb_bin_index* h, const uint8_t* queries, size_t nq, size_t dim, const size_t* ks, size_t k,
                                  const vdb_meta_mask* mask, size_t kstride, uint64_t* out_ids, float* out_dists, size_t* out_counts) {
    return guarded([&]() -> int {
    if (!h) return fail(VDB_ERR_INVALID_ARGUMENT, "null handle");
    if (!mask) return fail(VDB_ERR_INVALID_ARGUMENT, "null mask");
    if (mask->device != h->device)
        return fail(VDB_ERR_INVALID_ARGUMENT, "the compiled mask lives on device %d, the index on device %d", mask->device, h->device);
    int rc;
    if (nq && (rc = check_dim(dim))) return rc;
    MaskSrc m;
    m.compiled = mask->d_words; m.done = mask->done; m.bits = mask->bits;
    return search(h, queries, nq, dim, ks, k, m, kstride, out_ids, out_dists, out_counts);
    });
}

int vdb_bin_stats(const vdb_bin_index* h, uint64_t out[8]) {
    if (!h || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    out[0] = h->ids.size();
    out[1] = h->ids.size() - h->row_of.size();
    out[2] = h->dim;
    out[3] = h->ld;
    out[4] = h->last_segs;
    out[5] = h->last_groups;
    out[6] = h->last_keys;
    out[7] = ((uint64_t)vdb::BIN_QT << 32) | vdb::BIN_SEG_ROWS;
    return VDB_OK;
}

}  // extern "C"
