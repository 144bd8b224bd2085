// vdb_spv.cpp -- the sparse-VECTOR index (include/vdb_flat.h "Sparse vectors"): CSR rows in append order with a
// live bitmap and the id -> row map on the host, the inverted file rebuilt on the device by the flush after a mutation, and the
// batch search that runs kernels_spv.hip one workgroup per query over a workspace of accumulator slots -- or, on the row-major route
// (vdb_spv_set_route), kernels_spv_rows.hip over the CSR rows themselves, in passes of query tiles.
//
// What the kernels may assume is checked HERE, before anything reaches the device: every stored index is below 2^24 and below
// `vocab`, row_ptr is monotone and ends at the number of stored entries (below 2^32), every query has at most 1024 ascending
// indices.  The scatter and the two list walks have no other guard.  The row-major route adds: every pair's table slot is below
// the pass's count of distinct dimensions, those dimensions are below `vocab` = the size dim_slot is filled to, the table holds
// one row more than that count, and a pass's queries lie inside one chunk of accumulator slots.  The segmented walk
// (vdb_spv_set_segmented) adds: the file in place was built with the segment size the launch names, its segments
// cover the stored rows, its sub-list table has vocab * segments + 1 words, and a launch's partial lists fit their workspace.
#include <limits>

#include "kernels_spv.h"
#include "vdb_index.h"
#include "vdb_meta.h"

using namespace vdbi;

struct vdb_spv_index {
    int device = 0;
    Stream stream;                                                  // declared first: destroyed after every buffer below
    std::mutex mu;                                                  // searches share the workspace: one at a time
    // the rows, append order; an overwritten or removed row stays (dead) until the caller rebuilds the index
    std::vector<uint64_t> ids;
    std::vector<uint32_t> row_ptr{0}, idx, live;
    std::vector<float> val;
    std::unordered_map<uint64_t, uint32_t> row_of;                  // live ids only
    uint64_t live_nnz = 0;
    uint32_t vocab = 0;                                             // 1 + the largest index ever stored
    bool dirty = false;
    size_t up_rows = 0, up_nnz = 0;                                 // what d_ids / d_row_ptr / d_idx / d_val already hold
    DevBuf<uint64_t> d_ids, d_sorted;
    DevBuf<uint32_t> d_row_ptr, d_idx, d_live, d_rank, d_counts, d_list_ptr;
    DevBuf<float> d_val;
    DevBuf<vdb::SpvEntry> d_entries;
    // the workspace of a search
    size_t cap = DEFAULT_CAP;
    DevBuf<float> d_acc, d_qval, d_out_dists;
    DevBuf<uint32_t> d_qoff, d_qidx, d_ks, d_out_counts, d_flags;   // d_flags: [0] status, [2..7] the three 64-bit counters
    DevBuf<uint64_t> d_mask, d_out_ids;
    uint64_t rebuilds = 0, last_walked = 0, last_offered = 0, last_chunks = 0;
    // the row-major route
    int route = 0;                                                  // 0 inverted walk, 1 row-major, 2 by counted work
    std::vector<uint32_t> live_df;                                  // [vocab]: live rows that hold the index (the live list length)
    DevBuf<uint32_t> d_dim_slot, d_table, d_qslot, d_udims;
    bool slots_clean = false;                                       // d_dim_slot is SPV_NO_SLOT up to its size
    uint64_t last_route = 0, last_passes = 0, last_work_inv = 0, last_work_rows = 0;
    // the segmented walk
    uint32_t seg_rows = 0;                                          // what vdb_spv_set_segmented asked for; 0: off
    uint32_t file_segs = 0, file_shift = 0;                         // the file in place: its segments (0: not segmented) of 1 << file_shift rows
    DevBuf<uint32_t> d_sub_ptr, d_tiles, d_part_cnt;
    DevBuf<uint64_t> d_part;
    uint64_t last_seg[4] = {0, 0, 0, 0};

    static constexpr size_t DEFAULT_CAP = 256u << 20;
};

namespace {

constexpr uint64_t MAX_ENTRIES = 0xffffffffull;                     // row_ptr and list_ptr are 32-bit
// Automatic route: row-major when the inverted route's counted work exceeds this many times the row-major route's (DESIGN.md
// 4.20.1 "Measured": where the two routes' times cross, interpolated between two measured workloads).
constexpr double ROUTE_RHO = 0.46;
// A launch of the segmented walk has one workgroup of 1024 threads per segment along x: below 2^32 threads.
constexpr uint64_t SEG_MAX_SEGS = 1u << 21;

// One vector's pairs, sorted ascending by index into (oi, ov); refuses an index at or above 2^24 and a repeated index.
int sorted_pairs(const uint32_t* in_i, const float* in_v, size_t n, const char* what, size_t which, std::vector<uint32_t>& oi,
                 std::vector<float>& ov) {
    std::vector<std::pair<uint32_t, float>> p(n);
    for (size_t j = 0; j < n; ++j) {
        if (in_i[j] >= vdb::SPV_MAX_INDEX) return fail(VDB_ERR_INVALID_ARGUMENT, "%s %zu: index %u is not below 2^24", what, which, in_i[j]);
        p[j] = {in_i[j], in_v[j]};
    }
    std::sort(p.begin(), p.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    for (size_t j = 0; j < n; ++j) {
        if (j && p[j].first == p[j - 1].first) return fail(VDB_ERR_INVALID_ARGUMENT, "%s %zu: index %u occurs twice", what, which, p[j].first);
        oi.push_back(p[j].first);
        ov.push_back(p[j].second);
    }
    return VDB_OK;
}

int check_offsets(const size_t* off, size_t n, const char* what) {
    for (size_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return fail(VDB_ERR_INVALID_ARGUMENT, "%s offsets decrease at %zu", what, i);
    return VDB_OK;
}

void kill_row(vdb_spv_index* h, uint32_t row) {
    h->live[row >> 5] &= ~(1u << (row & 31));
    h->live_nnz -= h->row_ptr[row + 1] - h->row_ptr[row];
    for (uint32_t e = h->row_ptr[row]; e < h->row_ptr[row + 1]; ++e) --h->live_df[h->idx[e]];
    h->dirty = true;
}

// `host` [0, n) on the device: the tail behind `have` when the buffer is large enough, everything into a larger one otherwise
template <typename T> int upload_tail(DevBuf<T>& d, const std::vector<T>& host, size_t have, hipStream_t s) {
    if (host.size() > d.n) {
        HIP_TRY(d.alloc(std::max<size_t>(host.size() + host.size() / 2, 1024)));
        have = 0;
    }
    if (host.size() > have) HIP_TRY(hipMemcpyAsync(d.p + have, host.data() + have, (host.size() - have) * sizeof(T), hipMemcpyHostToDevice, s));
    return VDB_OK;
}

// The device sees the rows as the host has them, and the inverted file is rebuilt from the live ones.  The caller holds mu.
int flush_locked(vdb_spv_index* h) {
    if (!h->dirty) return VDB_OK;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const uint32_t n_rows = (uint32_t)h->ids.size();
    int rc;
    if (h->d_ids.n < h->ids.size() || h->d_row_ptr.n < h->row_ptr.size()) h->up_rows = 0;
    if (h->d_idx.n < h->idx.size() || h->d_val.n < h->val.size()) h->up_nnz = 0;
    if ((rc = upload_tail(h->d_ids, h->ids, h->up_rows, s)) || (rc = upload_tail(h->d_row_ptr, h->row_ptr, h->up_rows, s)) ||
        (rc = upload_tail(h->d_idx, h->idx, h->up_nnz, s)) || (rc = upload_tail(h->d_val, h->val, h->up_nnz, s)) ||
        (rc = upload_tail(h->d_live, h->live, 0, s)))
        return rc;
    // (distance, id) order needs ids in 32 bits of the key: the rank of each live row's id among the live ids
    std::vector<std::pair<uint64_t, uint32_t>> by_id;
    by_id.reserve(h->row_of.size());
    for (const auto& kv : h->row_of) by_id.push_back(kv);
    std::sort(by_id.begin(), by_id.end());
    std::vector<uint32_t> rank(n_rows, 0);
    std::vector<uint64_t> sorted(by_id.size());
    for (size_t r = 0; r < by_id.size(); ++r) { sorted[r] = by_id[r].first; rank[by_id[r].second] = (uint32_t)r; }
    if ((rc = upload_tail(h->d_rank, rank, 0, s)) || (rc = upload_tail(h->d_sorted, sorted, 0, s))) return rc;
    // segmented: at least two segments, and a sub-list table within its cap -- else the file is built as without the option
    uint32_t segs = 0, shift = 0;
    if (h->seg_rows && h->vocab) {
        const uint64_t want = ((uint64_t)n_rows + h->seg_rows - 1) / h->seg_rows;
        if (want >= 2 && want <= SEG_MAX_SEGS && (uint64_t)h->vocab * want + 1 <= vdb::SPV_SEG_TABLE_MAX) {
            segs = (uint32_t)want;
            while ((1u << shift) < h->seg_rows) ++shift;
        }
    }
    const size_t n_keys = segs ? (size_t)h->vocab * segs : h->vocab;
    const size_t n_tiles = (n_keys + vdb::SPV_SEG_SCAN_TILE - 1) / vdb::SPV_SEG_SCAN_TILE;
    if ((rc = h->d_counts.ensure(std::max<size_t>(n_keys, 1))) || (rc = h->d_list_ptr.ensure((size_t)h->vocab + 1)) ||
        (rc = h->d_entries.ensure(std::max<uint64_t>(h->live_nnz, 1))))
        return rc;
    if (segs && ((rc = h->d_sub_ptr.ensure(n_keys + 1)) || (rc = h->d_tiles.ensure(2 * n_tiles + 1)))) return rc;
    vdb::SpvBuildParams p{h->d_row_ptr, h->d_idx, h->d_val, h->d_live, n_rows, h->vocab, h->d_counts, segs ? h->d_sub_ptr : h->d_list_ptr,
                          h->d_entries, segs, shift};
    vdb::launch_spv_fill(h->d_counts, n_keys, 0, s);
    vdb::launch_spv_histogram(p, s);
    if (segs) {                                                     // (n_keys > 0: no store without an index is segmented)
        vdb::launch_spv_seg_scan(h->d_counts, h->d_sub_ptr, (uint32_t)n_keys, h->d_tiles, s);
        vdb::launch_spv_seg_lists(h->d_sub_ptr, segs, h->vocab, h->d_list_ptr, s);
    } else {
        vdb::launch_spv_scan(p, s);
    }
    vdb::launch_spv_scatter(p, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));                               // (rank and sorted are read by the copies until here)
    h->up_rows = h->ids.size();
    h->up_nnz = h->idx.size();
    h->dirty = false;
    h->file_segs = segs;
    h->file_shift = shift;
    ++h->rebuilds;
    return VDB_OK;
}

// The row-major route's plan of a batch: inside every chunk of `slots` queries, tiles of 64 queries are taken into one pass for
// as long as |U| * 64 * tiles * 4 B stays within the table budget (U = the distinct dimensions below vocab the pass's queries
// hold; one tile always fits: at most 64 * 1024 dimensions).  qslot[pair] = the rank of the pair's dimension in its pass's U.
struct RowPass { uint32_t qa, nq, tiles, y0, u_off, n_u; };          // y0: the first query's accumulator slot inside its chunk

void plan_row_passes(const std::vector<uint32_t>& qoff, const std::vector<uint32_t>& qidx, uint32_t vocab, size_t nq, size_t slots,
                     std::vector<RowPass>& passes, std::vector<uint32_t>& qslot, std::vector<uint32_t>& udims) {
    constexpr size_t T = vdb::SPV_ROWS_TILE;
    qslot.assign(qidx.size(), vdb::SPV_NO_SLOT);
    std::vector<uint32_t> U, cand;
    for (size_t c0 = 0; c0 < nq; c0 += slots) {
        const size_t c1 = std::min(c0 + slots, nq);
        for (size_t a = c0; a < c1;) {
            size_t b = a;
            U.clear();
            while (b < c1) {
                const size_t nb = std::min(b + T, c1);
                cand = U;
                for (uint32_t i = qoff[b]; i < qoff[nb]; ++i)
                    if (qidx[i] < vocab) cand.push_back(qidx[i]);
                std::sort(cand.begin(), cand.end());
                cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
                if (b > a && cand.size() * T * ((nb - a + T - 1) / T) * 4 > vdb::SPV_ROWS_TABLE_BYTES) break;
                U.swap(cand);
                b = nb;
            }
            for (uint32_t i = qoff[a]; i < qoff[b]; ++i)
                if (qidx[i] < vocab) qslot[i] = (uint32_t)(std::lower_bound(U.begin(), U.end(), qidx[i]) - U.begin());
            passes.push_back({(uint32_t)a, (uint32_t)(b - a), (uint32_t)((b - a + T - 1) / T), (uint32_t)(a - c0), (uint32_t)udims.size(),
                              (uint32_t)U.size()});
            udims.insert(udims.end(), U.begin(), U.end());
            a = b;
        }
    }
}

int search(vdb_spv_index* h, const size_t* q_offsets, const uint32_t* q_indices, const float* q_values, size_t nq, const size_t* ks,
           size_t k, const MaskSrc& mask, size_t kstride, uint64_t* out_ids, float* out_dists, size_t* out_counts) {
    if (!h) return fail(VDB_ERR_INVALID_ARGUMENT, "null handle");
    if (nq && (!q_offsets || !out_counts)) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (nq >= (1ull << 31)) return fail(VDB_ERR_INVALID_ARGUMENT, "too many queries");
    Batch b;
    b.nq = nq; b.ks = ks; b.k = k; b.kstride = kstride; b.ids = out_ids; b.dists = out_dists; b.counts = out_counts;
    size_t kmax = 0;
    int rc;
    if ((rc = batch_shape(b, &kmax))) return rc;
    if (kmax > vdb::SPV_MAX_K) return fail(VDB_ERR_INVALID_ARGUMENT, "k = %zu: a sparse search returns at most %u results", kmax, vdb::SPV_MAX_K);
    if (nq == 0) return VDB_OK;
    if ((rc = check_offsets(q_offsets, nq, "query"))) return rc;
    const size_t q_nnz = q_offsets[nq] - q_offsets[0];
    if (q_nnz && (!q_indices || !q_values)) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<uint32_t> qoff(nq + 1, 0), qidx, kq(nq);
    std::vector<float> qval;
    qidx.reserve(q_nnz);
    qval.reserve(q_nnz);
    for (size_t i = 0; i < nq; ++i) {
        const size_t len = q_offsets[i + 1] - q_offsets[i];
        if (len > vdb::SPV_MAX_QUERY_NNZ)
            return fail(VDB_ERR_INVALID_ARGUMENT, "query %zu has %zu non-zeros; at most %u are served", i, len, vdb::SPV_MAX_QUERY_NNZ);
        if ((rc = sorted_pairs(q_indices + q_offsets[i], q_values + q_offsets[i], len, "query", i, qidx, qval))) return rc;
        qoff[i + 1] = (uint32_t)qidx.size();
        kq[i] = (uint32_t)(ks ? ks[i] : k);
    }
    std::lock_guard<std::mutex> g(h->mu);
    if ((rc = flush_locked(h))) return rc;
    h->last_walked = h->last_offered = h->last_chunks = 0;
    // the two routes' counted work: the live lengths of the queried lists; the live non-zeros once per tile of 64 queries
    h->last_route = h->last_passes = h->last_work_inv = 0;
    for (uint32_t d : qidx)
        if (d < h->vocab) h->last_work_inv += h->live_df[d];
    h->last_work_rows = h->live_nnz * ((nq + vdb::SPV_ROWS_TILE - 1) / vdb::SPV_ROWS_TILE);
    const bool by_rows = h->route == 1 || (h->route == 2 && (double)h->last_work_inv > ROUTE_RHO * (double)h->last_work_rows);
    const bool by_segs = !by_rows && h->file_segs;                  // the inverted route over a segmented file: the segmented walk
    h->last_seg[0] = h->last_seg[1] = h->last_seg[2] = h->last_seg[3] = 0;
    if (h->row_of.empty() || kmax == 0 || q_nnz == 0) {             // nothing can be a candidate
        for (size_t i = 0; i < nq; ++i) out_counts[i] = 0;
        return VDB_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const uint32_t n_rows = (uint32_t)h->ids.size();
    if ((rc = upload_tail(h->d_qoff, qoff, 0, s)) || (rc = upload_tail(h->d_qidx, qidx, 0, s)) || (rc = upload_tail(h->d_qval, qval, 0, s)) ||
        (rc = upload_tail(h->d_ks, kq, 0, s)))
        return rc;
    const uint64_t* d_mask = nullptr;
    if ((rc = stage_mask(h->d_mask, mask, s, &d_mask))) return rc;
    if ((rc = h->d_out_ids.ensure(nq * kmax)) || (rc = h->d_out_dists.ensure(nq * kmax)) || (rc = h->d_out_counts.ensure(nq)) ||
        (rc = h->d_flags.ensure(8)))
        return rc;
    // the accumulator slots: as many queries at once as the cap allows, at least one
    const size_t slots = std::min<size_t>(nq, std::max<size_t>(h->cap / (4 * (size_t)n_rows), 1));
    if (!by_segs && h->d_acc.n < slots * n_rows) {                  // (the segmented walk's accumulators are in LDS; its chunks stay these)
        if ((rc = h->d_acc.ensure(slots * n_rows))) return rc;
        vdb::launch_spv_fill(reinterpret_cast<uint32_t*>(h->d_acc.p), h->d_acc.n, vdb::SPV_UNTOUCHED, s);   // every search leaves them so
    }
    vdb::launch_spv_fill(h->d_flags, 8, 0, s);
    vdb::SpvSearchParams p{};
    p.q_off = h->d_qoff; p.q_idx = h->d_qidx; p.q_val = h->d_qval; p.ks = h->d_ks;
    p.list_ptr = h->d_list_ptr; p.vocab = h->vocab; p.entries = h->d_entries;
    p.acc = h->d_acc; p.n_rows = n_rows;
    p.live = h->d_live; p.row_ids = h->d_ids; p.rank = h->d_rank; p.sorted_ids = h->d_sorted;
    p.id_mask = d_mask; p.mask_bits = mask.bits;
    p.out_ids = h->d_out_ids; p.out_dists = h->d_out_dists; p.out_counts = h->d_out_counts; p.kout = (uint32_t)kmax;
    p.status = h->d_flags; p.counters = reinterpret_cast<unsigned long long*>(h->d_flags.p + 2);
    std::vector<RowPass> passes;
    std::vector<uint32_t> qslot, udims;                             // (read by their copies until the stream is synchronised)
    if (by_rows) {
        plan_row_passes(qoff, qidx, h->vocab, nq, slots, passes, qslot, udims);
        size_t table = 0;
        for (const RowPass& a : passes) table = std::max(table, ((size_t)a.n_u + 1) * a.tiles * vdb::SPV_ROWS_TILE);
        udims.push_back(0);                                         // (never empty: upload_tail allocates)
        if ((rc = upload_tail(h->d_qslot, qslot, 0, s)) || (rc = upload_tail(h->d_udims, udims, 0, s)) || (rc = h->d_table.ensure(table)))
            return rc;
        if (!h->slots_clean || h->d_dim_slot.n < h->vocab) {        // a wider vocabulary, or a search that failed half-way
            if ((rc = h->d_dim_slot.ensure(h->vocab))) return rc;
            vdb::launch_spv_fill(h->d_dim_slot, h->d_dim_slot.n, vdb::SPV_NO_SLOT, s);
        }
        h->slots_clean = false;
        vdb::SpvRowsParams r{};
        r.q_off = h->d_qoff; r.q_val = h->d_qval; r.q_slot = h->d_qslot;
        r.dim_slot = h->d_dim_slot; r.table = h->d_table;
        r.row_ptr = h->d_row_ptr; r.idx = h->d_idx; r.val = h->d_val; r.live = h->d_live; r.n_rows = n_rows;
        r.ks = h->d_ks; r.row_ids = h->d_ids; r.rank = h->d_rank; r.sorted_ids = h->d_sorted;
        r.id_mask = d_mask; r.mask_bits = mask.bits;
        r.out_ids = h->d_out_ids; r.out_dists = h->d_out_dists; r.out_counts = h->d_out_counts; r.kout = (uint32_t)kmax;
        r.status = p.status; r.counters = p.counters;
        for (const RowPass& a : passes) {
            r.qa = a.qa; r.nq = a.nq; r.tiles = a.tiles; r.udims = h->d_udims.p + a.u_off; r.n_u = a.n_u;
            r.acc = h->d_acc.p + (size_t)a.y0 * n_rows;             // a.y0 + a.nq <= slots: the plan keeps a pass inside one chunk
            vdb::launch_spv_rows_slots(r, true, s);
            vdb::launch_spv_rows_table(r, s);
            vdb::launch_spv_rows_fold(r, s);
            vdb::launch_spv_rows_emit(r, s);
            vdb::launch_spv_rows_slots(r, false, s);
        }
        h->last_route = 1;
        h->last_passes = passes.size();
        h->last_chunks = (nq + slots - 1) / slots;
    } else if (by_segs) {
        // the partial lists, segs * kmax keys per query: a chunk is split further where they would exceed the cap (one query always runs)
        const size_t per_query = (size_t)h->file_segs * kmax;
        const size_t step = std::min<size_t>({slots, std::max<size_t>(h->cap / (8 * per_query), 1), 65535});   // (grid y)
        if ((rc = h->d_part.ensure(step * per_query)) || (rc = h->d_part_cnt.ensure(step * h->file_segs))) return rc;
        vdb::SpvSegParams g{};
        g.q = p;
        g.sub_ptr = h->d_sub_ptr; g.segs = h->file_segs; g.seg_shift = h->file_shift;
        g.part = h->d_part; g.part_cnt = h->d_part_cnt;
        for (size_t q0 = 0; q0 < nq; q0 += slots) {
            const size_t q1 = std::min(q0 + slots, nq);
            for (size_t a = q0; a < q1; a += step) {
                g.q.q0 = (uint32_t)a;
                vdb::launch_spv_seg_score(g, (uint32_t)std::min(step, q1 - a), s);
                vdb::launch_spv_seg_merge(g, (uint32_t)std::min(step, q1 - a), s);
            }
            ++h->last_chunks;
        }
        h->last_seg[0] = 1;
        h->last_seg[1] = h->file_segs;
        h->last_seg[2] = 1ull << h->file_shift;
    } else {
        for (size_t q0 = 0; q0 < nq; q0 += slots) {
            p.q0 = (uint32_t)q0;
            vdb::launch_spv_search(p, (uint32_t)std::min(slots, nq - q0), s);
            ++h->last_chunks;
        }
    }
    HIP_TRY(hipGetLastError());
    uint32_t flags[8] = {0};
    HIP_TRY(hipMemcpyAsync(flags, h->d_flags, sizeof(flags), hipMemcpyDeviceToHost, s));
    Lists d;
    d.ids = h->d_out_ids; d.dists = h->d_out_dists; d.counts = h->d_out_counts; d.stride = kmax;
    if ((rc = copy_out(d, b, s))) return rc;                        // synchronises s: flags are here, too
    if (by_rows) h->slots_clean = true;                             // every pass has put SPV_NO_SLOT back
    memcpy(&h->last_walked, flags + 2, 8);
    memcpy(&h->last_offered, flags + 4, 8);
    memcpy(&h->last_seg[3], flags + 6, 8);                          // (zero on the other routes)
    if (flags[0] & vdb::ST_NAN) return fail_nan();
    return VDB_OK;
}

}  // namespace

extern "C" {

int vdb_spv_create(int device, vdb_spv_index** out) {
    return guarded([&]() -> int {
    if (!out) return fail(VDB_ERR_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VDB_ERR_DEVICE, "no HIP device available: this engine has no CPU path");
    if (device < 0 || device >= ndev) return fail(VDB_ERR_INVALID_ARGUMENT, "device %d out of range (%d)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(VDB_ERR_DEVICE, "device %d is %s; the kernels are built for gfx950 only", device, prop.gcnArchName);
    auto h = std::make_unique<vdb_spv_index>();
    h->device = device;
    int rc;
    if ((rc = h->stream.create(hipStreamNonBlocking))) return rc;
    *out = h.release();
    return VDB_OK;
    });
}

void vdb_spv_destroy(vdb_spv_index* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    delete h;
}

int vdb_spv_add_bulk(vdb_spv_index* h, const uint64_t* ids, const size_t* offsets, const uint32_t* indices, const float* values, size_t n) {
    return guarded([&]() -> int {
    if (!h || (n && (!ids || !offsets))) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return VDB_OK;
    int rc;
    if ((rc = check_offsets(offsets, n, "row"))) return rc;
    const size_t nnz = offsets[n] - offsets[0];
    if (nnz && (!indices || !values)) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    // everything is checked before anything is stored: a refused call leaves the index as it was
    std::vector<uint32_t> ni;
    std::vector<float> nv;
    ni.reserve(nnz);
    nv.reserve(nnz);
    for (size_t i = 0; i < n; ++i)
        if ((rc = sorted_pairs(indices + offsets[i], values + offsets[i], offsets[i + 1] - offsets[i], "row", i, ni, nv))) return rc;
    std::lock_guard<std::mutex> g(h->mu);
    if (h->idx.size() + (uint64_t)nnz > MAX_ENTRIES || h->ids.size() + (uint64_t)n >= MAX_ENTRIES)
        return fail(VDB_ERR_INVALID_ARGUMENT, "the index holds fewer than 2^32 rows and fewer than 2^32 non-zeros (dead rows included)");
    size_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        const size_t len = offsets[i + 1] - offsets[i];
        auto it = h->row_of.find(ids[i]);
        if (it != h->row_of.end()) kill_row(h, it->second);         // HashMap::insert: the last vector of an id wins
        const uint32_t row = (uint32_t)h->ids.size();
        h->ids.push_back(ids[i]);
        h->idx.insert(h->idx.end(), ni.begin() + (ptrdiff_t)at, ni.begin() + (ptrdiff_t)(at + len));
        h->val.insert(h->val.end(), nv.begin() + (ptrdiff_t)at, nv.begin() + (ptrdiff_t)(at + len));
        h->row_ptr.push_back((uint32_t)h->idx.size());
        if ((row >> 5) >= h->live.size()) h->live.push_back(0);
        h->live[row >> 5] |= 1u << (row & 31);
        h->row_of[ids[i]] = row;
        h->live_nnz += len;
        if (len) h->vocab = std::max(h->vocab, ni[at + len - 1] + 1);
        if (h->live_df.size() < h->vocab) h->live_df.resize(h->vocab, 0);
        for (size_t j = at; j < at + len; ++j) ++h->live_df[ni[j]];
        at += len;
    }
    h->dirty = true;
    return VDB_OK;
    });
}

int vdb_spv_remove(vdb_spv_index* h, uint64_t id) {
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

size_t vdb_spv_len(const vdb_spv_index* h) { return h ? h->row_of.size() : 0; }

int vdb_spv_flush(vdb_spv_index* h) {
    return guarded([&]() -> int {
    if (!h) return fail(VDB_ERR_INVALID_ARGUMENT, "null handle");
    std::lock_guard<std::mutex> g(h->mu);
    return flush_locked(h);
    });
}

int vdb_spv_search_batch(vdb_spv_index* h, const size_t* q_offsets, const uint32_t* q_indices, const float* q_values, size_t nq,
                         const size_t* ks, size_t k, const uint64_t* id_mask, size_t mask_bits, size_t kstride, uint64_t* out_ids,
                         float* out_dists, size_t* out_counts) {
    return guarded([&]() -> int {
    MaskSrc m;
    m.host = id_mask; m.bits = id_mask ? mask_bits : 0;
    return search(h, q_offsets, q_indices, q_values, nq, ks, k, m, kstride, out_ids, out_dists, out_counts);
    });
}

int vdb_spv_search_batch_filtered(vdb_spv_index* h, const size_t* q_offsets, const uint32_t* q_indices, const float* q_values, size_t nq,
                                  const size_t* ks, size_t k, const vdb_meta_mask* mask, size_t kstride, uint64_t* out_ids,
                                  float* out_dists, size_t* out_counts) {
    return guarded([&]() -> int {
    if (!h) return fail(VDB_ERR_INVALID_ARGUMENT, "null handle");
    if (!mask) return fail(VDB_ERR_INVALID_ARGUMENT, "null mask");
    if (mask->device != h->device)
        return fail(VDB_ERR_INVALID_ARGUMENT, "the compiled mask lives on device %d, the index on device %d", mask->device, h->device);
    MaskSrc m;
    m.compiled = mask->d_words; m.done = mask->done; m.bits = mask->bits;
    return search(h, q_offsets, q_indices, q_values, nq, ks, k, m, kstride, out_ids, out_dists, out_counts);
    });
}

int vdb_spv_stats(const vdb_spv_index* h, uint64_t out[8]) {
    if (!h || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    out[0] = h->ids.size();
    out[1] = h->ids.size() - h->row_of.size();
    out[2] = h->idx.size();
    out[3] = h->vocab;
    out[4] = h->rebuilds;
    out[5] = h->last_walked;
    out[6] = h->last_offered;
    out[7] = h->last_chunks;
    return VDB_OK;
}

int vdb_spv_set_route(vdb_spv_index* h, int mode) {
    if (!h) return fail(VDB_ERR_INVALID_ARGUMENT, "null handle");
    if (mode < 0 || mode > 2) return fail(VDB_ERR_INVALID_ARGUMENT, "route %d: 0 (inverted file), 1 (row-major) or 2 (automatic)", mode);
    std::lock_guard<std::mutex> g(h->mu);
    h->route = mode;
    return VDB_OK;
}

int vdb_spv_route_stats(const vdb_spv_index* h, uint64_t out[4]) {
    if (!h || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    out[0] = h->last_route;
    out[1] = h->last_passes;
    out[2] = h->last_work_inv;
    out[3] = h->last_work_rows;
    return VDB_OK;
}

double vdb_spv_route_rho(void) { return ROUTE_RHO; }

int vdb_spv_set_segmented(vdb_spv_index* h, size_t rows_per_segment) {
    if (!h) return fail(VDB_ERR_INVALID_ARGUMENT, "null handle");
    const size_t r = rows_per_segment;
    if (r && (r < vdb::SPV_SEG_ROWS_MIN || r > vdb::SPV_SEG_ROWS_MAX || (r & (r - 1))))
        return fail(VDB_ERR_INVALID_ARGUMENT, "rows per segment %zu: 0 (off) or a power of two in [%u, %u]", r, vdb::SPV_SEG_ROWS_MIN,
                    vdb::SPV_SEG_ROWS_MAX);
    std::lock_guard<std::mutex> g(h->mu);
    if (r != h->seg_rows && h->rebuilds) h->dirty = true;           // the file in place has the other order: the next flush rebuilds it
    h->seg_rows = (uint32_t)r;
    return VDB_OK;
}

int vdb_spv_segment_stats(const vdb_spv_index* h, uint64_t out[4]) {
    if (!h || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    for (int i = 0; i < 4; ++i) out[i] = h->last_seg[i];
    return VDB_OK;
}

int vdb_spv_debug_set_workspace_cap(vdb_spv_index* h, size_t bytes) {
    if (!h) return fail(VDB_ERR_INVALID_ARGUMENT, "null handle");
    std::lock_guard<std::mutex> g(h->mu);
    h->cap = bytes ? std::min(bytes, vdb_spv_index::DEFAULT_CAP) : vdb_spv_index::DEFAULT_CAP;
    return VDB_OK;
}

}  // extern "C"
