// vdb_store.cpp -- the device-resident mirror of the reference's FlatIndex rows (src/flat_index.rs:12-50): host staging of
// single adds, upload at the next search, tombstones, rows of another dimension kept host-side.
//
// Device layout (all in HBM, one allocation each, grown by doubling):
//   rows     [cap][ld] f32   ld = dim rounded up to 32, zero padded (K stage of the MFMA kernel)
//   nd       [cap]     f32   exact-order row norm  (vector.rs:35-37)
//   alpha,beta [cap]   f32   ranking score = fma(dot, alpha, beta)
//   row_ids  [cap]     u64   device row -> reference internal id
//   live     [cap/32]  u32   tombstone bitmask (remove() clears a bit; rows are appended, and only compact_store renumbers them)
// Invariant kept by grow and by compact_store: rows, margin and the bf16 shadow read as zero over [n_uploaded, cap).
#include <numeric>

#include "vdb_index.h"

namespace vdbi {

// ------------------------------------------------------------------ the layout of the rows (row_split.h)
// One conversion of rows [0, n_uploaded), in place, on the handle's stream, with the whole device waited for before it (whatever
// was enqueued against the old layout, on any stream, has run) and the stream after it (whoever is enqueued next, on any stream,
// sees the new one).  The zero rows behind n_uploaded are the same in both layouts.
static int convert_rows(Index* ix, bool forward) {
    int prev = 0;
    HIP_TRY(hipGetDevice(&prev));
    if (prev != ix->device) HIP_TRY(hipSetDevice(ix->device));
    auto run = [&]() -> int {
        HIP_TRY(hipDeviceSynchronize());
        hipStream_t s = ix->stream;
        if (forward) {
            int rc = ix->d_split_flag.ensure(1);
            if (rc) return rc;
            HIP_TRY(hipMemsetAsync(ix->d_split_flag.p, 0, 4, s));
        }
        vdb::launch_row_split(ix->d_rows_store, ix->ld, ix->n_uploaded, forward, ix->d_split_flag.p, (uint32_t)ix->n_cu, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
        return VDB_OK;
    };
    const int rc = run();
    if (prev != ix->device) (void)hipSetDevice(prev);
    if (rc) { ix->store_broken = true; return rc; }                      // rows may be half converted: nothing is served from this handle any more
    ix->layout = forward ? vdb::LAYOUT_SPLIT : vdb::LAYOUT_F32;
    ++ix->split_conversions;
    return VDB_OK;
}

float* rows_f32(Index* ix) {
    ix->split_streak = 0;
    if (ix->layout == vdb::LAYOUT_SPLIT) (void)convert_rows(ix, false);
    return ix->d_rows_store;
}
float* rows_mut(Index* ix) {
    ix->split_refused = false;
    return rows_f32(ix);
}

int rows_to_split(Index* ix) {
    if (ix->layout == vdb::LAYOUT_SPLIT || ix->split_refused || !ix->d_rows_store || !ix->n_uploaded) return VDB_OK;
    if (ix->ld % 64 != 0 || ix->ld > 16384) return VDB_OK;
    int rc = convert_rows(ix, true);
    if (rc) return rc;
    uint32_t nonfinite = 0;
    HIP_TRY(hipMemcpy(&nonfinite, ix->d_split_flag.p, 4, hipMemcpyDeviceToHost));
    if (nonfinite) {                                                     // inf / NaN elements keep the f32-row kernel's behaviour
        ix->split_refused = true;
        return convert_rows(ix, false);
    }
    return VDB_OK;
}

// ------------------------------------------------------------------ device store management
// Re-allocates the store with room for `cap` rows (>= n_uploaded) and carries the uploaded rows over; old and new exist at once.
static int resize_store(Index* ix, uint32_t cap) {
    // built in locals and moved into the handle at the end: a failure anywhere frees every new array and leaves the old store in place
    DevBuf<float> rows, nd, al, be, mg;
    DevBuf<uint64_t> ids;
    DevBuf<uint32_t> lv;
    DevBuf<uint16_t> r16;
    size_t row_bytes = (size_t)ix->ld * sizeof(float);
    HIP_TRY(rows.alloc((size_t)cap * ix->ld));
    HIP_TRY(nd.alloc(cap));
    HIP_TRY(al.alloc(cap));
    HIP_TRY(be.alloc(cap));
    if (ix->metric != vdb::COSINE) HIP_TRY(mg.alloc(cap));
    HIP_TRY(ids.alloc(cap));
    HIP_TRY(lv.alloc((size_t)cap / 32));
    hipStream_t s = ix->stream;
    uint32_t old = ix->n_uploaded;
    const float* old_rows = rows_f32(ix);                                // the new store is F32 like the one it replaces
    if (ix->shadow) {
        HIP_TRY(r16.alloc((size_t)cap * ix->ld));
        if (old && ix->d_rows16) HIP_TRY(hipMemcpyAsync(r16, ix->d_rows16, (size_t)old * ix->ld * 2, hipMemcpyDeviceToDevice, s));
        else if (old) vdb::launch_rows_to_bf16(old_rows, r16, ix->ld, 0, old, s);     // no shadow yet: from the f32 rows, never left unset
        HIP_TRY(hipMemsetAsync((char*)r16.p + (size_t)old * ix->ld * 2, 0, (size_t)(cap - old) * ix->ld * 2, s));
    }
    if (old) {
        HIP_TRY(hipMemcpyAsync(rows, old_rows, (size_t)old * row_bytes, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(nd, ix->d_nd, (size_t)old * 4, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(al, ix->d_alpha, (size_t)old * 4, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(be, ix->d_beta, (size_t)old * 4, hipMemcpyDeviceToDevice, s));
        if (mg) HIP_TRY(hipMemcpyAsync(mg, ix->d_margin, (size_t)old * 4, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(ids, ix->d_row_ids, (size_t)old * 8, hipMemcpyDeviceToDevice, s));
    }
    if (mg) HIP_TRY(hipMemsetAsync(mg + old, 0, (size_t)(cap - old) * 4, s));   // rows past the last one are staged by the kernels (ragged tile)
    // zero the rest of the row block: the [dim, ld) padding columns must read as 0
    HIP_TRY(hipMemsetAsync((char*)rows.p + (size_t)old * row_bytes, 0, (size_t)(cap - old) * row_bytes, s));
    HIP_TRY(hipMemsetAsync(lv, 0, (size_t)cap / 8, s));
    HIP_TRY(hipStreamSynchronize(s));
    ix->d_rows16 = std::move(r16);
    ix->d_margin = std::move(mg);
    ix->d_rows_store = std::move(rows); ix->d_nd = std::move(nd); ix->d_alpha = std::move(al); ix->d_beta = std::move(be);
    ix->d_row_ids = std::move(ids); ix->d_live = std::move(lv);
    ix->cap_rows = cap;
    ix->live_dirty = true;
    return VDB_OK;
}

int grow(Index* ix, uint32_t need_rows) {
    if (need_rows <= ix->cap_rows) return VDB_OK;
    uint32_t cap = std::max<uint32_t>({need_rows, ix->cap_rows * 2u, 1024u});
    return resize_store(ix, round_up(cap, 256));
}

void free_store(Index* ix) {
    ix->d_rows_store.release(); ix->layout = vdb::LAYOUT_F32; ix->split_streak = 0; ix->split_refused = false;
    ix->d_nd.release(); ix->d_alpha.release(); ix->d_beta.release(); ix->d_margin.release();
    ix->d_row_ids.release(); ix->d_live.release();
    ix->d_rows16.release();
    ix->d_sample16.release(); ix->sample16_n = ix->sample16_S = 0;
    ix->cap_rows = 0;
}

// Reset to the empty state (keeps the handle, metric and workspace).
void reset_rows(Index* ix) {
    ix->row_ids.clear(); ix->live.clear(); ix->id2row.clear(); ix->pending.clear();
    ix->n_live = 0; ix->n_uploaded = 0; ix->dim = 0; ix->ld = 0; ix->ids_monotone = true;
    ix->zero_valid = false; ix->rank_valid = false; ix->live_dirty = false;
    free_store(ix);
    if (ix->d_scalars) (void)hipMemsetAsync(ix->d_scalars, 0, 32, ix->stream);
}

// A fresh index takes the dimension of what it is given (add, bulk add, reserve); rows of a store emptied by removes go first.
void adopt_dim(Index* ix, size_t dim) {
    if (ix->n_live != 0 || !ix->misfits.empty()) return;
    if (ix->dim != dim) reset_rows(ix);
    ix->dim = (uint32_t)dim;
    ix->ld = round_up(ix->dim, vdb::KSTAGE);
}

void kill_row(Index* ix, uint32_t row) {
    ix->live[row >> 5] &= ~(1u << (row & 31));
    --ix->n_live;
    ix->live_dirty = true;
    ix->zero_valid = false;
    ix->split_streak = 0;                                                // a mutation: the adaptive layout rule starts counting again
}

// Appends one primary-dimension row to the host staging area.
void append_row(Index* ix, uint64_t id, const float* v) {
    uint32_t row = ix->n_rows();
    if (row && id <= ix->row_ids.back()) ix->ids_monotone = false;
    ix->row_ids.push_back(id);
    ix->id_bound = std::max(ix->id_bound, id == ~0ull ? id : id + 1);
    if ((row >> 5) >= ix->live.size()) ix->live.push_back(0u);
    ix->live[row >> 5] |= 1u << (row & 31);
    ++ix->n_live;
    ix->id2row[id] = row;
    size_t off = ix->pending.size();
    ix->pending.resize(off + ix->ld, 0.0f);
    memcpy(ix->pending.data() + off, v, (size_t)ix->dim * sizeof(float));
    ix->live_dirty = true;
    ix->zero_valid = false;
    ix->rank_valid = false;
}

// When the last primary row is gone but rows of another dimension remain, the lowest-id
// such dimension becomes the primary one.
void promote_misfits(Index* ix) {
    if (ix->n_live != 0 || ix->misfits.empty()) return;
    uint64_t best = ~0ull;
    for (auto& kv : ix->misfits) best = std::min(best, kv.first);
    size_t nd = ix->misfits[best].size();
    reset_rows(ix);
    if (nd == 0) return;   // zero-length vectors stay host-side only
    ix->dim = (uint32_t)nd;
    ix->ld = round_up(ix->dim, vdb::KSTAGE);
    std::vector<uint64_t> ids;
    for (auto& kv : ix->misfits)
        if (kv.second.size() == nd) ids.push_back(kv.first);
    std::sort(ids.begin(), ids.end());
    for (uint64_t id : ids) {
        append_row(ix, id, ix->misfits[id].data());
        ix->misfits.erase(id);
    }
}

int remove_id(Index* ix, uint64_t id) {
    auto it = ix->id2row.find(id);
    if (it != ix->id2row.end()) {
        kill_row(ix, it->second);
        ix->id2row.erase(it);
        if (ix->n_live == 0) {
            if (ix->misfits.empty()) reset_rows(ix);
            else promote_misfits(ix);
        }
        return VDB_OK;
    }
    ix->misfits.erase(id);   // absent id is Ok(()) (flat_index.rs:43-46)
    return VDB_OK;
}

int add_one(Index* ix, uint64_t id, const float* v, size_t dim) {
    remove_id(ix, id);   // HashMap::insert overwrites (flat_index.rs:39)
    if (dim > 0) adopt_dim(ix, dim);
    if (dim == ix->dim && dim > 0) {
        append_row(ix, id, v);
    } else {
        ix->misfits[id] = std::vector<float>(v, v + dim);
        ix->id_bound = std::max(ix->id_bound, id == ~0ull ? id : id + 1);
        if (ix->n_live == 0) promote_misfits(ix);
    }
    return VDB_OK;
}

static int flush_upload(Index* ix) {
    if (ix->store_broken) return fail(VDB_ERR_DEVICE, "the row store is inconsistent after a failed compaction: destroy the handle");
    hipStream_t s = ix->stream;
    uint32_t n = ix->n_rows();
    if (n > ix->n_uploaded) {
        int rc = grow(ix, n);
        if (rc) return rc;
        uint32_t first = ix->n_uploaded, cnt = n - first;
        float* d_rows = rows_mut(ix);                                    // appends go to f32 rows
        HIP_TRY(hipMemcpyAsync(d_rows + (size_t)first * ix->ld, ix->pending.data(),
                               (size_t)cnt * ix->ld * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(ix->d_row_ids + first, ix->row_ids.data() + first, (size_t)cnt * 8,
                               hipMemcpyHostToDevice, s));
        const MarginPlan mp = margin_plan(ix);
        vdb::RowStatsParams rp{d_rows, ix->ld, ix->dim, first, n, ix->metric, ix->d_nd, ix->d_alpha,
                               ix->d_beta, ix->d_scalars, ix->d_margin, mp.m_e, mp.m_n, mp.m_b, mp.beta_shrink};
        vdb::launch_row_stats(rp, s);
        if (ix->d_rows16) vdb::launch_rows_to_bf16(d_rows, ix->d_rows16, ix->ld, first, n, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));   // pending is host memory about to be released
        ix->pending.clear();
        ix->pending.shrink_to_fit();
        ix->n_uploaded = n;
        ix->zero_valid = false;
    }
    if (ix->live_dirty && ix->d_live && n) {
        HIP_TRY(hipMemcpyAsync(ix->d_live, ix->live.data(), ix->live.size() * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        ix->live_dirty = false;
    }
    return VDB_OK;
}

// ------------------------------------------------------------------ compaction (vdb_flat_compact)
// The bounce buffer: 32 MiB of whole rows (every column of a row included), at least one 32-row word.  Large enough that one
// launch gives each of the 256 CUs 128 KiB to move, 1 % of a 3 GB store, and -- read back at once -- well inside the 256 MiB cache.
constexpr size_t COMPACT_BOUNCE_BYTES = (size_t)32 << 20;
static size_t bounce_row_bytes(uint32_t ld, bool shadow) { return (size_t)ld * 4 + (shadow ? (size_t)ld * 2 : 0) + 8 + 4 * 4; }
uint32_t compact_bounce_rows(uint32_t ld, bool shadow) {
    const size_t rows = COMPACT_BOUNCE_BYTES / bounce_row_bytes(ld, shadow);
    return (uint32_t)std::max<size_t>(32, rows & ~(size_t)31);
}

// The chunk plan.  prefix[w] = live rows below word w (nw + 1 entries), so dest(r) = prefix[r >> 5] + popc(live bits below r).
// Chunks are runs of whole 32-row words, in source order, starting at the first word that holds a dead row (everything below
// it stays where it is).  With gap = a - dest(a) dead rows below a chunk's first row a:
//   direct  [a, b): b the last word boundary with live(a, b) <= gap, i.e. dest(b) <= a -- no row written by the launch is one
//           it (or a later launch) still reads.  Taken when the gap is at least a quarter of the bounce buffer (below that a
//           bounced chunk moves more rows per launch than a direct one could) or when it reaches the end of the store;
//   bounce  [a, b): b the last word boundary with live(a, b) <= bounce_rows; gathered into the bounce buffer, then copied down.
// Words without a live row are skipped (they only widen the gap).
void compact_plan(const uint32_t* live, uint32_t n_rows, uint32_t bounce_rows, std::vector<uint32_t>* prefix, std::vector<CompactChunk>* out) {
    const uint32_t nw = (n_rows + 31) / 32;
    prefix->assign((size_t)nw + 1, 0u);
    for (uint32_t w = 0; w < nw; ++w) (*prefix)[w + 1] = (*prefix)[w] + (uint32_t)__builtin_popcount(live[w]);
    out->clear();
    const uint32_t* P = prefix->data();
    uint32_t aw = 0;
    while (aw < nw && P[aw + 1] - P[aw] == std::min(32u, n_rows - aw * 32u)) ++aw;      // full words: nothing moves
    while (aw < nw) {
        if (live[aw] == 0) { ++aw; continue; }
        const uint32_t a = aw * 32u, gap = a - P[aw];
        auto last_within = [&](uint32_t budget) {      // the largest word index bw >= aw with live(aw, bw) <= budget
            return (uint32_t)(std::upper_bound(P + aw, P + nw + 1, P[aw] + budget) - P) - 1u;
        };
        uint32_t bw = last_within(gap);
        uint32_t mode = 0;
        if (!(bw > aw && (bw == nw || gap >= bounce_rows / 4))) { bw = last_within(bounce_rows); mode = 1; }
        out->push_back({a, std::min(bw * 32u, n_rows), P[aw], mode});
        aw = bw;
    }
}

void store_stats(const Index* ix, uint64_t out[8]) {
    const uint64_t cap = ix->cap_rows;
    out[0] = ix->n_rows(); out[1] = ix->n_live; out[2] = cap;
    out[3] = ix->d_rows_store ? cap * ((uint64_t)ix->ld * 4 + 3 * 4 + (ix->d_margin ? 4 : 0) + 8) + cap / 8 + (ix->d_rows16 ? cap * ix->ld * 2 : 0) : 0;
    out[4] = ix->n_compactions; out[5] = ix->rows_reclaimed; out[6] = ix->last_compact_ns;
    // [7]: the last compaction's device part (bits 0-39, ns: plan uploaded .. last row moved and the stream synchronised) and its
    // chunk counts, saturating at 4095 (bits 40-51 through the bounce buffer, bits 52-63 moved directly)
    out[7] = std::min<uint64_t>(ix->last_device_ns, (1ull << 40) - 1) | (std::min<uint64_t>(ix->last_chunks_bounce, 4095) << 40) |
             (std::min<uint64_t>(ix->last_chunks_direct, 4095) << 52);
}

int compact_store(Index* ix, bool shrink, size_t* out_reclaimed) {
    if (out_reclaimed) *out_reclaimed = 0;
    int rc;
    if ((rc = flush_upload(ix))) return rc;             // staged rows go up first: the whole store is compacted, d_live is current
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = ix->stream;
    const uint32_t n = ix->n_uploaded, n_live = ix->n_live, ld = ix->ld;
    if (n > n_live) {
        float* const d_rows = rows_mut(ix);                              // rows move as f32 rows                                   // (n_live > 0: removing the last row resets the store)
        std::vector<uint32_t> prefix;
        std::vector<CompactChunk> plan;
        const bool shadow = ix->d_rows16 != nullptr;
        const uint32_t B = ix->bounce_rows_override ? std::max(32u, ix->bounce_rows_override & ~31u) : compact_bounce_rows(ld, shadow);
        compact_plan(ix->live.data(), n, B, &prefix, &plan);
        uint64_t n_direct = 0, n_bounce = 0;
        for (auto& c : plan) (c.mode ? n_bounce : n_direct)++;
        // every allocation happens before the first row moves
        DevBuf<uint32_t> d_prefix;
        DevBuf<char> d_bounce;
        HIP_TRY(d_prefix.alloc(prefix.size()));
        if (n_bounce && d_bounce.alloc((size_t)B * bounce_row_bytes(ld, shadow)) != hipSuccess) {
            return fail(VDB_ERR_DEVICE, "allocating the compaction bounce buffer (%zu bytes) failed", (size_t)B * bounce_row_bytes(ld, shadow));
        }
        // bounce layout: f32 rows | bf16 rows | ids | nd | alpha | beta | margin, B rows each
        float* b_rows = reinterpret_cast<float*>(d_bounce.p);
        uint16_t* b_rows16 = reinterpret_cast<uint16_t*>(d_bounce.p + (size_t)B * ld * 4);
        char* b_cols = d_bounce.p + (size_t)B * ld * 4 + (shadow ? (size_t)B * ld * 2 : 0);
        uint64_t* b_ids = reinterpret_cast<uint64_t*>(b_cols);
        float* b_nd = reinterpret_cast<float*>(b_cols + (size_t)B * 8);
        float *b_alpha = b_nd + B, *b_beta = b_nd + 2 * (size_t)B, *b_margin = b_nd + 3 * (size_t)B;
        bool moved = false;
        auto run = [&]() -> hipError_t {
            hipError_t e = hipMemcpyAsync(d_prefix, prefix.data(), prefix.size() * 4, hipMemcpyHostToDevice, s);
            if (e != hipSuccess) return e;
            vdb::CompactMoveParams mp{};
            mp.ld = ld; mp.lanes_log2 = vdb::compact_lanes_log2(ld);
            for (const CompactChunk& c : plan) {
                const uint32_t cnt = prefix[(c.b + 31) / 32] - prefix[c.a / 32];
                // source: the store, rows [a, b)
                mp.live = ix->d_live; mp.prefix = d_prefix; mp.row_begin = c.a; mp.row_end = c.b;
                mp.src_rows = d_rows; mp.src_rows16 = ix->d_rows16; mp.src_nd = ix->d_nd; mp.src_alpha = ix->d_alpha; mp.src_beta = ix->d_beta;
                mp.src_margin = ix->d_margin; mp.src_ids = ix->d_row_ids;
                if (c.mode == 0) {
                    mp.dst_sub = 0;
                    mp.dst_rows = d_rows; mp.dst_rows16 = ix->d_rows16; mp.dst_nd = ix->d_nd; mp.dst_alpha = ix->d_alpha; mp.dst_beta = ix->d_beta;
                    mp.dst_margin = ix->d_margin; mp.dst_ids = ix->d_row_ids;
                    moved = true;
                    vdb::launch_compact_move(mp, (uint32_t)ix->n_cu, s);
                } else {
                    mp.dst_sub = c.dst;
                    mp.dst_rows = b_rows; mp.dst_rows16 = shadow ? b_rows16 : nullptr; mp.dst_nd = b_nd; mp.dst_alpha = b_alpha; mp.dst_beta = b_beta;
                    mp.dst_margin = ix->d_margin ? b_margin : nullptr; mp.dst_ids = b_ids;
                    vdb::launch_compact_move(mp, (uint32_t)ix->n_cu, s);
                    // the contiguous copy down: bounce rows [0, cnt) -> store rows [dst, dst + cnt)
                    mp.live = nullptr; mp.prefix = nullptr; mp.row_begin = 0; mp.row_end = cnt; mp.dst_sub = 0;
                    mp.src_rows = b_rows; mp.src_rows16 = shadow ? b_rows16 : nullptr; mp.src_nd = b_nd; mp.src_alpha = b_alpha; mp.src_beta = b_beta;
                    mp.src_margin = ix->d_margin ? b_margin : nullptr; mp.src_ids = b_ids;
                    mp.dst_rows = d_rows + (size_t)c.dst * ld; mp.dst_rows16 = shadow ? ix->d_rows16 + (size_t)c.dst * ld : nullptr;
                    mp.dst_nd = ix->d_nd + c.dst; mp.dst_alpha = ix->d_alpha + c.dst; mp.dst_beta = ix->d_beta + c.dst;
                    mp.dst_margin = ix->d_margin ? ix->d_margin + c.dst : nullptr; mp.dst_ids = ix->d_row_ids + c.dst;
                    moved = true;
                    vdb::launch_compact_move(mp, (uint32_t)ix->n_cu, s);
                }
                if ((e = hipGetLastError()) != hipSuccess) return e;
            }
            // the freed tail reads as zero again (padding columns of later adds, rows staged past the last one by ragged tiles)
            moved = true;
            if ((e = hipMemsetAsync(d_rows + (size_t)n_live * ld, 0, (size_t)(n - n_live) * ld * 4, s)) != hipSuccess) return e;
            if (ix->d_margin && (e = hipMemsetAsync(ix->d_margin + n_live, 0, (size_t)(n - n_live) * 4, s)) != hipSuccess) return e;
            if (shadow && (e = hipMemsetAsync(ix->d_rows16 + (size_t)n_live * ld, 0, (size_t)(n - n_live) * ld * 2, s)) != hipSuccess) return e;
            if ((e = hipMemsetAsync(ix->d_live, 0, (size_t)ix->cap_rows / 8, s)) != hipSuccess) return e;
            return hipStreamSynchronize(s);
        };
        const auto t_dev = std::chrono::steady_clock::now();
        const hipError_t e = run();
        ix->last_device_ns = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_dev).count();
        if (e != hipSuccess) (void)hipStreamSynchronize(s);
        if (e != hipSuccess) {
            if (moved) ix->store_broken = true;         // rows may be half moved: nothing is served from this handle any more
            return fail(VDB_ERR_DEVICE, "HIP error %d (%s) during the compaction%s", (int)e, hipGetErrorString(e),
                        moved ? "; the handle is unusable" : "; nothing was moved");
        }
        // host bookkeeping: the survivors in their old order (rows below the first dead one keep their number)
        uint32_t d = 0;
        while (d < n && ix->is_live(d)) ++d;
        bool mono = true;
        for (uint32_t r = 1; r < d && mono; ++r) mono = ix->row_ids[r] > ix->row_ids[r - 1];
        for (uint32_t r = d; r < n; ++r)
            if (ix->is_live(r)) {
                const uint64_t id = ix->row_ids[r];
                if (d && id <= ix->row_ids[d - 1]) mono = false;
                ix->row_ids[d] = id;
                ix->id2row[id] = d;
                ++d;
            }
        ix->row_ids.resize(n_live);
        ix->live.assign((n_live + 31) / 32, 0xffffffffu);
        if (n_live & 31) ix->live.back() = (1u << (n_live & 31)) - 1u;
        ix->n_uploaded = n_live;
        ix->ids_monotone = mono;
        ix->rank_valid = false;
        ix->zero_valid = false;
        ix->sample16_n = ix->sample16_S = 0;            // keyed by rows uploaded; row positions changed
        ix->live_dirty = true;
        ix->n_compactions++;
        ix->rows_reclaimed += n - n_live;
        ix->last_chunks_direct = n_direct; ix->last_chunks_bounce = n_bounce;
        if (out_reclaimed) *out_reclaimed = n - n_live;
        if ((rc = flush_upload(ix))) return rc;         // d_live: all ones over [0, n_live)
        ix->last_compact_ns = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    }
    if (shrink && ix->cap_rows) {
        const uint32_t cap = round_up(std::max<uint32_t>(ix->n_uploaded, 1024u), 256);      // what grow picks for a fresh index of this many rows
        if (cap < ix->cap_rows && (rc = resize_store(ix, cap))) return rc;
        if ((rc = flush_upload(ix))) return rc;         // the new d_live
    }
    return VDB_OK;
}

int flush(Index* ix) {
    int rc = flush_upload(ix);
    if (rc) return rc;
    // vdb_flat_set_auto_compact: never while another search of this handle is in flight (its kernels read the rows)
    if (ix->auto_compact > 0.0 && ix->n_uploaded > ix->n_live && !in_flight(ix) &&
        (double)(ix->n_uploaded - ix->n_live) > ix->auto_compact * (double)ix->n_uploaded)
        return compact_store(ix, false, nullptr);
    return VDB_OK;
}

int ensure_zero_count(Index* ix) {
    if (ix->zero_valid) return VDB_OK;
    hipStream_t s = ix->stream;
    HIP_TRY(hipMemsetAsync(ix->d_scalars + 1, 0, 4, s));
    vdb::launch_count_zero_live(ix->d_nd, ix->d_live, ix->n_uploaded, ix->d_scalars + 1, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&ix->zero_live, ix->d_scalars + 1, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    ix->zero_valid = true;
    return VDB_OK;
}

// id rank tables so that exact-scan keys order by (distance, id) even when ids were not
// appended in increasing order.
int ensure_ranks(Index* ix) {
    if (ix->ids_monotone || ix->rank_valid) return VDB_OK;
    uint32_t n = ix->n_rows();
    std::vector<uint32_t> order(n), rank(n);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return ix->row_ids[a] != ix->row_ids[b] ? ix->row_ids[a] < ix->row_ids[b] : a < b;
    });
    for (uint32_t r = 0; r < n; ++r) rank[order[r]] = r;
    int rc;
    if ((rc = ix->d_idrank.ensure(n)) || (rc = ix->d_rank2row.ensure(n))) return rc;
    HIP_TRY(hipMemcpyAsync(ix->d_idrank.p, rank.data(), (size_t)n * 4, hipMemcpyHostToDevice, ix->stream));
    HIP_TRY(hipMemcpyAsync(ix->d_rank2row.p, order.data(), (size_t)n * 4, hipMemcpyHostToDevice, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    ix->rank_valid = true;
    return VDB_OK;
}

}  // namespace vdbi
