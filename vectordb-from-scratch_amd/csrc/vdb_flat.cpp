// vdb_flat.cpp -- the extern "C" shims of include/vdb_flat.h over the device-resident mirror of the reference's FlatIndex
// (src/flat_index.rs:12-74; vdb_store.cpp) and the search pipeline that drives the HIP kernels (vdb_search.cpp).  No CPU
// compute path exists in this library: every distance is produced on the GPU, and every entry point fails with
// VDB_ERR_DEVICE when no HIP device is usable.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "vdb_index.h"
#include "vdb_meta.h"

namespace vdbi {

namespace {
thread_local std::string g_err;
thread_local size_t g_expected = 0, g_actual = 0;
}  // namespace

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
int fail_dim(size_t expected, size_t actual) {
    g_expected = expected;
    g_actual = actual;
    // same text as error.rs:12
    return fail(VDB_ERR_DIMENSION_MISMATCH, "Dimension mismatch: expected %zu, got %zu", expected, actual);
}
// (the texts are compared with the reference's by the tests)
int fail_zero_vector() { return fail(VDB_ERR_INVALID_VECTOR, "Invalid vector: Cannot compute cosine distance with zero vector"); }
int fail_nan() { return fail(VDB_ERR_NAN, "NaN distance (the reference panics here, flat_index.rs:62)"); }
void last_error(std::string* msg, size_t* expected, size_t* actual) {
    if (msg) *msg = g_err;
    if (expected) *expected = g_expected;
    if (actual) *actual = g_actual;
}

}  // namespace vdbi

using namespace vdbi;

// =================================================================== C ABI
extern "C" {

int vdb_abi_version(void) { return 1; }
const char* vdb_build_arch(void) { return "gfx950"; }

void vdb_last_error(char* buf, size_t cap, size_t* expected, size_t* actual) {
    std::string msg;
    vdbi::last_error(&msg, expected, actual);
    if (buf && cap) {
        size_t n = std::min(cap - 1, msg.size());
        memcpy(buf, msg.data(), n);
        buf[n] = 0;
    }
}

int vdb_flat_create(int metric, int device, vdb_flat_index** out) {
    return guarded([&]() -> int {
    if (!out) return fail(VDB_ERR_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
    if (metric < 0 || metric > 2) return fail(VDB_ERR_INVALID_ARGUMENT, "unknown metric %d", metric);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(VDB_ERR_DEVICE, "no HIP device available: this engine has no CPU path");
    if (device < 0 || device >= ndev) return fail(VDB_ERR_INVALID_ARGUMENT, "device %d out of range (%d)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(VDB_ERR_DEVICE, "device %d is %s; the kernels are built for gfx950 only", device, prop.gcnArchName);
    auto ix = std::make_unique<vdb_flat_index>();
    ix->metric = metric;
    ix->device = device;
    ix->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
#ifdef VDB_DIAG
    {
        vdb_knobs& kn = ix->kn;
        auto num = [&](const char* name, uint32_t& dst) { if (const char* e = getenv(name)) { dst = (uint32_t)std::max(0, atoi(e)); kn.any = true; } };
        auto flag = [&](const char* name, bool& dst) { if (getenv(name)) { dst = true; kn.any = true; } };
        if (const char* e = getenv("VDB_EPS_SCALE")) { kn.eps_scale = atof(e); kn.any = true; }
        num("VDB_BF16_ABLATE", kn.bf16_ablate); num("VDB_FUSED_ABLATE", kn.fused_ablate);
        num("VDB_KT16", kn.kt16); num("VDB_SAMPLE16", kn.sample16); num("VDB_SAMPLE", kn.sample); num("VDB_KP_FIRST", kn.kp_first);
        flag("VDB_RR_DEPTH", kn.rr_depth); flag("VDB_SAMPLE_BLOCK", kn.sample_block);
        flag("VDB_FUSED_SHAPE4", kn.shape4); flag("VDB_FUSED_REGSTAGE", kn.regstage); flag("VDB_FUSED_DMA2", kn.dma2);
        if (const char* e = getenv("VDB_FUSED_PIPE")) { kn.fused_pipe = strcmp(e, "0") != 0; kn.any = true; }
    }
#endif
    int rc;
    if ((rc = ix->stream.create(hipStreamNonBlocking)) || (rc = ix->stream_alt.create(hipStreamNonBlocking))) return rc;
    if ((rc = ix->d_scalars.ensure(8))) return rc;
    HIP_TRY(hipMemset(ix->d_scalars, 0, 32));
    ix->wsv.reset(new Workspace[2]);
    ix->wsv[0].stream = ix->stream;
    ix->wsv[1].stream = ix->stream_alt;
    *out = ix.release();
    return VDB_OK;
    });
}

// Only what ordering requires: nothing is freed under a kernel that still runs.  The members free themselves afterwards,
// the streams (declared first) last.
vdb_flat_index::~vdb_flat_index() {
    if (!stream) return;
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(stream);
    (void)hipStreamSynchronize(stream_alt);
}

void vdb_flat_destroy(vdb_flat_index* ix) {
    if (!ix) return;
    if (ix->multi) { multi_destroy(ix); return; }
    delete ix;
}

int vdb_flat_add(vdb_flat_index* ix, uint64_t id, const float* v, size_t dim) {
    return guarded([&]() -> int {
    if (!ix || (!v && dim)) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) return multi_add(ix, id, v, dim);
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    int rc = set_device(ix);
    if (rc) return rc;
    return add_one(ix, id, v, dim);
    });
}

int vdb_flat_add_bulk(vdb_flat_index* ix, const uint64_t* ids, uint64_t first_id, const float* rows, size_t n,
                      size_t dim) {
    return guarded([&]() -> int {
    if (!ix || (!rows && n && dim)) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) return multi_add_bulk(ix, ids, first_id, rows, n, dim, false);
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    int rc = set_device(ix);
    if (rc) return rc;
    if (ix->n_rows() + n > 0xfffffff0ull) return fail(VDB_ERR_INVALID_ARGUMENT, "more than 2^32 rows per index");
    ix->row_ids.reserve(ix->row_ids.size() + n);
    for (size_t i = 0; i < n; ++i) {
        rc = add_one(ix, ids ? ids[i] : first_id + i, rows + i * dim, dim);
        if (rc) return rc;
        // bound the host staging area: upload every 64 MiB
        if (ix->pending.size() * sizeof(float) >= (64u << 20)) {
            if ((rc = flush(ix))) return rc;
        }
    }
    return VDB_OK;
    });
}

int vdb_flat_add_bulk_device(vdb_flat_index* ix, const uint64_t* ids, uint64_t first_id, const float* d_rows,
                             size_t n, size_t dim) {
    return guarded([&]() -> int {
    if (!ix || (!d_rows && n)) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return VDB_OK;
    if (dim == 0) return fail(VDB_ERR_INVALID_ARGUMENT, "dim must be > 0");
    if (ix->multi) return multi_add_bulk(ix, ids, first_id, d_rows, n, dim, true);
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    int rc = set_device(ix);
    if (rc) return rc;
    if (ix->n_rows() + n > 0xfffffff0ull) return fail(VDB_ERR_INVALID_ARGUMENT, "more than 2^32 rows per index");
    adopt_dim(ix, dim);
    if (dim != ix->dim) return fail_dim(ix->dim, dim);   // the device bulk path requires the index dimension
    // overwrite semantics for ids already present
    for (size_t i = 0; i < n; ++i) {
        uint64_t id = ids ? ids[i] : first_id + i;
        if (!ix->id2row.empty() || !ix->misfits.empty()) remove_id(ix, id);
    }
    if (ix->dim != dim) {   // remove_id may have emptied and reset the index
        ix->dim = (uint32_t)dim;
        ix->ld = round_up(ix->dim, vdb::KSTAGE);
    }
    if ((rc = flush(ix))) return rc;
    uint32_t first = ix->n_rows();
    if ((rc = grow(ix, first + (uint32_t)n))) return rc;
    hipStream_t s = ix->stream;
    HIP_TRY(hipMemcpy2DAsync(rows_mut(ix) + (size_t)first * ix->ld, (size_t)ix->ld * 4, d_rows, dim * 4, dim * 4, n,
                             hipMemcpyDeviceToDevice, s));
    ix->row_ids.reserve(first + n);
    ix->id2row.reserve(first + n);
    for (size_t i = 0; i < n; ++i) {
        uint64_t id = ids ? ids[i] : first_id + i;
        uint32_t row = first + (uint32_t)i;
        if (row && id <= ix->row_ids.back()) ix->ids_monotone = false;
        ix->row_ids.push_back(id);
        ix->id_bound = std::max(ix->id_bound, id == ~0ull ? id : id + 1);
        if ((row >> 5) >= ix->live.size()) ix->live.push_back(0u);
        ix->live[row >> 5] |= 1u << (row & 31);
        ++ix->n_live;
        // the same id twice in ONE batch: HashMap::insert is last-wins (flat_index.rs:38-41) -- the earlier row of this
        // call dies (ids stored before the call were removed above)
        auto ins = ix->id2row.emplace(id, row);
        if (!ins.second) { kill_row(ix, ins.first->second); ins.first->second = row; }
    }
    HIP_TRY(hipMemcpyAsync(ix->d_row_ids + first, ix->row_ids.data() + first, n * 8, hipMemcpyHostToDevice, s));
    const MarginPlan mp = margin_plan(ix);
    vdb::RowStatsParams rp{rows_f32(ix), ix->ld, ix->dim, first, first + (uint32_t)n, ix->metric, ix->d_nd,
                           ix->d_alpha, ix->d_beta, ix->d_scalars, ix->d_margin, mp.m_e, mp.m_n, mp.m_b, mp.beta_shrink};
    vdb::launch_row_stats(rp, s);
    if (ix->d_rows16) vdb::launch_rows_to_bf16(rows_f32(ix), ix->d_rows16, ix->ld, first, first + (uint32_t)n, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    ix->n_uploaded = first + (uint32_t)n;
    ix->live_dirty = true;
    ix->zero_valid = false;
    ix->rank_valid = false;
    return VDB_OK;
    });
}

int vdb_flat_load_vector_file(vdb_flat_index* ix, const char* path, uint64_t first_id, size_t* out_count) {
    return guarded([&]() -> int {
    if (!ix || !path) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (out_count) *out_count = 0;
    int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(VDB_ERR_INVALID_ARGUMENT, "cannot open %s", path);
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size < 8) {
        close(fd);
        return fail(VDB_ERR_INVALID_ARGUMENT, "File too small for header");          // mmap.rs:52-54
    }
    void* map = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (map == MAP_FAILED) return fail(VDB_ERR_INVALID_ARGUMENT, "mmap of %s failed", path);
    const unsigned char* b = (const unsigned char*)map;
    auto le32 = [&](size_t o) { return (uint32_t)b[o] | ((uint32_t)b[o + 1] << 8) | ((uint32_t)b[o + 2] << 16) | ((uint32_t)b[o + 3] << 24); };
    const size_t dim = le32(0), count = le32(4);                                      // mmap.rs:161-172
    int rc = VDB_OK;
    if (dim == 0 && count) rc = fail(VDB_ERR_INVALID_ARGUMENT, "vector file with dimension 0");
    else if (dim > 16384) rc = fail(VDB_ERR_INVALID_ARGUMENT, "vector file dimension %zu exceeds the supported 16384", dim);
    // (count * dim * 4 can wrap a size_t -- both come from the file -- so the check divides instead)
    else if (dim && count > ((size_t)st.st_size - 8) / 4 / dim) rc = fail(VDB_ERR_INVALID_ARGUMENT, "vector file truncated: %zu rows of %zu floats do not fit %zu bytes", count, dim, (size_t)st.st_size);
    else if (count) {
        // the body starts at byte 8, so rows are 4-byte aligned; x86 is little-endian like the file
        rc = vdb_flat_add_bulk(ix, nullptr, first_id, (const float*)(b + 8), count, dim);
        if (rc == VDB_OK) rc = vdb_flat_flush(ix);
    }
    munmap(map, (size_t)st.st_size);
    if (rc == VDB_OK && out_count) *out_count = count;
    return rc;
    });
}

int vdb_flat_remove(vdb_flat_index* ix, uint64_t id) {
    return guarded([&]() -> int {
    if (!ix) return fail(VDB_ERR_INVALID_ARGUMENT, "null handle");
    if (ix->multi) return multi_remove(ix, id);
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    int rc = set_device(ix);
    if (rc) return rc;
    return remove_id(ix, id);
    });
}

int vdb_flat_get_vector(vdb_flat_index* ix, uint64_t id, float* out, size_t cap, size_t* dim) {
    return guarded([&]() -> int {
    if (!ix) return fail(VDB_ERR_INVALID_ARGUMENT, "null handle");
    if (ix->multi) return multi_get_vector(ix, id, out, cap, dim);
    std::lock_guard<std::mutex> g(ix->mu);
    int rc = set_device(ix);
    if (rc) return rc;
    auto m = ix->misfits.find(id);
    if (m != ix->misfits.end()) {
        if (dim) *dim = m->second.size();
        if (out) memcpy(out, m->second.data(), std::min(cap, m->second.size()) * sizeof(float));
        return VDB_OK;
    }
    auto it = ix->id2row.find(id);
    if (it == ix->id2row.end()) return fail(VDB_ERR_NOT_FOUND, "Vector not found: %llu", (unsigned long long)id);
    if (ix->store_broken) return fail(VDB_ERR_DEVICE, "the row store is inconsistent after a failed compaction: destroy the handle");
    if (dim) *dim = ix->dim;
    if (!out) return VDB_OK;
    size_t ncopy = std::min<size_t>(cap, ix->dim);
    uint32_t row = it->second;
    if (row >= ix->n_uploaded) {
        memcpy(out, ix->pending.data() + (size_t)(row - ix->n_uploaded) * ix->ld, ncopy * sizeof(float));
    } else {
        HIP_TRY(hipMemcpy(out, rows_f32(ix) + (size_t)row * ix->ld, ncopy * sizeof(float), hipMemcpyDeviceToHost));
    }
    return VDB_OK;
    });
}

size_t vdb_flat_len(const vdb_flat_index* ix) { return !ix ? 0 : ix->multi ? multi_len(ix) : ix->n_live + ix->misfits.size(); }
int vdb_flat_metric(const vdb_flat_index* ix) { return ix ? ix->metric : -1; }
size_t vdb_flat_dim(const vdb_flat_index* ix) { return !ix ? 0 : ix->multi ? multi_dim(ix) : ix->dim; }

int vdb_flat_reserve(vdb_flat_index* ix, size_t rows, size_t dim) {
    return guarded([&]() -> int {
    if (!ix || !dim) return fail(VDB_ERR_INVALID_ARGUMENT, "bad argument");
    if (ix->multi) return multi_reserve(ix, rows, dim);
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    int rc = set_device(ix);
    if (rc) return rc;
    adopt_dim(ix, dim);
    if (dim != ix->dim) return fail_dim(ix->dim, dim);
    if (rows > 0xfffffff0ull) return fail(VDB_ERR_INVALID_ARGUMENT, "more than 2^32 rows per index");
    if ((rc = flush(ix))) return rc;
    return grow(ix, (uint32_t)rows);
    });
}

int vdb_flat_flush(vdb_flat_index* ix) {
    return guarded([&]() -> int {
    if (!ix) return fail(VDB_ERR_INVALID_ARGUMENT, "null handle");
    if (ix->multi) return multi_for_each(ix, [](vdb_flat_index* c) { return vdb_flat_flush(c); });
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    int rc = set_device(ix);
    if (rc) return rc;
    if ((rc = flush(ix))) return rc;
    if (ix->metric == vdb::COSINE && ix->n_uploaded) return ensure_zero_count(ix);
    return VDB_OK;
    });
}

int vdb_flat_compact(vdb_flat_index* ix, int shrink, size_t* out_reclaimed) {
    return guarded([&]() -> int {
    if (!ix) return fail(VDB_ERR_INVALID_ARGUMENT, "null handle");
    if (out_reclaimed) *out_reclaimed = 0;
    if (ix->multi) {
        std::mutex m;
        size_t total = 0;
        int rc = multi_for_each(ix, [&](vdb_flat_index* c) {
            size_t got = 0;
            int r = vdb_flat_compact(c, shrink, &got);
            std::lock_guard<std::mutex> g(m);
            total += got;
            return r;
        });
        if (out_reclaimed) *out_reclaimed = total;
        return rc;
    }
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    int rc = set_device(ix);
    if (rc) return rc;
    return compact_store(ix, shrink != 0, out_reclaimed);
    });
}

int vdb_flat_set_auto_compact(vdb_flat_index* ix, double dead_fraction) {
    return guarded([&]() -> int {
    if (!ix || !(dead_fraction >= 0.0 && dead_fraction < 1.0)) return fail(VDB_ERR_INVALID_ARGUMENT, "dead_fraction must be in [0, 1)");
    if (ix->multi) return multi_for_each(ix, [dead_fraction](vdb_flat_index* c) { return vdb_flat_set_auto_compact(c, dead_fraction); });
    std::lock_guard<std::mutex> g(ix->mu);
    ix->auto_compact = dead_fraction;
    return VDB_OK;
    });
}

int vdb_flat_store_stats(const vdb_flat_index* ix, uint64_t out[8]) {
    return guarded([&]() -> int {
    if (!ix || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) { multi_store_stats(ix, out); return VDB_OK; }
    std::lock_guard<std::mutex> g(const_cast<vdb_flat_index*>(ix)->mu);
    store_stats(ix, out);
    return VDB_OK;
    });
}

size_t vdb_flat_debug_compact_plan(const uint32_t* live, size_t n_rows, size_t bounce_rows, size_t ld, uint32_t* out, size_t cap) {
    size_t n = 0;
    (void)guarded([&]() -> int {
    if (!live || n_rows > 0xfffffff0ull) return VDB_OK;
    const uint32_t B = bounce_rows ? std::max<uint32_t>(32u, (uint32_t)std::min<size_t>(bounce_rows, 0xffffffe0u) & ~31u) : compact_bounce_rows((uint32_t)std::max<size_t>(ld, 1), false);
    std::vector<uint32_t> prefix;
    std::vector<CompactChunk> plan;
    compact_plan(live, (uint32_t)n_rows, B, &prefix, &plan);
    n = plan.size();
    for (size_t i = 0; out && i < std::min(n, cap); ++i) { out[4 * i] = plan[i].a; out[4 * i + 1] = plan[i].b; out[4 * i + 2] = plan[i].dst; out[4 * i + 3] = plan[i].mode; }
    return VDB_OK;
    });
    return n;
}

int vdb_flat_debug_set_compact_bounce(vdb_flat_index* ix, size_t rows) {
    return guarded([&]() -> int {
    if (!ix || rows > 0xffffffe0ull) return fail(VDB_ERR_INVALID_ARGUMENT, "bad argument");
    if (ix->multi) return multi_for_each(ix, [rows](vdb_flat_index* c) { return vdb_flat_debug_set_compact_bounce(c, rows); });
    std::lock_guard<std::mutex> g(ix->mu);
    ix->bounce_rows_override = (uint32_t)rows;
    return VDB_OK;
    });
}

int vdb_flat_search_batch_device(vdb_flat_index* ix, const float* d_queries, size_t nq, size_t dim, size_t k,
                                 const uint64_t* d_id_mask, size_t mask_bits, uint64_t* d_out_ids,
                                 float* d_out_dists, uint32_t* d_out_counts, void* stream) {
    return guarded([&]() -> int {
    if (!ix || (nq && (!d_queries || !d_out_counts || (k && (!d_out_ids || !d_out_dists)))))
        return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) return multi_search_device(ix, d_queries, nq, dim, k, d_id_mask, mask_bits, d_out_ids, d_out_dists, d_out_counts, (hipStream_t)stream);
    std::lock_guard<std::mutex> g(ix->mu);
    Workspace* W;
    int rc = idle_workspace(ix, &W);
    if (rc) return rc;
    return search_device(ix, *W, d_queries, nq, dim, k, d_id_mask, mask_bits, d_out_ids, d_out_dists, d_out_counts,
                         (hipStream_t)stream);
    });
}

int vdb_flat_search_batch_device_begin(vdb_flat_index* ix, const float* d_queries, size_t nq, size_t dim, size_t k,
                                       const uint64_t* d_id_mask, size_t mask_bits, uint64_t* d_out_ids,
                                       float* d_out_dists, uint32_t* d_out_counts, int32_t* d_code, void* stream) {
    return guarded([&]() -> int {
    if (!ix || (nq && (!d_queries || !d_out_counts || (k && (!d_out_ids || !d_out_dists)))))
        return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) return refuse_multi("vdb_flat_search_batch_device_begin");
    ix->mu.lock();
    if (ix->begin_locked) { ix->mu.unlock(); return fail(VDB_ERR_INVALID_ARGUMENT, "a search is already pending on this handle"); }
    if (in_flight(ix)) { ix->mu.unlock(); return refuse_in_flight(); }
    Workspace& W = ix->wsv[0];                                   // (nothing is in flight; _finish takes the same one)
    // (the handle is locked by hand here: an exception must not skip the unlock below)
    int rc = guarded([&]() -> int { return search_part1(ix, W, d_queries, nq, dim, k, d_id_mask, mask_bits, d_out_ids, d_out_dists, d_out_counts, (hipStream_t)stream, true); });
    if (rc == VDB_OK && d_code) {
        hipStream_t s = stream ? (hipStream_t)stream : ix->stream;
        // (a forced hand-over to the slower tiers -- vdb_flat_set_tiers, tests -- rewrites the outputs in _finish whatever the
        // first tier certified: the word says "pending" then, so that a caller exchanging partial results exchanges again)
        if (W.ctx.pending && (ix->tiers & (VDB_TIERS_FORCE_EXACT | VDB_TIERS_FORCE_F32 | VDB_TIERS_FORCE_RETHRESHOLD))) {
            if (hipMemsetD32Async((hipDeviceptr_t)d_code, VDB_PENDING_HOST, 1, s) != hipSuccess) rc = fail(VDB_ERR_DEVICE, "hipMemsetD32Async failed");
        } else if (W.ctx.pending) vdb::launch_write_code(SearchFlags(W.w_flags.p, W.ctx.nq32).status, d_code, s);
        else if (hipMemsetAsync(d_code, 0, 4, s) != hipSuccess) rc = fail(VDB_ERR_DEVICE, "hipMemsetAsync failed");
    }
    if (rc == VDB_OK && !stream) {
        // the work went to the handle's own (non-blocking) stream: whatever the caller enqueues next on the null stream
        // -- the exchange -- must wait for it
        rc = ix->ev_order.create(hipEventDisableTiming);
        if (rc == VDB_OK && (hipEventRecord(ix->ev_order, ix->stream) != hipSuccess || hipStreamWaitEvent(nullptr, ix->ev_order, 0) != hipSuccess))
            rc = fail(VDB_ERR_DEVICE, "stream ordering failed");
    }
    if (rc) {
        if (W.ctx.pending) (void)hipStreamSynchronize(W.ctx.s);
        W.ctx.pending = false; ix->mu.unlock(); return rc;
    }
    ix->begin_locked = true;                                   // released by vdb_flat_search_batch_device_finish (same thread)
    return VDB_OK;
    });
}

int vdb_flat_search_batch_device_finish(vdb_flat_index* ix, int* changed) {
    return guarded([&]() -> int {
    if (!ix) return fail(VDB_ERR_INVALID_ARGUMENT, "null handle");
    if (ix->multi) return refuse_multi("vdb_flat_search_batch_device_finish");
    if (!ix->begin_locked) return fail(VDB_ERR_INVALID_ARGUMENT, "no search pending on this handle");
    Workspace& W = ix->wsv[0];                                   // (the one _begin took)
    int rc = guarded([&]() -> int { return search_part2(ix, W, changed); });
    publish_stats(ix, W);
    W.ctx.pending = false;
    ix->begin_locked = false;
    ix->mu.unlock();
    return rc;
    });
}

int vdb_flat_search_batch_device_submit(vdb_flat_index* ix, const float* d_queries, size_t nq, size_t dim, size_t k,
                                        const uint64_t* d_id_mask, size_t mask_bits, uint64_t* d_out_ids, float* d_out_dists,
                                        uint32_t* d_out_counts, void* stream, int* ticket) {
    return guarded([&]() -> int {
    if (!ix || !ticket || (nq && (!d_queries || !d_out_counts || (k && (!d_out_ids || !d_out_dists)))))
        return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) return refuse_multi("vdb_flat_search_batch_device_submit");
    *ticket = -1;
    std::lock_guard<std::mutex> g(ix->mu);
    if (ix->begin_locked) return fail(VDB_ERR_INVALID_ARGUMENT, "a search is pending between begin and finish");
    if (ix->profile) return fail(VDB_ERR_INVALID_ARGUMENT, "kernel profiling synchronises inside the search: not available for submitted searches");
    int slot = !ix->wsv[0].busy ? 0 : (!ix->wsv[1].busy ? 1 : -1);
    if (slot < 0) return fail(VDB_ERR_INVALID_ARGUMENT, "two searches are already in flight on this handle");
    Workspace& W = ix->wsv[slot];
    int rc = guarded([&]() -> int { return search_part1(ix, W, d_queries, nq, dim, k, d_id_mask, mask_bits, d_out_ids, d_out_dists, d_out_counts, (hipStream_t)stream); });
    if (rc) {
        // part 1 may have failed AFTER kernels were enqueued (a later allocation, a launch error): they could still write the
        // caller's buffers after this return -- wait for them, as _begin does
        hipStream_t s = stream ? (hipStream_t)stream : W.stream;
        if (s) (void)hipStreamSynchronize(s);
        if (ix->wsv[slot ^ 1].stream && !ix->wsv[slot ^ 1].busy) (void)hipStreamSynchronize(ix->wsv[slot ^ 1].stream);   // alternating passes of a large batch
        W.ctx.pending = false; return rc;
    }
    W.busy = true;                              // (a search part 1 answered completely has pending = false: wait() returns at once)
    *ticket = slot;
    return VDB_OK;
    });
}

int vdb_flat_search_batch_device_wait(vdb_flat_index* ix, int ticket) {
    return guarded([&]() -> int {
    if (!ix || ticket < 0 || ticket > 1) return fail(VDB_ERR_INVALID_ARGUMENT, "bad ticket");
    if (ix->multi) return refuse_multi("vdb_flat_search_batch_device_wait");
    std::lock_guard<std::mutex> g(ix->mu);
    if (!ix->wsv[ticket].busy) return fail(VDB_ERR_INVALID_ARGUMENT, "no submitted search behind this ticket");
    int rc = set_device(ix);
    if (rc) return rc;
    Workspace& W = ix->wsv[ticket];
    // (whatever part 2 does -- an exception from its host vectors included -- the ticket is retired: a workspace left busy
    // would refuse add / remove / flush on the handle for ever)
    rc = guarded([&]() -> int { return search_part2(ix, W, nullptr); });
    publish_stats(ix, W);
    W.ctx.pending = false;
    W.busy = false;
    return rc;
    });
}

}  // extern "C"

// The device rows of the query ids of a search by stored id, after the flush.  An id that is not stored fails the batch
// (VDB_ERR_NOT_FOUND names the first); an id whose vector could not be searched with -- a row of another dimension -- fails it
// exactly as the search with that vector would.
static int resolve_query_ids(vdb_flat_index* ix, const uint64_t* ids, size_t nq, std::vector<uint32_t>* rows) {
    rows->assign(nq, 0xffffffffu);
    for (size_t b = 0; b < nq; ++b) {
        auto it = ix->id2row.find(ids[b]);
        if (it != ix->id2row.end()) (*rows)[b] = it->second;
        else if (!ix->misfits.count(ids[b])) return fail(VDB_ERR_NOT_FOUND, "Vector not found: %llu", (unsigned long long)ids[b]);
    }
    size_t checked = ~(size_t)0;
    for (size_t b = 0; b < nq; ++b) {
        const size_t d = (*rows)[b] == 0xffffffffu ? ix->misfits.find(ids[b])->second.size() : ix->dim;
        if (d == checked) continue;
        int rc = query_dim_check(ix, d);
        if (rc) return rc;
        checked = d;
    }
    // (every check passed: no row of another dimension is stored at all, so every query id has a device row)
    for (size_t b = 0; b < nq; ++b)
        if ((*rows)[b] >= ix->n_uploaded) return fail(VDB_ERR_DEVICE, "internal error: row %u of id %llu is not on the device", (*rows)[b], (unsigned long long)ids[b]);
    return VDB_OK;
}

static_assert(vdb::RECOMMEND_MAX_EXAMPLES == VDB_RECOMMEND_MAX_EXAMPLES, "the kernels' LDS set and the public limit");
// The argument checks of vdb_flat_recommend_batch, before any lock or device work; fills r->total and r->mmax.
static int recommend_check(RecommendReq* r, size_t nq) {
    r->total = r->mmax = 0;
    if (nq == 0) return VDB_OK;
    if (!r->offsets || !r->n_pos) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (r->offsets[0] != 0) return fail(VDB_ERR_INVALID_ARGUMENT, "offsets[0] is %zu, not 0", r->offsets[0]);
    for (size_t b = 0; b < nq; ++b) {
        if (r->offsets[b + 1] < r->offsets[b]) return fail(VDB_ERR_INVALID_ARGUMENT, "offsets decrease at request %zu", b);
        const size_t m = r->offsets[b + 1] - r->offsets[b];
        if (m > VDB_RECOMMEND_MAX_EXAMPLES) return fail(VDB_ERR_INVALID_ARGUMENT, "request %zu has %zu examples, more than %d", b, m, VDB_RECOMMEND_MAX_EXAMPLES);
        if (r->n_pos[b] == 0) return fail(VDB_ERR_INVALID_ARGUMENT, "request %zu has no positive example", b);
        if (r->n_pos[b] > m) return fail(VDB_ERR_INVALID_ARGUMENT, "request %zu: %u positives among %zu examples", b, r->n_pos[b], m);
        r->mmax = std::max(r->mmax, m);
    }
    r->total = r->offsets[nq];
    if (r->total > ((size_t)1 << 20)) return fail(VDB_ERR_INVALID_ARGUMENT, "%zu examples in one call, more than 2^20", r->total);
    if (!r->ids) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    return VDB_OK;
}

int vdbi::recommend_stage(RecommendWs& W, const RecommendReq& r, size_t nq, const uint32_t* rows, hipStream_t s, vdb::RecommendLists* L) {
    // offsets [nq + 1] | n_pos [nq] | reciprocals [nq][2] | row numbers [total]
    const size_t o_np = nq + 1, o_rc = o_np + nq, o_row = o_rc + 2 * nq, words = o_row + r.total;
    std::vector<uint32_t> meta(words);
    for (size_t b = 0; b <= nq; ++b) meta[b] = (uint32_t)r.offsets[b];
    for (size_t b = 0; b < nq; ++b) {
        const uint32_t np = r.n_pos[b], nn = (uint32_t)(r.offsets[b + 1] - r.offsets[b]) - np;
        const float rc[2] = {1.0f / (float)np, nn ? 1.0f / (float)nn : 0.0f};   // f32, once, here: the kernel multiplies
        meta[o_np + b] = np;
        memcpy(&meta[o_rc + 2 * b], rc, sizeof(rc));
    }
    memcpy(meta.data() + o_row, rows, r.total * 4);
    int rc;
    if ((rc = W.meta.ensure(words))) return rc;
    if ((rc = W.ids.ensure(r.total))) return rc;
    if ((rc = W.stat.ensure(1))) return rc;
    HIP_TRY(hipMemcpyAsync(W.meta.p, meta.data(), words * 4, hipMemcpyHostToDevice, s));   // (pageable: the copy has left `meta` when this returns)
    HIP_TRY(hipMemcpyAsync(W.ids.p, r.ids, r.total * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(W.stat.p, 0, 4, s));
    *L = vdb::RecommendLists{W.meta.p, W.meta.p + o_np, reinterpret_cast<const float*>(W.meta.p + o_rc), W.meta.p + o_row, W.ids.p};
    return VDB_OK;
}

int vdbi::strike_stage(StrikeBufs B, const HostSearch& r, hipStream_t s) {
    if (r.rec) return VDB_OK;                                      // (recommend_stage has sent the lists and zeroed the counter)
    int rc;
    if ((rc = B.selfid.ensure(r.nq))) return rc;
    if ((rc = B.bystat.ensure(2))) return rc;
    HIP_TRY(hipMemcpyAsync(B.selfid.p, r.by, r.nq * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(B.bystat.p, 0, 8, s));
    return VDB_OK;
}

int vdbi::strike_copy_out(Index* H, const HostSearch& r, StrikeBufs B, const vdb::RecommendLists& L, const Lists& found, size_t kcut, hipStream_t s) {
    uint64_t* d_ids = const_cast<uint64_t*>(found.ids);            // (the search's own output buffers: the strike rewrites them in place)
    float* d_dists = const_cast<float*>(found.dists);
    uint32_t* d_counts = const_cast<uint32_t*>(found.counts);
    uint32_t stat[2] = {0, 0};                                     // struck | cut, valid after the copy-out's synchronisation
    if (r.rec) {
        vdb::StrikeSetParams sp{d_ids, d_dists, d_counts, (uint32_t)found.stride, L.offs, L.ids, (uint32_t)kcut, B.rec.stat.p};
        vdb::launch_strike_set(sp, (uint32_t)r.nq, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(stat, B.rec.stat.p, 4, hipMemcpyDeviceToHost, s));
    } else {
        vdb::StrikeSelfParams sp{d_ids, d_dists, d_counts, (uint32_t)found.stride, B.selfid.p, (uint32_t)kcut, B.bystat.p};
        vdb::launch_strike_self(sp, (uint32_t)r.nq, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(stat, B.bystat.p, 8, hipMemcpyDeviceToHost, s));
    }
    int rc = copy_out(found, r, s);
    if (rc) return rc;
    if (r.rec) { H->recommend_stats[0] = r.nq; H->recommend_stats[1] = r.rec->total; H->recommend_stats[2] = stat[0]; H->recommend_stats[3] = found.stride; }
    else { H->by_id_stats[0] = r.nq; H->by_id_stats[1] = stat[0]; H->by_id_stats[2] = stat[1]; }
    return VDB_OK;
}

static_assert(vdb::MMR_MAX_CANDIDATES == VDB_MMR_MAX_CANDIDATES, "the kernel's LDS arrays and the public limit");
// The second half of a diverse top-k call (r.mmr), on s behind the device search that left the candidate lists `found` at depth
// found.stride: the ids come down, the host's id -> row map names their device rows (the handle is locked and flushed: a candidate
// cannot be missing), the rows go up beside k | lambda | mu of every query in ONE copy, mmr_select_kernel picks at most kcut per
// query, and the picks leave through the copy-out every host-pointer search shares.
static int mmr_copy_out(vdb_flat_index* ix, MmrWs& W, const HostSearch& r, const Lists& found, size_t kcut, hipStream_t s) {
    const size_t nq = r.nq, stride = found.stride, n = nq * stride;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint64_t> ids(n);
    std::vector<uint32_t> cnt(nq);
    HIP_TRY(hipMemcpyAsync(cnt.data(), found.counts, nq * 4, hipMemcpyDeviceToHost, s));
    if (n) HIP_TRY(hipMemcpyAsync(ids.data(), found.ids, n * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // k [nq] | lambda [nq] | mu [nq] | device rows [nq][stride]
    const size_t o_l = nq, o_m = 2 * nq, o_row = 3 * nq, words = o_row + n;
    std::vector<uint32_t> meta(words, 0xffffffffu);
    uint64_t cands = 0, pairs = 0;
    for (size_t b = 0; b < nq; ++b) {
        const size_t c = std::min<size_t>(cnt[b], stride), kq = std::min(r.ks ? r.ks[b] : r.k, kcut), count = std::min(kq, c);
        const float lambda = r.mmr->lambdas ? r.mmr->lambdas[b] : r.mmr->lambda, mu = 1.0f - lambda;   // f32, once, here
        meta[b] = (uint32_t)kq;
        memcpy(&meta[o_l + b], &lambda, 4);
        memcpy(&meta[o_m + b], &mu, 4);
        for (size_t i = 0; i < c; ++i) {
            const uint64_t id = ids[b * stride + i];
            auto it = ix->id2row.find(id);
            if (it == ix->id2row.end() || it->second >= ix->n_uploaded)
                return fail(VDB_ERR_DEVICE, "internal error: candidate %llu has no row on the device", (unsigned long long)id);
            meta[o_row + b * stride + i] = it->second;
        }
        cands += c;
        for (size_t t = 1; t < count; ++t) pairs += c - t;             // the pairs the contract evaluates
    }
    int rc;
    const size_t no = nq * std::max<size_t>(kcut, 1);
    if ((rc = W.meta.ensure(words))) return rc;
    if ((rc = W.outi.ensure(no)) || (rc = W.outd.ensure(no)) || (rc = W.outs.ensure(no))) return rc;
    if ((rc = W.outc.ensure(nq)) || (rc = W.stat.ensure(1))) return rc;
    HIP_TRY(hipMemcpyAsync(W.meta.p, meta.data(), words * 4, hipMemcpyHostToDevice, s));   // (pageable: the copy has left `meta` when this returns)
    const uint64_t ns = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    HIP_TRY(hipMemsetAsync(W.stat.p, 0, 4, s));
    vdb::MmrParams mp{};
    mp.rows = rows_f32(ix); mp.ld = ix->ld; mp.dim = ix->dim; mp.n_rows = ix->n_uploaded; mp.metric = ix->metric;
    mp.ids = found.ids; mp.dists = found.dists; mp.counts = found.counts; mp.cand_rows = W.meta.p + o_row; mp.stride = (uint32_t)stride;
    mp.ks = W.meta.p; mp.lambda = reinterpret_cast<const float*>(W.meta.p + o_l); mp.mu = reinterpret_cast<const float*>(W.meta.p + o_m);
    mp.out_ids = W.outi.p; mp.out_dists = W.outd.p; mp.out_scores = W.outs.p; mp.out_counts = W.outc.p; mp.kout = (uint32_t)kcut;
    mp.status = W.stat.p;
    vdb::launch_mmr_select(mp, (uint32_t)nq, s);
    HIP_TRY(hipGetLastError());
    uint32_t status = 0;                                           // valid after the copy-out's synchronisation
    HIP_TRY(hipMemcpyAsync(&status, W.stat.p, 4, hipMemcpyDeviceToHost, s));
    size_t total = 0;
    if ((rc = copy_out(Lists{W.outi.p, W.outd.p, W.outc.p, nullptr, kcut, W.outs.p}, r, s, &total))) return rc;
    if (status & 2u) return fail(VDB_ERR_DEVICE, "internal error: a candidate row beyond the device store");
    const uint64_t st[8] = {nq, stride, cands, pairs, total, ns, 0, 0};
    memcpy(ix->mmr_stats, st, sizeof(st));
    if (status & 1u) return fail_nan();
    return VDB_OK;
}

vdbi::MaskSrc vdbi::mask_src(const HostSearch& r) {
    return MaskSrc{r.id_mask, r.mask_bits, r.cm ? r.cm->d_words.p : nullptr, r.cm ? (hipEvent_t)r.cm->done : nullptr, r.dm};
}

// A compiled mask serves a search on the device it lives on.
static int compiled_mask_check(const vdb_meta_mask* cm, int dev) {
    if (cm->device != dev) return fail(VDB_ERR_INVALID_ARGUMENT, "the compiled mask lives on device %d, the index on device %d", cm->device, dev);
    return VDB_OK;
}

// vdb_flat_search_batch and vdb_flat_search_batch_filtered: the id mask comes from the host (id_mask, uploaded here) or is a
// compiled one already in HBM (cm: the stream is ordered behind its event, nothing is uploaded); everything below is the same.
// r.dm (vdb_internal::search_batch_device_mask): mask_bits bits at a device address, written on the handle's own stream.
// r.by (vdb_flat_search_batch_by_id; `queries` and `dim` are then unused): the queries are the STORED vectors of these ids.  Their
// device rows are gathered into the query block on the device, the search runs with one result more, and the entry whose id
// equals the query's own is struck from each list on the device before the usual copy-out.
// r.rec (vdb_flat_recommend_batch; `by` is then rec->ids): the queries are FOLDS of stored vectors.  All examples resolve to device
// rows as by-id's queries do, the fold kernel writes the query block straight from d_rows, the search runs with as many results
// more as the longest request has examples, and the set strike removes every example from its request's list.
// r.mmr (vdb_flat_search_batch_mmr, checked by mmr_check): the search runs at the candidate depth instead of k, and mmr_copy_out
// re-ranks its lists on the device before the copy-out; k is the number of picks.
static int search_batch_host(vdb_flat_index* ix, HostSearch r) {
    return guarded([&]() -> int {
    const size_t nq = r.nq;
    const uint64_t* const by = r.by;
    const RecommendReq* const rec = r.rec;
    if (!ix || (nq && ((!r.queries && !by) || !r.counts))) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    if (r.cm) {
        if ((rc = compiled_mask_check(r.cm, ix->multi ? multi_home(ix) : ix->device))) return rc;
        r.mask_bits = r.cm->bits;
    }
    if (ix->multi) {
        if (r.dm) return refuse_multi("a search under a raw device mask");
        return by ? multi_search_by_id(ix, r) : multi_search_host(ix, r);
    }
    size_t kmax;
    if ((rc = batch_shape(r, &kmax))) return rc;
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    if ((rc = set_device(ix))) return rc;
    if (rec) memset(ix->recommend_stats, 0, sizeof(ix->recommend_stats));
    else if (by) memset(ix->by_id_stats, 0, sizeof(ix->by_id_stats));
    if (r.mmr) memset(ix->mmr_stats, 0, sizeof(ix->mmr_stats));
    if (nq == 0) return VDB_OK;
    size_t dim = r.dim;
    std::vector<uint32_t> self_rows;
    if (by) {
        // staged adds and removes first: an id resolves to what the search below sees
        if (nq > 0x7fffffffull / 2) return fail(VDB_ERR_INVALID_ARGUMENT, "batch too large");
        if ((rc = flush(ix))) return rc;
        if ((rc = resolve_query_ids(ix, by, rec ? rec->total : nq, &self_rows))) return rc;
        dim = ix->dim;
    }
    // Index::search returns at most len results; clamp before sizing device buffers
    size_t len = ix->n_live + ix->misfits.size();
    size_t kdev = std::min(kmax, std::max<size_t>(len, 1));
    const size_t kcut = kdev;                                      // by id: what is left of a list after the strike, at most
    if (by) kdev = std::min(kdev + (rec ? rec->mmax : 1), len);    // (k was clamped to len first: k = SIZE_MAX cannot wrap)
    if (r.mmr) kdev = std::min(r.mmr->candidates, std::max<size_t>(len, 1));   // the search runs at the candidate depth; kcut picks leave
    hipStream_t s = ix->stream;
    Workspace& W = ix->wsv[0];                                     // (nothing is in flight: staged into and searched in the first workspace)
    // Small index, a few queries (BASELINE configs[0]: Index::search itself, one query): queries and results go through MAPPED
    // host memory -- the two kernels of the direct path read and write it in place, nothing is copied by the runtime
    if (direct_eligible(ix, ix->n_rows(), nq, kdev) && ix->misfits.empty() && dim == ix->dim && !r.id_mask && !r.cm && !r.dm && !by && !r.mmr) {
        const size_t qb = nq * dim * sizeof(float), ib = nq * kdev * sizeof(uint64_t), db = nq * kdev * sizeof(float), cb = nq * sizeof(uint32_t);
        const size_t o_i = (qb + 15) & ~(size_t)15, o_d = o_i + ib, o_c = o_d + ((db + 15) & ~(size_t)15);
        if ((rc = ensure_host_io(W, o_c + cb))) return rc;
        memcpy(W.h_io, r.queries, qb);
        rc = search_device(ix, W, reinterpret_cast<const float*>(W.h_io.d), nq, dim, kdev, nullptr, 0, reinterpret_cast<uint64_t*>(W.h_io.d + o_i),
                           reinterpret_cast<float*>(W.h_io.d + o_d), reinterpret_cast<uint32_t*>(W.h_io.d + o_c), nullptr);
        if (rc) return rc;
        emit_lists(Lists{reinterpret_cast<const uint64_t*>(W.h_io + o_i), reinterpret_cast<const float*>(W.h_io + o_d),
                         reinterpret_cast<const uint32_t*>(W.h_io + o_c), nullptr, kdev}, r);
        return VDB_OK;
    }
    if ((rc = W.w_qin.ensure(nq * std::max<size_t>(dim, 1)))) return rc;
    if ((rc = W.w_outi.ensure(nq * std::max<size_t>(kdev, 1)))) return rc;
    if ((rc = W.w_outd.ensure(nq * std::max<size_t>(kdev, 1)))) return rc;
    if ((rc = W.w_outc.ensure(nq))) return rc;
    vdb::RecommendLists rl{};
    const StrikeBufs strike{W.w_selfid, W.w_bystat, W.w_rec};
    if (rec) {
        // only the lists go up; the fold reads the examples where they are stored
        if ((rc = recommend_stage(W.w_rec, *rec, nq, self_rows.data(), s, &rl))) return rc;
        vdb::launch_fold_examples(rows_f32(ix), ix->ld, ix->dim, ix->n_uploaded, rl, (uint32_t)nq, W.w_qin.p, s);
        HIP_TRY(hipGetLastError());
    } else if (by) {
        // only the row numbers and the ids go up; the vectors never leave HBM
        if ((rc = W.w_selfrow.ensure(nq))) return rc;
        HIP_TRY(hipMemcpyAsync(W.w_selfrow.p, self_rows.data(), nq * 4, hipMemcpyHostToDevice, s));
        if ((rc = strike_stage(strike, r, s))) return rc;
        vdb::launch_gather_rows(rows_f32(ix), ix->ld, ix->dim, ix->n_uploaded, W.w_selfrow.p, (uint32_t)nq, W.w_qin.p, s);
        HIP_TRY(hipGetLastError());
    } else if (dim) HIP_TRY(hipMemcpyAsync(W.w_qin.p, r.queries, nq * dim * sizeof(float), hipMemcpyHostToDevice, s));
    const uint64_t* d_mask;
    if ((rc = stage_mask(W.w_mask_ids, mask_src(r), s, &d_mask))) return rc;
    if ((rc = search_device(ix, W, W.w_qin.p, nq, dim, kdev, d_mask, r.mask_bits, W.w_outi.p, W.w_outd.p, W.w_outc.p, nullptr))) return rc;
    const Lists found{W.w_outi.p, W.w_outd.p, W.w_outc.p, nullptr, kdev};
    if (by) return strike_copy_out(ix, r, strike, rl, found, kcut, s);
    if (r.mmr) return mmr_copy_out(ix, W.w_mmr, r, found, kcut, s);
    return copy_out(found, r, s);
    });
}

// What every host-pointer shim fills the same way; then the mask in the form the shim got it, and the stored ids the queries
// come from (an empty batch may come without an id array).
static HostSearch host_search(const float* queries, size_t nq, size_t dim, const size_t* ks, size_t k, size_t kstride, uint64_t* out_ids,
                              float* out_dists, size_t* out_counts) {
    HostSearch r;
    r.nq = nq; r.ks = ks; r.k = k; r.kstride = kstride;
    r.ids = out_ids; r.dists = out_dists; r.counts = out_counts;
    r.queries = queries; r.dim = dim;
    return r;
}
static HostSearch under(HostSearch r, const uint64_t* id_mask, size_t mask_bits) { r.id_mask = id_mask; r.mask_bits = mask_bits; return r; }
static HostSearch under(HostSearch r, const vdb_meta_mask* cm) { r.cm = cm; return r; }
static HostSearch of_ids(HostSearch r, const uint64_t* ids, const RecommendReq* rec = nullptr) {
    static const uint64_t none = 0;
    r.by = ids ? ids : &none; r.rec = rec;
    return r;
}

extern "C" {

int vdb_flat_search_batch(vdb_flat_index* ix, const float* queries, size_t nq, size_t dim, const size_t* ks,
                          size_t k, const uint64_t* id_mask, size_t mask_bits, size_t kstride, uint64_t* out_ids,
                          float* out_dists, size_t* out_counts) {
    return search_batch_host(ix, under(host_search(queries, nq, dim, ks, k, kstride, out_ids, out_dists, out_counts), id_mask, mask_bits));
}

int vdb_flat_search_batch_filtered(vdb_flat_index* ix, const float* queries, size_t nq, size_t dim, const size_t* ks, size_t k,
                                   const vdb_meta_mask* mask, size_t kstride, uint64_t* out_ids, float* out_dists,
                                   size_t* out_counts) {
    if (!mask) return fail(VDB_ERR_INVALID_ARGUMENT, "null mask");
    return search_batch_host(ix, under(host_search(queries, nq, dim, ks, k, kstride, out_ids, out_dists, out_counts), mask));
}

// ---- search by stored id (no reference counterpart; search_batch_host with r.by)
int vdb_flat_search_batch_by_id(vdb_flat_index* ix, const uint64_t* query_ids, size_t nq, const size_t* ks, size_t k,
                                const uint64_t* id_mask, size_t mask_bits, size_t kstride, uint64_t* out_ids, float* out_dists,
                                size_t* out_counts) {
    if (nq && !query_ids) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    return search_batch_host(ix, under(of_ids(host_search(nullptr, nq, 0, ks, k, kstride, out_ids, out_dists, out_counts), query_ids), id_mask, mask_bits));
}

int vdb_flat_search_batch_by_id_filtered(vdb_flat_index* ix, const uint64_t* query_ids, size_t nq, const size_t* ks, size_t k,
                                         const vdb_meta_mask* mask, size_t kstride, uint64_t* out_ids, float* out_dists,
                                         size_t* out_counts) {
    if (!mask) return fail(VDB_ERR_INVALID_ARGUMENT, "null mask");
    if (nq && !query_ids) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    return search_batch_host(ix, under(of_ids(host_search(nullptr, nq, 0, ks, k, kstride, out_ids, out_dists, out_counts), query_ids), mask));
}

int vdb_flat_by_id_stats(const vdb_flat_index* ix, uint64_t out[4]) {
    if (!ix || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    memcpy(out, ix->by_id_stats, sizeof(ix->by_id_stats));
    return VDB_OK;
}

// ---- recommend from positive and negative stored ids (no reference counterpart; search_batch_host with r.rec)
int vdb_flat_recommend_batch(vdb_flat_index* ix, const uint64_t* example_ids, const size_t* offsets, const uint32_t* n_pos, size_t nq,
                             const size_t* ks, size_t k, const uint64_t* id_mask, size_t mask_bits, size_t kstride, uint64_t* out_ids,
                             float* out_dists, size_t* out_counts) {
    RecommendReq rec{example_ids, offsets, n_pos};
    int rc = recommend_check(&rec, nq);
    if (rc) return rc;
    return search_batch_host(ix, under(of_ids(host_search(nullptr, nq, 0, ks, k, kstride, out_ids, out_dists, out_counts), example_ids, &rec), id_mask, mask_bits));
}

int vdb_flat_recommend_batch_filtered(vdb_flat_index* ix, const uint64_t* example_ids, const size_t* offsets, const uint32_t* n_pos,
                                      size_t nq, const size_t* ks, size_t k, const vdb_meta_mask* mask, size_t kstride,
                                      uint64_t* out_ids, float* out_dists, size_t* out_counts) {
    if (!mask) return fail(VDB_ERR_INVALID_ARGUMENT, "null mask");
    RecommendReq rec{example_ids, offsets, n_pos};
    int rc = recommend_check(&rec, nq);
    if (rc) return rc;
    return search_batch_host(ix, under(of_ids(host_search(nullptr, nq, 0, ks, k, kstride, out_ids, out_dists, out_counts), example_ids, &rec), mask));
}

int vdb_flat_recommend_stats(const vdb_flat_index* ix, uint64_t out[4]) {
    if (!ix || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    memcpy(out, ix->recommend_stats, sizeof(ix->recommend_stats));
    return VDB_OK;
}

// ---- recommend by best score (no reference counterpart; vdb_search.cpp recommend_best_drive)
static_assert(vdb::RB_MAX_ROWS == VDB_RECOMMEND_BEST_MAX_K, "the walk's candidate list and the public limit");
size_t vdb_flat_recommend_best_depth(size_t k, size_t m, size_t len, int stage) {
    const size_t cap = vdb::RB_MAX_ROWS;
    if (stage == 0) return std::min(len, std::min(cap, std::max(2 * (std::min(k, cap) + std::min(m, cap)), (size_t)32)));
    if (stage == 1) return std::min(len, cap);
    return 0;
}

// The front end of both forms: recommend's argument checks before any lock or device work, then the lock, the flush, the
// examples' device rows (VDB_ERR_NOT_FOUND, VDB_ERR_DIMENSION_MISMATCH as recommend), then the driver.
static int recommend_best_host(vdb_flat_index* ix, HostSearch r, RecommendReq rec, float* out_neg_dists) {
    return guarded([&]() -> int {
    const size_t nq = r.nq;
    int rc;
    if ((rc = recommend_check(&rec, nq))) return rc;
    if (!ix || (nq && !r.counts)) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) return refuse_multi("vdb_flat_recommend_best_batch");
    if (r.cm) {
        if ((rc = compiled_mask_check(r.cm, ix->device))) return rc;
        r.mask_bits = r.cm->bits;
    }
    size_t kmax;
    if ((rc = batch_shape(r, &kmax))) return rc;
    r.scores = out_neg_dists;
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    if ((rc = set_device(ix))) return rc;
    memset(ix->recommend_best_stats, 0, sizeof(ix->recommend_best_stats));
    ix->recommend_best_stats[0] = nq; ix->recommend_best_stats[1] = rec.total;
    if (nq == 0) return VDB_OK;
    // staged adds and removes first: an id resolves to what the searches below see
    if ((rc = flush(ix))) return rc;
    std::vector<uint32_t> ex_rows;
    if ((rc = resolve_query_ids(ix, rec.ids, rec.total, &ex_rows))) return rc;
    return recommend_best_drive(ix, r, rec, ex_rows.data(), kmax);
    });
}

int vdb_flat_recommend_best_batch(vdb_flat_index* ix, const uint64_t* example_ids, const size_t* offsets, const uint32_t* n_pos, size_t nq,
                                  const size_t* ks, size_t k, const uint64_t* id_mask, size_t mask_bits, size_t kstride, uint64_t* out_ids,
                                  float* out_dists, float* out_neg_dists, size_t* out_counts) {
    return recommend_best_host(ix, under(host_search(nullptr, nq, 0, ks, k, kstride, out_ids, out_dists, out_counts), id_mask, mask_bits),
                               RecommendReq{example_ids, offsets, n_pos}, out_neg_dists);
}

int vdb_flat_recommend_best_batch_filtered(vdb_flat_index* ix, const uint64_t* example_ids, const size_t* offsets, const uint32_t* n_pos,
                                           size_t nq, const size_t* ks, size_t k, const vdb_meta_mask* mask, size_t kstride,
                                           uint64_t* out_ids, float* out_dists, float* out_neg_dists, size_t* out_counts) {
    if (!mask) return fail(VDB_ERR_INVALID_ARGUMENT, "null mask");
    return recommend_best_host(ix, under(host_search(nullptr, nq, 0, ks, k, kstride, out_ids, out_dists, out_counts), mask),
                               RecommendReq{example_ids, offsets, n_pos}, out_neg_dists);
}

int vdb_flat_recommend_best_stats(const vdb_flat_index* ix, uint64_t out[8]) {
    if (!ix || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) return refuse_multi("vdb_flat_recommend_best_stats");
    memcpy(out, ix->recommend_best_stats, sizeof(ix->recommend_best_stats));
    return VDB_OK;
}

int vdb_flat_debug_set_recommend_best_route(vdb_flat_index* ix, int mode) {
    return guarded([&]() -> int {
    if (!ix || mode < 0 || mode > 2) return fail(VDB_ERR_INVALID_ARGUMENT, "bad argument");
    if (ix->multi) return refuse_multi("vdb_flat_debug_set_recommend_best_route");
    std::lock_guard<std::mutex> g(ix->mu);
    ix->rb_route = mode;
    return VDB_OK;
    });
}

// ---- discovery search (no reference counterpart; vdb_search.cpp discover_drive)
static_assert(vdb::DISCOVER_MAX_LIST == VDB_DISCOVER_MAX_K && vdb::DISCOVER_MAX_PAIRS == VDB_DISCOVER_MAX_PAIRS, "the kernels' LDS arrays and the public limits");
constexpr size_t DISCOVER_DEPTH_MAX_SHIFT = 10;                    // 2 k 2^10 is beyond the cap for every k >= 1
size_t vdb_flat_discover_depth(size_t k, size_t P, size_t len, int stage) {
    const size_t cap = vdb::DISCOVER_MAX_LIST;
    // (a pair of unrelated examples is satisfied by about half of the rows, so about 2^-P of a list has rank P: room for twice
    // the k_b rows the answered rule waits for, and for the examples the strike removes)
    const size_t Pc = std::min(P, (size_t)DISCOVER_DEPTH_MAX_SHIFT);
    if (stage == 0) return std::min(len, std::min(cap, std::max(((2 * std::min(k, cap)) << Pc) + 2 * Pc + 1, (size_t)64)));
    if (stage == 1) return std::min(len, cap);
    return 0;
}

// The argument checks of vdb_flat_discover_batch that need no handle, before any lock or device work; fills r->pairs and r->pmax.
static int discover_check(DiscoverReq* r, size_t nq) {
    r->pairs = r->pmax = 0;
    if (nq == 0) return VDB_OK;
    if (!r->targets || !r->offsets) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (r->offsets[0] != 0) return fail(VDB_ERR_INVALID_ARGUMENT, "offsets[0] is %zu, not 0", r->offsets[0]);
    for (size_t b = 0; b < nq; ++b) {
        if (r->offsets[b + 1] < r->offsets[b]) return fail(VDB_ERR_INVALID_ARGUMENT, "offsets decrease at request %zu", b);
        const size_t P = r->offsets[b + 1] - r->offsets[b];
        if (P > VDB_DISCOVER_MAX_PAIRS) return fail(VDB_ERR_INVALID_ARGUMENT, "request %zu has %zu pairs, more than %d", b, P, VDB_DISCOVER_MAX_PAIRS);
        r->pmax = std::max(r->pmax, P);
    }
    r->pairs = r->offsets[nq];
    if (nq > ((size_t)1 << 20)) return fail(VDB_ERR_INVALID_ARGUMENT, "%zu requests in one call, more than 2^20", nq);
    if (r->pairs && !r->pair_ids) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    return VDB_OK;
}

// The front end of both forms: the argument checks before any lock or device work, then the lock, the k limit, the flush, the
// examples' device rows (VDB_ERR_NOT_FOUND, VDB_ERR_DIMENSION_MISMATCH as recommend), then the driver.
static int discover_host(vdb_flat_index* ix, HostSearch r, DiscoverReq req, uint32_t* out_ranks) {
    return guarded([&]() -> int {
    const size_t nq = r.nq;
    int rc;
    if ((rc = discover_check(&req, nq))) return rc;
    if (!ix || (nq && !r.counts)) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) return refuse_multi("vdb_flat_discover_batch");
    if (r.cm) {
        if ((rc = compiled_mask_check(r.cm, ix->device))) return rc;
        r.mask_bits = r.cm->bits;
    }
    size_t kmax;
    if ((rc = batch_shape(r, &kmax))) return rc;
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    // (staged adds and removes are counted already: the flush below does not change len)
    const size_t kcut = std::min(kmax, (size_t)ix->n_live + ix->misfits.size());
    if (kcut > VDB_DISCOVER_MAX_K)
        return fail(VDB_ERR_INVALID_ARGUMENT, "a discovery search returns at most %d rows per request, not %zu", VDB_DISCOVER_MAX_K, kcut);
    if ((rc = set_device(ix))) return rc;
    memset(ix->discover_stats, 0, sizeof(ix->discover_stats));
    ix->discover_stats[0] = nq; ix->discover_stats[1] = nq + 2 * req.pairs;
    if (nq == 0) return VDB_OK;
    // staged adds and removes first: an id resolves to what the searches below see
    if ((rc = flush(ix))) return rc;
    // the examples of every request side by side: the target, then p_1 n_1 p_2 n_2 ...
    std::vector<uint64_t> ex_ids;
    ex_ids.reserve(nq + 2 * req.pairs);
    for (size_t b = 0; b < nq; ++b) {
        ex_ids.push_back(req.targets[b]);
        ex_ids.insert(ex_ids.end(), req.pair_ids + 2 * req.offsets[b], req.pair_ids + 2 * req.offsets[b + 1]);
    }
    std::vector<uint32_t> ex_rows;
    if ((rc = resolve_query_ids(ix, ex_ids.data(), ex_ids.size(), &ex_rows))) return rc;
    return discover_drive(ix, r, req, ex_ids.data(), ex_rows.data(), kcut, out_ranks);
    });
}

int vdb_flat_discover_batch(vdb_flat_index* ix, const uint64_t* target_ids, const uint64_t* pair_ids, const size_t* offsets, size_t nq,
                            const size_t* ks, size_t k, const uint64_t* id_mask, size_t mask_bits, size_t kstride, uint64_t* out_ids,
                            float* out_dists, uint32_t* out_ranks, size_t* out_counts) {
    return discover_host(ix, under(host_search(nullptr, nq, 0, ks, k, kstride, out_ids, out_dists, out_counts), id_mask, mask_bits),
                         DiscoverReq{target_ids, pair_ids, offsets}, out_ranks);
}

int vdb_flat_discover_batch_filtered(vdb_flat_index* ix, const uint64_t* target_ids, const uint64_t* pair_ids, const size_t* offsets,
                                     size_t nq, const size_t* ks, size_t k, const vdb_meta_mask* mask, size_t kstride, uint64_t* out_ids,
                                     float* out_dists, uint32_t* out_ranks, size_t* out_counts) {
    if (!mask) return fail(VDB_ERR_INVALID_ARGUMENT, "null mask");
    return discover_host(ix, under(host_search(nullptr, nq, 0, ks, k, kstride, out_ids, out_dists, out_counts), mask),
                         DiscoverReq{target_ids, pair_ids, offsets}, out_ranks);
}

int vdb_flat_discover_stats(const vdb_flat_index* ix, uint64_t out[8]) {
    if (!ix || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) return refuse_multi("vdb_flat_discover_stats");
    memcpy(out, ix->discover_stats, sizeof(ix->discover_stats));
    return VDB_OK;
}

int vdb_flat_debug_set_discover_route(vdb_flat_index* ix, int mode) {
    return guarded([&]() -> int {
    if (!ix || mode < 0 || mode > 2) return fail(VDB_ERR_INVALID_ARGUMENT, "bad argument");
    if (ix->multi) return refuse_multi("vdb_flat_debug_set_discover_route");
    std::lock_guard<std::mutex> g(ix->mu);
    ix->discover_route = mode;
    return VDB_OK;
    });
}

// ---- diverse top-k (no reference counterpart; search_batch_host with r.mmr)
// The checks of include/vdb_flat.h "DIVERSE TOP-K" item 8, in its order, before any lock or device work.  *done: the call is
// answered (an empty index, or no query asks for a row).
static int mmr_check(const vdb_flat_index* ix, const HostSearch& r, const MmrReq& m, bool* done) {
    *done = false;
    if (!ix || (r.nq && !r.counts)) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (r.nq == 0) return VDB_OK;
    size_t kmax = r.ks ? 0 : r.k;
    for (size_t b = 0; r.ks && b < r.nq; ++b) kmax = std::max(kmax, r.ks[b]);
    if (kmax == 0 || vdb_flat_len(ix) == 0) {
        for (size_t b = 0; b < r.nq; ++b) r.counts[b] = 0;
        *done = true;
        return VDB_OK;
    }
    if (!r.queries || !r.ids || !r.dists) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    for (size_t b = 0; b < (m.lambdas ? r.nq : 1); ++b) {
        const float l = m.lambdas ? m.lambdas[b] : m.lambda;
        if (!(l >= 0.0f && l <= 1.0f)) return fail(VDB_ERR_INVALID_ARGUMENT, "lambda %g is not within [0, 1]", (double)l);
    }
    if (m.candidates == 0) return fail(VDB_ERR_INVALID_ARGUMENT, "candidates is 0");
    if (m.candidates > VDB_MMR_MAX_CANDIDATES) return fail(VDB_ERR_INVALID_ARGUMENT, "%zu candidates, more than %d", m.candidates, VDB_MMR_MAX_CANDIDATES);
    if (kmax > m.candidates) return fail(VDB_ERR_INVALID_ARGUMENT, "the largest k %zu is above the %zu candidates", kmax, m.candidates);
    if (ix->multi) return refuse_multi("vdb_flat_search_batch_mmr");
    return VDB_OK;
}

static int search_mmr_host(vdb_flat_index* ix, HostSearch r, MmrReq m, float* out_scores) {
    r.scores = out_scores; r.mmr = &m;
    bool done = false;
    int rc = guarded([&]() -> int { return mmr_check(ix, r, m, &done); });
    if (rc || done || r.nq == 0) {
        if (!rc && ix && !ix->multi) { std::lock_guard<std::mutex> g(ix->mu); memset(ix->mmr_stats, 0, sizeof(ix->mmr_stats)); ix->mmr_stats[0] = r.nq; }
        return rc;
    }
    return search_batch_host(ix, r);
}

int vdb_flat_search_batch_mmr(vdb_flat_index* ix, const float* queries, size_t nq, size_t dim, const size_t* ks, size_t k,
                              size_t candidates, const float* lambdas, float lambda, const uint64_t* id_mask, size_t mask_bits,
                              size_t kstride, uint64_t* out_ids, float* out_dists, float* out_scores, size_t* out_counts) {
    return search_mmr_host(ix, under(host_search(queries, nq, dim, ks, k, kstride, out_ids, out_dists, out_counts), id_mask, mask_bits),
                           MmrReq{candidates, lambdas, lambda}, out_scores);
}

int vdb_flat_search_batch_mmr_filtered(vdb_flat_index* ix, const float* queries, size_t nq, size_t dim, const size_t* ks, size_t k,
                                       size_t candidates, const float* lambdas, float lambda, const vdb_meta_mask* mask, size_t kstride,
                                       uint64_t* out_ids, float* out_dists, float* out_scores, size_t* out_counts) {
    if (!mask) return fail(VDB_ERR_INVALID_ARGUMENT, "null mask");
    return search_mmr_host(ix, under(host_search(queries, nq, dim, ks, k, kstride, out_ids, out_dists, out_counts), mask),
                           MmrReq{candidates, lambdas, lambda}, out_scores);
}

int vdb_flat_mmr_stats(const vdb_flat_index* ix, uint64_t out[8]) {
    if (!ix || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) return refuse_multi("vdb_flat_mmr_stats");
    memcpy(out, ix->mmr_stats, sizeof(ix->mmr_stats));
    return VDB_OK;
}

// ---- one nearest row per group (no reference counterpart; vdb_search.cpp distinct_drive)
size_t vdb_flat_distinct_depth(size_t k, size_t len, int stage) {
    const size_t cap = vdb::DISTINCT_MAX_LIST;
    if (stage == 0) return std::min(len, std::min(cap, std::max(k > cap / 4 ? cap : 4 * k, (size_t)32)));
    if (stage == 1) return std::min(len, cap);
    return 0;
}

// pg: the call is vdb_flat_search_batch_per_group -- the same checks, locks and flushes, then per_group_drive
static int search_distinct_host(vdb_flat_index* ix, HostSearch r, vdb_meta_table* table, uint32_t slot, const PerGroupOut* pg = nullptr) {
    return guarded([&]() -> int {
    const size_t nq = r.nq, dim = r.dim;
    if (!ix || (nq && (!r.queries || !r.counts))) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    size_t kmax;
    int rc;
    if ((rc = batch_shape(r, &kmax))) return rc;
    std::lock_guard<std::mutex> g(ix->mu);                         // (a sharded parent's lock too: the shards are searched under it)
    if (!ix->multi && in_flight(ix)) return refuse_in_flight();
    memset(ix->distinct_stats, 0, sizeof(ix->distinct_stats));
    ix->distinct_stats[0] = nq;
    if (pg) {
        memset(ix->per_group_stats, 0, sizeof(ix->per_group_stats));
        ix->per_group_stats[0] = nq;
    }
    if (nq == 0) return VDB_OK;
    const int dev = ix->multi ? multi_home(ix) : ix->device;
    const size_t len = ix->multi ? multi_len(ix) : ix->n_live + ix->misfits.size();
    if (len == 0 || kmax == 0) {                                   // storage.rs:218-220: empty store -> Ok(vec![]) before any check
        for (size_t b = 0; b < nq; ++b) r.counts[b] = 0;
        return VDB_OK;
    }
    // every refusal below comes before any device search
    if (pg) {
        if (pg->g == 0 || pg->g > VDB_PER_GROUP_MAX_SIZE)
            return fail(VDB_ERR_INVALID_ARGUMENT, "group_size %zu outside [1, %d]", pg->g, VDB_PER_GROUP_MAX_SIZE);
        if (!pg->sizes) return fail(VDB_ERR_INVALID_ARGUMENT, "null out_sizes");
    }
    int tdev = 0;
    if ((rc = meta_column_check(table, slot, &tdev))) return rc;
    if (kmax > vdb::DISTINCT_MAX_LIST) return fail(VDB_ERR_INVALID_ARGUMENT, "a search by group returns at most %u rows per query, not %zu", vdb::DISTINCT_MAX_LIST, kmax);
    if (tdev != dev) return fail(VDB_ERR_INVALID_ARGUMENT, "the metadata table lives on device %d, the index on device %d", tdev, dev);
    const uint64_t id_bound = ix->multi ? multi_id_bound(ix) : ix->id_bound;
    if (id_bound > (1ull << 32)) return fail(VDB_ERR_INVALID_ARGUMENT, "the index has held an id at or above 2^32: a metadata table cannot describe it");
    if (r.cm) {
        if ((rc = compiled_mask_check(r.cm, dev))) return rc;
        r.mask_bits = r.cm->bits;
    }
    // (the member rows of a sharded handle live on several devices: the limit vdb_flat_search_batch_mmr has)
    if (pg && ix->multi) return fail(VDB_ERR_INVALID_ARGUMENT, "vdb_flat_search_batch_per_group is not available on a sharded handle (vdb_flat_create_sharded)");
    if (nq > 0x3fffffffull) return fail(VDB_ERR_INVALID_ARGUMENT, "batch too large");
    HIP_TRY(hipSetDevice(dev));
    // staged adds first, then the table's staged column writes; the handle's stream waits for those by an event
    if ((rc = ix->multi ? multi_flush_nolock(ix) : flush(ix))) return rc;
    hipStream_t s = ix->multi ? multi_home_stream(ix) : (hipStream_t)ix->stream;
    MetaColumn col;
    if ((rc = meta_column_acquire(table, slot, s, &col))) return rc;
    struct Release { vdb_meta_table* t; ~Release() { meta_column_release(t); } } release{table};
    DistinctArgs a{r, kmax, len, col.d_codes, col.len, id_bound, (uint32_t)ix->n_cu};
    DistinctSearch search;
    if (ix->multi)
        search = [&](const float* d_q, size_t n, size_t depth, const uint64_t* d_mask, size_t bits, uint64_t* oi, float* od, uint32_t* oc) {
            return multi_search_nolock(ix, d_q, n, dim, depth, d_mask, bits, oi, od, oc);
        };
    else
        search = [&](const float* d_q, size_t n, size_t depth, const uint64_t* d_mask, size_t bits, uint64_t* oi, float* od, uint32_t* oc) {
            return search_device(ix, ix->wsv[0], d_q, n, dim, depth, d_mask, bits, oi, od, oc, nullptr);   // (nothing is in flight)
        };
    return pg ? per_group_drive(ix, s, search, a, *pg) : distinct_drive(ix, s, search, a);
    });
}

int vdb_flat_search_batch_distinct(vdb_flat_index* ix, const float* queries, size_t nq, size_t dim, const size_t* ks, size_t k,
                                   vdb_meta_table* table, uint32_t slot, const uint64_t* id_mask, size_t mask_bits, size_t kstride,
                                   uint64_t* out_ids, float* out_dists, int32_t* out_codes, size_t* out_counts) {
    HostSearch r = under(host_search(queries, nq, dim, ks, k, kstride, out_ids, out_dists, out_counts), id_mask, mask_bits);
    r.codes = out_codes;
    return search_distinct_host(ix, r, table, slot);
}

int vdb_flat_search_batch_distinct_filtered(vdb_flat_index* ix, const float* queries, size_t nq, size_t dim, const size_t* ks, size_t k,
                                            vdb_meta_table* table, uint32_t slot, const vdb_meta_mask* mask, size_t kstride,
                                            uint64_t* out_ids, float* out_dists, int32_t* out_codes, size_t* out_counts) {
    if (!mask) return fail(VDB_ERR_INVALID_ARGUMENT, "null mask");
    HostSearch r = under(host_search(queries, nq, dim, ks, k, kstride, out_ids, out_dists, out_counts), mask);
    r.codes = out_codes;
    return search_distinct_host(ix, r, table, slot);
}

int vdb_flat_distinct_stats(const vdb_flat_index* ix, uint64_t out[8]) {
    if (!ix || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    memcpy(out, ix->distinct_stats, sizeof(ix->distinct_stats));
    return VDB_OK;
}

// ---- up to g rows of each of the k nearest groups (no reference counterpart; vdb_search.cpp per_group_drive)
int vdb_flat_search_batch_per_group(vdb_flat_index* ix, const float* queries, size_t nq, size_t dim, const size_t* ks, size_t k,
                                    size_t group_size, vdb_meta_table* table, uint32_t slot, const uint64_t* id_mask, size_t mask_bits,
                                    size_t kstride, uint64_t* out_ids, float* out_dists, int32_t* out_codes, uint32_t* out_sizes,
                                    size_t* out_counts) {
    HostSearch r = under(host_search(queries, nq, dim, ks, k, kstride, out_ids, out_dists, out_counts), id_mask, mask_bits);
    r.codes = out_codes;
    const PerGroupOut pg{group_size, out_sizes};
    return search_distinct_host(ix, r, table, slot, &pg);
}

int vdb_flat_search_batch_per_group_filtered(vdb_flat_index* ix, const float* queries, size_t nq, size_t dim, const size_t* ks, size_t k,
                                             size_t group_size, vdb_meta_table* table, uint32_t slot, const vdb_meta_mask* mask,
                                             size_t kstride, uint64_t* out_ids, float* out_dists, int32_t* out_codes, uint32_t* out_sizes,
                                             size_t* out_counts) {
    if (!mask) return fail(VDB_ERR_INVALID_ARGUMENT, "null mask");
    HostSearch r = under(host_search(queries, nq, dim, ks, k, kstride, out_ids, out_dists, out_counts), mask);
    r.codes = out_codes;
    const PerGroupOut pg{group_size, out_sizes};
    return search_distinct_host(ix, r, table, slot, &pg);
}

int vdb_flat_per_group_stats(const vdb_flat_index* ix, uint64_t out[8]) {
    if (!ix || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) return refuse_multi("vdb_flat_per_group_stats");
    memcpy(out, ix->per_group_stats, sizeof(ix->per_group_stats));
    return VDB_OK;
}

size_t vdb_flat_debug_per_group_plan(const int32_t* codes, const uint32_t* kept, const size_t* ks, size_t nq, size_t kmax, int32_t* wanted,
                                     size_t cap, uint32_t* index) {
    size_t n = 0;
    (void)guarded([&]() -> int {
    if ((nq && !kept) || (nq && kmax && !codes) || nq > 0x3fffffffull || kmax > vdb::DISTINCT_MAX_LIST) { n = ~(size_t)0; return VDB_OK; }
    std::vector<int32_t> w;
    std::vector<uint32_t> at;
    per_group_plan(codes, kept, ks, nq, kmax, &w, &at);
    n = w.size();
    for (size_t i = 0; wanted && i < std::min(n, cap); ++i) wanted[i] = w[i];
    for (size_t i = 0; index && i < nq * kmax; ++i) index[i] = at[i];
    return VDB_OK;
    });
    return n;
}

int vdb_flat_debug_set_per_group_scan_cap(vdb_flat_index* ix, size_t rows) {
    return guarded([&]() -> int {
    if (!ix) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) return refuse_multi("vdb_flat_debug_set_per_group_scan_cap");
    if (rows > SPARSE_MAX_E) return fail(VDB_ERR_INVALID_ARGUMENT, "a scan cap of %zu rows is above the capacity %u", rows, SPARSE_MAX_E);
    std::lock_guard<std::mutex> g(ix->mu);
    ix->per_group_scan_cap = (uint32_t)rows;
    return VDB_OK;
    });
}

}  // extern "C"

// ---- one batch, a filter per query (no reference counterpart; vdb_search.cpp search_grouped).  The masks come from
// the host (id_masks: n_masks x words, the referenced ones uploaded here) or are compiled ones already in HBM (cms).
static int search_grouped_host(vdb_flat_index* ix, const char* what, const HostSearch& r, const uint64_t* id_masks,
                               const vdb_meta_mask* const* cms, bool compiled, size_t n_masks, const uint32_t* group_of) {
    return guarded([&]() -> int {
    const size_t nq = r.nq, dim = r.dim, mask_bits = r.mask_bits;
    if (!ix || (nq && (!r.queries || !r.counts))) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) return refuse_multi(what);
    size_t kmax;
    int rc;
    if ((rc = batch_shape(r, &kmax))) return rc;
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    memset(ix->grouped_stats, 0, sizeof(ix->grouped_stats));
    ix->grouped_stats[0] = nq;
    if (nq == 0) return VDB_OK;
    const size_t len = ix->n_live + ix->misfits.size();
    if (len == 0 || kmax == 0) {                                   // storage.rs:218-220: empty store -> Ok(vec![]) before any check
        for (size_t b = 0; b < nq; ++b) r.counts[b] = 0;
        return VDB_OK;
    }
    // ---- argument errors, before any device work
    if (!group_of) return fail(VDB_ERR_INVALID_ARGUMENT, "null group_of");
    for (size_t b = 0; b < nq; ++b)
        if (group_of[b] != VDB_GROUP_NONE && group_of[b] >= n_masks)
            return fail(VDB_ERR_INVALID_ARGUMENT, "query %zu names mask %u of %zu", b, group_of[b], n_masks);
    if (n_masks > 1024) return fail(VDB_ERR_INVALID_ARGUMENT, "%zu masks: a grouped search takes at most 1024", n_masks);
    if (n_masks && (compiled ? !cms : !id_masks)) return fail(VDB_ERR_INVALID_ARGUMENT, "null mask array");
    // the referenced masks, in the order of their indices: slot[b] = the query's place among them
    std::vector<uint32_t> place(n_masks, VDB_GROUP_NONE), ref, slot(nq);
    for (size_t b = 0; b < nq; ++b)
        if (group_of[b] != VDB_GROUP_NONE) place[group_of[b]] = 0;
    for (size_t m = 0; m < n_masks; ++m)
        if (place[m] == 0) { place[m] = (uint32_t)ref.size(); ref.push_back((uint32_t)m); }
    for (size_t b = 0; b < nq; ++b) slot[b] = group_of[b] == VDB_GROUP_NONE ? VDB_GROUP_NONE : place[group_of[b]];
    const size_t R = ref.size();
    if (compiled)
        for (uint32_t m : ref) {
            if (!cms[m]) return fail(VDB_ERR_INVALID_ARGUMENT, "mask %u is null", m);
            if ((rc = compiled_mask_check(cms[m], ix->device))) return rc;
        }
    if (nq > 0x3fffffffull) return fail(VDB_ERR_INVALID_ARGUMENT, "batch too large");
    ix->grouped_stats[1] = R;
    if ((rc = set_device(ix))) return rc;
    if ((rc = flush(ix))) return rc;                               // staged adds first
    const size_t kdev = std::min(kmax, std::max<size_t>(len, 1));  // Index::search returns at most len results
    hipStream_t s = ix->stream;
    GroupedWs& G = ix->gws;
    if ((rc = G.q.ensure(nq * std::max<size_t>(dim, 1))) || (rc = G.oi.ensure(nq * kdev)) || (rc = G.od.ensure(nq * kdev)) || (rc = G.oc.ensure(nq)) ||
        (rc = G.desc.ensure(std::max<size_t>(R, 1))))
        return rc;
    if (dim) HIP_TRY(hipMemcpyAsync(G.q.p, r.queries, nq * dim * sizeof(float), hipMemcpyHostToDevice, s));
    std::vector<vdb::GroupedMask> desc(R);
    if (compiled) {
        for (size_t j = 0; j < R; ++j) {
            const vdb_meta_mask* cm = cms[ref[j]];
            HIP_TRY(hipStreamWaitEvent(s, cm->done, 0));
            desc[j] = vdb::GroupedMask{cm->d_words, cm->bits};
        }
    } else {
        // (R masks side by side in ONE buffer: not the single-mask stager of vdb_hostio.h)
        const size_t words = (mask_bits + 63) / 64;
        if ((rc = G.masks.ensure(std::max<size_t>(R * words, 1)))) return rc;
        for (size_t j = 0; j < R; ++j) {
            if (words) HIP_TRY(hipMemcpyAsync(G.masks.p + j * words, id_masks + (size_t)ref[j] * words, words * 8, hipMemcpyHostToDevice, s));
            desc[j] = vdb::GroupedMask{G.masks.p + j * words, mask_bits};
        }
    }
    if (R) HIP_TRY(hipMemcpyAsync(G.desc.p, desc.data(), R * sizeof(vdb::GroupedMask), hipMemcpyHostToDevice, s));
    GroupedArgs a{G.q.p, nq, dim, kdev, slot.data(), G.desc.p, desc.data(), R, G.oi.p, G.od.p, G.oc.p};
    if ((rc = search_grouped(ix, ix->wsv[0], s, a))) {                // (nothing is in flight: the first workspace)
        (void)hipStreamSynchronize(s);                             // (desc and the plan are host vectors of this frame)
        return rc;
    }
    return copy_out(Lists{G.oi.p, G.od.p, G.oc.p, nullptr, kdev}, r, s);
    });
}

extern "C" {

int vdb_flat_search_batch_grouped(vdb_flat_index* ix, const float* queries, size_t nq, size_t dim, const size_t* ks, size_t k,
                                  const uint64_t* id_masks, size_t n_masks, size_t mask_bits, const uint32_t* group_of, size_t kstride,
                                  uint64_t* out_ids, float* out_dists, size_t* out_counts) {
    // (mask_bits: of every one of the n_masks host masks)
    return search_grouped_host(ix, "vdb_flat_search_batch_grouped", under(host_search(queries, nq, dim, ks, k, kstride, out_ids, out_dists, out_counts), nullptr, mask_bits),
                               id_masks, nullptr, false, n_masks, group_of);
}

int vdb_flat_search_batch_grouped_filtered(vdb_flat_index* ix, const float* queries, size_t nq, size_t dim, const size_t* ks, size_t k,
                                           const vdb_meta_mask* const* masks, size_t n_masks, const uint32_t* group_of, size_t kstride,
                                           uint64_t* out_ids, float* out_dists, size_t* out_counts) {
    return search_grouped_host(ix, "vdb_flat_search_batch_grouped_filtered", host_search(queries, nq, dim, ks, k, kstride, out_ids, out_dists, out_counts),
                               nullptr, masks, true, n_masks, group_of);
}

int vdb_flat_grouped_stats(const vdb_flat_index* ix, uint64_t out[8]) {
    return guarded([&]() -> int {
    if (!ix || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) return refuse_multi("vdb_flat_grouped_stats");
    memcpy(out, ix->grouped_stats, sizeof(ix->grouped_stats));
    return VDB_OK;
    });
}

size_t vdb_flat_debug_group_plan(const uint32_t* group_of, size_t nq, const uint32_t* elig, size_t n_masks, uint32_t* perm, uint32_t* tiles,
                                 size_t cap) {
    size_t n = 0;
    (void)guarded([&]() -> int {
    if ((nq && !group_of) || (n_masks && !elig) || nq > 0x3fffffffull) { n = ~(size_t)0; return VDB_OK; }
    GroupPlan plan;
    if (!group_plan(group_of, nq, elig, n_masks, true, &plan)) { n = ~(size_t)0; return VDB_OK; }
    n = plan.tiles.size();
    for (size_t i = 0; perm && i < nq; ++i) perm[i] = plan.perm[i];
    for (size_t i = 0; tiles && i < std::min(n, cap); ++i) {
        tiles[4 * i] = plan.tiles[i].group; tiles[4 * i + 1] = plan.tiles[i].j0; tiles[4 * i + 2] = plan.tiles[i].q0; tiles[4 * i + 3] = plan.tiles[i].nq;
    }
    return VDB_OK;
    });
    return n;
}

int vdb_flat_search(vdb_flat_index* ix, const float* query, size_t dim, size_t k, uint64_t* out_ids,
                    float* out_dists, size_t* out_count) {
    return guarded([&]() -> int {
    if (!out_count) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    return vdb_flat_search_batch(ix, query, 1, dim, nullptr, k, nullptr, 0, k, out_ids, out_dists, out_count);
    });
}

// the merge kernels index keys with 32 bits and launch up to nq * nparts*k / 256 workgroups
// ---- exact range search (vdb_search.cpp range_search_device)
int vdb_flat_range_search_batch_device(vdb_flat_index* ix, const float* d_queries, size_t nq, size_t dim, const float* d_radii,
                                       const uint64_t* d_id_mask, size_t mask_bits, size_t max_results, uint64_t* d_out_ids,
                                       float* d_out_dists, uint32_t* d_out_counts, uint64_t* d_out_totals, void* stream) {
    return guarded([&]() -> int {
    if (!ix || (nq && (!d_queries || !d_radii || !d_out_counts || !d_out_ids || !d_out_dists)))
        return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) return refuse_multi("vdb_flat_range_search_batch_device");
    std::lock_guard<std::mutex> g(ix->mu);
    if (ix->begin_locked) return fail(VDB_ERR_INVALID_ARGUMENT, "a search is pending between begin and finish");
    return range_search_device(ix, d_queries, nq, dim, d_radii, d_id_mask, mask_bits, max_results, d_out_ids, d_out_dists,
                               d_out_counts, d_out_totals, (hipStream_t)stream);
    });
}

int vdb_flat_range_search_batch(vdb_flat_index* ix, const float* queries, size_t nq, size_t dim, const float* radii, float radius,
                                const uint64_t* id_mask, size_t mask_bits, size_t max_results, uint64_t* out_ids, float* out_dists,
                                size_t* out_counts, uint64_t* out_totals) {
    return guarded([&]() -> int {
    if (!ix || (nq && (!queries || !out_counts || !out_ids || !out_dists))) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) return refuse_multi("vdb_flat_range_search_batch");
    if (max_results == 0 || max_results > MAX_SELECT)
        return fail(VDB_ERR_INVALID_ARGUMENT, "max_results %zu outside [1, %u]", max_results, MAX_SELECT);
    std::vector<float> rad(nq, radius);
    if (radii) std::copy(radii, radii + nq, rad.begin());
    for (size_t b = 0; b < nq; ++b)
        if (rad[b] != rad[b]) return fail(VDB_ERR_INVALID_ARGUMENT, "the radius of query %zu is NaN", b);
    std::lock_guard<std::mutex> g(ix->mu);
    if (ix->begin_locked) return fail(VDB_ERR_INVALID_ARGUMENT, "a search is pending between begin and finish");
    if (in_flight(ix)) return refuse_in_flight();
    int rc = set_device(ix);
    if (rc) return rc;
    if (nq == 0) return VDB_OK;
    Workspace* W = &ix->wsv[0];
    hipStream_t s = ix->stream;
    if ((rc = W->w_qin.ensure(nq * std::max<size_t>(dim, 1)))) return rc;
    if ((rc = W->w_radii.ensure(nq))) return rc;
    if ((rc = W->w_outi.ensure(nq * max_results))) return rc;
    if ((rc = W->w_outd.ensure(nq * max_results))) return rc;
    if ((rc = W->w_outc.ensure(nq))) return rc;
    if ((rc = W->w_totals.ensure(nq))) return rc;
    if (dim) HIP_TRY(hipMemcpyAsync(W->w_qin.p, queries, nq * dim * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(W->w_radii.p, rad.data(), nq * sizeof(float), hipMemcpyHostToDevice, s));
    const uint64_t* d_mask;
    if ((rc = stage_mask(W->w_mask_ids, MaskSrc{id_mask, mask_bits}, s, &d_mask))) return rc;
    rc = range_search_device(ix, W->w_qin.p, nq, dim, W->w_radii.p, d_mask, mask_bits, max_results, W->w_outi.p, W->w_outd.p,
                             W->w_outc.p, W->w_totals.p, nullptr);
    if (rc) return rc;
    // every list has room for max_results entries: the caller's stride is the device's.  The totals come down with the lists.
    std::vector<uint64_t> tot(nq);
    HIP_TRY(hipMemcpyAsync(tot.data(), W->w_totals.p, nq * 8, hipMemcpyDeviceToHost, s));
    Batch out;
    out.nq = nq; out.k = out.kstride = max_results;
    out.ids = out_ids; out.dists = out_dists; out.counts = out_counts;
    if ((rc = copy_out(Lists{W->w_outi.p, W->w_outd.p, W->w_outc.p, nullptr, max_results}, out, s))) return rc;
    if (out_totals) std::copy(tot.begin(), tot.end(), out_totals);
    return VDB_OK;
    });
}

int vdb_flat_range_stats(const vdb_flat_index* ix, uint64_t out[8]) {
    if (!ix || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) return refuse_multi("vdb_flat_range_stats");
    memcpy(out, ix->range_stats, sizeof(ix->range_stats));
    return VDB_OK;
}

static bool merge_fits(size_t nparts, size_t nq, size_t k) {
    if (nparts && k > 0xffffffffull / nparts) return false;
    const unsigned long long bpq = (nparts * k + 255) / 256;
    return nq <= 0x7fffffffull && (!bpq || nq <= 0x7fffffffull / bpq);
}

int vdb_merge_topk_device(int device, const uint64_t* d_part_ids, const float* d_part_dists,
                          const uint32_t* d_part_counts, size_t nparts, size_t nq, size_t k, uint64_t* d_out_ids,
                          float* d_out_dists, uint32_t* d_out_counts, void* stream) {
    return guarded([&]() -> int {
    if (!d_part_ids || !d_part_dists || !d_part_counts || !d_out_ids || !d_out_dists || !d_out_counts)
        return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (!merge_fits(nparts, nq, k)) return fail(VDB_ERR_INVALID_ARGUMENT, "nq = %zu queries of nparts*k = %zu keys: too large", nq, nparts * k);
    HIP_TRY(hipSetDevice(device));
    vdb::launch_merge_parts(d_part_ids, d_part_dists, d_part_counts, (uint32_t)nparts, (uint32_t)nq, (uint32_t)k,
                            d_out_ids, d_out_dists, d_out_counts, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return VDB_OK;
    });
}

int vdb_flat_distances_batch(vdb_flat_index* ix, const float* queries, size_t nq, size_t dim, const size_t* offsets,
                             const uint64_t* ids, float* out_dists) {
    return guarded([&]() -> int {
    if (!ix || !offsets || (nq && !queries)) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) return refuse_multi("vdb_flat_distances_batch");
    const size_t total = offsets[nq];
    if (total && (!ids || !out_dists)) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    int rc = set_device(ix);
    if (rc) return rc;
    Workspace& W = ix->wsv[0];                                     // (nothing is in flight: the first workspace)
    if ((rc = flush(ix))) return rc;
    if (total == 0) return VDB_OK;
    if (total > 0xfffffff0ull || nq > 0x7fffffffull) return fail(VDB_ERR_INVALID_ARGUMENT, "too many pairs");
    // distance.rs:21-26: a stored row of another dimension fails the call
    for (size_t i = 0; i < total; ++i) {
        auto m = ix->misfits.find(ids[i]);
        if (m != ix->misfits.end() && m->second.size() != dim) return fail_dim(dim, m->second.size());
    }
    if (ix->n_live && ix->dim != dim) return fail_dim(dim, ix->dim);
    hipStream_t s = ix->stream;
    const uint32_t ld = ix->ld ? ix->ld : round_up((uint32_t)dim, vdb::KSTAGE);
    const uint32_t nq32 = (uint32_t)nq, bp = round_up(nq32, SUPER);
    std::vector<uint32_t> prow(total), pq(total);
    for (uint32_t q = 0; q < nq32; ++q)
        for (size_t i = offsets[q]; i < offsets[q + 1]; ++i) {
            auto it = ix->id2row.find(ids[i]);
            prow[i] = it == ix->id2row.end() ? 0xffffffffu : it->second;
            pq[i] = q;
        }
    if ((rc = W.w_qin.ensure(nq * dim))) return rc;
    if ((rc = W.w_qp.ensure((size_t)bp * ld))) return rc;
    if ((rc = W.w_qnorm.ensure(bp))) return rc;
    if ((rc = W.w_thr.ensure(bp))) return rc;
    if ((rc = W.w_flags.ensure(4))) return rc;
    if ((rc = W.w_rowmask.ensure(2 * total))) return rc;      // pair_row | pair_query
    if ((rc = W.w_outd.ensure(total))) return rc;
    HIP_TRY(hipMemsetAsync(W.w_flags.p, 0, 16, s));
    HIP_TRY(hipMemcpyAsync(W.w_qin.p, queries, nq * dim * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(W.w_rowmask.p, prow.data(), total * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(W.w_rowmask.p + total, pq.data(), total * 4, hipMemcpyHostToDevice, s));
    vdb::QueryPrepParams qp{W.w_qin.p, (uint32_t)dim, nq32, W.w_qp.p, ld, bp, W.w_qnorm.p, W.w_thr.p, vdb::EUCLID,
                            W.w_flags.p, nullptr, nullptr, nullptr, 0.0f, nullptr, nullptr};   // metric EUCLID here: zero norms are judged per PAIR below
    vdb::launch_query_prep(qp, s);
    vdb::PairDistParams pp{rows_f32(ix), ld, (uint32_t)dim, W.w_qp.p, W.w_qnorm.p, ix->d_nd, W.w_rowmask.p + total,
                           W.w_rowmask.p, (uint32_t)total, ix->metric, W.w_outd.p, W.w_flags.p};
    vdb::launch_pair_distances(pp, s);
    HIP_TRY(hipGetLastError());
    uint32_t st = 0;
    HIP_TRY(hipMemcpyAsync(out_dists, W.w_outd.p, total * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&st, W.w_flags.p, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (st & vdb::ST_ZERO_QUERY)
        return fail_zero_vector();
    return VDB_OK;   // a NaN distance is returned as NaN (only the sort in FlatIndex::search panics on it)
    });
}

int vdb_merge_topk_packed_device(int device, const int32_t* d_packed, size_t nparts, size_t words_per_part, size_t nq,
                                 size_t k, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                                 uint32_t* d_out_status, void* stream) {
    return guarded([&]() -> int {
    if (!d_packed || !d_out_ids || !d_out_dists || !d_out_counts)
        return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (!merge_fits(nparts, nq, k)) return fail(VDB_ERR_INVALID_ARGUMENT, "nq = %zu queries of nparts*k = %zu keys: too large", nq, nparts * k);
    if ((words_per_part & 1) || words_per_part < nq * (3 * k + 1) + 1)
        return fail(VDB_ERR_INVALID_ARGUMENT, "words_per_part must be even and >= nq*(3k+1)+1");
    HIP_TRY(hipSetDevice(device));
    vdb::launch_merge_packed(d_packed, words_per_part, (uint32_t)nparts, (uint32_t)nq, (uint32_t)k, d_out_ids,
                             d_out_dists, d_out_counts, d_out_status, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return VDB_OK;
    });
}

int vdb_flat_set_profile(vdb_flat_index* ix, int on) {
    return guarded([&]() -> int {
    if (!ix) return fail(VDB_ERR_INVALID_ARGUMENT, "null handle");
    if (ix->multi) return multi_for_each(ix, [on](vdb_flat_index* c) { return vdb_flat_set_profile(c, on); });
    std::lock_guard<std::mutex> g(ix->mu);
    int rc = set_device(ix);
    if (rc) return rc;
    if (on && ((rc = ix->ev0.create(hipEventDefault)) || (rc = ix->ev1.create(hipEventDefault)))) return rc;
    ix->profile = on != 0;
    return VDB_OK;
    });
}

int vdb_flat_last_stats(const vdb_flat_index* ix, uint64_t out[8]) {
    return guarded([&]() -> int {
    if (!ix || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    memcpy(out, ix->stats, 8 * sizeof(uint64_t));
    return VDB_OK;
    });
}

int vdb_flat_last_stats_ex(const vdb_flat_index* ix, uint64_t* out, size_t n) {
    return guarded([&]() -> int {
    if (!ix || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    // (a plain handle: the first workspace's counters, not the published copy vdb_flat_last_stats reads -- the two differ only
    // after the wait for ticket 1 was the last thing to finish)
    for (size_t i = 0; i < n; ++i) out[i] = i < STAT_COUNT ? (ix->multi ? ix->stats[i] : ix->wsv[0].stats[i]) : 0;
    return VDB_OK;
    });
}

// ------------------------------------------------------------------ certificate diagnostics (include/vdb_flat.h)
int vdb_flat_debug_screen_scores(vdb_flat_index* ix, const float* queries, size_t nq, size_t dim, int raw, float* out_scores,
                                 float* out_qinfo, double* out_consts) {
    return guarded([&]() -> int {
    if (ix && ix->multi) return refuse_multi("vdb_flat_debug_screen_scores");
    if (!ix || !queries || !out_scores || !nq) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (raw < 0 || (raw & ~(3 | VDB_DEBUG_SCORES_SPLIT | VDB_DEBUG_SCORES_WIDE))) return fail(VDB_ERR_INVALID_ARGUMENT, "unknown bits in raw");
    const bool over_split = (raw & VDB_DEBUG_SCORES_SPLIT) != 0, wide = (raw & VDB_DEBUG_SCORES_WIDE) != 0;
    raw &= 3;
    if (over_split && wide) return fail(VDB_ERR_INVALID_ARGUMENT, "the wide kernel reads f32 rows: not over SPLIT rows");
    if ((over_split || wide) && raw == 2) return fail(VDB_ERR_INVALID_ARGUMENT, "the f32 tier reads f32 rows and has one kernel");
    if (wide && nq <= SUPER) return fail(VDB_ERR_INVALID_ARGUMENT, "the wide kernel serves batches above %u queries only", SUPER);
    if (nq > (wide ? 2 * SUPER : SUPER)) return fail(VDB_ERR_INVALID_ARGUMENT, "at most %u queries per call", wide ? 2 * SUPER : SUPER);
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    int rc;
    if ((rc = set_device(ix))) return rc;
    Workspace& W = ix->wsv[0];                                     // (nothing is in flight: the first workspace)
    if ((rc = flush(ix))) return rc;
    const uint32_t n = ix->n_uploaded, ld = ix->ld;
    if (!n) return fail(VDB_ERR_INVALID_ARGUMENT, "empty index");
    if (ix->dim != dim) return fail_dim(dim, ix->dim);
    if (!ix->misfits.empty()) return fail(VDB_ERR_INVALID_ARGUMENT, "rows of another dimension are stored");
    // what the two kernels need, asked BEFORE anything touches the rows: a refused call leaves them in the layout they had
    if ((over_split || wide) && shadow_usable(ix)) return fail(VDB_ERR_INVALID_ARGUMENT, "the filter pass of this index runs over its bf16 shadow");
    if (over_split && (ld % 64 != 0 || ld > 16384)) return fail(VDB_ERR_INVALID_ARGUMENT, "rows of pitch %u cannot be SPLIT", ld);
    if (over_split && !ix->d_rows_store) return fail(VDB_ERR_INVALID_ARGUMENT, "empty store");
    if (over_split && ix->split_refused) return fail(VDB_ERR_INVALID_ARGUMENT, "the rows hold a non-finite element and stay F32");
    hipStream_t s = ix->stream;
    // the dense dump needs every row of a workgroup's range in its sub-pools (none "counted, not stored"): a sub-pool takes a
    // quarter of a 256-row tile; of the wide kernel's 128-row tile a quarter as well (32 rows) -- sized here for 64, a whole row
    // half, which holds however the kernel deals a row half to its two lane halves; the counts are checked after the launch
    const uint32_t tile = wide ? vdb::fused_bf16w_tile_rows() : vdb::fused_bf16_tile_rows();
    const uint32_t nblk = (n + tile - 1) / tile;
    const uint32_t n_wg = std::min<uint32_t>((uint32_t)ix->n_cu, nblk);
    const uint32_t n_sub = vdb::fused_bf16_subpools_per_query(n_wg);
    const uint32_t capl = 64u * ((nblk + n_wg - 1) / n_wg);
    const uint32_t n_blocks = wide ? 2u : 1u, nqp = n_blocks * SUPER;
    const size_t pool_block = (size_t)SUPER * n_sub * capl, cnt_block = (size_t)SUPER * n_sub;   // the production strides (pass_bf16)
    const size_t pool_keys = n_blocks * pool_block;
    if (pool_keys * 8 > ((size_t)6 << 30)) return fail(VDB_ERR_INVALID_ARGUMENT, "index too large for the score dump");
    if ((rc = W.w_qin.ensure(nq * dim))) return rc;
    if ((rc = W.w_qp.ensure((size_t)nqp * ld))) return rc;
    if ((rc = W.w_qnorm.ensure(nqp))) return rc;
    if ((rc = W.w_thr.ensure(nqp))) return rc;
    if ((rc = W.w_qb.ensure((size_t)nqp * ld))) return rc;
    if ((rc = W.w_qerr.ensure(nqp))) return rc;
    if ((rc = W.w_qg.ensure(nqp))) return rc;
    if ((rc = W.w_flags.ensure(SearchFlags::words(nqp)))) return rc;
    if ((rc = W.w_pool.ensure(pool_keys))) return rc;
    if ((rc = W.w_subcnt.ensure(n_blocks * cnt_block))) return rc;
    if ((rc = W.w_dbg.ensure(nq * (size_t)n))) return rc;
    // raw | VDB_DEBUG_SCORES_SPLIT: the store goes SPLIT (whatever split_mode says; the adaptive run is neither fed nor reset)
    // and stays so.  A non-finite element sends it straight back, as in a search (rows_to_split), and the call is refused.
    if (over_split) {
        if ((rc = rows_to_split(ix))) return rc;
        if (ix->layout != vdb::LAYOUT_SPLIT) return fail(VDB_ERR_INVALID_ARGUMENT, "the rows hold a non-finite element and stay F32");
    }
    W.status_dirty = true;
    HIP_TRY(hipMemsetAsync(W.w_flags.p, 0, 16, s));
    HIP_TRY(hipMemcpyAsync(W.w_qin.p, queries, nq * dim * sizeof(float), hipMemcpyHostToDevice, s));
    const bool lb = ix->d_margin && raw == 0;
    if (raw == 2) {
        // the f32 MFMA tier's scores: dense_scores_kernel over EVERY row -- the production kernel of indexes up to 16384 rows,
        // and bit-identical to the fused f32 kernel's scores by construction (same K order, same score expression)
        if ((size_t)nq * n > ((size_t)1 << 28)) return fail(VDB_ERR_INVALID_ARGUMENT, "index too large for the f32-tier score dump");
        if ((rc = W.w_dense.ensure((size_t)SUPER * n))) return rc;
        HIP_TRY(hipMemcpyAsync(W.w_qin.p, queries, nq * dim * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(W.w_flags.p, 0, 16, s));
        vdb::QueryPrepParams qp2{W.w_qin.p, (uint32_t)dim, (uint32_t)nq, W.w_qp.p, ld, SUPER, W.w_qnorm.p, W.w_thr.p, vdb::EUCLID,
                                 W.w_flags.p, nullptr, nullptr, nullptr, 0.0f, nullptr, nullptr};
        vdb::launch_query_prep(qp2, s);
        vdb::DenseParams dp{rows_f32(ix), ld, n, W.w_qp.p, round_up((uint32_t)nq, 32), ix->d_alpha, ix->d_beta, ix->d_live, n, W.w_dense.p, n};
        vdb::launch_dense_scores(dp, s);
        HIP_TRY(hipGetLastError());
        std::vector<uint64_t> keys((size_t)nq * n);
        std::vector<float> qn2(nq);
        uint32_t sc2[8] = {0};
        HIP_TRY(hipMemcpyAsync(keys.data(), W.w_dense.p, keys.size() * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(qn2.data(), W.w_qnorm.p, nq * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(sc2, ix->d_scalars, 32, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (size_t i = 0; i < keys.size(); ++i) {
            uint32_t bits = 0xffffffffu;                                    // no key (tombstoned row)
            if (keys[i] != vdb::EMPTY_KEY) { const float f = vdb::ordered_to_f32((uint32_t)(keys[i] >> 32)); memcpy(&bits, &f, 4); }
            memcpy(out_scores + i, &bits, 4);
        }
        if (out_qinfo)
            for (size_t q = 0; q < nq; ++q) { out_qinfo[4 * q] = qn2[q]; out_qinfo[4 * q + 1] = 0.0f; out_qinfo[4 * q + 2] = 0.0f; out_qinfo[4 * q + 3] = 0.0f; }
        if (out_consts) {
            auto f = [](uint32_t b) { float v; memcpy(&v, &b, 4); return (double)v; };
            out_consts[0] = eps_coef(ix); out_consts[1] = 0.0; out_consts[2] = 0.0; out_consts[3] = std::sqrt(f(sc2[0]));
            out_consts[4] = 0.0; out_consts[5] = 0.0; out_consts[6] = 0.0; out_consts[7] = (double)ld;
        }
        W.dbg_nq = (uint32_t)nq; W.dbg_lb = false; W.dbg_f32 = true;
        return VDB_OK;
    }
    W.dbg_f32 = false;
    vdb::QueryPrepParams qp{W.w_qin.p, (uint32_t)dim, (uint32_t)nq, W.w_qp.p, ld, nqp, W.w_qnorm.p, W.w_thr.p, vdb::EUCLID,
                            W.w_flags.p, W.w_qb.p, W.w_qerr.p, ix->d_margin ? W.w_qg.p : nullptr, margin_plan(ix).kappa,
                            nullptr, nullptr};
    vdb::launch_query_prep(qp, s);
    std::vector<float> thr(nq, std::numeric_limits<float>::infinity());            // everything passes; padding queries keep -inf
    HIP_TRY(hipMemcpyAsync(W.w_thr.p, thr.data(), nq * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(W.w_dbg.p, 0xff, nq * (size_t)n * 4, s));            // NaN pattern = no key for this (query, row)
    vdb::FusedBf16Params fp{};
    fp.rows = over_split ? ix->d_rows_store.p : rows_f32(ix);                     // (SPLIT: as the store lies; launch_filter_pass reads its hi pieces)
    fp.ld = ld; fp.n_rows = n; fp.qb = W.w_qb.p; fp.alpha = ix->d_alpha; fp.beta = ix->d_beta;
    fp.margin = lb ? ix->d_margin : nullptr; fp.qg = lb ? W.w_qg.p : nullptr;
    fp.rowmask = ix->d_live; fp.thr = W.w_thr.p; fp.pool = W.w_pool.p; fp.pool_cnt = W.w_subcnt.p; fp.capl = capl; fp.n_wg = n_wg;
    fp.scalars = ix->d_scalars; fp.qmax_bits = status_qmax(W.w_flags.p);
    if (wide) {                                                                   // the launch of pass_bf16's wide pass
        fp.pool_block_stride = pool_block; fp.cnt_block_stride = cnt_block;
        vdb::launch_fused_bf16w(fp, s);
        HIP_TRY(hipGetLastError());
        std::vector<uint32_t> cnts(n_blocks * cnt_block);                         // a dump with holes is no dump
        HIP_TRY(hipMemcpyAsync(cnts.data(), W.w_subcnt.p, cnts.size() * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (uint32_t c : cnts)
            if (c > capl) return fail(VDB_ERR_DEVICE, "a sub-pool of the wide kernel counted %u keys, room for %u", c, capl);
    } else launch_filter_pass(ix, fp, s);                                         // the PRODUCTION filter pass (shadow rows if enabled)
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const uint32_t nb = std::min<uint32_t>(SUPER, (uint32_t)nq - b * SUPER);
        vdb::launch_pool_to_dense(W.w_pool.p + b * pool_block, W.w_subcnt.p + b * cnt_block, n_sub, capl, nb, n,
                                  W.w_dbg.p + (size_t)b * SUPER * n, s);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_scores, W.w_dbg.p, nq * (size_t)n * 4, hipMemcpyDeviceToHost, s));
    std::vector<float> qn(nq), qe(nq), qg(nq, 0.0f);
    uint32_t sc[8] = {0};
    HIP_TRY(hipMemcpyAsync(qn.data(), W.w_qnorm.p, nq * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(qe.data(), W.w_qerr.p, nq * 4, hipMemcpyDeviceToHost, s));
    if (ix->d_margin) HIP_TRY(hipMemcpyAsync(qg.data(), W.w_qg.p, nq * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(sc, ix->d_scalars, 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (out_qinfo)
        for (size_t q = 0; q < nq; ++q) { out_qinfo[4 * q] = qn[q]; out_qinfo[4 * q + 1] = qe[q]; out_qinfo[4 * q + 2] = qg[q]; out_qinfo[4 * q + 3] = 0.0f; }
    if (out_consts) {
        auto f = [](uint32_t b) { float v; memcpy(&v, &b, 4); return (double)v; };
        const MarginPlan mp = margin_plan(ix);
        out_consts[0] = eps_coef(ix); out_consts[1] = c_acc_bf16(ix); out_consts[2] = mp.kappa;
        out_consts[3] = std::sqrt(f(sc[0])); out_consts[4] = std::sqrt(f(sc[2])); out_consts[5] = std::sqrt(f(sc[3]));   // max |d|, max |e_d|, max |e_d|/|d|
        out_consts[6] = lb ? 1.0 : 0.0; out_consts[7] = (double)ld;
    }
    W.dbg_nq = (uint32_t)nq; W.dbg_lb = lb;
    return VDB_OK;
    });
}

size_t vdb_flat_debug_rows(const vdb_flat_index* ix) { return (ix && !ix->multi) ? ix->row_ids.size() : 0; }

int vdb_flat_debug_last_thresholds(vdb_flat_index* ix, float* out, size_t nq) {
    return guarded([&]() -> int {
    if (ix && ix->multi) return refuse_multi("vdb_flat_debug_last_thresholds");
    if (!ix || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    int rc;
    if ((rc = set_device(ix))) return rc;
    Workspace& W = ix->wsv[0];                                     // (nothing is in flight: the first workspace)
    if (nq > W.w_thr.n) return fail(VDB_ERR_INVALID_ARGUMENT, "more queries than the last search prepared");
    HIP_TRY(hipMemcpy(out, W.w_thr.p, nq * 4, hipMemcpyDeviceToHost));
    return VDB_OK;
    });
}

int vdb_flat_debug_row_info(vdb_flat_index* ix, float* out, size_t n_rows) {
    return guarded([&]() -> int {
    if (ix && ix->multi) return refuse_multi("vdb_flat_debug_row_info");
    if (!ix || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    int rc;
    if ((rc = set_device(ix))) return rc;
    if ((rc = flush(ix))) return rc;
    const size_t n = std::min<size_t>(n_rows, ix->n_uploaded);
    std::vector<float> a(n), b(n), c(n), d(n, 0.0f);
    if (n) {
        HIP_TRY(hipMemcpy(a.data(), ix->d_nd, n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(b.data(), ix->d_alpha, n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(c.data(), ix->d_beta, n * 4, hipMemcpyDeviceToHost));
        if (ix->d_margin) HIP_TRY(hipMemcpy(d.data(), ix->d_margin, n * 4, hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < n; ++i) { out[4 * i] = a[i]; out[4 * i + 1] = b[i]; out[4 * i + 2] = c[i]; out[4 * i + 3] = d[i]; }
    return VDB_OK;
    });
}

int vdb_flat_debug_cert_probe(vdb_flat_index* ix, const uint32_t* qi, const float* T, const float* ek, size_t n, uint32_t* out) {
    return guarded([&]() -> int {
    if (ix && ix->multi) return refuse_multi("vdb_flat_debug_cert_probe");
    if (!ix || !qi || !T || !ek || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    int rc;
    if ((rc = set_device(ix))) return rc;
    Workspace& W = ix->wsv[0];                                     // (nothing is in flight: the first workspace)
    if (!W.dbg_nq) return fail(VDB_ERR_INVALID_ARGUMENT, "call vdb_flat_debug_screen_scores first");
    if (n == 0) return VDB_OK;
    if (n > 0x7fffffffull) return fail(VDB_ERR_INVALID_ARGUMENT, "too many probes");
    for (size_t i = 0; i < n; ++i)
        if (qi[i] >= W.dbg_nq) return fail(VDB_ERR_INVALID_ARGUMENT, "query index %u out of range", qi[i]);
    hipStream_t s = ix->stream;
    DevBuf<uint32_t> d_qi, d_out; DevBuf<float> d_T, d_ek;
    auto done = [&](int r) { d_qi.release(); d_out.release(); d_T.release(); d_ek.release(); return r; };
    if ((rc = d_qi.ensure(n)) || (rc = d_out.ensure(n)) || (rc = d_T.ensure(n)) || (rc = d_ek.ensure(n))) return done(rc);
    if (hipMemcpyAsync(d_qi.p, qi, n * 4, hipMemcpyHostToDevice, s) != hipSuccess || hipMemcpyAsync(d_T.p, T, n * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d_ek.p, ek, n * 4, hipMemcpyHostToDevice, s) != hipSuccess)
        return done(fail(VDB_ERR_DEVICE, "copy failed"));
    // the same parameter block the screening tier's re-rank gets (pass_bf16)
    vdb::RerankParams rp{};
    rp.metric = ix->metric; rp.eps_coef = eps_coef(ix); rp.nd2max_bits = ix->d_scalars; rp.qnorm = W.w_qnorm.p; rp.ld = ix->ld;
    rp.qerr = W.dbg_f32 ? nullptr : W.w_qerr.p; rp.c_acc = c_acc_bf16(ix); rp.lb_scores = W.dbg_lb ? 1u : 0u;   // dbg_f32: the f32 tier's parameter block (pass_f32)
    vdb::launch_cert_probe(rp, d_qi.p, d_T.p, d_ek.p, (uint32_t)n, d_out.p, s);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(out, d_out.p, n * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return done(fail(VDB_ERR_DEVICE, "cert probe failed"));
    return done(VDB_OK);
    });
}

int vdb_flat_set_sample_cache(vdb_flat_index* ix, int on) {
    return guarded([&]() -> int {
    if (!ix || on < 0 || on > 1) return fail(VDB_ERR_INVALID_ARGUMENT, "on must be 0 or 1");
    if (ix->multi) return multi_for_each(ix, [on](vdb_flat_index* c) { return vdb_flat_set_sample_cache(c, on); });
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    ix->sample_cache = on != 0;
    if (!on && ix->d_sample16) {
        HIP_TRY(hipSetDevice(ix->device));
        HIP_TRY(hipDeviceSynchronize());
        ix->d_sample16.release(); ix->sample16_n = ix->sample16_S = 0;
    }
    return VDB_OK;
    });
}

int vdb_flat_set_shadow(vdb_flat_index* ix, int on) {
    return guarded([&]() -> int {
    if (!ix || on < 0 || on > 1) return fail(VDB_ERR_INVALID_ARGUMENT, "on must be 0 or 1");
    if (ix->multi) return multi_for_each(ix, [on](vdb_flat_index* c) { return vdb_flat_set_shadow(c, on); });
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    HIP_TRY(hipSetDevice(ix->device));
    int rc;
    if ((rc = flush(ix))) return rc;
    if (!on) {
        if (ix->d_rows16) { HIP_TRY(hipStreamSynchronize(ix->stream)); ix->d_rows16.release(); }
        ix->shadow = false;
        return VDB_OK;
    }
    if (!ix->d_rows16 && ix->cap_rows) {
        DevBuf<uint16_t> r16;
        HIP_TRY(r16.alloc((size_t)ix->cap_rows * ix->ld));
        hipError_t e = hipMemsetAsync(r16, 0, (size_t)ix->cap_rows * ix->ld * 2, ix->stream);
        if (e == hipSuccess) { vdb::launch_rows_to_bf16(rows_f32(ix), r16, ix->ld, 0, ix->n_uploaded, ix->stream); e = hipGetLastError(); }
        if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
        if (e != hipSuccess) return fail(VDB_ERR_DEVICE, "building the bf16 shadow failed: %s", hipGetErrorString(e));
        ix->d_rows16 = std::move(r16);                                   // only a COMPLETE shadow is ever visible to a search
    }
    ix->shadow = true;
    return VDB_OK;
    });
}

int vdb_flat_set_tiers(vdb_flat_index* ix, unsigned flags) {
    return guarded([&]() -> int {
    if (!ix || (flags & ~31u)) return fail(VDB_ERR_INVALID_ARGUMENT, "flags must be a combination of VDB_TIERS_*");
    if (ix->multi) return multi_for_each(ix, [flags](vdb_flat_index* c) { return vdb_flat_set_tiers(c, flags); });
    std::lock_guard<std::mutex> g(ix->mu);
    ix->tiers = flags;
    return VDB_OK;
    });
}

int vdb_flat_set_screen(vdb_flat_index* ix, int mode) {
    return guarded([&]() -> int {
    if (!ix || mode < 0 || mode > 1) return fail(VDB_ERR_INVALID_ARGUMENT, "mode must be 0 (f32 MFMA tier only) or 1 (bf16 screening tier first)");
    if (ix->multi) return multi_for_each(ix, [mode](vdb_flat_index* c) { return vdb_flat_set_screen(c, mode); });
    std::lock_guard<std::mutex> g(ix->mu);
    ix->screen = mode;
    return VDB_OK;
    });
}

int vdb_flat_set_wide(vdb_flat_index* ix, int on) {
    return guarded([&]() -> int {
    if (!ix || on < 0 || on > 1) return fail(VDB_ERR_INVALID_ARGUMENT, "on must be 0 or 1");
    if (ix->multi) return multi_for_each(ix, [on](vdb_flat_index* c) { return vdb_flat_set_wide(c, on); });
    std::lock_guard<std::mutex> g(ix->mu);
    ix->wide = on != 0;
    return VDB_OK;
    });
}

int vdb_flat_set_split(vdb_flat_index* ix, int mode) {
    return guarded([&]() -> int {
    if (!ix || mode < 0 || mode > 2) return fail(VDB_ERR_INVALID_ARGUMENT, "mode must be 0, 1 or 2");
    if (ix->multi) return multi_for_each(ix, [mode](vdb_flat_index* c) { return vdb_flat_set_split(c, mode); });
    std::lock_guard<std::mutex> g(ix->mu);
    ix->split_mode = mode;
    ix->split_streak = 0;
    return VDB_OK;
    });
}

int vdb_flat_layout(vdb_flat_index* ix, uint64_t out[2]) {
    return guarded([&]() -> int {
    if (!ix || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (ix->multi) {
        std::mutex m;                                               // (the shards answer on their own threads)
        uint64_t all = 1, conv = 0;
        int rc = multi_for_each(ix, [&](vdb_flat_index* c) {
            uint64_t o[2] = {0, 0};
            int r = vdb_flat_layout(c, o);
            std::lock_guard<std::mutex> g(m);
            all &= o[0]; conv += o[1];
            return r;
        });
        out[0] = all; out[1] = conv;
        return rc;
    }
    std::lock_guard<std::mutex> g(ix->mu);
    out[0] = ix->layout == vdb::LAYOUT_SPLIT ? 1u : 0u;
    out[1] = ix->split_conversions;
    return VDB_OK;
    });
}

int vdb_flat_debug_set_split_after(vdb_flat_index* ix, size_t searches) {
    return guarded([&]() -> int {
    if (!ix || searches > 0xffffffffull) return fail(VDB_ERR_INVALID_ARGUMENT, "bad argument");
    if (ix->multi) return multi_for_each(ix, [searches](vdb_flat_index* c) { return vdb_flat_debug_set_split_after(c, searches); });
    std::lock_guard<std::mutex> g(ix->mu);
    ix->split_after = searches ? (uint32_t)searches : SPLIT_AFTER;
    ix->split_streak = 0;
    return VDB_OK;
    });
}

int vdb_flat_set_large_k(vdb_flat_index* ix, int on) {
    return guarded([&]() -> int {
    if (!ix || on < 0 || on > 1) return fail(VDB_ERR_INVALID_ARGUMENT, "on must be 0 or 1");
    if (ix->multi) return multi_for_each(ix, [on](vdb_flat_index* c) { return vdb_flat_set_large_k(c, on); });
    std::lock_guard<std::mutex> g(ix->mu);
    ix->large_k = on != 0;
    return VDB_OK;
    });
}
size_t vdb_flat_large_k_min_rows(size_t k) {
    return (k <= BF16_MAX_K || k > LARGE_K_MAX) ? 0 : (size_t)std::max<uint64_t>(large_k_min_rows(k), BF16_MIN_ROWS);
}

// ------------------------------------------------------------------ sparse-filter route (vdb_search.cpp search_sparse)
int vdb_flat_set_sparse_filter(vdb_flat_index* ix, int mode) {
    return guarded([&]() -> int {
    if (!ix || mode < 0 || mode > 2) return fail(VDB_ERR_INVALID_ARGUMENT, "mode must be 0, 1 or 2");
    if (ix->multi) return multi_for_each(ix, [mode](vdb_flat_index* c) { return vdb_flat_set_sparse_filter(c, mode); });
    std::lock_guard<std::mutex> g(ix->mu);
    ix->sparse_mode = mode;
    return VDB_OK;
    });
}

int vdb_flat_sparse_stats(vdb_flat_index* ix, uint64_t out[4]) {
    return guarded([&]() -> int {
    if (!ix || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (ix->multi) {
        std::mutex acc;                                            // (the shards are visited concurrently)
        return multi_for_each(ix, [&](vdb_flat_index* c) -> int {
            uint64_t v[4];
            int rc = vdb_flat_sparse_stats(c, v);
            if (rc) return rc;
            std::lock_guard<std::mutex> a(acc);
            out[0] |= v[0]; out[1] += v[1]; out[2] += v[2];
            return VDB_OK;
        });
    }
    std::lock_guard<std::mutex> g(ix->mu);
    out[0] = ix->sparse_last; out[1] = ix->sparse_E; out[2] = ix->sparse_count;
    return VDB_OK;
    });
}

size_t vdb_flat_sparse_limit(size_t n_rows, size_t ld, size_t dim, size_t nq) { return sparse_limit(n_rows, ld, dim, nq); }
size_t vdb_flat_debug_sparse_tile_rows(void) { return vdb::SPARSE_TILE_R; }
size_t vdb_flat_debug_sparse_tile_queries(void) { return vdb::SPARSE_TILE_Q; }

int vdb_flat_debug_eligible_rows(vdb_flat_index* ix, const uint64_t* id_mask, size_t mask_bits, uint32_t* out, size_t cap, size_t* count) {
    return guarded([&]() -> int {
    if (ix && ix->multi) return refuse_multi("vdb_flat_debug_eligible_rows");
    if (!ix || !id_mask || !count || (cap && !out)) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return refuse_in_flight();
    int rc;
    if ((rc = set_device(ix))) return rc;
    Workspace& W = ix->wsv[0];                                     // (nothing is in flight: the first workspace)
    if ((rc = flush(ix))) return rc;
    *count = 0;
    const uint32_t n = ix->n_uploaded;
    if (!n) return VDB_OK;
    hipStream_t s = ix->stream;
    // the mask may be handed over in host memory: it is copied to the device like vdb_flat_search_batch's
    const uint64_t* d_mask = id_mask;
    hipPointerAttribute_t at{};
    const bool on_device = hipPointerGetAttributes(&at, id_mask) == hipSuccess && at.type == hipMemoryTypeDevice;
    if (!on_device) {
        (void)hipGetLastError();
        if ((rc = stage_mask(W.w_mask_ids, MaskSrc{id_mask, mask_bits}, s, &d_mask))) return rc;
    }
    if ((rc = W.w_rowmask.ensure((n + 31) / 32))) return rc;
    vdb::launch_build_rowmask(ix->d_row_ids, (ix->n_live == n) ? nullptr : ix->d_live, d_mask, mask_bits, n, W.w_rowmask.p, s);
    uint32_t E = 0;
    if ((rc = eligible_count(ix, W, s, W.w_rowmask.p, &E))) return rc;
    *count = E;
    if (!E) return VDB_OK;
    if ((rc = eligible_list(ix, W, s, W.w_rowmask.p, E))) return rc;
    const size_t take = std::min<size_t>(cap, E);
    if (take) HIP_TRY(hipMemcpyAsync(out, W.w_elig.p, take * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VDB_OK;
    });
}

int vdb_flat_create_sharded(int metric, const int* devices, size_t n_devices, vdb_flat_index** out) {
    return guarded([&]() -> int { return multi_create(metric, devices, n_devices, out); });
}
size_t vdb_flat_shards(const vdb_flat_index* ix) { return !ix ? 0 : ix->multi ? multi_shards(ix) : 1; }
size_t vdb_flat_shard_len(const vdb_flat_index* ix, size_t shard) {
    return !ix ? 0 : ix->multi ? multi_shard_len(ix, shard) : (shard == 0 ? vdb_flat_len(ix) : 0);
}
int vdb_flat_set_exchange(vdb_flat_index* ix, int mode) {
    return guarded([&]() -> int {
    if (!ix) return fail(VDB_ERR_INVALID_ARGUMENT, "null handle");
    if (!ix->multi) return fail(VDB_ERR_INVALID_ARGUMENT, "not a sharded handle");
    return multi_set_exchange(ix, mode);
    });
}
int vdb_flat_shard_stats(const vdb_flat_index* ix, uint64_t out[8]) {
    return guarded([&]() -> int {
    if (!ix || !out) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (!ix->multi) return fail(VDB_ERR_INVALID_ARGUMENT, "not a sharded handle");
    multi_stats(ix, out);
    return VDB_OK;
    });
}

}  // extern "C"

// =================================================================== internal hooks (vdb_internal.h)
namespace vdb_internal {

static int ensure_pair_buffers(vdb_flat_index* ix, size_t n_pairs, size_t n_out) {
    int rc;
    if ((rc = ix->h_pairs.ensure(2 * std::max<size_t>(n_pairs, 4096)))) return rc;
    return ix->h_pout.ensure(std::max<size_t>(n_out, 4096));
}

int pairs_begin(vdb_flat_index* ix, const float* queries, size_t nq, size_t dim) {
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return fail(VDB_ERR_INVALID_ARGUMENT, "a submitted search is still in flight on this handle");
    int rc;
    if ((rc = set_device(ix))) return rc;
    Workspace& W = ix->wsv[0];                                     // (nothing is in flight: the first workspace)
    if ((rc = flush(ix))) return rc;
    ix->pairs_nq = 0;
    if (nq == 0) return VDB_OK;
    if (ix->n_live && ix->dim != dim) return fail_dim(dim, ix->dim);
    if (nq > 0x7fffffffull) return fail(VDB_ERR_INVALID_ARGUMENT, "too many queries");
    const uint32_t ld = ix->ld ? ix->ld : round_up((uint32_t)dim, vdb::KSTAGE);
    const uint32_t bp = round_up((uint32_t)nq, SUPER);
    hipStream_t s = ix->stream;
    if ((rc = W.w_qin.ensure(nq * dim))) return rc;
    if ((rc = W.w_qp.ensure((size_t)bp * ld))) return rc;
    if ((rc = W.w_qnorm.ensure(bp))) return rc;
    if ((rc = W.w_thr.ensure(bp))) return rc;
    if ((rc = W.w_flags.ensure(4))) return rc;
    HIP_TRY(hipMemcpyAsync(W.w_qin.p, queries, nq * dim * sizeof(float), hipMemcpyHostToDevice, s));
    vdb::QueryPrepParams qp{W.w_qin.p, (uint32_t)dim, (uint32_t)nq, W.w_qp.p, ld, bp, W.w_qnorm.p, W.w_thr.p, vdb::EUCLID,
                            W.w_flags.p, nullptr, nullptr, nullptr, 0.0f, nullptr, nullptr};   // metric EUCLID: zero norms are judged per pair
    vdb::launch_query_prep(qp, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    ix->pairs_nq = (uint32_t)nq;
    return VDB_OK;
}

static int run_pair_eval(vdb_flat_index* ix, int mode, const uint32_t* a, const uint32_t* b, uint32_t q0, size_t n, float* out) {
    std::lock_guard<std::mutex> g(ix->mu);
    if (in_flight(ix)) return fail(VDB_ERR_INVALID_ARGUMENT, "a submitted search is still in flight on this handle");
    int rc;
    if ((rc = set_device(ix))) return rc;
    Workspace& W = ix->wsv[0];                                     // (nothing is in flight: the first workspace)
    if (n == 0) return VDB_OK;
    if (n > 0xfffffff0ull) return fail(VDB_ERR_INVALID_ARGUMENT, "too many pairs");
    if (mode == 1 && (rc = flush(ix))) return rc;
    if ((rc = ensure_pair_buffers(ix, mode == 2 ? 1 : n, n))) return rc;
    uint32_t* d_pairs = ix->h_pairs.d; float* d_out = ix->h_pout.d;
    if (mode != 2) {
        memcpy(ix->h_pairs, a, n * sizeof(uint32_t));
        memcpy(ix->h_pairs + n, b, n * sizeof(uint32_t));
    }
    vdb::PairEvalParams pp{};
    pp.rows = rows_f32(ix); pp.ld = ix->ld; pp.dim = ix->dim; pp.nd = ix->d_nd; pp.qp = W.w_qp.p; pp.qnorm = W.w_qnorm.p;
    pp.a = d_pairs; pp.b = d_pairs + n; pp.n = (uint32_t)n; pp.q0 = q0; pp.mode = mode; pp.metric = ix->metric;
    pp.mark = ZERO_NORM_MARK; pp.out = d_out;
    // A SMALL request (an HNSW insert's misses: a dozen pairs) is waited for by watching the mapped result buffer instead of
    // synchronising the stream: the host fills it with a bit pattern no distance has, the kernel's stores land in host memory as
    // they retire, and the last one to change ends the wait -- the stream synchronisation's wake-up (~15-20 us) was a third of such
    // a round trip, and a 1M-row build makes a million of them.  (Bounded: after 2 ms the stream is synchronised after all.)
    constexpr uint32_t SENTINEL = 0xffc0fee1u;
    const bool poll = mode == 1 && n <= 256;
    volatile uint32_t* hw = reinterpret_cast<volatile uint32_t*>(ix->h_pout.h);
    if (poll) for (size_t i = 0; i < n; ++i) hw[i] = SENTINEL;
    vdb::launch_pair_eval(pp, ix->stream);
    HIP_TRY(hipGetLastError());
    bool landed = false;
    if (poll) {
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t spin = 0; !landed; ++spin) {
            size_t i = 0;
            while (i < n && hw[i] != SENTINEL) ++i;
            landed = i == n;
            if (!landed && (spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
        }
    }
    if (!landed) HIP_TRY(hipStreamSynchronize(ix->stream));
    memcpy(out, ix->h_pout, n * sizeof(float));
    return VDB_OK;
}

int pairs_eval(vdb_flat_index* ix, const uint32_t* pair_q, const uint32_t* pair_row, size_t n, float* out) {
    return run_pair_eval(ix, 0, pair_q, pair_row, 0, n, out);
}
int rows_eval(vdb_flat_index* ix, const uint32_t* row_a, const uint32_t* row_b, size_t n, float* out) {
    return run_pair_eval(ix, 1, row_a, row_b, 0, n, out);
}
int query_vs_rows(vdb_flat_index* ix, uint32_t q, uint32_t n_rows_, float* out) {
    if (n_rows_ > ix->n_uploaded) return fail(VDB_ERR_INVALID_ARGUMENT, "rows not uploaded");
    return run_pair_eval(ix, 2, nullptr, nullptr, q, n_rows_, out);
}
uint32_t row_of(vdb_flat_index* ix, uint64_t id) {
    std::lock_guard<std::mutex> g(ix->mu);
    auto it = ix->id2row.find(id);
    return it == ix->id2row.end() ? 0xffffffffu : it->second;
}
uint32_t n_rows(vdb_flat_index* ix) { return ix->n_rows(); }
int device_view(vdb_flat_index* ix, DeviceView* out) {
    std::lock_guard<std::mutex> g(ix->mu);
    int rc;
    if ((rc = set_device(ix))) return rc;
    Workspace& W = ix->wsv[0];
    if ((rc = W.w_flags.ensure(4))) return rc;
    out->rows = rows_f32(ix); out->ld = ix->ld; out->dim = ix->dim; out->nd = ix->d_nd; out->qp = W.w_qp.p; out->qnorm = W.w_qnorm.p;
    out->metric = ix->metric; out->stream = (void*)ix->stream; out->status = W.w_flags.p;
    return VDB_OK;
}
int search_batch_device_mask(vdb_flat_index* ix, const float* queries, size_t nq, size_t dim, size_t k, const uint64_t* d_mask,
                             size_t mask_bits, uint64_t* out_ids, float* out_dists, size_t* out_counts) {
    if (!d_mask) return fail(VDB_ERR_INVALID_ARGUMENT, "null mask");
    HostSearch r = under(host_search(queries, nq, dim, nullptr, k, k, out_ids, out_dists, out_counts), nullptr, mask_bits);
    r.dm = d_mask;
    return search_batch_host(ix, r);
}
int set_error(int code, const char* msg) { return fail(code, "%s", msg); }
int zero_vector_error() { return fail_zero_vector(); }
int set_dim_error(size_t expected, size_t actual) { return fail_dim(expected, actual); }

}  // namespace vdb_internal
