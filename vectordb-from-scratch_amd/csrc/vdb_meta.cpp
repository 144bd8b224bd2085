// vdb_meta.cpp -- the store's metadata resident in HBM, and filters compiled from it on the device (include/vdb_flat.h
// "Metadata filters compiled on the device").  A table holds one int32 dictionary-code column per slot and a
// presence bitmap, both by internal id.  Writes are staged on the host (the store makes N single-row writes) and reach the
// device as one dirty range per array in front of the next compile, the add / flush pattern of the row store.  A compile is
// uploads + ONE kernel (kernels_filter.hip) on the table's stream; the host never waits for it.
#include "vdb_meta.h"

#include <limits>
#include <memory>

#include "vdb_index.h"

using namespace vdbi;

namespace {

constexpr size_t BLOCK_HEADER = 16;                                 // the eligible count (8 bytes) + padding, in front of the program
// (a numeric leaf's FilterNum follows the ops of ITS program directly, so one copy uploads both)
constexpr size_t BLOCK_BYTES = BLOCK_HEADER + vdb::FILTER_MAX_OPS * (sizeof(vdb::FilterOp) + sizeof(vdb::FilterNum));
constexpr uint64_t MAX_IDS = 1ull << 32;
constexpr uint64_t MAX_CODES = 1ull << 31;                          // dictionary codes are non-negative int32
constexpr uint32_t MAX_SLOTS = 65536;
constexpr size_t MAX_CONSTS = 1024;
static_assert(VDB_META_EQ == (int)vdb::FOP_EQ && VDB_META_NE == (int)vdb::FOP_NE && VDB_META_EXISTS == (int)vdb::FOP_EXISTS && VDB_META_CONST == (int)vdb::FOP_CONST &&
              VDB_META_AND == (int)vdb::FOP_AND && VDB_META_OR == (int)vdb::FOP_OR && VDB_META_LT == (int)vdb::FOP_LT && VDB_META_LE == (int)vdb::FOP_LE &&
              VDB_META_GT == (int)vdb::FOP_GT && VDB_META_GE == (int)vdb::FOP_GE, "the ABI's opcodes are the kernel's");
static_assert(sizeof(vdb::FilterOp) % alignof(vdb::FilterNum) == 0 && BLOCK_HEADER % alignof(vdb::FilterNum) == 0, "FilterNum behind the ops is aligned");

// a host array with its device copy; [lo, hi) is what the device has not seen yet
template <typename T> struct Staged {
    std::vector<T> h;
    DevBuf<T> d;
    size_t lo = SIZE_MAX, hi = 0;
    T fill{};
    void grow(size_t n) {                                           // the new tail reads as `fill` on both sides
        if (n <= h.size()) return;
        touch(h.size(), n);
        h.resize(n, fill);
    }
    void touch(size_t a, size_t b) { lo = std::min(lo, a); hi = std::max(hi, b); }
    int upload(hipStream_t s) {
        if (h.size() > d.n) {
            DevBuf<T> nd;
            HIP_TRY(nd.alloc(std::max<size_t>(std::max(h.size(), d.n * 2), 1024)));
            if (d) (void)hipStreamSynchronize(s);                   // an earlier compile may still read the old copy
            d = std::move(nd);
            touch(0, h.size());
        }
        if (lo < hi) HIP_TRY(hipMemcpyAsync(d + lo, h.data() + lo, (hi - lo) * sizeof(T), hipMemcpyHostToDevice, s));
        lo = SIZE_MAX; hi = 0;
        return VDB_OK;
    }
};

}  // namespace

struct vdb_meta_table {
    int device = 0, n_cu = 256;
    Stream stream;                                                  // declared first: destroyed after every buffer below
    std::mutex mu;                                                  // compiles are reads of the caller and may come from several threads
    std::vector<std::unique_ptr<Staged<int32_t>>> cols;             // by slot; null = slot never written
    std::vector<std::unique_ptr<Staged<double>>> luts;              // by slot: the number of each dictionary code, NaN = none; null = no LUT (length 0)
    Staged<uint64_t> present;
    std::vector<std::unique_ptr<vdb_meta_mask>> masks;              // every mask ever handed out (owned here)
    std::vector<vdb_meta_mask*> free_masks;                         // released ones, most recently released last
    Event col_ready;                                                // meta_column_acquire: recorded behind the uploads a grouping search waits for
};

namespace {

// what was written since the last upload reaches the device, on the table's stream (the caller holds the table's lock)
int upload_staged(vdb_meta_table* t, hipStream_t s) {
    int rc;
    for (auto& c : t->cols) if (c && (rc = c->upload(s))) return rc;
    for (auto& l : t->luts) if (l && (rc = l->upload(s))) return rc;
    return t->present.upload(s);
}

// a mask of at least `words` words from the pool (the most recently released one that is large enough, else any released one,
// regrown), or a new one
int take_mask(vdb_meta_table* t, size_t words, vdb_meta_mask** out) {
    vdb_meta_mask* m = nullptr;
    for (size_t i = t->free_masks.size(); i-- > 0 && !m;)
        if (t->free_masks[i]->d_words.n >= words) { m = t->free_masks[i]; t->free_masks.erase(t->free_masks.begin() + (ptrdiff_t)i); }
    if (!m && !t->free_masks.empty()) { m = t->free_masks.back(); t->free_masks.pop_back(); }
    if (!m) {
        auto nm = std::make_unique<vdb_meta_mask>();
        nm->table = t; nm->device = t->device;
        if (nm->d_block.alloc(BLOCK_BYTES) != hipSuccess || nm->h_block.alloc(BLOCK_BYTES) != hipSuccess || nm->done.create(hipEventDisableTiming))
            return fail(VDB_ERR_DEVICE, "allocating a filter mask failed");
        memset(nm->h_block, 0, BLOCK_BYTES);
        m = nm.get();
        t->masks.push_back(std::move(nm));
    } else {
        // the pinned image is about to be rewritten: the upload of the compile that used it last must be over (it is, unless
        // the mask was released before anybody waited for it)
        HIP_TRY(hipEventSynchronize(m->done));
    }
    if (m->d_words.n < words && m->d_words.alloc(std::max<size_t>(words + words / 2, 64)) != hipSuccess) {
        t->free_masks.push_back(m);
        return fail(VDB_ERR_DEVICE, "allocating the words of a filter mask failed");
    }
    *out = m;
    return VDB_OK;
}

}  // namespace

extern "C" {

int vdb_meta_create(int device, vdb_meta_table** out) {
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
    auto t = std::make_unique<vdb_meta_table>();
    t->device = device;
    t->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    t->present.fill = 0;
    int rc;
    if ((rc = t->stream.create(hipStreamNonBlocking))) return rc;
    *out = t.release();
    return VDB_OK;
    });
}

void vdb_meta_destroy(vdb_meta_table* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    (void)hipStreamSynchronize(t->stream);
    delete t;
}

int vdb_meta_set_codes(vdb_meta_table* t, uint32_t slot, uint64_t first_id, const int32_t* codes, size_t n) {
    return guarded([&]() -> int {
    if (!t || (n && !codes)) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (slot >= MAX_SLOTS) return fail(VDB_ERR_INVALID_ARGUMENT, "slot %u out of range (%u)", slot, MAX_SLOTS);
    if (first_id > MAX_IDS || n > MAX_IDS - first_id) return fail(VDB_ERR_INVALID_ARGUMENT, "metadata ids must be below 2^32");
    std::lock_guard<std::mutex> g(t->mu);
    if (t->cols.size() <= slot) t->cols.resize(slot + 1);
    if (!t->cols[slot]) { t->cols[slot] = std::make_unique<Staged<int32_t>>(); t->cols[slot]->fill = -1; }
    if (n == 0) return VDB_OK;
    auto& c = *t->cols[slot];
    c.grow(first_id + n);
    memcpy(c.h.data() + first_id, codes, n * sizeof(int32_t));
    c.touch(first_id, first_id + n);
    return VDB_OK;
    });
}

int vdb_meta_set_numbers(vdb_meta_table* t, uint32_t slot, uint32_t first_code, const double* values, size_t n) {
    return guarded([&]() -> int {
    if (!t || (n && !values)) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (slot >= MAX_SLOTS) return fail(VDB_ERR_INVALID_ARGUMENT, "slot %u out of range (%u)", slot, MAX_SLOTS);
    if (first_code > MAX_CODES || n > MAX_CODES - first_code) return fail(VDB_ERR_INVALID_ARGUMENT, "dictionary codes must be below 2^31");
    std::lock_guard<std::mutex> g(t->mu);
    if (t->luts.size() <= slot) t->luts.resize(slot + 1);
    if (!t->luts[slot]) { t->luts[slot] = std::make_unique<Staged<double>>(); t->luts[slot]->fill = std::numeric_limits<double>::quiet_NaN(); }
    if (n == 0) return VDB_OK;
    auto& l = *t->luts[slot];
    l.grow((size_t)first_code + n);
    memcpy(l.h.data() + first_code, values, n * sizeof(double));
    l.touch(first_code, (size_t)first_code + n);
    return VDB_OK;
    });
}

int vdb_meta_set_present(vdb_meta_table* t, uint64_t first_id, size_t n, int on) {
    return guarded([&]() -> int {
    if (!t) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    if (first_id > MAX_IDS || n > MAX_IDS - first_id) return fail(VDB_ERR_INVALID_ARGUMENT, "metadata ids must be below 2^32");
    if (n == 0) return VDB_OK;
    std::lock_guard<std::mutex> g(t->mu);
    auto& p = t->present;
    const uint64_t end = first_id + n, w0 = first_id >> 6, w1 = (end - 1) >> 6;
    p.grow(w1 + 1);
    for (uint64_t w = w0; w <= w1; ++w) {
        uint64_t m = ~0ull;
        if (w == w0) m &= ~0ull << (first_id & 63);
        if (w == w1 && (end & 63)) m &= ~0ull >> (64 - (end & 63));
        if (on) p.h[w] |= m; else p.h[w] &= ~m;
    }
    p.touch(w0, w1 + 1);
    return VDB_OK;
    });
}

int vdb_meta_compile(vdb_meta_table* t, const vdb_meta_op* ops, size_t n_ops, size_t mask_bits, vdb_meta_mask** out) {
    return vdb_meta_compile_num(t, ops, n_ops, nullptr, 0, mask_bits, out);     // no constants: a numeric op is refused
}

int vdb_meta_compile_num(vdb_meta_table* t, const vdb_meta_op* ops, size_t n_ops, const double* consts, size_t n_consts, size_t mask_bits,
                         vdb_meta_mask** out) {
    return guarded([&]() -> int {
    if (!t || !out || (n_ops && !ops) || (n_consts && !consts)) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (mask_bits > MAX_IDS) return fail(VDB_ERR_INVALID_ARGUMENT, "mask_bits must be at most 2^32");
    if (n_ops == 0 || n_ops > vdb::FILTER_MAX_OPS) return fail(VDB_ERR_INVALID_ARGUMENT, "a filter program has 1 to %u ops, not %zu", vdb::FILTER_MAX_OPS, n_ops);
    if (n_consts > MAX_CONSTS) return fail(VDB_ERR_INVALID_ARGUMENT, "a filter program has at most %zu constants, not %zu", MAX_CONSTS, n_consts);
    for (size_t i = 0; i < n_consts; ++i)
        if (consts[i] != consts[i]) return fail(VDB_ERR_INVALID_ARGUMENT, "constant %zu is NaN", i);
    std::lock_guard<std::mutex> g(t->mu);
    // 1. the program: well-formed postfix, stack depth within the register, every slot known, every constant index in range
    uint32_t depth = 0;
    size_t n_nums = 0;
    for (size_t i = 0; i < n_ops; ++i) {
        const vdb_meta_op& o = ops[i];
        switch (o.op) {
        case VDB_META_LT: case VDB_META_LE: case VDB_META_GT: case VDB_META_GE:
            if (o.code < 0 || (size_t)o.code >= n_consts) return fail(VDB_ERR_INVALID_ARGUMENT, "op %zu names constant %d of %zu", i, o.code, n_consts);
            ++n_nums;
            [[fallthrough]];
        case VDB_META_EQ: case VDB_META_NE: case VDB_META_EXISTS:
            if (o.slot >= t->cols.size() || !t->cols[o.slot]) return fail(VDB_ERR_INVALID_ARGUMENT, "op %zu names slot %u, which was never written", i, o.slot);
            ++depth;
            break;
        case VDB_META_CONST:
            if (o.code != 0 && o.code != 1) return fail(VDB_ERR_INVALID_ARGUMENT, "op %zu: CONST takes 0 or 1", i);
            ++depth;
            break;
        case VDB_META_AND: case VDB_META_OR:
            if (depth < 2) return fail(VDB_ERR_INVALID_ARGUMENT, "op %zu: AND / OR needs two operands", i);
            --depth;
            break;
        default:
            return fail(VDB_ERR_INVALID_ARGUMENT, "op %zu: unknown opcode %u", i, o.op);
        }
        if (depth > vdb::FILTER_MAX_DEPTH) return fail(VDB_ERR_INVALID_ARGUMENT, "the program needs an evaluation stack deeper than %u", vdb::FILTER_MAX_DEPTH);
    }
    if (depth != 1) return fail(VDB_ERR_INVALID_ARGUMENT, "the program leaves %u values, not 1", depth);
    HIP_TRY(hipSetDevice(t->device));
    hipStream_t s = t->stream;
    // 2. what was written since the last compile
    int rc;
    if ((rc = upload_staged(t, s))) return rc;
    // 3. the mask, its program (the leaves take their column's address and length now), the zeroed count, one launch
    const size_t words = (mask_bits + 63) / 64;
    vdb_meta_mask* m = nullptr;
    if ((rc = take_mask(t, std::max<size_t>(words, 1), &m))) return rc;   // (never a null pointer: to a search that means "no filter")
    m->bits = mask_bits;
    auto* hops = reinterpret_cast<vdb::FilterOp*>(m->h_block + BLOCK_HEADER);
    auto* hnums = reinterpret_cast<vdb::FilterNum*>(hops + n_ops);  // one per numeric leaf, in program order, right behind the ops
    size_t k = 0;
    for (size_t i = 0; i < n_ops; ++i) {
        const vdb_meta_op& o = ops[i];
        vdb::FilterOp f{nullptr, 0, (uint32_t)o.op, o.code};
        const bool numeric = o.op >= VDB_META_LT;
        if (o.op <= VDB_META_EXISTS || numeric) { f.codes = t->cols[o.slot]->d; f.len = t->cols[o.slot]->h.size(); }
        if (numeric) {
            const Staged<double>* l = o.slot < t->luts.size() ? t->luts[o.slot].get() : nullptr;
            hnums[k] = vdb::FilterNum{l ? l->d.p : nullptr, l && l->d ? l->h.size() : 0, consts[o.code]};   // (no LUT: length 0, every leaf false)
            f.code = (int32_t)k++;
        }
        hops[i] = f;
    }
    const size_t up = BLOCK_HEADER + n_ops * sizeof(vdb::FilterOp) + n_nums * sizeof(vdb::FilterNum);
    hipError_t e = hipMemcpyAsync(m->d_block, m->h_block, up, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        vdb::FilterParams p{};
        p.ops = reinterpret_cast<const vdb::FilterOp*>(m->d_block + BLOCK_HEADER); p.n_ops = (uint32_t)n_ops;
        p.nums = reinterpret_cast<const vdb::FilterNum*>(p.ops + n_ops); p.n_nums = (uint32_t)n_nums;
        p.present = t->present.d; p.present_words = t->present.d ? t->present.h.size() : 0;
        p.mask_bits = mask_bits; p.mask = m->d_words;
        p.count = reinterpret_cast<unsigned long long*>(m->d_block.p);
        vdb::launch_filter_compile(p, (uint32_t)t->n_cu, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(m->done, s);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);
        t->free_masks.push_back(m);
        return fail(VDB_ERR_DEVICE, "HIP error %d (%s) while compiling a filter", (int)e, hipGetErrorString(e));
    }
    *out = m;
    return VDB_OK;
    });
}

const uint64_t* vdb_meta_mask_ptr(const vdb_meta_mask* m) { return m ? m->d_words : nullptr; }
size_t vdb_meta_mask_bits(const vdb_meta_mask* m) { return m ? m->bits : 0; }

int vdb_meta_mask_count(vdb_meta_mask* m, uint64_t* eligible) {
    return guarded([&]() -> int {
    if (!m || !eligible) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipEventSynchronize(m->done));
    HIP_TRY(hipMemcpy(eligible, m->d_block, 8, hipMemcpyDeviceToHost));
    return VDB_OK;
    });
}

int vdb_meta_mask_wait_on(vdb_meta_mask* m, void* stream) {
    return guarded([&]() -> int {
    if (!m) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, m->done, 0));
    return VDB_OK;
    });
}

int vdb_meta_mask_release(vdb_meta_mask* m) {
    return guarded([&]() -> int {
    if (!m) return fail(VDB_ERR_INVALID_ARGUMENT, "null argument");
    vdb_meta_table* t = m->table;
    std::lock_guard<std::mutex> g(t->mu);
    for (auto* f : t->free_masks) if (f == m) return fail(VDB_ERR_INVALID_ARGUMENT, "the mask was released already");
    t->free_masks.push_back(m);
    return VDB_OK;
    });
}

}  // extern "C"

namespace vdbi {

int meta_column_check(vdb_meta_table* t, uint32_t slot, int* device) {
    if (!t) return fail(VDB_ERR_INVALID_ARGUMENT, "null table");
    std::lock_guard<std::mutex> g(t->mu);
    if (slot >= t->cols.size() || !t->cols[slot]) return fail(VDB_ERR_INVALID_ARGUMENT, "slot %u was never written", slot);
    *device = t->device;
    return VDB_OK;
}

int meta_column_acquire(vdb_meta_table* t, uint32_t slot, hipStream_t waiter, MetaColumn* out) {
    std::unique_lock<std::mutex> g(t->mu);
    if (slot >= t->cols.size() || !t->cols[slot]) return fail(VDB_ERR_INVALID_ARGUMENT, "slot %u was never written", slot);
    int rc;
    if ((rc = upload_staged(t, t->stream))) return rc;
    if ((rc = t->col_ready.create(hipEventDisableTiming))) return rc;
    HIP_TRY(hipEventRecord(t->col_ready, t->stream));
    HIP_TRY(hipStreamWaitEvent(waiter, t->col_ready, 0));
    out->d_codes = t->cols[slot]->d;
    out->len = t->cols[slot]->d ? t->cols[slot]->h.size() : 0;
    g.release();                                                    // stays locked: meta_column_release
    return VDB_OK;
}

void meta_column_release(vdb_meta_table* t) { t->mu.unlock(); }

}  // namespace vdbi
