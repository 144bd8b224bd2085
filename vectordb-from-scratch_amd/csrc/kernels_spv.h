// kernels_spv.h -- parameter blocks and launchers of the sparse-VECTOR index (kernels_spv.hip, vdb_spv.cpp).
// "spv", not "sparse": kernels_sparse.hip is the sparse-FILTER route of the dense index.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

namespace vdb {

constexpr uint32_t SPV_MAX_INDEX = 1u << 24;        // indices are below this
constexpr uint32_t SPV_MAX_QUERY_NNZ = 1024;        // non-zeros of one query (its table lives in LDS)
constexpr uint32_t SPV_MAX_K = 1024;
constexpr uint32_t SPV_THREADS = 1024;              // one workgroup per query
constexpr uint32_t SPV_SELECT_CAP = 4096;           // keys of the select buffer (LDS); pruned to k when a round of 1024 may not fit
// An accumulator nobody has added to.  A NaN pattern no fold can produce: every NaN a fold yields is stored as 0x7fc00000.
constexpr uint32_t SPV_UNTOUCHED = 0x7fffbeefu;

struct SpvEntry { uint32_t row; float val; };       // one posting: the row and its weight in the list's dimension

// words[i] = value, i < n
void launch_spv_fill(uint32_t* words, size_t n, uint32_t value, hipStream_t s);

// The inverted file from the CSR rows, live rows only.  The host guarantees: row_ptr is monotone with row_ptr[n_rows] entries in
// idx / val, every idx[e] < vocab, and the number of entries of live rows is below 2^32.
// With segs > 1 (the segmented file below) the histogram and the scatter key an entry by index * segs + (row >> seg_shift), and
// counts / list_ptr are the caller's tables over vocab * segs keys.
struct SpvBuildParams {
    const uint32_t* row_ptr; const uint32_t* idx; const float* val; const uint32_t* live; uint32_t n_rows;
    uint32_t vocab;
    uint32_t* counts;                                  // [vocab]: zero before the histogram; the scan leaves it zero for the scatter's cursors
    uint32_t* list_ptr;                                // [vocab + 1]
    SpvEntry* entries;                                 // [list_ptr[vocab]]
    uint32_t segs, seg_shift;                          // 0 or 1 segment: keyed by the index alone
};
void launch_spv_histogram(const SpvBuildParams& p, hipStream_t s);
void launch_spv_scan(const SpvBuildParams& p, hipStream_t s);
void launch_spv_scatter(const SpvBuildParams& p, hipStream_t s);

// One workgroup per query y < nq of a chunk (query b = q0 + y of the batch): fold, emit, select.
struct SpvSearchParams {
    const uint32_t* q_off; const uint32_t* q_idx; const float* q_val;   // the batch's queries, CSR, indices ascending; q_off[nq_batch + 1]
    const uint32_t* ks; uint32_t q0;                   // k of query b (<= SPV_MAX_K, <= kout)
    const uint32_t* list_ptr; uint32_t vocab; const SpvEntry* entries;
    float* acc; uint32_t n_rows;                       // acc[y * n_rows + row]: SPV_UNTOUCHED on entry and on exit
    const uint32_t* live; const uint64_t* row_ids; const uint32_t* rank;   // by row; rank = position of the row's id among the live ids
    const uint64_t* sorted_ids;                        // by rank
    const uint64_t* id_mask; uint64_t mask_bits;       // may be null
    uint64_t* out_ids; float* out_dists; uint32_t* out_counts; uint32_t kout;   // [nq_batch][kout]
    uint32_t* status;                                  // |= ST_NAN: a NaN score in an eligible row
    unsigned long long* counters;                      // [0] += list entries walked (once per entry), [1] += candidates offered to the select
};
void launch_spv_search(const SpvSearchParams& p, uint32_t nq, hipStream_t s);

// ---------------------------------------------------------------- the row-major route (kernels_spv_rows.hip)
// A PASS serves the queries [qa, qa + nq) of a batch, nq <= 64 * tiles: every CSR row is read once per tile of 64 queries.
constexpr uint32_t SPV_ROWS_TILE = 64;              // queries per tile (a lane is a query), and rows per row tile
constexpr uint32_t SPV_NO_SLOT = 0xffffffffu;       // dim_slot of a dimension no query of the pass holds
// A table cell of a (dimension, query) pair the query does not hold.  A NaN pattern no query value is stored as: every NaN
// value goes into the table as 0x7fc00000 (any NaN factor makes the score NaN, and a NaN score has one pattern already).
constexpr uint32_t SPV_ABSENT = 0x7fa5ab5eu;
constexpr size_t SPV_ROWS_TABLE_BYTES = 32u << 20;  // the table budget of a pass (one tile always fits: 65536 * 64 * 4 B)

struct SpvRowsParams {
    // the pass's queries: q_slot[pair] = the rank of the pair's dimension among the pass's distinct dimensions below vocab
    // (udims[n_u], ascending), SPV_NO_SLOT for a dimension at or above vocab
    const uint32_t* q_off; const float* q_val; const uint32_t* q_slot; uint32_t qa, nq, tiles;
    const uint32_t* udims; uint32_t n_u;
    uint32_t* dim_slot;                                // [vocab]: SPV_NO_SLOT on entry and on exit of a pass
    uint32_t* table;                                   // [(n_u + 1)][tiles * 64] f32 bits; row n_u stays SPV_ABSENT everywhere
    const uint32_t* row_ptr; const uint32_t* idx; const float* val; const uint32_t* live; uint32_t n_rows;
    float* acc;                                        // acc[y * n_rows + row], y < nq: SPV_UNTOUCHED on entry and after the emit
    // the emit (SpvSearchParams' fields of the same names)
    const uint32_t* ks; const uint64_t* row_ids; const uint32_t* rank; const uint64_t* sorted_ids;
    const uint64_t* id_mask; uint64_t mask_bits;
    uint64_t* out_ids; float* out_dists; uint32_t* out_counts; uint32_t kout;
    uint32_t* status; unsigned long long* counters;    // [0] += fold steps (= list entries the inverted route walks), [1] += offers
};
void launch_spv_rows_slots(const SpvRowsParams& p, bool set, hipStream_t s);   // dim_slot[udims[u]] = set ? u : SPV_NO_SLOT
void launch_spv_rows_table(const SpvRowsParams& p, hipStream_t s);             // the table: SPV_ABSENT, then the pairs
void launch_spv_rows_fold(const SpvRowsParams& p, hipStream_t s);
void launch_spv_rows_emit(const SpvRowsParams& p, hipStream_t s);

// ---------------------------------------------------------------- the segmented inverted walk (kernels_spv_seg.hip)
// The rows are cut into `segs` segments of seg_rows = 1 << seg_shift consecutive rows, and the postings are ordered by the key
// (index, segment): sub_ptr[index * segs + segment] is where that segment's slice of the index's list starts, so that
// list_ptr[index] = sub_ptr[index * segs] and the lists stay what the one-workgroup walk reads.
constexpr uint32_t SPV_SEG_ROWS_MIN = 64, SPV_SEG_ROWS_MAX = 16384;   // rows per segment: a power of two (the accumulators: 4 B each in LDS)
constexpr uint64_t SPV_SEG_TABLE_MAX = 1ull << 26;                    // words of sub_ptr; a larger table is not built (the file stays unsegmented)
constexpr uint32_t SPV_SEG_SCAN_TILE = 4096;                          // keys per workgroup of the scan

// sub_ptr[n_keys + 1] = the exclusive scan of counts[n_keys], which is left zero (the scatter's cursors), by
// ceil(n_keys / SPV_SEG_SCAN_TILE) workgroups; tiles[2 * that + 1] is scratch.  n_keys > 0.
void launch_spv_seg_scan(uint32_t* counts, uint32_t* sub_ptr, uint32_t n_keys, uint32_t* tiles, hipStream_t s);
// list_ptr[d] = sub_ptr[d * segs], d <= vocab
void launch_spv_seg_lists(const uint32_t* sub_ptr, uint32_t segs, uint32_t vocab, uint32_t* list_ptr, hipStream_t s);

// One workgroup per (segment, query y < nq of a launch; query b = q.q0 + y of the batch): fold into LDS, emit, select; then one
// workgroup per query merges the segments' partial lists.  q.acc is not used.
struct SpvSegParams {
    SpvSearchParams q;
    const uint32_t* sub_ptr; uint32_t segs, seg_shift;
    uint64_t* part; uint32_t* part_cnt;                // part[(y * segs + segment) * q.kout + i], i < part_cnt[y * segs + segment] <= k of the query
};                                                     // q.counters[2] += the workgroups that met a posting
void launch_spv_seg_score(const SpvSegParams& p, uint32_t nq, hipStream_t s);
void launch_spv_seg_merge(const SpvSegParams& p, uint32_t nq, hipStream_t s);

}  // namespace vdb
