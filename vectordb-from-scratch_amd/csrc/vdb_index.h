// vdb_index.h -- internal declarations shared by the host-side translation units of libvdbflat.so:
//   vdb_flat.cpp     the extern "C" shims of include/vdb_flat.h (argument checks, locking, exception guard)
//   vdb_store.cpp    the device-resident mirror of FlatIndex's rows (src/flat_index.rs:12-50): staging, upload, tombstones
//   vdb_cert.cpp     the coefficients of the "certified top-k" bounds and the tier plans
//   vdb_search.cpp   the tier scheduler: screening pass, re-threshold pass, f32 MFMA tier, exact scan
//   vdb_flags.h      the flag blocks of a search by name and the tier hand-over decided from them (no HIP: tested on the CPU)
//   vdb_multi.cpp    ONE index over several GPUs in one process (vdb_flat_create_sharded)
// vdb_hostio.h holds the steps every host-pointer batch search shares (shape check, mask staging, copy-out); HostSearch below is
// the request those entry points hand on.
// Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/vdb_flat.h"
#include "kernels.h"
#include "vdb_device.h"
#include "vdb_flags.h"
#include "vdb_hostio.h"
#include "vdb_internal.h"

namespace vdbi {

// ---- thread-local last error (vdb_last_error); the exception guard of every extern "C" body is in vdb_device.h
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail_dim(size_t expected, size_t actual);
int fail_zero_vector();   // distance.rs:51-55: a zero-norm vector under Cosine fails the whole search
int fail_nan();           // flat_index.rs:62: the reference panics on a NaN distance
void last_error(std::string* msg, size_t* expected, size_t* actual);

inline uint32_t round_up(uint32_t x, uint32_t m) { return (x + m - 1) / m * m; }
inline uint32_t pow2_ceil(uint64_t x) {
    uint32_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

constexpr uint32_t SMALL_N = 16384;     // at or below: dense scores of every row, no fused pass
constexpr uint32_t SUPER = 256;         // queries per pipeline pass
constexpr uint32_t MAX_SELECT = 2048;   // select kernel capacity (kk)
constexpr uint32_t DIRECT_MAX_Q = 8;    // the direct exact path of small indexes takes batches up to this many queries
// vdb_flat_set_split mode 1: eligible screened searches in a row before the next one converts the rows to the SPLIT layout.  From
// the measured conversion times against the step time they buy back: the worst alternating workload -- SPLIT_AFTER
// searches, one f32 reader -- loses at most 10 %.
constexpr uint32_t SPLIT_AFTER = 64;
constexpr uint32_t SPARSE_MAX_E = 131072;   // sparse-filter route: eligible rows at most (one pass's key buffer: 256 x 131072 x 8 B = 256 MiB)

// The slots of Workspace::stats / vdb_flat_index::stats: what vdb_flat_last_stats_ex reports (include/vdb_flat.h says what each means)
enum SearchStat {
    STAT_MFMA = 0,          // queries answered by the MFMA path
    STAT_EXACT,             // queries re-done by the exact-scan fallback (or answered by an exact route)
    STAT_OVERFLOW,          // candidate-pool overflows
    STAT_ROWS_SCANNED,      // rows scanned by the fused kernel
    STAT_SAMPLE,            // sample rows used for the thresholds
    STAT_KP,                // k' (candidates kept per query)
    STAT_UNCERTIFIED,       // uncertified queries
    STAT_KERNEL_NS,         // fused-kernel time of the search, ns (profiling on)
    STAT_SCREENED,          // 1 when the bf16 screening tier answered the batch first
    STAT_TO_F32,            // queries the screening tier handed to the f32 MFMA tier
    STAT_ENQUEUED_NS,       // host clock of the call, ns: first tier enqueued
    STAT_FLAGS_NS,          // ... its flags on the host
    STAT_TOTAL_NS,          // ... return
    STAT_RETHRESHOLD,       // queries answered by the re-threshold pass
    STAT_SHADOW,            // 1 when the screening pass read the bf16 shadow rows
    STAT_DIAG,              // 1 in the diagnostics build with a knob set
    STAT_COUNT
};
static_assert(STAT_COUNT == 16, "vdb_flat_last_stats_ex reports sixteen counters");

}  // namespace vdbi

// What one recommend call owns on the device (vdb_flat_recommend_batch) beside the search workspace; a sharded
// parent's live on devices[0].  RecommendReq is the call as the caller passed it, checked by recommend_check.
struct RecommendWs {
    vdbi::DevBuf<uint32_t> meta, stat;                            // offsets [nq + 1] | n_pos [nq] | reciprocals [nq][2] | row numbers [total] ; struck entries
    vdbi::DevBuf<uint64_t> ids;                                   // the example ids [total]
};
struct RecommendReq {
    const uint64_t* ids; const size_t* offsets; const uint32_t* n_pos;
    size_t total = 0, mmax = 0;                                   // offsets[nq]; the longest request (recommend_check)
};

// A diverse top-k request (vdb_flat_search_batch_mmr) as the caller passed it, checked by mmr_check: the candidate
// depth m and one lambda per query or the scalar (the scores go to Batch::scores, which may be null).
struct MmrReq {
    size_t candidates; const float* lambdas; float lambda;
};
// What one such call owns on the device beside the search workspace: k | lambda | mu per query and the candidates' device rows in
// one upload; the picks; the NaN-pair status word.
struct MmrWs {
    vdbi::DevBuf<uint32_t> meta, outc, stat;
    vdbi::DevBuf<uint64_t> outi; vdbi::DevBuf<float> outd, outs;
};

// What one recommend-by-best-score call owns on the device beside the search workspace (vdb_search.cpp recommend_best_drive,
// DESIGN.md 4.17): the requests, the stage's selection (requests | first lists | positive rows), the gathered positives, the
// ranked lists, the candidates of the walk or of the scan's select, the flags, and the answers.
struct RecBestWs {
    vdbi::DevBuf<uint32_t> meta, sel, lc, cc, open, answered, outc, stat;
    vdbi::DevBuf<uint64_t> ids, li, ci, outi, mask_in;
    vdbi::DevBuf<float> q, ld, cd, outd, outn;
};

// What one discovery search owns on the device beside the search workspace (vdb_search.cpp discover_drive): the
// requests, the stage's selection (requests | target rows | offsets of the stage's example sets) and those sets' ids, the
// gathered targets, the ranked lists with their counts before and after the strike, the scan's key counts, the flags, the
// status words, and the answers.
struct DiscoverWs {
    vdbi::DevBuf<uint32_t> meta, sel, lc, raw, answered, outc, outr, stat, struck;
    vdbi::DevBuf<uint64_t> ids, sids, li, outi, mask_in;
    vdbi::DevBuf<float> q, ld, outd;
};
// A discovery request as the caller passed it, checked by discover_check: request b has the target targets[b] and the pairs
// [offsets[b], offsets[b + 1]) of pair_ids (two ids each).
struct DiscoverReq {
    const uint64_t* targets; const uint64_t* pair_ids; const size_t* offsets;
    size_t pairs = 0, pmax = 0;                                   // offsets[nq]; the most pairs of a request (discover_check)
};

// A host-pointer batch search as its entry point received it (the extern "C" shims fill it): the batch and its outputs (Batch),
// the queries -- vectors [nq][dim], or the stored vectors of `by` (then queries is null and dim unused), or folds of stored
// vectors (rec, checked by recommend_check; by is then rec->ids) -- and the id mask in the form it came in.  mmr: the lists of the
// search at depth mmr->candidates are re-ranked on the device before the copy-out (k is then the number of picks).
struct HostSearch : vdbi::Batch {
    const float* queries = nullptr; size_t dim = 0;
    const uint64_t* by = nullptr; const RecommendReq* rec = nullptr;
    const MmrReq* mmr = nullptr;
    const uint64_t* id_mask = nullptr; size_t mask_bits = 0;      // mask_bits bits in host memory
    const struct vdb_meta_mask* cm = nullptr;                     // a compiled mask (vdb_meta.h); mask_bits becomes its size
    const uint64_t* dm = nullptr;                                 // mask_bits bits already on the device (vdb_internal::search_batch_device_mask)
};

struct Workspace {
    vdbi::DevBuf<float> w_qp, w_qnorm, w_thr, w_qin, w_outd, w_qerr, w_qg, w_dbg;
    uint32_t dbg_nq = 0; bool dbg_lb = false, dbg_f32 = false;             // vdb_flat_debug_screen_scores left this many prepared queries in the workspace
    vdbi::DevBuf<uint64_t> w_dense, w_samp, w_pool, w_cand, w_exact, w_exsel, w_mask_ids, w_outi;
    vdbi::DevBuf<uint32_t> w_cnt, w_rowmask, w_flags, w_outc, w_subcnt, w_depth;
    vdbi::DevBuf<uint32_t> w_elig, w_eligblk;                     // sparse-filter route: the eligible-row list; block counts | block offsets | E
    vdbi::DevBuf<float> w_radii; vdbi::DevBuf<uint64_t> w_totals; // range search, host-pointer form: radii in, totals out
    vdbi::DevBuf<uint32_t> w_selfrow, w_bystat; vdbi::DevBuf<uint64_t> w_selfid;   // search by stored id: device rows and ids of the queries, struck | cut counters
    RecommendWs w_rec;                                            // recommend: the requests' lists
    MmrWs w_mmr;                                                  // diverse top-k: per-query parameters, candidate rows, picks
    vdbi::DevBuf<uint16_t> w_qb;                                  // bf16 copy of the padded queries (screening tier)
    // compact block of the queries the screening tier could not certify (re-run by the f32 tier)
    vdbi::DevBuf<float> w2_qp, w2_qnorm, w2_thr, w2_outd, w2_qerr, w2_qg;
    vdbi::DevBuf<uint64_t> w2_outi, w2_cand;
    vdbi::DevBuf<uint16_t> w2_qb;
    vdbi::DevBuf<uint32_t> w2_outc, w2_flags, w2_qidx;
    vdbi::HostBuf<uint32_t> h_flags{hipHostMallocDefault};
    // the direct path of small indexes (search_direct): a device status word known to be zero between searches, and MAPPED host
    // memory -- the kernels write results and status straight into it (h_io: the host-pointer entry point's queries and outputs)
    vdbi::DevBuf<uint32_t> w_dstat; bool dstat_ready = false;
    vdbi::HostBuf<uint32_t> h_dstat;                                  // [16] host view / device view
    vdbi::HostBuf<char> h_io;
    bool status_dirty = true; uint32_t* status_buf = nullptr;   // device status block known to be zero?
    // a search between its two halves (search_part1 enqueues the first tier, search_part2 reads its flags and runs
    // the fallback tiers): vdb_flat_search_batch_device_begin / _finish keep the handle locked in between
    struct SearchCtx {
        bool pending = false;                               // part 2 still has to run
        uint32_t nq32 = 0, kp = 0, kp16 = 0;
        size_t k = 0;
        hipStream_t s = nullptr;
        const uint32_t* d_rowmask = nullptr;
        uint64_t* d_out_ids = nullptr; float* d_out_dists = nullptr; uint32_t* d_out_counts = nullptr;
        std::chrono::steady_clock::time_point t_entry;
    } ctx;
    uint64_t stats[vdbi::STAT_COUNT] = {0};
    hipStream_t stream = nullptr;                           // this context's stream, owned by the handle (used when the caller passes none)
    bool busy = false;                                      // submitted, not yet waited for
};

// What one search by group owns on the device (vdb_search.cpp distinct_drive): the query block, the ranked lists
// of the search in hand, the answers, and -- only once an exclusion round runs -- the mask of that round.
struct DistinctWs {
    vdbi::DevBuf<float> q, q2, ld, ad;                            // queries | the incomplete ones, dense | list and answer distances
    vdbi::DevBuf<uint64_t> li, ai, mask_in, xmask;                // list and answer ids | the caller's host mask | the exclusion mask
    vdbi::DevBuf<int32_t> ac;                                     // answer codes
    vdbi::DevBuf<uint32_t> lc, kept, complete, sel;               // list counts | rows per answer | completeness flags | the incomplete queries
};

// What one search per group owns on the device beside DistinctWs (vdb_search.cpp per_group_drive): the table of
// wanted codes, their counters, the plan (offsets | lengths | cursors), the member lists, the pairs of the fill, the members and
// sizes of every pair, the status words, and -- only when a giant is searched -- its mask, query block and result lists.
struct PerGroupWs {
    vdbi::DevBuf<int32_t> wanted;
    vdbi::DevBuf<uint32_t> cnt, plan, pairs, sizes, stat, sel, dest, gc;
    vdbi::DevBuf<uint64_t> list, oi, gmask, gi;
    vdbi::DevBuf<float> od, gq, gd;
};

// What one grouped search owns on the device (vdb_search.cpp search_grouped) beside the search workspace: the
// caller's queries and masks, the row masks and lists of all groups, the plan, and the results -- permuted as the passes emit
// them (s*) and in the caller's order (o*).
struct GroupedWs {
    vdbi::DevBuf<float> q, q2, sd, od;                            // queries | the gathered block of an ordinary sub-search | distances
    vdbi::DevBuf<uint64_t> masks, si, oi;                         // host-form masks of the referenced groups, side by side | ids
    vdbi::DevBuf<vdb::GroupedMask> desc;                          // where each referenced group's mask is and how many bits it has
    vdbi::DevBuf<uint32_t> rowmask, blk, lists, plan, sel, sc, oc;   // [R][words] | block counts, offsets, totals | lists | perm, key counts, glist, tiles | sub-search queries | counts
};

// Diagnostic knobs: ablation switches, A/B kernel variants, scaled certificates, sample-size overrides.  Several of them
// VOID the exact-result guarantee, so they exist only in the diagnostics build (-DVDB_DIAG -> libvdbflat_diag.so,
// `make diag`), where vdb_flat_create reads them from the environment ONCE into the handle.  In the release library
// this struct is a set of constants and there is no getenv anywhere.
struct vdb_knobs {
    double eps_scale = 1.0;               // VDB_EPS_SCALE: scales both certification coefficients (0 = no margin!)
    uint32_t bf16_ablate = 0;             // VDB_BF16_ABLATE: phases of the screening kernel switched off (wrong results)
    uint32_t fused_ablate = 0;            // VDB_FUSED_ABLATE: the same for the f32 MFMA kernel
    uint32_t kt16 = 0, sample16 = 0;      // VDB_KT16 / VDB_SAMPLE16: threshold rank / sample size of the screening tier
    uint32_t sample = 0;                  // VDB_SAMPLE: sample size of the f32 tier
    uint32_t kp_first = 0;                // VDB_KP_FIRST: first re-rank round
    bool rr_depth = false;                // VDB_RR_DEPTH: print the re-rank depth distribution
    bool sample_block = false;            // VDB_SAMPLE_BLOCK: contiguous-block sampling
    bool shape4 = false, regstage = false, dma2 = false;   // VDB_FUSED_SHAPE4 / _REGSTAGE / _DMA2: A/B variants of the f32 kernel
    bool fused_pipe = true;               // VDB_FUSED_PIPE=0: unpipelined screening filter pass
    bool any = false;                     // some knob differs from its default -> last_stats_ex()[15] = 1
};

struct vdb_multi;                          // vdb_multi.cpp: the shards of a vdb_flat_create_sharded handle

struct vdb_flat_index {
    int metric = 0, device = 0;
    vdb_multi* multi = nullptr;           // non-null: this handle is the PARENT of a sharded index and owns nothing below but mu / stats
    vdb_knobs kn;
    uint32_t tiers = 0;                   // vdb_flat_set_tiers: VDB_TIERS_* bits (tier hand-over forced; results identical)
    vdbi::Stream stream, stream_alt;      // of the two workspaces; declared before every buffer, so destroyed after them
    int n_cu = 256;
    std::mutex mu;

    uint32_t dim = 0, ld = 0;             // primary dimension and padded row stride (floats)
    // host bookkeeping of the device rows
    std::vector<uint64_t> row_ids;
    std::vector<uint32_t> live;           // bit per row
    std::unordered_map<uint64_t, uint32_t> id2row;
    uint32_t n_live = 0;
    bool ids_monotone = true;
    // rows whose dimension differs from `dim` (reference add() has no check, flat_index.rs:38-41)
    std::unordered_map<uint64_t, std::vector<float>> misfits;
    // rows staged on the host, not yet uploaded: device rows [n_uploaded, row_ids.size())
    std::vector<float> pending;
    uint32_t n_uploaded = 0;
    bool live_dirty = false;

    // device store
    // compact bf16 copy of the screening tier's S sample rows (kernels_fused_s16.hip SAMPLE mode): +S*ld*2 bytes (3 % of a 1M-row
    // index), rebuilt when rows were added; the sample pass then streams 100 MB of contiguous bf16 instead of gathering 200 MB of
    // f32 rows.  Thresholds are identical (same roundings, same MFMA order).  vdb_flat_set_sample_cache(h, 0) turns it off.
    vdbi::DevBuf<uint16_t> d_sample16;
    uint32_t sample16_n = 0, sample16_S = 0;                            // what the copy was built for (rows uploaded, sample size)
    bool sample_cache = true;
    vdbi::DevBuf<uint16_t> d_rows16;      // opt-in bf16 shadow of d_rows [cap_rows][ld] (vdb_flat_set_shadow), else null
    bool shadow = false;
    // The rows [cap_rows][ld], in the layout `layout` names (row_split.h): plain f32 rows, or every row split in place into its
    // bf16 piece and its low halves, which the screening tier's filter pass (launch_filter_pass) and its re-ranks read at 2 bytes
    // per element.  Only those read d_rows_store as it lies (screen_params, rerank_params); EVERY other reader and every writer
    // asks rows_f32(ix) / rows_mut(ix), which convert back first.
    vdbi::DevBuf<float> d_rows_store, d_nd, d_alpha, d_beta;
    int layout = 0;                                         // vdb::LAYOUT_F32 / LAYOUT_SPLIT
    int split_mode = 1;                                     // vdb_flat_set_split: 0 never, 1 adaptive (default), 2 before the next eligible search
    uint32_t split_after = vdbi::SPLIT_AFTER;               // adaptive: eligible searches in a row before the next one converts
    uint32_t split_streak = 0;                              // ... counted so far; any rows_f32 / rows_mut call resets it
    bool split_refused = false;                             // the rows hold a non-finite element: F32 until they change (rows_mut)
    uint64_t split_conversions = 0;                         // conversions so far, both directions
    vdbi::DevBuf<uint32_t> d_split_flag;                    // the forward conversion's non-finite report
    vdbi::DevBuf<float> d_margin;         // [cap] per-row error margin of the screening tier's lower-bound scores (Dot / Euclid; null under Cosine)
    vdbi::DevBuf<uint64_t> d_row_ids; vdbi::DevBuf<uint32_t> d_live, d_scalars;  // [0]=nd2max bits [1]=zero count [2],[3]=max bf16 rounding error of a row (abs^2, rel^2)
    uint32_t cap_rows = 0;
    bool zero_valid = false; uint32_t zero_live = 0;
    // vdb_flat_compact (vdb_store.cpp compact_store): dead rows are taken back by an in-place stable compaction on the device
    double auto_compact = 0.0;                              // vdb_flat_set_auto_compact: flush compacts above this dead fraction (0 = never)
    uint32_t bounce_rows_override = 0;                      // vdb_flat_debug_set_compact_bounce (tests): bounce buffer in rows, 0 = compact_bounce_rows()
    bool store_broken = false;                              // a compaction failed after its first row moved: every later call is refused
    uint64_t n_compactions = 0, rows_reclaimed = 0, last_compact_ns = 0, last_device_ns = 0, last_chunks_direct = 0, last_chunks_bounce = 0;
    vdbi::DevBuf<uint32_t> d_idrank, d_rank2row; bool rank_valid = false;

    // search workspace: everything one search in flight owns.  Two of them, so that two batches can be in flight on two
    // streams (vdb_flat_search_batch_device_submit / _wait).  An entry point picks one under the handle mutex (idle_workspace; the
    // first when nothing may be in flight) and passes it down: the search code holds no "current" workspace.
    std::unique_ptr<Workspace[]> wsv;                       // [2]
    // mapped host memory for the pair hooks (vdb_internal.h): the kernel reads the pairs and writes the distances in place
    vdbi::HostBuf<uint32_t> h_pairs; vdbi::HostBuf<float> h_pout;
    uint32_t pairs_nq = 0;
    bool begin_locked = false;
    vdbi::Event ev_pass[2];                                 // fork / join of the alternating passes of a large batch (pass_bf16)
    vdbi::Event ev_order;                                   // orders the handle's stream before the null stream (search_batch_device_begin)
    int screen = 1;                                         // 1: bf16 screening tier first (default), 0: f32 MFMA tier only
    bool wide = true;                                       // batches above 256 queries: the 512-query filter kernel (vdb_flat_set_wide)
    bool large_k = true;                                    // 112 < k <= 1024 on the screening tier (vdb_flat_set_large_k)
    uint64_t stats[vdbi::STAT_COUNT] = {0};                 // counters of the last COMPLETED search (copied from its workspace: publish_stats)
    // vdb_flat_set_sparse_filter: 0 never (default), 1 always, 2 automatic -- masked searches scan only the eligible rows (search_sparse)
    int sparse_mode = 0;
    uint64_t sparse_last = 0, sparse_E = 0, sparse_count = 0;  // vdb_flat_sparse_stats [0] [1] [2]
    uint64_t range_stats[8] = {0};                          // vdb_flat_range_stats: counters of the last range search
    uint64_t by_id_stats[4] = {0};                          // vdb_flat_by_id_stats: counters of the last search by stored id (also on a sharded parent)
    uint64_t recommend_stats[4] = {0};                      // vdb_flat_recommend_stats: counters of the last recommend call (also on a sharded parent)
    uint64_t mmr_stats[8] = {0};                            // vdb_flat_mmr_stats: counters of the last diverse top-k call
    uint64_t recommend_best_stats[8] = {0};                 // vdb_flat_recommend_best_stats: counters of the last recommend-by-best-score call
    RecBestWs rbw;                                          // its device buffers
    int rb_route = 0;                                       // vdb_flat_debug_set_recommend_best_route (tests): 0 auto, 1 lists first, 2 scan only
    uint64_t discover_stats[8] = {0};                       // vdb_flat_discover_stats: counters of the last discovery search
    DiscoverWs dcw;                                         // its device buffers
    int discover_route = 0;                                 // vdb_flat_debug_set_discover_route (tests): 0 auto, 1 lists first, 2 scan only
    uint64_t distinct_stats[8] = {0};                       // vdb_flat_distinct_stats: counters of the last search by group (also on a sharded parent)
    DistinctWs dws;                                         // its device buffers (a sharded parent's live on devices[0])
    uint64_t per_group_stats[8] = {0};                      // vdb_flat_per_group_stats: counters of the last search per group
    PerGroupWs pgw;                                         // its device buffers
    uint32_t per_group_scan_cap = 0;                        // vdb_flat_debug_set_per_group_scan_cap (tests): rows of a list the fill takes, 0 = SPARSE_MAX_E
    uint64_t grouped_stats[8] = {0};                        // vdb_flat_grouped_stats: counters of the last grouped search
    GroupedWs gws;                                          // its device buffers
    uint64_t id_bound = 0;                                  // 1 + the largest id ever added (saturating), raised at add time only: never lowered by a remove
    bool profile = false; vdbi::Event ev0, ev1;

    uint32_t n_rows() const { return (uint32_t)row_ids.size(); }
    bool is_live(uint32_t r) const { return (live[r >> 5] >> (r & 31)) & 1u; }
    ~vdb_flat_index();                    // vdb_flat.cpp: waits for the streams; the members free themselves
};

namespace vdbi {

using Index = vdb_flat_index;

inline int set_device(const Index* ix) {
    HIP_TRY(hipSetDevice(ix->device));
    return VDB_OK;
}

// ---- vdb_store.cpp: the device row store
// The rows as plain f32 (null before the first row): converts a SPLIT store back first -- every stream of the device waited for,
// so no kernel enqueued earlier still reads the other layout -- and resets the adaptive counter.  The caller holds the handle
// mutex.  rows_mut: for a caller that changes rows; also forgets that the old rows held a non-finite element.  A conversion
// that fails leaves the store unusable (store_broken: every later call is refused).
float* rows_f32(Index* ix);
float* rows_mut(Index* ix);
// F32 -> SPLIT now (the caller has checked that nobody reads the rows: handle mutex held, other workspace idle).  A store with a
// non-finite element is converted straight back and remembered (split_refused).
int rows_to_split(Index* ix);
int grow(Index* ix, uint32_t need_rows);
void free_store(Index* ix);
void reset_rows(Index* ix);
void adopt_dim(Index* ix, size_t dim);   // a store without rows takes the dimension of what comes next
void kill_row(Index* ix, uint32_t row);
int remove_id(Index* ix, uint64_t id);
int add_one(Index* ix, uint64_t id, const float* v, size_t dim);
int flush(Index* ix);
// the chunk plan of a compaction: source rows [a, b) whose live rows go to [dst, ...), directly (mode 0) or through the bounce buffer (mode 1)
struct CompactChunk { uint32_t a, b, dst, mode; };
void compact_plan(const uint32_t* live, uint32_t n_rows, uint32_t bounce_rows, std::vector<uint32_t>* prefix, std::vector<CompactChunk>* out);
uint32_t compact_bounce_rows(uint32_t ld, bool shadow);
int compact_store(Index* ix, bool shrink, size_t* out_reclaimed);
void store_stats(const Index* ix, uint64_t out[8]);
int ensure_zero_count(Index* ix);
int ensure_ranks(Index* ix);

// ---- vdb_cert.cpp: certificate coefficients and tier plans
float eps_coef(const Index* ix);
float c_acc_bf16(const Index* ix);
struct MarginPlan { float m_e = 0, m_n = 0, m_b = 0, kappa = 0, beta_shrink = 0; };
MarginPlan margin_plan(const Index* ix);
constexpr uint32_t BF16_MIN_ROWS = 65536;
struct Bf16Plan { uint32_t kp = 0, S = 0, shift = 0, kt = 0, large = 0; };
constexpr uint32_t BF16_MAX_K = 112, LARGE_K_MAX = 1024;   // k ranges of the screening tier's two re-ranks
Bf16Plan plan_bf16(const Index* ix, uint32_t n, size_t k);
uint64_t large_k_min_rows(size_t k);
uint32_t pick_kp(size_t k);

// ---- vdb_search.cpp: the tier scheduler
bool shadow_usable(const Index* ix);
void launch_filter_pass(Index* ix, vdb::FusedBf16Params& fp, hipStream_t s);
// Every function below that needs a workspace takes it from its caller.  idle_workspace: the one no submitted search is using, or
// the refusal when two are in flight; other_workspace: the handle's second one, seen from W.
int idle_workspace(Index* ix, Workspace** W);
Workspace& other_workspace(Index* ix, Workspace& W);
int search_part1(Index* ix, Workspace& W, const float* d_q, size_t nq, size_t dim, size_t k, const uint64_t* d_idmask,
                 size_t mask_bits, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                 hipStream_t user_stream, bool allow_alt = false);
int search_part2(Index* ix, Workspace& W, int* changed);
bool direct_eligible(const Index* ix, size_t n_rows, size_t nq, size_t k);
size_t sparse_limit(size_t n_rows, size_t ld, size_t dim, size_t nq);
int eligible_count(Index* ix, Workspace& W, hipStream_t s, const uint32_t* d_rowmask, uint32_t* out_E);
int eligible_list(Index* ix, Workspace& W, hipStream_t s, const uint32_t* d_rowmask, uint32_t E);
int ensure_host_io(Workspace& W, size_t bytes);
void publish_stats(Index* ix, const Workspace& W);
bool in_flight(const Index* ix);
int refuse_in_flight();
int search_device(Index* ix, Workspace& W, const float* d_q, size_t nq, size_t dim, size_t k, const uint64_t* d_idmask,
                  size_t mask_bits, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                  hipStream_t user_stream);
// what search_part1 answers for a query of `dim` elements before any device work: VDB_OK, or the dimension error of the first
// stored row that differs (distance.rs:21-26) -- the check a search by stored id makes for the vector its id names
int query_dim_check(const Index* ix, size_t dim);
// ---- vdb_flat.cpp: the device side of a recommend call, the same on a plain handle and on the home device of a sharded one.
// recommend_stage packs the checked request with the row number of every example (in the block the fold will read) and sends it
// up on s in two copies; *L then names the lists on the device.
int recommend_stage(RecommendWs& W, const RecommendReq& r, size_t nq, const uint32_t* rows, hipStream_t s, vdb::RecommendLists* L);
// The strike of a search by stored id or of a recommend call, on s, around the device search: strike_stage sends the query ids up
// and zeroes the counters (a recommend's lists L and counter are staged by recommend_stage already); strike_copy_out runs the self
// strike or the set strike over the search's lists `found`, cutting them to kcut, reads the struck counters with the copy-out and
// writes H->by_id_stats / H->recommend_stats.  The buffers are the plain handle's workspace's or the sharded parent's.
struct StrikeBufs { vdbi::DevBuf<uint64_t>& selfid; vdbi::DevBuf<uint32_t>& bystat; RecommendWs& rec; };
int strike_stage(StrikeBufs B, const HostSearch& r, hipStream_t s);
int strike_copy_out(Index* H, const HostSearch& r, StrikeBufs B, const vdb::RecommendLists& L, const Lists& found, size_t kcut, hipStream_t s);
// the mask of a request whose compiled mask, if any, has passed the device check
MaskSrc mask_src(const HostSearch& r);
// Recommend by best score (vdb_flat_recommend_best_batch) behind the entry point's checks, the flush and the
// resolution of every example to its device row (ex_rows [rec.total]): the list stages, the exact scan for what they cannot
// settle, the copy-out (dn goes to r.scores) and ix->recommend_best_stats.  kmax: the largest k of the batch.
int recommend_best_drive(Index* ix, const HostSearch& r, const RecommendReq& rec, const uint32_t* ex_rows, size_t kmax);
// Discovery search (vdb_flat_discover_batch) behind the entry point's checks, the flush and the resolution of
// every example to its device row: ex_ids / ex_rows hold, request by request, the target and then p_1 n_1 p_2 n_2 ...
// (2 P_b + 1 entries; nq + 2 req.pairs in all).  The list stages, the exact scan for what they cannot settle, the copy-out (the
// ranks go to out_ranks, which may be null) and ix->discover_stats.  kcut = min(the largest k of the batch, len) > 0.
int discover_drive(Index* ix, const HostSearch& r, const DiscoverReq& req, const uint64_t* ex_ids, const uint32_t* ex_rows, size_t kcut,
                   uint32_t* out_ranks);
int range_search_device(Index* ix, const float* d_q, size_t nq, size_t dim, const float* d_radii, const uint64_t* d_idmask,
                        size_t mask_bits, size_t max_results, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                        uint64_t* d_out_totals, hipStream_t user_stream);

// One nearest row per group (vdb_flat_search_batch_distinct).  The driver is the same on a plain and on a sharded handle: H owns
// the buffers and the counters, s is the stream its kernels run on (the home device is current), `search` is the handle's ordinary
// device-pointer search -- outputs complete when it returns -- and everything in DistinctArgs has passed the entry point's checks.
struct DistinctArgs {
    const HostSearch& r; size_t kmax, len;
    const int32_t* d_codes; size_t codes_len;
    uint64_t id_bound; uint32_t n_cu;
};
using DistinctSearch = std::function<int(const float* d_q, size_t nq, size_t depth, const uint64_t* d_mask, size_t mask_bits,
                                         uint64_t* d_ids, float* d_dists, uint32_t* d_counts)>;
int distinct_drive(Index* H, hipStream_t s, const DistinctSearch& search, const DistinctArgs& a);
// The driver without its copy-out: the answers (ids, distances, codes [nq][kmax], kept [nq]) are left in H->dws (ai, ad, ac, kept),
// enqueued on s; *d_mask, if given, receives the staged mask the searches ran under (a.r.mask_bits bits; null: none).
int distinct_groups(Index* H, hipStream_t s, const DistinctSearch& search, const DistinctArgs& a, const uint64_t** d_mask = nullptr);

// Up to g rows of each of the k nearest groups (vdb_flat_search_batch_per_group); plain handles only.
// The caller's arrays beside those of a.r (ids and dists are then [nq][kstride][g]); sizes is [nq][kstride].
struct PerGroupOut { size_t g; uint32_t* sizes; };
int per_group_drive(Index* ix, hipStream_t s, const DistinctSearch& search, const DistinctArgs& a, const PerGroupOut& o);
// The host plan: the wanted codes -- the codes >= 0 among the first min(kept[b], kmax, ks[b] if given) entries of every row of
// codes [nq][kmax] -- ascending and distinct in *wanted, and in (*index)[b * kmax + j] the place of each such entry's code in
// it (0xffffffff for every other entry).
void per_group_plan(const int32_t* codes, const uint32_t* kept, const size_t* ks, size_t nq, size_t kmax, std::vector<int32_t>* wanted,
                    std::vector<uint32_t>* index);

// One batch, a filter per query (vdb_flat_search_batch_grouped).  The plan is host arithmetic alone: the
// permutation that makes every group's queries contiguous (scanned groups first, then the groups nothing is eligible for, the
// groups beyond the scan's capacity, the unfiltered queries), and per pass of SUPER permuted queries the tile table of the scan.
struct GroupTile { uint32_t group, j0, q0, nq; };                  // 64 list positions from j0 x nq <= 64 permuted queries from q0, ONE group
struct GroupPass { uint32_t q0, nq, tile0, n_tiles, stride; };     // permuted queries [q0, q0 + nq), tiles [tile0, tile0 + n_tiles), longest list rounded up to 64
struct GroupPlan {
    std::vector<uint32_t> perm;                                    // perm[i] = the caller's index of permuted query i
    std::vector<GroupTile> tiles; std::vector<GroupPass> passes;
    uint32_t n_scan = 0, n_empty = 0, n_over = 0, n_none = 0;      // queries of each kind, in the order of perm
};
// elig[g] = E_g; can_scan = false sends every non-empty group to the ordinary search (k beyond the select).  false: a group index
// that is neither below n_masks nor VDB_GROUP_NONE
bool group_plan(const uint32_t* group_of, size_t nq, const uint32_t* elig, size_t n_masks, bool can_scan, GroupPlan* out);
// Everything below has passed the entry point's checks.  slot[b]: the query's place among the R referenced masks (desc / h_desc:
// on the device and on the host) or VDB_GROUP_NONE; outputs [nq][k] on the device, complete when it returns.
struct GroupedArgs {
    const float* d_q; size_t nq, dim, k;
    const uint32_t* slot; const vdb::GroupedMask* d_desc; const vdb::GroupedMask* h_desc; size_t n_ref;
    uint64_t* d_out_ids; float* d_out_dists; uint32_t* d_out_counts;
};
int search_grouped(Index* ix, Workspace& W, hipStream_t s, const GroupedArgs& a);

// ---- vdb_multi.cpp: one index over several GPUs in one process (the parent handle dispatches here)
int multi_create(int metric, const int* devices, size_t n, vdb_flat_index** out);
void multi_destroy(vdb_flat_index* P);
int multi_add(vdb_flat_index* P, uint64_t id, const float* v, size_t dim);
int multi_add_bulk(vdb_flat_index* P, const uint64_t* ids, uint64_t first_id, const float* rows, size_t n, size_t dim, bool on_device);
int multi_remove(vdb_flat_index* P, uint64_t id);
int multi_get_vector(vdb_flat_index* P, uint64_t id, float* out, size_t cap, size_t* dim);
size_t multi_len(const vdb_flat_index* P);
size_t multi_dim(const vdb_flat_index* P);
int multi_reserve(vdb_flat_index* P, size_t rows, size_t dim);
int multi_for_each(vdb_flat_index* P, const std::function<int(vdb_flat_index*)>& f);
int multi_search_device(vdb_flat_index* P, const float* d_q, size_t nq, size_t dim, size_t k, const uint64_t* d_mask, size_t mask_bits,
                        uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts, hipStream_t user_stream);
// the host-pointer searches on a sharded handle; a compiled mask of r lives on the home device
int multi_search_host(vdb_flat_index* P, const HostSearch& r);
// vdb_flat_search_batch_by_id on a sharded handle (r.by): every shard gathers the rows of ITS query ids on its own device, the
// blocks meet on devices[0] device-to-device, the ordinary sharded search runs with k + 1 and the strike runs on devices[0].
// r.rec (vdb_flat_recommend_batch): one staged row per EXAMPLE, folded on devices[0] in list order into the nq queries; the
// search runs with k + the longest request and the set strike replaces the self strike
int multi_search_by_id(vdb_flat_index* P, const HostSearch& r);
// vdb_flat_search_batch_distinct on a sharded handle (the caller holds the parent's lock): the shards' staged adds flushed; the
// stream of devices[0] that distinct_drive's kernels run on; the sharded search behind a host wait for that stream (the shards'
// streams read what it wrote); the largest id bound of the shards
int multi_flush_nolock(vdb_flat_index* P);
hipStream_t multi_home_stream(const vdb_flat_index* P);
int multi_search_nolock(vdb_flat_index* P, const float* d_q, size_t nq, size_t dim, size_t k, const uint64_t* d_mask, size_t mask_bits,
                        uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts);
uint64_t multi_id_bound(const vdb_flat_index* P);
int multi_home(const vdb_flat_index* P);                           // devices[0]: where queries, masks and outputs live
int multi_set_exchange(vdb_flat_index* P, int mode);
size_t multi_shards(const vdb_flat_index* P);
size_t multi_shard_len(const vdb_flat_index* P, size_t g);
void multi_store_stats(const vdb_flat_index* P, uint64_t out[8]);
void multi_stats(const vdb_flat_index* P, uint64_t out[8]);
inline int refuse_multi(const char* what) { return fail(VDB_ERR_INVALID_ARGUMENT, "%s is not available on a sharded handle (vdb_flat_create_sharded)", what); }

}  // namespace vdbi
