// kernels.h -- parameter blocks and launchers shared by the HIP translation units
// and the host-side index (vdb_flat.cpp).  gfx950 (MI355X) only.
#pragma once
#include <hip/hip_runtime.h>

#include "row_split.h"
#include <stddef.h>
#include <stdint.h>

namespace vdb {

enum Metric : int { EUCLID = 0, COSINE = 1, DOT = 2 };

// Status bits written by kernels into the per-search status word.
enum : uint32_t {
    ST_NAN = 1u,          // a NaN distance was produced (reference: panic, flat_index.rs:62)
    ST_ZERO_QUERY = 2u,   // zero-norm query under Cosine (distance.rs:51-55)
};

constexpr uint64_t EMPTY_KEY = ~0ull;   // pool / candidate slot that holds no row
constexpr int KSTAGE = 32;              // K elements per LDS stage; device row stride is a multiple of it

// Order-preserving map f32 -> u32 (ascending unsigned == ascending float; -0 < +0).
__host__ __device__ inline uint32_t f32_to_ordered(float f) {
#ifdef __HIP_DEVICE_COMPILE__
    uint32_t b = __float_as_uint(f);
#else
    union { float f; uint32_t u; } c; c.f = f; uint32_t b = c.u;
#endif
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ inline float ordered_to_f32(uint32_t k) {
    uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(b);
#else
    union { float f; uint32_t u; } c; c.u = b; return c.f;
#endif
}
// Candidate key: ranking score in the high word, device row (or id rank) in the low word.
// A NaN score gets the smallest key so that it is always selected and reported.
__host__ __device__ inline uint64_t make_key(float score, uint32_t row) {
    uint32_t hi = (score != score) ? 0u : f32_to_ordered(score);
    return ((uint64_t)hi << 32) | row;
}

// Raw pool entry written by the fused kernels' epilogue: the score's f32 bits and the row (0xffffffff =
// ineligible row).  The select's gather turns it into an ordered candidate key (cheaper than doing the
// order-preserving transform and the NaN test inside the MFMA kernel, where every VALU instruction
// takes cycles from the f32 MFMA pipe).
__host__ __device__ inline uint64_t make_raw_key(float score, uint32_t row) {
#ifdef __HIP_DEVICE_COMPILE__
    return ((uint64_t)__float_as_uint(score) << 32) | row;
#else
    union { float f; uint32_t u; } c; c.f = score; return ((uint64_t)c.u << 32) | row;
#endif
}
__device__ inline uint64_t raw_to_key(uint64_t raw) {
    const uint32_t row = (uint32_t)raw;
    return row == 0xffffffffu ? EMPTY_KEY : make_key(__uint_as_float((uint32_t)(raw >> 32)), row);
}

// ---------------------------------------------------------------- row store statistics
struct RowStatsParams {
    const float* rows; uint32_t ld; uint32_t dim;
    uint32_t row_begin, row_end;
    int metric;
    float* nd;        // exact-order norm  sqrt(fold(x*x))      (vector.rs:35-37)
    float* alpha;     // score = fma(dot, alpha, beta)
    float* beta;
    uint32_t* nd2max_bits;   // atomicMax of the f32 bits of fold(x*x); [2] / [3]: max of the bf16 rounding error of a
                             // row, as f32 bits of |x - bf16(x)|^2 (slot 2) and of |x - bf16(x)|^2 / |x|^2 (slot 3);
                             // [4]: atomicMin of ~bits of the smallest positive finite margin (stored complemented so that 0 = none yet)
    // Screening-tier certificate, LOCAL form (Dot / Euclid; null under Cosine, whose relative row error is bounded by
    // 2^-9 whatever the data): margin[row] = max(m_e |x - bf16(x)| + m_n |x|, m_b |x|), rounded up, so that
    // g_q * margin[row] >= the whole row-dependent part of the score error for a query with g_q = |q| + kappa |q - bf16(q)|
    // (QueryPrepParams::kappa, m_b = B/kappa); beta_shrink: Euclid's beta = |x|^2 (1 - beta_shrink), rounded down.
    float* margin; float m_e, m_n, m_b, beta_shrink;
};
void launch_row_stats(const RowStatsParams& p, hipStream_t s);
// bf16 shadow of rows [row_begin, row_end): v_cvt_pk_bf16_f32 (RNE) of every element of the padded row -- the rounding the
// f32-row screening kernels apply to their fragments in registers
void launch_rows_to_bf16(const float* rows, uint16_t* rows16, uint32_t ld, uint32_t row_begin, uint32_t row_end, hipStream_t s);
// compact bf16 copy of the S = 2^shift sample rows of the screening tier: out[j] = bf16(rows[screen_sample_row(j)]), j < S
void launch_sample_to_bf16(const float* rows, uint32_t ld, uint32_t n_rows, uint32_t n_sample, uint32_t shift, uint16_t* out, hipStream_t s);
// kernels_split.hip: rows [0, n_rows) converted in place between the F32 and the SPLIT layout (row_split.h; ld a multiple of 32,
// at most 16384).  forward: *nonfinite is OR-ed with 1 if any element has an all-ones exponent (the caller zeroes it first).
void launch_row_split(float* rows, uint32_t ld, uint32_t n_rows, bool forward, uint32_t* nonfinite, uint32_t n_cu, hipStream_t s);

// count live rows whose norm is exactly zero (Cosine: distance.rs:51-55)
void launch_count_zero_live(const float* nd, const uint32_t* livemask, uint32_t n_rows,
                            uint32_t* out_count, hipStream_t s);

// rowmask[w] = live[w] & (id mask bits gathered through row_ids)
void launch_build_rowmask(const uint64_t* row_ids, const uint32_t* livemask, const uint64_t* idmask,
                          uint64_t mask_bits, uint32_t n_rows, uint32_t* out_mask, hipStream_t s);

// ---------------------------------------------------------------- row store compaction (kernels_compact.hip)
// One chunk of vdb_flat_compact: the live rows of source rows [row_begin, row_end) move, with every per-row column, to
// dst[dest(r) - dst_sub], dest(r) = prefix[r >> 5] + popc(live[r >> 5] & ((1 << (r & 31)) - 1)).  src == dst is the in-place
// form (the host guarantees dest(row_end) <= row_begin); live == null is the identity form (row r -> r - dst_sub).
struct CompactMoveParams {
    const uint32_t* live; const uint32_t* prefix;      // old live mask and its exclusive per-word popcount prefix
    uint32_t row_begin, row_end, dst_sub;
    uint32_t ld, lanes_log2;                           // lanes per row: 2^lanes_log2 in [8, 64] (compact_lanes_log2)
    const float* src_rows; float* dst_rows;
    const uint16_t* src_rows16; uint16_t* dst_rows16;  // null without the bf16 shadow
    const float* src_nd; float* dst_nd; const float* src_alpha; float* dst_alpha; const float* src_beta; float* dst_beta;
    const float* src_margin; float* dst_margin;        // null under Cosine
    const uint64_t* src_ids; uint64_t* dst_ids;
};
inline uint32_t compact_lanes_log2(uint32_t ld) { uint32_t l = 3; while (l < 6 && (1u << l) < (ld >> 2)) ++l; return l; }
void launch_compact_move(const CompactMoveParams& p, uint32_t n_cu, hipStream_t s);

// ---------------------------------------------------------------- query preparation
struct QueryPrepParams {
    const float* q_in; uint32_t dim; uint32_t nq;      // [nq][dim] as handed over
    float* qp; uint32_t ld; uint32_t nq_pad;           // [nq_pad][ld], zero padded
    float* qnorm;                                      // exact-order norm per query [nq_pad]
    float* thr;                                        // padding queries get -inf here (nothing passes)
    int metric;
    uint32_t* status;
    uint16_t* qb;                                      // may be null: [nq_pad][ld] bf16 (RNE) copy for the screening tier
    float* qerr;                                       // with qb: |q - bf16(q)| per query (upper bound)
    float* qg; float kappa;                            // with qb (may be null): g_q = |q| + kappa |q - bf16(q)|, rounded up (RowStatsParams::margin)
    uint32_t* clear_a; uint32_t* clear_b;              // may be null: per-query flag words this kernel zeroes (cert, overflow)
};
void launch_query_prep(const QueryPrepParams& p, hipStream_t s);

// ---------------------------------------------------------------- dense scores (sample / small N)
struct DenseParams {
    const float* rows; uint32_t ld; uint32_t n_rows;
    const float* qp; uint32_t nq_pad;                  // multiple of 32
    const float* alpha; const float* beta;
    const uint32_t* rowmask;                           // may be null (all rows eligible)
    uint32_t n_sample;                                 // sample j -> row j*n_rows/n_sample
    uint64_t* keys; uint32_t key_stride;               // keys[q*key_stride + j]
};
void launch_dense_scores(const DenseParams& p, hipStream_t s);

// ---------------------------------------------------------------- per-query radix select
struct SelectParams {
    const uint64_t* keys; size_t stride;               // per-query key block
    const uint32_t* counts; uint32_t n_fixed;          // counts != null: n = min(counts[q], cap)
    uint32_t cap;
    // gather mode (n_sub > 0): the query's keys live in n_sub sub-pools of capacity capl,
    // keys[(q*n_sub + s)*capl + j], j < sub_counts[q*n_sub + s]
    const uint32_t* sub_counts; uint32_t n_sub; uint32_t capl;
    uint32_t wg_major;                                 // 1: sub-pool i = wg*4 + r of query q has its count at VDB_BF16_SUBPOOL_R(wg, q, r) and its keys at that * capl (bf16 tier)
    size_t blk_keys, blk_cnts;                         // wg_major, more than 256 queries in one launch: query q lives in block q >> 8, whose pools start blk_keys keys / blk_cnts counts after the previous block's
    uint32_t kk;                                       // how many smallest keys to keep (<= 2048)
    uint64_t* out_keys; uint32_t out_stride;           // sorted ascending, padded with EMPTY_KEY
    uint32_t* out_cnt;
    float* out_thr;                                    // may be null: score of the kk-th key, +inf if fewer
    const float* shift_g; const uint32_t* shift_m_bits; // may be null: out_thr[q] -= shift_g[q] * f32(*shift_m_bits)  (plain-score
                                                       // sample threshold -> lower-bound units, see launch_sample_bf16)
    uint32_t* ovf;                                     // may be null: set when counts[q] > cap
    uint32_t* summary;                                 // may be null: OR-ed with 2 whenever an overflow flag is set
    uint32_t flag_truncation;                          // 1: more valid keys than kk also sets ovf[q] (the caller needs ALL of them)
    const uint64_t* lo_excl;                           // may be null: only keys > lo_excl[q] take part (chunked large k)
    uint64_t* out_last;                                // may be null: largest selected key per query (unchanged if none)
    // EMIT (may be null; keys = ordered(exact distance) << 32 | id rank, as the exact scans write them): the selected keys are
    // also written as final results -- emit_ids / emit_dists [q * emit_stride + i], emit_counts[q] -- and the search's status
    // word is copied to emit_status[q].  The outputs may live in mapped host memory (the small-index direct path).
    uint64_t* emit_ids; float* emit_dists; uint32_t* emit_counts; uint32_t emit_stride;
    const uint32_t* emit_rank2row; const uint64_t* emit_row_ids;
    const uint32_t* emit_status_in; uint32_t* emit_status;
};
void launch_select(const SelectParams& p, uint32_t nq, hipStream_t s);
// The screening tier's THRESHOLD select: only the score of the kk-th smallest of n_fixed <= 4096 keys per query is wanted
// (out_thr, with the shift_g / shift_m_bits adjustment) -- no sorted list.  A 256-thread workgroup keeps the keys' score
// words in registers and finds the value with four 8-bit radix passes: ~5 us against the general kernel's ~15.
void launch_thr_select(const SelectParams& p, uint32_t nq, hipStream_t s);

// ---------------------------------------------------------------- fused MFMA score + threshold filter
struct FusedParams {
    const float* rows; uint32_t ld; uint32_t n_rows;
    const float* qp;                                   // padded queries, row q_base is the first of this launch
    uint32_t q_base;
    const float* alpha; const float* beta;
    const uint32_t* rowmask;                           // NEVER null here: the live mask when there is no filter
    const float* thr;                                  // [nq_pad] inclusive threshold per query
    // candidate pools: one private sub-pool per (query, row range, row part, lane half):
    //   sub = ((q*n_wg + range)*RP + part)*2 + half ; keys at pool[sub*capl ..], count at pool_cnt[sub]
    uint64_t* pool; uint32_t* pool_cnt; uint32_t capl;
    uint32_t n_wg;                                     // row ranges = grid.x
    uint32_t ablate;                                   // diagnostics only (VDB_FUSED_ABLATE): 1 skip MFMAs, 2 skip staging, 4 skip barriers, 8 skip epilogue
};
// nqt = number of 32-query tiles handled per workgroup (1, 2, 4 or 8); grid.y super-tiles of 32*nqt queries
void launch_fused(const FusedParams& p, int nqt, uint32_t n_super, hipStream_t s);
size_t fused_lds_bytes(int nqt);
uint32_t fused_tile_rows(int nqt);
uint32_t fused_subpools_per_query(int nqt, uint32_t n_wg);
#ifdef VDB_DIAG
// 2-image LDS-DMA variant of the headline shape (nqt = 8; diagnostics build: A/B against dma3)
void launch_fused_dma(const FusedParams& p, uint32_t n_super, hipStream_t s);
#endif
// three-image ring, barrier in the middle of a stage (kernels_fused_dma3.hip)
void launch_fused_dma3(const FusedParams& p, uint32_t n_super, hipStream_t s);

// ---------------------------------------------------------------- bf16 screening tier (fused_bf16_common.h)
// CANDIDATE-POOL LAYOUT, workgroup-major: workgroup wg of a filter pass owns, for query q of the pass's 256-query block, the
// four private sub-pools r = 2 * row half + lane half.  Sub-pool (wg, q, r) has its count at pool_cnt[index] and its keys at
// pool[index * capl ..].  Workgroup-major, so that the few scattered appends of one workgroup fall into ONE 2 MB region
// instead of one region per query (256 regions 2 MB apart: every append then missed the CU's address-translation cache in
// front of the row stream), and its 1024 counts are one 4 KB block written in whole lines.  The filter kernels, the select's
// gather (SelectParams::wg_major) and pool_to_dense all go through this one function: a writer and a reader that disagree
// lose candidates silently.
__host__ __device__ constexpr size_t fused_bf16_subpool(size_t wg, uint32_t q, uint32_t row_half, uint32_t lane_half) { return ((wg * 256 + q) * 2 + row_half) * 2 + lane_half; }
// The same index from r = 2 * row half + lane half, for the readers (which walk r = 0..3) and the wide kernel (which derives r
// on its rare path).  A macro whose R lands unparenthesised at the end of the sum, on purpose: the wide kernel sits at the
// 256-VGPR limit, and every function form of this line -- forwarding to the one above included -- reordered its integer
// arithmetic and with it the register allocation of the whole kernel (tools/isa_diff.py).  The static_assert ties the two.
#define VDB_BF16_SUBPOOL_R(WG, Q, R) (((size_t)(WG) * 256 + (Q)) * 4 + R)
static_assert(fused_bf16_subpool(7, 201, 1, 0) == VDB_BF16_SUBPOOL_R(7, 201, 2) && fused_bf16_subpool(7, 201, 1, 1) == VDB_BF16_SUBPOOL_R(7, 201, 3), "one layout");
__host__ __device__ inline uint32_t fused_bf16_subpools_per_query(uint32_t n_wg) { return 4u * n_wg; }
// SAMPLE INDEX -> DEVICE ROW.  The S = n_sample = 2^shift <= n_rows sample positions are spread evenly over the rows
// ((pos * n) >> shift), and CONSECUTIVE positions go to DIFFERENT tiles (index j = tile*256 + tile-row sits at position
// tile-row*tiles + tile): when near neighbours are stored next to each other (data ordered by cluster) their sample rows then
// land in different groups, each contributes its own group minimum, and the threshold stays as tight as on shuffled data (with
// consecutive positions in one tile a 500-row cluster was represented by 4 minima, the threshold came from far rows and
// thousands of keys overflowed the pools).  sample_block != 0 (diagnostics): tiles of sample_block contiguous rows.  The
// sample kernels and the compact sample copy (launch_sample_to_bf16) are only valid together if they all use this function.
__host__ __device__ inline uint32_t screen_sample_row(uint32_t j, uint32_t n_sample, uint32_t shift, uint32_t n_rows, uint32_t sample_block = 0) {
    if (sample_block) return (j >> 8) * sample_block + (j & 255u);
    const uint32_t pos = (j & 255u) * (n_sample >> 8) + (j >> 8);
    return (uint32_t)(((uint64_t)pos * n_rows) >> shift);
}
struct FusedBf16Params {
    const float* rows; uint32_t ld; uint32_t n_rows;
    const uint16_t* rows16;                            // bf16 shadow of `rows`, same pitch (kernels_fused_s16.hip; null unless vdb_flat_set_shadow and ld % 64 == 0)
    uint32_t rows16_pitch;                             // 16-bit words between two rows of rows16; 0 = ld (the shadow, the sample copy).  2 * ld: rows16 is the
                                                       // store itself in the SPLIT layout (row_split.h) and the kernel streams the hi piece of every row
    const uint16_t* qb;                                // [256][ld] bf16 queries of this pass (zero padded)
    const float* alpha; const float* beta;
    // non-null (Dot / Euclid): the kernels rank by the LOWER-BOUND score  fma(-qg[q], margin[row], fma(dot, alpha, beta)),
    // i.e. the score minus everything the bf16 rounding, the MFMA accumulation and the oracle's own f32 fold can
    // contribute for THIS row and query -- the certificate then needs no per-index maxima (kernels_aux.hip cert_test)
    const float* margin; const float* qg;
    const uint32_t* rowmask;                           // NEVER null: the live mask when there is no filter
    // "No score of this launch can be NaN" (fused_no_nan below): the index scalars (max |d|^2, smallest positive |d|^2 under
    // Cosine) and the largest query norm of the search as f32 bits (query_prep: status block word 2).  May be null (= unknown).
    const uint32_t* scalars; const uint32_t* qmax_bits;
    // filter mode: keys with score <= thr[q] go to the lane's private sub-pool, fused_bf16_subpool(wg, q, row half, lane half)
    const float* thr;                                  // [256]
    uint64_t* pool; uint32_t* pool_cnt; uint32_t capl;
    uint32_t n_wg;                                     // row ranges = grid.x
    // the WIDE filter kernel (kernels_fused_bf16w.hip) serves two consecutive 256-query blocks per launch: qb / thr / qg cover
    // 512 queries, block b's pools start at pool + b * pool_block_stride (keys) and pool_cnt + b * cnt_block_stride
    size_t pool_block_stride, cnt_block_stride;
    // sample mode: n_sample = 2^sample_shift <= n_rows, sample j -> screen_sample_row(j); per query and group of 64 sample
    // rows the smallest key
    uint32_t n_sample, sample_shift, sample_block; uint64_t* minkeys; uint32_t minkey_stride;   // minkeys[q*minkey_stride + group]
    uint32_t ablate;                                   // diagnostics only (VDB_BF16_ABLATE): 1 skip LDS reads + MFMAs (unpipelined kernel only), 2 skip the row DMA, 4 skip the query DMA, 8 skip the epilogue, 16 (pipelined kernel) thresholds = -inf: nothing passes the filter
};
#ifdef VDB_DIAG
void launch_fused_bf16(const FusedBf16Params& p, hipStream_t s);      // unpipelined filter pass (diagnostics build: A/B against bf16p)
#endif
void launch_sample_bf16(const FusedBf16Params& p, hipStream_t s);
void launch_fused_bf16p(const FusedBf16Params& p, hipStream_t s);     // the filter pass, software-pipelined (default)
void launch_fused_bf16w(const FusedBf16Params& p, hipStream_t s);     // kernels_fused_bf16w.hip: the WIDE filter pass, 128 rows x 512 queries per workgroup (batches above 256 queries)
uint32_t fused_bf16w_tile_rows();
// With every row norm and query norm in [2^-40, 2^40] (zero allowed) no accumulator can overflow and no alpha / beta is
// non-finite, so fma(acc, alpha, beta) is never NaN -- the filter epilogues may then test the MINIMUM of four scores against the
// threshold (v_min_f32 drops a NaN operand; a NaN score must pass the filter, flat_index.rs:62).  Otherwise they add a NaN
// test per group.  Wave-uniform, evaluated once per launch.
__device__ inline bool fused_no_nan(const uint32_t* scalars, const uint32_t* qmax_bits, bool cosine) {
    if (!scalars || !qmax_bits) return false;
    const uint32_t n2max = scalars[0], qmax = *qmax_bits;
    bool ok = n2max <= 0x67800000u /* 2^80 */ && qmax <= 0x53800000u /* 2^40 */;
    if (cosine) { const uint32_t mb = scalars[5]; ok = ok && mb != 0u && (~mb) >= 0x17800000u /* 2^-80 */; }
    return ok;
}
void launch_fused_s16(const FusedBf16Params& p, hipStream_t s);       // kernels_fused_s16.hip: the filter pass over p.rows16 (ld % 64 == 0)
void launch_sample_s16(const FusedBf16Params& p, hipStream_t s);      // the sample pass over a COMPACT bf16 copy of the sample rows (p.rows16 = the copy)
uint32_t fused_bf16_tile_rows();
uint32_t fused_bf16_sample_groups(uint32_t n_sample);

// compact re-run of uncertified queries: gather padded query rows / norms, scatter results back
void launch_gather_queries(const float* qp, const float* qnorm, uint32_t ld, const uint32_t* qidx, uint32_t n,
                           uint32_t n_pad, float* qp_out, float* qnorm_out, float* thr_out, hipStream_t s);
void launch_scatter_results(const uint64_t* ids, const float* dists, const uint32_t* counts, const uint32_t* qidx,
                            uint32_t n, uint32_t k, uint64_t* out_ids, float* out_dists, uint32_t* out_counts,
                            hipStream_t s);

// the same for an explicit (source, destination) list
void launch_scatter_results_list(const uint64_t* ids, const float* dists, const uint32_t* counts, const uint32_t* src,
                                 const uint32_t* dst, uint32_t n, uint32_t k, uint64_t* out_ids, float* out_dists,
                                 uint32_t* out_counts, hipStream_t s);

// ---------------------------------------------------------------- exact re-rank + certification
struct RerankParams {
    const float* rows; uint32_t ld; uint32_t dim; uint32_t n_rows;
    const float* qp; const float* qnorm;
    const float* nd;
    const uint64_t* row_ids;
    const uint32_t* rowmask;                           // may be null
    const uint64_t* cand; uint32_t cand_stride; const uint32_t* cand_cnt; uint32_t kp;   // kp <= 256 candidates, sorted by score
    uint32_t kp_first, kp_step;                        // adaptive depth: re-rank kp_first, then kp_step more per round (0: kp at once)
    uint32_t* depth;                                   // may be null: candidates re-ranked per query (diagnostics)
    float* thr_next;                                   // may be null: for an UNCERTIFIED query the score cut above which no row can
                                                       // enter the top k (from the k-th exact distance found so far); NaN: no cut known
    uint32_t cut_always;                               // 1 (VDB_TIERS_FORCE_RETHRESHOLD): thr_next gets the cut of EVERY query that has one
                                                       // (a k-th exact distance, no NaN / ineligible candidate), certified or not
    int metric;
    uint32_t k;                                        // results wanted per query
    float eps_coef; const uint32_t* nd2max_bits;       // certification bound inputs (max row norm^2, f32 bits)
    uint64_t* out_ids; float* out_dists; uint32_t* out_counts; uint32_t out_stride;
    uint32_t* cert;                                    // [nq]: 1 = certified exact
    uint32_t* status;
    const float* thr;                                  // may be null: the filter threshold the candidates passed; a short
                                                       // candidate list under a FINITE threshold is never certified
    const float* qerr; float c_acc;                    // bf16 screening tier (qerr != null): |q - bf16(q)| per query and the
                                                       // MFMA accumulation coefficient; the row-side error maxima are
                                                       // nd2max_bits[2] and [3]
    uint32_t lb_scores;                                // 1 (with qerr; Dot / Euclid): candidate scores and thresholds are the
                                                       // LOWER-BOUND scores of FusedBf16Params::margin -- every row-dependent
                                                       // error term is already inside them
    uint32_t lds_row_stride, lds_chunk;                // filled by launch_rerank
    uint32_t split;                                    // 1: `rows` is in the SPLIT layout (row_split.h; ld % 64 == 0): launch_rerank, _rerank_all, _rerank_large and
                                                       // _rerank_all_large stage the hi and the lo piece of a slice and rebuild each f32 in the fold
};
void launch_rerank(const RerankParams& p, uint32_t nq, hipStream_t s);
// the large-k re-rank of the screening tier: 112 < k <= 1024, up to 2048 candidates per query (kernels_aux.hip)
void launch_rerank_large(const RerankParams& p, uint32_t nq, hipStream_t s);
// exhaustive variant: EVERY candidate of the list (up to cand_stride, any order) is re-ranked, the best k are kept;
// cert[q] = 1 unless the list was truncated upstream (the caller's overflow flag) or a NaN score was seen
void launch_rerank_all(const RerankParams& p, uint32_t nq, hipStream_t s);
// the same for 112 < k <= 1024: up to 2048 keys per query through the sweep and sort area of the large-k re-rank
void launch_rerank_all_large(const RerankParams& p, uint32_t nq, hipStream_t s);

// ---------------------------------------------------------------- direct exact scan of a SMALL index for a few queries
// Index::search as it stands (flat_index.rs:52-65) for indexes of at most 16384 rows and batches of at most 8 queries -- the shape
// of BASELINE configs[0] (10k x 128, ONE query): every row's exact distance in the reference's operation order, straight from
// the raw queries (which may live in mapped host memory): no query preparation pass, no MFMA scores, no certificate.
struct SmallScanParams {
    const float* rows; uint32_t ld; uint32_t dim; uint32_t n_rows;
    const float* q_in; uint32_t nq;                    // [nq][dim] as handed over
    const float* nd; const uint32_t* rowmask; const uint32_t* idrank; int metric;
    uint64_t* keys; uint32_t key_stride;               // key = ordered(dist) << 32 | id rank, EMPTY if ineligible
    // keep == 0: keys[q * key_stride + row], every row's key.  keep = k' < 256: every workgroup of 256 rows keeps only its k'
    // smallest keys (any global top-k with k <= k' is among them): keys[q * key_stride + workgroup * k' + i], EMPTY padded --
    // the select then sees n/256 * k' keys instead of n (10k rows, k = 10: 400 keys, ranked by counting in ~3 us instead of
    // seven radix passes over 10k keys in 57 us)
    uint32_t keep;
    uint32_t* status;                                  // ST_NAN / ST_ZERO_QUERY
};
void launch_small_scan(const SmallScanParams& p, hipStream_t s);
uint32_t small_scan_groups(uint32_t n_rows);           // workgroups along the rows

// ---------------------------------------------------------------- exact scan (fallback, any k)
struct ExactScanParams {
    const float* rows; uint32_t ld; uint32_t dim; uint32_t n_rows;
    const float* q; const float* qnorm;                // one padded query row and its exact-order norm
    const float* nd;
    const uint32_t* rowmask;
    const uint32_t* idrank;                            // may be null: rank == row
    int metric;
    uint64_t* keys;                                    // [n_rows]: ordered(exact dist)<<32 | idrank, EMPTY if ineligible
    uint32_t* status;
};
void launch_exact_scan(const ExactScanParams& p, hipStream_t s);

// The bounded exact scan: ONE pass over the rows for up to 8 queries; a row is kept for query j only if its exact distance
// passes the query's bound, so the survivors are a handful of keys per query.  The bound is one of
//   radii != null (the exact range scan):  d <= radii[qidx[j]]
//   radii == null (the kNN fallback):      !(d > bound_j), bound_j = the k-th exact distance the re-rank already produced (an
//                                          upper bound of the true k-th distance), +inf where prev_counts says there is none
struct BoundedScanParams {
    const float* rows; uint32_t ld; uint32_t dim; uint32_t n_rows;
    const float* qp; const float* qnorm;               // padded query block and norms of the whole batch
    const float* nd; const uint32_t* rowmask; const uint32_t* idrank;
    int metric;
    uint32_t nqf; uint32_t qidx[8];                    // batch indices of the queries of this pass
    const float* radii;                                // range: [batch]; null for the kNN fallback, which reads instead
    const float* prev_dists; const uint32_t* prev_counts; uint32_t k;   // the re-rank outputs: bound = dists[q*k + k-1] if counts[q] == k
    uint64_t* keys; uint32_t cap; uint32_t* cnt;       // keys[j*cap + slot], cnt[j] = ALL survivors (may exceed cap: overflow)
    uint32_t* status;                                  // ST_NAN
};
void launch_bounded_scan(const BoundedScanParams& p, hipStream_t s);

// ---------------------------------------------------------------- exact range search (kernels_range.hip)
// thr[q] = score_cut(radii[q]) from the constants of the re-rank's certificate (cert: metric, ld, qnorm, qerr, c_acc, eps_coef,
// nd2max_bits, lb_scores -- what rerank_kernel hands to score_cut); -inf for an empty answer (r < 0 under Euclid / Cosine) and
// for a query without a finite cut, which gets nocut[q] = 1
struct RangeCutParams {
    RerankParams cert;
    const float* radii; uint32_t nq;
    float* thr; uint32_t* nocut;
};
void launch_range_cut(const RangeCutParams& p, hipStream_t s);
// the tail of the screened route: every key of cand[q * cand_stride ..] (cand_cnt[q] of them, any order) evaluated exactly, the
// rows with d <= radii[q] sorted by (distance, id); out_*[q * max_results ..] padded with (~0, NaN)
struct RangeRerankParams {
    const float* rows; uint32_t ld; uint32_t dim; uint32_t n_rows;
    const float* qp; const float* qnorm; const float* nd;
    const uint64_t* row_ids; const uint32_t* rowmask;  // rowmask may be null
    const uint64_t* cand; uint32_t cand_stride; const uint32_t* cand_cnt;   // cand_stride <= 2048
    const float* radii; int metric; uint32_t max_results;
    uint64_t* out_ids; float* out_dists; uint32_t* out_counts; uint64_t* out_totals;   // out_totals may be null
    uint32_t* complete;                                // [nq]: 0 = a NaN-score key was in the list (the exact range scan answers)
    uint32_t* n_keys;                                  // [nq]: keys evaluated
    uint32_t* status;                                  // ST_NAN
    uint32_t lds_row_stride, lds_chunk;                // filled by launch_range_rerank
};
void launch_range_rerank(const RangeRerankParams& p, uint32_t nq, hipStream_t s);

// ---------------------------------------------------------------- sparse-filter route (kernels_sparse.hip)
// The ascending list of the rows whose bit is set in a search's row mask (bits at or above n_rows never count), in two steps
// with the host in between: launch_sparse_count leaves E in *total (block_cnt / block_off: sparse_list_blocks(n_rows) words
// each), the host reads it and sizes elig[], launch_sparse_scatter writes elig[0..E) (positions >= cap are dropped).
uint32_t sparse_list_blocks(uint32_t n_rows);
void launch_sparse_count(const uint32_t* rowmask, uint32_t n_rows, uint32_t* block_cnt, uint32_t* block_off, uint32_t* total, hipStream_t s);
void launch_sparse_scatter(const uint32_t* rowmask, uint32_t n_rows, const uint32_t* block_off, uint32_t* elig, uint32_t cap, hipStream_t s);
// The exact reference distance of every (query, eligible row) pair; one workgroup = SPARSE_TILE_R list positions x SPARSE_TILE_Q queries.
constexpr uint32_t SPARSE_TILE_R = 64, SPARSE_TILE_Q = 64;
struct SparseScanParams {
    const float* rows; uint32_t ld; uint32_t dim; uint32_t n_rows;
    const uint32_t* elig; uint32_t n_elig;             // device rows, ascending; an entry >= n_rows is skipped
    const float* qp; const float* qnorm; uint32_t nq;  // prepared queries of this pass (query_prep), their exact-order norms
    const float* nd; const uint32_t* idrank; int metric;
    uint64_t* keys; uint32_t key_stride;               // keys[q * key_stride + j], j = position in elig; key = ordered(dist) << 32 | id rank.
                                                       // key_stride = n_elig rounded up to SPARSE_TILE_R: the padding gets EMPTY_KEY
    uint32_t* status;                                  // ST_NAN
};
void launch_sparse_scan(const SparseScanParams& p, hipStream_t s);

// ---------------------------------------------------------------- grouped route (kernels_grouped.hip)
// One batch, a filter per query: the queries that share an id mask are a group, and every group gets the scan above.
struct GroupedMask { const uint64_t* words; uint64_t bits; };          // an id mask in the layout of launch_build_rowmask's
// rowmasks[g][w] = live AND mask_g gathered through row_ids, (n_rows + 31) / 32 words per group; row_ids and the live word are
// read once for all groups
void launch_grouped_rowmasks(const uint64_t* row_ids, const uint32_t* livemask, const GroupedMask* masks, uint32_t n_groups, uint32_t n_rows,
                             uint32_t* rowmasks, hipStream_t s);
// launch_sparse_count for every group: block_cnt / block_off [n_groups][sparse_list_blocks(n_rows)], totals[g] = E_g
void launch_grouped_count(const uint32_t* rowmasks, uint32_t n_groups, uint32_t n_rows, uint32_t* block_cnt, uint32_t* block_off,
                          uint32_t* totals, hipStream_t s);
// launch_sparse_scatter for every group: glist[g] = {offset, length} of group g's list inside lists[0..lists_cap); length 0 = no list
void launch_grouped_scatter(const uint32_t* rowmasks, uint32_t n_groups, uint32_t n_rows, const uint32_t* block_off, const uint32_t* glist,
                            uint32_t* lists, uint32_t lists_cap, hipStream_t s);
// The scan of one pass over a tile table.  scan: as launch_sparse_scan sees a pass, with elig / n_elig = ALL lists and their total
// length, qp / qnorm / nq = the permuted queries of the pass, key_stride = the pass's longest list rounded up to SPARSE_TILE_R.
// tiles[i] = {group, first list position (a multiple of SPARSE_TILE_R), first permuted query (batch-wide: q_base is the pass's
// first), queries (<= SPARSE_TILE_Q)}.  Key positions of a query past its group's rounded list length are NOT written: the
// select reads counts.
struct GroupedScanParams {
    SparseScanParams scan;
    const uint32_t* tiles; uint32_t n_tiles;
    const uint32_t* glist; uint32_t n_groups;
    uint32_t q_base;
};
void launch_grouped_scan(const GroupedScanParams& p, hipStream_t s);

// ---------------------------------------------------------------- metadata filters compiled on the device (kernels_filter.hip)
// A MetadataFilter as a postfix program over the resident metadata columns (vdb_meta.cpp).  Every leaf carries its
// column: codes[id] for id < len, -1 ("no such field") at and above len -- such an id reads no memory.
// A numeric leaf (FOP_LT .. FOP_GE) compares the NUMBER of the row's string with a constant: v = lut[codes[id]], the column's
// f64 table by dictionary code; a code that is negative or at / beyond lut_len, and a NaN entry, mean "no number" and match
// nothing.  Its lut, lut_len and constant live in a second array, nums[op.code], so that FilterOp stays 24 bytes.
enum : uint32_t { FOP_EQ = 0, FOP_NE = 1, FOP_EXISTS = 2, FOP_CONST = 3, FOP_AND = 4, FOP_OR = 5, FOP_LT = 16, FOP_LE = 17, FOP_GT = 18, FOP_GE = 19 };
constexpr uint32_t FILTER_MAX_OPS = 1024, FILTER_MAX_DEPTH = 32;   // the evaluation stack is the bits of one 32-bit register
struct FilterOp { const int32_t* codes; uint64_t len; uint32_t op; int32_t code; };   // FOP_CONST: code = 0 | 1; numeric: code = index into nums
struct FilterNum { const double* lut; uint64_t lut_len; double c; };                  // c is never NaN (the host checked)
struct FilterParams {
    const FilterOp* ops; uint32_t n_ops;               // device memory; well-formed, n_ops <= FILTER_MAX_OPS, depth <= FILTER_MAX_DEPTH (the host checked)
    uint32_t n_nums; const FilterNum* nums;            // device memory; one per numeric leaf, n_nums <= n_ops; every numeric op's code < n_nums
    const uint64_t* present; uint64_t present_words;   // presence bitmap by id; words at and above present_words read as 0
    uint64_t mask_bits;                                // ids at and above contribute 0
    uint64_t* mask;                                    // out: (mask_bits + 63) / 64 words, every one written
    unsigned long long* count;                         // += popcount of the mask (zeroed by the caller on the same stream)
};
void launch_filter_compile(const FilterParams& p, uint32_t n_cu, hipStream_t s);   // mask_bits == 0: no launch

// A rank or row at or beyond n_rows is written as padding (~0, NaN), never dereferenced.
struct EmitParams {                                    // sorted exact keys -> (id, dist) outputs
    const uint64_t* keys; uint32_t cnt_max; const uint32_t* cnt;
    const uint32_t* rank2row; const uint64_t* row_ids;
    uint64_t* out_ids; float* out_dists; uint32_t* out_count; uint32_t k;
    uint32_t accumulate;                               // 1: *out_count += n (chunked large k), 0: *out_count = n
    uint32_t n_rows;
};
// emit for several queries at once: query j (= blockIdx.y) reads keys + j*key_stride, cnt[j] (selected) and writes
// to out_*[qidx[j]*k ..] / out_count[qidx[j]]; with out_totals, out_totals[qidx[j]] = survivors[j] (the range scan's total)
struct EmitMultiParams {
    const uint64_t* keys; uint32_t key_stride; const uint32_t* cnt;
    const uint32_t* survivors; uint64_t* out_totals;   // both may be null
    const uint32_t* rank2row; const uint64_t* row_ids; uint32_t n_rows;
    uint64_t* out_ids; float* out_dists; uint32_t* out_count; uint32_t k;
    uint32_t nqf; uint32_t qidx[8];
};
void launch_emit_multi(const EmitMultiParams& p, hipStream_t s);
void launch_emit(const EmitParams& p, hipStream_t s);

// ---------------------------------------------------------------- multi-GPU partial merge
void launch_merge_parts(const uint64_t* ids, const float* dists, const uint32_t* counts, uint32_t nparts,
                        uint32_t nq, uint32_t k, uint64_t* out_ids, float* out_dists, uint32_t* out_counts,
                        hipStream_t s);

// ---------------------------------------------------------------- candidate-list distances (HNSW offload hook)
struct PairDistParams {
    const float* rows; uint32_t ld; uint32_t dim;
    const float* qp; const float* qnorm; const float* nd;
    const uint32_t* pair_query; const uint32_t* pair_row; uint32_t n_pairs;   // pair_row 0xffffffff = unknown id
    int metric;
    float* out; uint32_t* status;                                            // ST_NAN / ST_ZERO_QUERY (zero norm on either side)
};
void launch_pair_distances(const PairDistParams& p, hipStream_t s);
// HNSW hooks: zero-norm Cosine pairs are written as the NaN bit pattern `mark` (status is not touched)
struct PairEvalParams {
    const float* rows; uint32_t ld; uint32_t dim; const float* nd;
    const float* qp; const float* qnorm;                 // prepared queries (query side of mode 0 / 2)
    const uint32_t* a; const uint32_t* b; uint32_t n;    // mode 0: (query a[i], row b[i]); mode 1: (row a[i], row b[i]); mode 2: (query q0, row i)
    uint32_t q0; int mode; int metric; uint32_t mark;
    float* out;
};
void launch_pair_eval(const PairEvalParams& p, hipStream_t s);
// HNSW build: exact reference distances of up to 16 STORED rows (the vectors being inserted) against device rows
// [0, n_scan) in ONE pass over the rows -- out[j * ldm + r] = distance(row qrow[j], row r); zero-norm Cosine pairs are
// written as `mark`.  `out` may live in mapped host memory.
struct ScanRowsParams {
    const float* rows; uint32_t ld; uint32_t dim; const float* nd; int metric; uint32_t mark;
    uint32_t nq; uint32_t qrow[16];
    uint32_t n_scan; float* out; size_t ldm;
};
void launch_scan_rows(const ScanRowsParams& p, hipStream_t s);

// ---------------------------------------------------------------- certificate diagnostics (vdb_flat_debug_*)
// dense[q*n_rows + row] = score bits of every key the filter pass wrote for query q (wg-major pools of the bf16 tier)
void launch_pool_to_dense(const uint64_t* pool, const uint32_t* pool_cnt, uint32_t n_sub, uint32_t capl, uint32_t nq,
                          uint32_t n_rows, float* dense, hipStream_t s);
// out[i] = cert_test(p, qi[i], T[i], ek[i]) -- the PRODUCTION certification function of rerank_kernel, probed directly
void launch_cert_probe(const RerankParams& p, const uint32_t* qi, const float* T, const float* ek, uint32_t n, uint32_t* out,
                       hipStream_t s);

// *code = VDB_PENDING_HOST (100) when the status block of a search (flags[0] status bits, flags[1] summary of
// uncertified / overflowed queries) is non-zero, else 0
void launch_write_code(const uint32_t* flags, int32_t* code, hipStream_t s);

// ---------------------------------------------------------------- device-resident HNSW search (kernels_hnsw.hip)
struct HnswSearchParams {
    const float* rows; uint32_t ld; uint32_t dim; const float* nd; int metric;
    const float* qp; const float* qnorm;                 // prepared queries
    // the graph of vdb_hnsw.cpp mirrored in HBM, indexed by node id
    const uint32_t* row_of; uint32_t n_ids;                              // row_of = 0xffffffff: absent / deleted
    // lists are padded with 0xffffffff; *_row holds the device row of each listed neighbour (0xffffffff = deleted)
    const uint32_t* nbr0; const uint32_t* nbr0_row; uint32_t stride0;    // layer 0 lists
    const uint32_t* up_off; const uint32_t* nbrU; const uint32_t* nbrU_row; uint32_t strideU;   // list (id, l >= 1) = up_off[id] + l - 1
    const uint32_t* level; const uint32_t* cnt0; const uint32_t* cntU;   // (unused by the kernel; kept for inspection)
    uint32_t entry_point, max_level, ef, k;
    uint64_t* out_ids; float* out_dists; uint32_t* out_counts;           // [nq][k]
    uint32_t* fail;                                                      // [nq]: 1 = structures overflowed, redo on the host
    uint32_t* status;
    // INSERT WALKS (vdb_hnsw.cpp build): the "query" is a STORED row (qrow[q], its norm nd[qrow[q]]) that the graph does not hold
    // yet, the walk is insert()'s (graph.rs:262-297): ef = 1 above the node's level qlevel[q], ef at and below it, and every
    // distance it evaluates is RECORDED -- rec_row (the evaluated node's ID) / rec_d [q * rec_cap + i], rec_cnt[q] entries (may exceed rec_cap: the rest
    // was dropped) -- for the host's authoritative replay.  All null in a search.  A zero-norm Cosine pair is recorded as
    // rec_zero_mark and ends the walk.
    const uint32_t* qrow; const uint32_t* qlevel;
    uint32_t* rec_row; float* rec_d; uint32_t* rec_cnt; uint32_t rec_cap; uint32_t rec_zero_mark;
    uint32_t chunk, stage_rows;                                          // set by launch_hnsw_search: staging chunk (elements), rows per staging buffer
    // PRE-FILTERED search (id_mask != null; searches only): bit i of id_mask (LSB-first in 64-bit words) marks node id i eligible,
    // ids >= mask_bits (<= n_ids) are not.  Layer 0 then admits every accepted neighbour to the candidate heap but only eligible
    // ones to the results, and its visited set is a bitmap in HBM: vis_bits[q * vis_words ..], n_ids bits per query, zeroed by
    // launch_hnsw_search.
    const uint64_t* id_mask; uint32_t mask_bits;
    uint32_t* vis_bits; uint32_t vis_words;
};
void launch_hnsw_search(const HnswSearchParams& p, uint32_t nq, hipStream_t s);
// queries of one filtered launch: the HBM visited bitmaps of a launch stay within hnsw_filter_vis_bytes()
uint32_t hnsw_filter_launch_queries(uint32_t n_ids);
size_t hnsw_filter_vis_bytes(uint32_t n_ids, uint32_t nq);
// incremental update of the graph mirror: n0 layer-0 records [id, row, level, up_off, ids[stride0], rows[stride0]] and nU
// upper-list records [list index, ids[strideU], rows[strideU]] (uint32 words), scattered into the mirror arrays
struct HnswScatterParams {
    const uint32_t* rec0; uint32_t n0; const uint32_t* recU; uint32_t nU;
    uint32_t* row_of; uint32_t* level; uint32_t* up_off; uint32_t* nbr0; uint32_t* nbr0_row; uint32_t stride0;
    uint32_t* nbrU; uint32_t* nbrU_row; uint32_t strideU;
};
void launch_hnsw_scatter(const HnswScatterParams& p, hipStream_t s);
// a compiled filter mask ANDed with the graph's presence (vdb_hnsw_search_batch_filtered): out[w] for w < ceil(bits / 64), bit i
// set when i < bits (= min(the mask's bits, n_ids), the caller's clamp), bit i of src is set (src holds src_words words) and
// row_of[i] != 0xffffffff; *count += the set bits (a 64-bit word the caller zeroes on the same stream).  bits = 0 launches nothing.
struct HnswPresentMaskParams {
    const uint64_t* src; uint64_t src_words;
    const uint32_t* row_of; uint32_t n_ids;
    uint32_t bits;
    uint64_t* out; unsigned long long* count;
};
void launch_hnsw_present_mask(const HnswPresentMaskParams& p, hipStream_t s);
bool hnsw_search_supported(uint32_t dim, uint32_t ef, uint32_t k, uint32_t max_list);

void launch_merge_packed(const int32_t* packed, size_t words_per_part, uint32_t nparts, uint32_t nq, uint32_t k,
                         uint64_t* out_ids, float* out_dists, uint32_t* out_counts, uint32_t* out_status, hipStream_t s);

// ---------------------------------------------------------------- search by stored id (kernels_by_id.hip)
// out[b * dim .. + dim) = rows[row[b] * ld .. + dim) for b < nq: the stored rows become the dense query block (row[b] < n_rows)
void launch_gather_rows(const float* rows, uint32_t ld, uint32_t dim, uint32_t n_rows, const uint32_t* row, uint32_t nq, float* out,
                        hipStream_t s);
// Query b's result list ids / dists [b * kdev ..], counts[b] entries: the entry whose id equals self_id[b] is removed and the gap
// closed in order (counts[b] - 1 entries remain, stats[0] += 1); when the id is not among them and counts[b] > k, counts[b] = k
// (stats[1] += 1).  Nothing at or past counts[b] is written.
struct StrikeSelfParams {
    uint64_t* ids; float* dists; uint32_t* counts; uint32_t kdev;
    const uint64_t* self_id; uint32_t k;
    uint32_t* stats;                                                       // [2], zeroed by the caller
};
void launch_strike_self(const StrikeSelfParams& p, uint32_t nq, hipStream_t s);

// ---------------------------------------------------------------- one nearest row per group (kernels_distinct.hip)
constexpr uint32_t DISTINCT_MAX_LIST = 1024;                               // entries of one list, and rows of one answer, at most
// List j -- ids / dists [j * stride ..], counts[j] entries, ascending by (distance, id) -- collapsed by the group code of its ids
// (codes[id] when id < codes_len, else -1) into answer row dest[j] (j when dest is null; >= n_answers: nothing is done): entry i is
// kept iff its code is -1 or no earlier entry of the list has it.  The first k kept go to out_* [b * kstride ..] behind the
// kept[b] rows already there (append) or from slot 0; the rest of the row is padded (~0, NaN, -1).  kept[b] = rows in the answer,
// complete[b] = 1 when that is k, or counts[j] < depth, or exhaustive (the depth covered every row of the index).
struct DistinctFirstParams {
    const uint64_t* ids; const float* dists; const uint32_t* counts; uint32_t stride, depth, exhaustive;
    const int32_t* codes; uint64_t codes_len;
    const uint32_t* dest; uint32_t n_answers;
    uint32_t k, kstride, append;
    uint64_t* out_ids; float* out_dists; int32_t* out_codes; uint32_t* kept; uint32_t* complete;
};
void launch_distinct_first(const DistinctFirstParams& p, uint32_t n_lists, hipStream_t s);
// mask[0, ceil(bits / 64)) = src (all ones when null) over [0, bits), minus every id whose code is among the kept[answer] codes
// of answer row `answer` (out_codes), minus every kept id of that row whose code is -1; bits at or beyond `bits` are clear
struct ExcludeGroupsParams {
    const uint64_t* src; uint64_t bits; uint64_t* mask;
    const int32_t* codes; uint64_t codes_len;
    const uint64_t* out_ids; const int32_t* out_codes; const uint32_t* kept; uint32_t kstride, answer;
};
void launch_exclude_groups(const ExcludeGroupsParams& p, uint32_t n_cu, hipStream_t s);

// ---------------------------------------------------------------- up to g rows of each of the k nearest groups (kernels_per_group.hip)
constexpr uint32_t PER_GROUP_MAX_SIZE = 32;                                // members of one group at most (VDB_PER_GROUP_MAX_SIZE)
// One pass over the device rows [0, n_rows).  A row belongs to the list of wanted code wanted[u] (ascending, distinct, >= 0) when
// it is live (live null: every row), its id is admitted by mask (null: every id; else id < mask_bits and the bit set), id <
// codes_len and codes[id] == wanted[u].  COUNT: counts[u] += 1.  SCATTER: the row takes place cursor[u]++ of its list and, when
// that is below lens[u], is written as the candidate key (1 << 32) | row to list[offs[u] + place] (below list_cap); lens[u] = 0
// lists nothing.  counts and cursor are zeroed by the caller.
struct PerGroupListParams {
    const uint64_t* row_ids; const uint32_t* live; uint32_t n_rows;
    const uint64_t* mask; uint64_t mask_bits;
    const int32_t* codes; uint64_t codes_len;
    const int32_t* wanted; uint32_t n_wanted;
    uint32_t* counts;
    const uint32_t* offs; const uint32_t* lens; uint32_t* cursor; uint64_t* list; uint64_t list_cap;
};
void launch_per_group_list(const PerGroupListParams& p, bool scatter, uint32_t n_cu, hipStream_t s);
// Pair (b, j), slot = b * kmax + j, of the answers rep_ids / rep_dists [nq][kmax] with kept[b] groups: out_ids / out_dists
// [slot * g ..] = the representative and padding (~0, NaN), out_sizes[slot] = 1 for j < kept[b]; padding and 0 otherwise.
struct PerGroupInitParams {
    const uint64_t* rep_ids; const float* rep_dists; const uint32_t* kept; uint32_t nq, kmax, g;
    uint64_t* out_ids; float* out_dists; uint32_t* out_sizes;
};
void launch_per_group_init(const PerGroupInitParams& p, hipStream_t s);
// Workgroup i fills pair slot pairs[2 i] (< nq * kmax) from the list of wanted code pairs[2 i + 1] (< n_wanted): the best
// min(g, valid rows) of list[offs[u] .. + lens[u]) for query slot / kmax (q: [nq][dim], the rows' dimension) ascending by
// (distance, id) to out_ids / out_dists [slot * g ..], the rest of the g slots padded, the number to out_sizes[slot].
// status[0] |= ST_NAN for a NaN distance; status[1] += 1 when member 0 is not the representative (id and distance bits).
struct PerGroupFillParams {
    const float* rows; uint32_t ld, dim, n_rows; const float* nd; const uint64_t* row_ids; int metric;
    const float* q; uint32_t nq, kmax, g;
    const uint32_t* pairs; const uint32_t* offs; const uint32_t* lens; uint32_t n_wanted; const uint64_t* list; uint64_t list_cap;
    const uint64_t* rep_ids; const float* rep_dists;
    uint64_t* out_ids; float* out_dists; uint32_t* out_sizes;
    uint32_t* status;                                                      // [2], zeroed by the caller
    uint32_t lds_row_stride, lds_chunk;                                    // set by the launcher
};
void launch_per_group_fill(const PerGroupFillParams& p, uint32_t n_pairs, hipStream_t s);
// mask[0, ceil(bits / 64)) = src (all ones when null) over [0, bits) AND "id < codes_len and codes[id] == code"
struct PerGroupCodeMaskParams {
    const uint64_t* src; uint64_t bits; uint64_t* mask;
    const int32_t* codes; uint64_t codes_len; int32_t code;
};
void launch_per_group_code_mask(const PerGroupCodeMaskParams& p, uint32_t n_cu, hipStream_t s);
// Result list i of a search -- ids / dists [i * stride ..], counts[i] entries -- becomes the members of pair slot dest[i]: the
// first min(counts[i], stride, g), the rest padded; status[1] += 1 when member 0 is not the representative.
struct PerGroupPlaceParams {
    const uint64_t* ids; const float* dists; const uint32_t* counts; uint32_t stride;
    const uint32_t* dest; uint32_t nq, kmax, g;
    const uint64_t* rep_ids; const float* rep_dists;
    uint64_t* out_ids; float* out_dists; uint32_t* out_sizes;
    uint32_t* status;
};
void launch_per_group_place(const PerGroupPlaceParams& p, uint32_t n_lists, hipStream_t s);

// ---------------------------------------------------------------- recommend from stored examples (kernels_recommend.hip)
constexpr uint32_t RECOMMEND_MAX_EXAMPLES = 64;                            // per request, positives + negatives (VDB_RECOMMEND_MAX_EXAMPLES)
// The requests of one call on the device: request b owns entries [offs[b], offs[b + 1]) of rows / ids, the first n_pos[b] of
// them positives, the rest negatives; recip[2 b] = 1.0f / positives, recip[2 b + 1] = 1.0f / negatives (unused when there are none)
struct RecommendLists {
    const uint32_t* offs; const uint32_t* n_pos; const float* recip;
    const uint32_t* rows;                                                  // row numbers in the block the fold reads
    const uint64_t* ids;                                                   // the stored ids of the same entries
};
// out[b * dim .. + dim) = the query of request b (include/vdb_flat.h: left fold in list order, multiply by the reciprocal,
// ap + (ap - an)) from rows[row * ld .. + dim), row < n_rows
void launch_fold_examples(const float* rows, uint32_t ld, uint32_t dim, uint32_t n_rows, const RecommendLists& L, uint32_t nq,
                          float* out, hipStream_t s);
// Request b's result list ids / dists [b * kdev ..], counts[b] entries: every entry whose id is among ex_ids[offs[b], offs[b + 1])
// is removed and the gaps closed in order; counts[b] = min(entries kept, kcut).  stats[0] += the removed entries that stood in
// front of the kcut-th kept one.  Nothing at or past counts[b] (as it was), or at or past kcut, is written.
struct StrikeSetParams {
    uint64_t* ids; float* dists; uint32_t* counts; uint32_t kdev;
    const uint32_t* offs; const uint64_t* ex_ids; uint32_t kcut;
    uint32_t* stats;                                                       // [1], zeroed by the caller
};
void launch_strike_set(const StrikeSetParams& p, uint32_t nq, hipStream_t s);

// ---------------------------------------------------------------- diverse top-k: MMR over the candidates (kernels_mmr.hip)
constexpr uint32_t MMR_MAX_CANDIDATES = 1024;                              // entries of one candidate list (VDB_MMR_MAX_CANDIDATES)
// Query b's candidates: ids / dists / cand_rows [b * stride ..], min(counts[b], stride) entries ascending by (distance, id);
// cand_rows holds the device row of every entry (< n_rows; an entry at or above it ends the query with status bit 1 and count 0).
// The greedy selection of include/vdb_flat.h "DIVERSE TOP-K" with ks[b] picks, lambda[b] and mu[b] writes the picks in pick order to
// out_ids / out_dists / out_scores [b * kout ..] (ks[b] <= kout) and out_counts[b] = min(ks[b], candidates).  A NaN among the
// evaluated pair distances sets status bit 0.  stride <= MMR_MAX_CANDIDATES.
struct MmrParams {
    const float* rows; uint32_t ld, dim, n_rows; int metric;
    const uint64_t* ids; const float* dists; const uint32_t* counts; const uint32_t* cand_rows; uint32_t stride;
    const uint32_t* ks; const float* lambda; const float* mu;
    uint64_t* out_ids; float* out_dists; float* out_scores; uint32_t* out_counts; uint32_t kout;
    uint32_t* status;                                                      // [1], zeroed by the caller
};
void launch_mmr_select(const MmrParams& p, uint32_t nq, hipStream_t s);

// ---------------------------------------------------------------- recommend by best score (kernels_recommend_best.hip)
constexpr uint32_t RB_MAX_ROWS = 1024;                                     // rows one walk of the lists hands to the veto (VDB_RECOMMEND_BEST_MAX_K)
constexpr uint32_t RB_MAX_ENTRIES = 4096;                                  // list entries one walk sorts in LDS
// The requests of one call on the device: request b owns entries [offs[b], offs[b + 1]) of rows / ids (at most
// RECOMMEND_MAX_EXAMPLES), the first n_pos[b] >= 1 of them positives, the rest negatives; ks[b] rows are wanted.  rows: device
// rows below the store's n_rows (the host resolved them).
struct RbRequests {
    const uint32_t* offs; const uint32_t* n_pos; const uint32_t* ks; const uint32_t* rows; const uint64_t* ids;
};
// Workgroup j merges the n_pos lists of request sel[j] (j itself without sel): lists list0[j] .. of ids / dists [list][depth],
// counts[list] entries each, ascending (distance, id).  The candidates -- at most min(cand_stride, RB_MAX_ROWS) rows ascending by
// (ordered dp, id), examples struck -- go to cand_ids / cand_dists [j * cand_stride ..], their number to cand_cnt[j]; open[j] = 1
// when rows may exist behind them (a list came back full, or the walk was cut by either capacity).
struct RbMergeParams {
    RbRequests R; const uint32_t* sel; const uint32_t* list0;
    const uint64_t* ids; const float* dists; const uint32_t* counts; uint32_t depth;
    uint64_t* cand_ids; float* cand_dists; uint32_t* cand_cnt; uint32_t* open; uint32_t cand_stride;
};
void launch_rb_merge(const RbMergeParams& p, uint32_t n_req, hipStream_t s);
// Workgroup j takes the candidates of request sel[j] in order: the kept rule against every negative's stored row, the dn fold, and
// the first min(ks[b], kout) kept rows to out_ids / out_dists / out_neg [b * kout ..], their number to out_counts[b].
// answered[j] (may be null) = 1 when that many were kept or open (may be null) says nothing lies behind the candidates.
// row_ids / rank2row (null: rows are in id order) / live name the live row of an id; status bit 1: a candidate without one.
struct RbVetoParams {
    const float* rows; uint32_t ld, dim, n_rows; int metric; const float* nd;
    const uint64_t* row_ids; const uint32_t* rank2row; const uint32_t* live;
    RbRequests R; const uint32_t* sel;
    const uint64_t* cand_ids; const float* cand_dists; const uint32_t* cand_cnt; const uint32_t* open; uint32_t cand_stride;
    uint64_t* out_ids; float* out_dists; float* out_neg; uint32_t* out_counts; uint32_t kout;
    uint32_t* answered; uint32_t* status;
};
void launch_rb_veto(const RbVetoParams& p, uint32_t n_req, hipStream_t s);
// The exact scan: keys[y * key_stride + row] = (ordered dp, id rank) of every eligible row that request sel[y] keeps, EMPTY_KEY
// for every other row below n_rows; ST_NAN into status for a NaN positive distance at an eligible row.
struct RbScanParams {
    const float* rows; uint32_t ld, dim, n_rows; int metric; const float* nd;
    const uint32_t* rowmask; const uint32_t* idrank;                       // null: every row / ranks are rows
    RbRequests R; const uint32_t* sel;
    uint64_t* keys; size_t key_stride; uint32_t* status;
};
void launch_rb_scan(const RbScanParams& p, uint32_t n_req, hipStream_t s);

// ---------------------------------------------------------------- discovery search (kernels_discover.hip)
constexpr uint32_t DISCOVER_MAX_PAIRS = 16;                                // (positive, negative) pairs of one request (VDB_DISCOVER_MAX_PAIRS)
constexpr uint32_t DISCOVER_MAX_LIST = 1024;                               // candidates of one list stage, and rows of one answer (VDB_DISCOVER_MAX_K)
// the scan's key: (P - rank) above the ordered d(t, x) above the id rank -- 5 + 32 + 27 bits
constexpr uint32_t DISCOVER_KEY_ID_BITS = 27, DISCOVER_KEY_LEVEL_SHIFT = 59;
// The requests of one call on the device: request b owns entries [offs[b], offs[b + 1]) of rows / ids -- the target, then
// p_1 n_1 p_2 n_2 ..., 2P + 1 entries with P <= DISCOVER_MAX_PAIRS; ks[b] rows are wanted.  rows: device rows below the store's
// n_rows (the host resolved them).
struct DiscoverRequests {
    const uint32_t* offs; const uint32_t* ks; const uint32_t* rows; const uint64_t* ids;
};
// Workgroup j takes the candidates of request sel[j] (j itself without sel): cand_ids / cand_dists [j * cand_stride ..], cand_cnt[j]
// of them (at most DISCOVER_MAX_LIST), ascending by (d(t, x), id), the examples struck.  raw_cnt[j] is what the search at `depth`
// returned before the strike: the list is complete when that is below depth, or when exhaustive says the depth covered every row.
// answered[j] = 1 when ks[b] candidates have rank P or the list is complete; only then the first min(ks[b], kout) candidates by
// (rank descending, list order) go to out_ids / out_dists / out_ranks [b * kout ..] and their number to out_counts[b].
// row_ids / rank2row (null: rows are in id order) / live name the live row of an id; status bit 1: a candidate without one.
struct DiscoverRankParams {
    const float* rows; uint32_t ld, dim, n_rows; int metric; const float* nd;
    const uint64_t* row_ids; const uint32_t* rank2row; const uint32_t* live;
    DiscoverRequests R; const uint32_t* sel;
    const uint64_t* cand_ids; const float* cand_dists; const uint32_t* cand_cnt; const uint32_t* raw_cnt; uint32_t cand_stride, depth, exhaustive;
    uint64_t* out_ids; float* out_dists; uint32_t* out_ranks; uint32_t* out_counts; uint32_t kout;
    uint32_t* answered; uint32_t* status;
};
void launch_discover_rank(const DiscoverRankParams& p, uint32_t n_req, hipStream_t s);
// The exact scan: keys[y * key_stride + row] = ((P - rank) << 59 | ordered d(t, row) << 27 | id rank) of every eligible row of
// request sel[y] that is none of its examples, EMPTY_KEY for every other row below n_rows (n_rows < 2^27); ST_NAN into status for
// a NaN d(t, row) at an eligible row, the examples included.
struct DiscoverScanParams {
    const float* rows; uint32_t ld, dim, n_rows; int metric; const float* nd;
    const uint32_t* rowmask; const uint32_t* idrank;                       // null: every row / ranks are rows
    DiscoverRequests R; const uint32_t* sel;
    uint64_t* keys; size_t key_stride; uint32_t* status;
};
void launch_discover_scan(const DiscoverScanParams& p, uint32_t n_req, hipStream_t s);
// The first min(key_cnt[y], ks[b], kout) of the ascending keys [y * key_stride ..] of request b = sel[y], taken apart into
// out_ids / out_dists / out_ranks [b * kout ..]; their number to out_counts[b].  status bit 1: a key that names no row.
struct DiscoverEmitParams {
    const uint64_t* keys; const uint32_t* key_cnt; uint32_t key_stride;
    DiscoverRequests R; const uint32_t* sel;
    const uint32_t* rank2row; const uint64_t* row_ids; uint32_t n_rows;
    uint64_t* out_ids; float* out_dists; uint32_t* out_ranks; uint32_t* out_counts; uint32_t kout;
    uint32_t* status;
};
void launch_discover_emit(const DiscoverEmitParams& p, uint32_t n_req, hipStream_t s);

}  // namespace vdb
