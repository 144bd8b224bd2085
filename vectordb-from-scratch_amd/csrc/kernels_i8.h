// kernels_i8.h -- parameter blocks and launchers of the int8 flat index (kernels_i8.hip, vdb_i8.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

namespace vdb {

constexpr uint32_t I8_MAX_DIM = 16384;
constexpr uint32_t I8_MAX_K = 1024;
constexpr uint32_t I8_LD_ALIGN = 64;                // a row is a whole number of 64-byte K steps, zero-padded
constexpr uint32_t I8_THREADS = 512;                // 8 waves; a wave scores 32 rows against the whole query tile
constexpr uint32_t I8_ROUND_ROWS = I8_THREADS / 64 * 32;   // rows of one round of a workgroup: 256
constexpr uint32_t I8_SEG_ROWS = 4096;              // R: consecutive rows of one workgroup (a multiple of I8_ROUND_ROWS)
constexpr uint32_t I8_QT = 64, I8_QT_LARGE_K = 16;  // queries of one workgroup; the small tile where k is above I8_QT_MAX_K
constexpr uint32_t I8_QT_MAX_K = 128;
constexpr size_t I8_LDS_BUDGET = 144 * 1024;        // bytes of LDS a score workgroup plans with: the select buffers, then the query image

// keys one query's select buffer holds for a request of k: room for a round of late offers above k, never as many as the
// 4096 of the sparse select -- QT queries share one LDS
__host__ __device__ inline uint32_t i8_select_cap(uint32_t k) { return k + (k < 32 ? 32 : k > 64 ? 64 : k); }
inline uint32_t i8_query_tile(uint32_t kmax) { return kmax <= I8_QT_MAX_K ? I8_QT : I8_QT_LARGE_K; }

// nx[row] = the sum of the squares of the row's ld bytes, rows [row_begin, row_end)
void launch_i8_row_norms(const int8_t* rows, uint32_t ld, uint32_t row_begin, uint32_t row_end, int32_t* nx, hipStream_t s);
// *count += the live rows below n_rows whose nx is 0 (the caller zeroes it: launch_i8_fill)
void launch_i8_zero_rows(const int32_t* nx, const uint32_t* live, uint32_t n_rows, uint32_t* count, hipStream_t s);
void launch_i8_fill(uint32_t* words, size_t n, uint32_t value, hipStream_t s);

// One workgroup per (segment, tile of qt queries of a launch): query y of the launch is query q0 + y of the batch.
struct I8SearchParams {
    const int8_t* rows; uint32_t ld, n_rows; const int32_t* nx;       // [n_rows][ld], ld a multiple of 64; the padding is zero
    const uint32_t* live; const uint64_t* row_ids; const uint32_t* rank;   // by row; rank = position of the row's id among the live ids
    const uint64_t* sorted_ids;                                       // by rank
    const int8_t* q; const int32_t* nq; const uint32_t* ks;           // the batch: [nq_batch][ld] zero-padded, the norms, k of every query
    uint32_t q0, n_q;                                                 // the launch's queries: [q0, q0 + n_q)
    int metric;
    const uint64_t* id_mask; uint64_t mask_bits;                      // may be null
    uint32_t seg_rows, segs, qt, cap;                                 // segs = ceil(n_rows / seg_rows); cap = i8_select_cap(largest k)
    uint32_t kc;                                                      // bytes of every query the LDS image holds at a time (launch_i8_score fills it)
    uint64_t* part; uint32_t* part_cnt;                               // part[(y * segs + segment) * kout + i], i < part_cnt[y * segs + segment]
    uint64_t* out_ids; float* out_dists; uint32_t* out_counts; uint32_t kout;   // [nq_batch][kout]
    unsigned long long* counters;                                     // [0] += keys the workgroups wrote to part
};
void launch_i8_score(const I8SearchParams& p, hipStream_t s);
void launch_i8_merge(const I8SearchParams& p, hipStream_t s);

}  // namespace vdb
