// kernels_bin.h -- parameter blocks and launchers of the binary flat index (kernels_bin.hip, vdb_bin.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

namespace vdb {

enum BinMetric : int { BIN_HAMMING = 0, BIN_JACCARD = 1 };

constexpr uint32_t BIN_MAX_DIM = 32768;             // bits
constexpr uint32_t BIN_MAX_K = 1024;
constexpr uint32_t BIN_LD_ALIGN = 64;               // a packed row is a whole number of 64-byte (512-bit) chunks, zero-padded
constexpr uint32_t BIN_THREADS = 512;               // 8 waves; a wave scores 32 rows against the whole query tile
constexpr uint32_t BIN_ROUND_ROWS = BIN_THREADS / 64 * 32;   // rows of one round of a workgroup: 256
constexpr uint32_t BIN_SEG_ROWS = 4096;             // R: consecutive rows of one workgroup (a multiple of BIN_ROUND_ROWS)
constexpr uint32_t BIN_QT = 64, BIN_QT_LARGE_K = 16;   // queries of one workgroup; the small tile where k is above BIN_QT_MAX_K
constexpr uint32_t BIN_QT_MAX_K = 128;
constexpr size_t BIN_LDS_BUDGET = 156 * 1024;       // bytes of LDS a score workgroup plans with: the select buffers, then the query image
constexpr uint32_t BIN_OPEN = 0xffffffffu;          // a shared threshold nobody has proven yet

// keys one query's select buffer holds for a request of k: room for late offers above k
__host__ __device__ inline uint32_t bin_select_cap(uint32_t k) { return k + (k < 32 ? 32 : k > 64 ? 64 : k); }
inline uint32_t bin_query_tile(uint32_t kmax) { return kmax <= BIN_QT_MAX_K ? BIN_QT : BIN_QT_LARGE_K; }

// nx[row] = the set bits of the row's ld packed bytes, rows [row_begin, row_end)
void launch_bin_row_popcounts(const uint8_t* rows, uint32_t ld, uint32_t row_begin, uint32_t row_end, int32_t* nx, hipStream_t s);
void launch_bin_fill(uint32_t* words, size_t n, uint32_t value, hipStream_t s);
// qw[b][8 ld]: query b's ld packed bytes widened to one 0/1 byte per bit, in the K order in which the score kernel widens a row
void launch_bin_widen(const uint8_t* q, uint32_t ld, size_t nq, uint8_t* qw, hipStream_t s);

// One workgroup per (segment, tile of qt queries of a launch): query y of the launch is query q0 + y of the batch.
struct BinSearchParams {
    const uint8_t* rows; uint32_t ld, n_rows; const int32_t* nx;      // [n_rows][ld] packed, ld a multiple of 64; the padding is zero
    const uint32_t* live; const uint64_t* row_ids; const uint32_t* rank;   // by row; rank = position of the row's id among the live ids
    const uint64_t* sorted_ids;                                       // by rank
    const uint8_t* qw; const int32_t* nq; const uint32_t* ks;         // the batch: [nq_batch][8 ld] widened, the popcounts, k of every query
    uint32_t q0, n_q;                                                 // the launch's queries: [q0, q0 + n_q)
    int metric;
    const uint64_t* id_mask; uint64_t mask_bits;                      // may be null
    uint32_t seg_rows, segs, qt, cap;                                 // segs = ceil(n_rows / seg_rows); cap = bin_select_cap(largest k)
    uint32_t kc;                                                      // widened bytes of every query the LDS image holds at a time, a multiple of 512
    uint32_t* gthr;                                                   // [n_q] the f32 bits of the best proven k-th distance, BIN_OPEN at launch
    uint64_t* part; uint32_t* part_cnt;                               // part[(y * segs + segment) * kout + i], i < part_cnt[y * segs + segment]
    uint64_t* out_ids; float* out_dists; uint32_t* out_counts; uint32_t kout;   // [nq_batch][kout]
    unsigned long long* counters;                                     // [0] += keys the workgroups wrote to part
};
void launch_bin_score(const BinSearchParams& p, hipStream_t s);
void launch_bin_merge(const BinSearchParams& p, hipStream_t s);

}  // namespace vdb
