// kernels_compact.hip -- the row mover of vdb_flat_compact (vdb_store.cpp compact_store): a STABLE stream compaction of the
// device row store and its per-row columns, in place.  gfx950 (MI355X) only.
//
// One launch moves the live rows of ONE chunk [row_begin, row_end) of source rows (the host plans the chunks so that no
// launch writes a row that it, or a later launch, still has to read -- vdb_store.cpp compact_plan):
//   row r -> dest(r) - dst_sub,  dest(r) = prefix[r >> 5] + popc(live[r >> 5] & ((1 << (r & 31)) - 1))
// with everything that belongs to the row: the f32 row (ld * 4 bytes, 128-byte aligned), the bf16 shadow row when the index
// keeps one (ld * 2 bytes, 64-byte aligned), nd / alpha / beta / margin (4 bytes each) and the id (8 bytes).  Values are
// moved bit for bit; nothing is recomputed.  Dead rows are never read.  live == null is the IDENTITY form (every row moves
// to r - dst_sub): the contiguous copy out of the bounce buffer.
//
// Shape: 256-thread workgroups, n_cu * 8 of them at most, waves striding over groups of 64 / G consecutive source rows, G
// lanes per row (G = 8 .. 64, the power of two covering the row's 16-byte vectors).  Each lane keeps up to four 16-byte
// loads in flight before their stores: with 32 waves per CU that is ~128 KiB in flight per CU, more than the ~72 KiB an
// HBM-bound stream needs.  Plain loads and stores: a bounced chunk is read again at once and is meant to stay in the cache.
#include <algorithm>

#include "kernels.h"

namespace vdb {

namespace {

__device__ __forceinline__ void move_vectors(const uint4* __restrict__ src, uint4* __restrict__ dst, uint32_t nvec, uint32_t sub, uint32_t G) {
    for (uint32_t j = sub; j < nvec; j += 4 * G) {
        const bool p1 = j + G < nvec, p2 = j + 2 * G < nvec, p3 = j + 3 * G < nvec;
        uint4 v0 = src[j], v1 = v0, v2 = v0, v3 = v0;
        if (p1) v1 = src[j + G];
        if (p2) v2 = src[j + 2 * G];
        if (p3) v3 = src[j + 3 * G];
        dst[j] = v0;
        if (p1) dst[j + G] = v1;
        if (p2) dst[j + 2 * G] = v2;
        if (p3) dst[j + 3 * G] = v3;
    }
}

__global__ __launch_bounds__(256) void compact_move_kernel(const CompactMoveParams p) {
    const uint32_t G = 1u << p.lanes_log2, rows_per_wave = 64u >> p.lanes_log2;
    const uint32_t lane = threadIdx.x & 63u, sub = lane & (G - 1u), slot = lane >> p.lanes_log2;
    const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = gridDim.x * (blockDim.x >> 6);
    const uint32_t nvec = p.ld >> 2, nvec16 = p.ld >> 3;                  // 16-byte vectors of an f32 row / a bf16 row
    const uint32_t n = p.row_end - p.row_begin;
    const uint32_t n_groups = (n + rows_per_wave - 1) / rows_per_wave;
    for (uint32_t g = wave; g < n_groups; g += n_waves) {
        const uint32_t off = g * rows_per_wave + slot;
        if (off >= n) continue;
        const uint32_t r = p.row_begin + off;
        uint32_t d = r;
        if (p.live) {
            const uint32_t w = p.live[r >> 5], bit = r & 31u;
            if (!((w >> bit) & 1u)) continue;                             // dead: never read
            d = p.prefix[r >> 5] + __popc(w & ((1u << bit) - 1u));
        }
        d -= p.dst_sub;
        if (p.src_rows == p.dst_rows && d == r) continue;                 // in place and nothing dead below: the row stays
        move_vectors(reinterpret_cast<const uint4*>(p.src_rows + (size_t)r * p.ld), reinterpret_cast<uint4*>(p.dst_rows + (size_t)d * p.ld), nvec, sub, G);
        if (p.src_rows16)
            move_vectors(reinterpret_cast<const uint4*>(p.src_rows16 + (size_t)r * p.ld), reinterpret_cast<uint4*>(p.dst_rows16 + (size_t)d * p.ld), nvec16, sub, G);
        if (sub == 0) {
            const float a = p.src_nd[r], b = p.src_alpha[r], c = p.src_beta[r];
            const uint64_t id = p.src_ids[r];
            p.dst_nd[d] = a; p.dst_alpha[d] = b; p.dst_beta[d] = c; p.dst_ids[d] = id;
            if (p.src_margin) p.dst_margin[d] = p.src_margin[r];
        }
    }
}

}  // namespace

void launch_compact_move(const CompactMoveParams& p, uint32_t n_cu, hipStream_t s) {
    if (p.row_end <= p.row_begin) return;
    const uint32_t rows_per_wg = 4u * (64u >> p.lanes_log2);
    const uint32_t want = (p.row_end - p.row_begin + rows_per_wg - 1) / rows_per_wg;
    const uint32_t grid = std::max(1u, std::min(want, n_cu * 8u));
    hipLaunchKernelGGL(compact_move_kernel, dim3(grid), dim3(256), 0, s, p);
}

}  // namespace vdb
