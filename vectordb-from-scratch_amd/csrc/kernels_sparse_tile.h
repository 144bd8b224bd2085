// kernels_sparse_tile.h -- what the eligible-row scans share (kernels_sparse.hip: one list for the whole batch;
// kernels_grouped.hip: one list per filter group): the mask-word and block-sum helpers of the list kernels, the
// geometry of the scan's 64 x 64 tile and its LDS budget.  The tile itself is kernels_sparse_tile_body.h.
// gfx950 only.  Include from a translation unit built with -ffp-contract=off.
#pragma once
#include "kernels.h"

namespace vdb {

constexpr uint32_t SPL_THREADS = 256;                              // mask words per workgroup of the count / scatter kernels

// word w of the row mask with the bits at or above n_rows cleared (they must never produce a row)
__device__ __forceinline__ uint32_t sparse_mask_word(const uint32_t* __restrict__ rowmask, uint32_t w, uint32_t n_words, uint32_t n_rows) {
    if (w >= n_words) return 0u;
    uint32_t x = rowmask[w];
    const uint32_t base = w << 5;                                  // (n_rows > base for every w < n_words)
    if (n_rows - base < 32u) x &= (1u << (n_rows - base)) - 1u;
    return x;
}

// sum over the workgroup (256 threads); every thread gets the total.  sRed: 4 words of LDS.
__device__ __forceinline__ uint32_t sparse_block_sum(uint32_t v, uint32_t* sRed) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = v;
    __syncthreads();
    return sRed[0] + sRed[1] + sRed[2] + sRed[3];
}

// ---------------------------------------------------------------------------------------------
// The scan.  256 threads = 4 waves.  Wave w owns queries 16w .. 16w+15 of the tile (a wave none of whose queries exists skips
// the arithmetic -- a batch of one query costs one wave per workgroup, not four); inside a wave lane & 3 picks 4 consecutive
// queries and lane >> 2 the rows tr, tr+16, tr+32, tr+48.
// LDS: two images of (64 rows + 64 queries) x 36 floats = 36 KB.  Pitch 36 floats: 16-byte aligned for ds_read_b128,
// and the 16 row addresses of a wave's read (tr * 36 floats) fall into 16 different groups of four banks, the 4 query addresses
// (144 floats apart) into 4 more: no bank conflicts.  After the fold the same memory carries the tile's keys to coalesced
// stores (64 x 64 x 8 B = 32 KB).
// ---------------------------------------------------------------------------------------------
constexpr uint32_t SP_TR = SPARSE_TILE_R, SP_TQ = SPARSE_TILE_Q, SP_LD = 36;
constexpr uint32_t SP_IMG = (SP_TR + SP_TQ) * SP_LD;               // floats per LDS image
static_assert(SP_TR == 64 && SP_TQ == 64 && KSTAGE == 32, "the thread layout below is written for 64 x 64 x 32");
static_assert(2 * SP_IMG * 4 >= SP_TR * SP_TQ * 8 && 2 * SP_IMG * 4 <= 65536, "LDS: keys fit the staging images, two workgroups per CU");

__device__ __attribute__((aligned(16))) const float sparse_zero_chunk[KSTAGE] = {0.0f};   // what a masked row or query stages

}  // namespace vdb
