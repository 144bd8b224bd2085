// kernels_sparse.hip -- the sparse-filter route of the flat index (vdb_flat_set_sparse_filter): under a
// selective id mask only the ELIGIBLE rows are read.
//   1. eligible-row list: the set bits of the search's row mask (live rows AND the id mask) as an ascending list of device rows.
//      Three plain launches -- per-block popcount, a one-workgroup exclusive scan of the block counts, scatter.  No workgroup
//      ever waits for another one: the order between the phases is the order of the launches on the stream.
//   2. the scan: the exact reference distance of every (query, eligible row) pair, a tile of SPARSE_TILE_R rows x SPARSE_TILE_Q
//      queries per workgroup, both staged through LDS in K chunks of KSTAGE floats (double buffered), 4 x 4 pairs per thread.
//      Every pair is ONE sequential left fold over the dimension in the reference's operation order (distance.rs:37-73) -- the
//      16 chains of a thread are independent of each other (that is the ILP), the chain of one pair is never split.
// Every index read from elig[] is compared with n_rows before it becomes an address; rows and queries past the end of the list
// or the batch are masked (they read nothing and write EMPTY_KEY or nothing), never clamped onto a neighbour.
// gfx950 only.  Built with -ffp-contract=off.
#include "kernels_sparse_tile.h"

#pragma clang fp contract(off)

namespace vdb {

// ---------------------------------------------------------------------------------------------
// Eligible-row list
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SPL_THREADS) void sparse_count_kernel(const uint32_t* __restrict__ rowmask, uint32_t n_rows, uint32_t n_words,
                                                                   uint32_t* __restrict__ block_cnt) {
    __shared__ uint32_t sRed[4];
    const uint32_t w = blockIdx.x * SPL_THREADS + threadIdx.x;
    const uint32_t c = __popc(sparse_mask_word(rowmask, w, n_words, n_rows));
    const uint32_t total = sparse_block_sum(c, sRed);
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = total;
}

// ONE workgroup: block_off[b] = sum of block_cnt[0..b), *total = E.  Walks the counts 256 at a time with a running carry.
__global__ __launch_bounds__(SPL_THREADS) void sparse_scan_kernel(const uint32_t* __restrict__ block_cnt, uint32_t n_blocks,
                                                                  uint32_t* __restrict__ block_off, uint32_t* __restrict__ total) {
    __shared__ uint32_t sWave[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += SPL_THREADS) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t c = b < n_blocks ? block_cnt[b] : 0u;
        uint32_t incl = c;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if ((int)lane >= o) incl += t; }
        if (lane == 63) sWave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t v = 0; v < 4; ++v) { const uint32_t t = sWave[v]; if (v < wave) before += t; all += t; }
        if (b < n_blocks) block_off[b] = carry + before + incl - c;
        carry += all;
        __syncthreads();                                           // sWave is rewritten by the next round
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(SPL_THREADS) void sparse_scatter_kernel(const uint32_t* __restrict__ rowmask, uint32_t n_rows, uint32_t n_words,
                                                                     const uint32_t* __restrict__ block_off, uint32_t* __restrict__ elig,
                                                                     uint32_t cap) {
    __shared__ uint32_t sWave[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t w = blockIdx.x * SPL_THREADS + threadIdx.x;
    uint32_t x = sparse_mask_word(rowmask, w, n_words, n_rows);
    const uint32_t c = __popc(x);
    uint32_t incl = c;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if ((int)lane >= o) incl += t; }
    if (lane == 63) sWave[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (uint32_t v = 0; v < 4; ++v) if (v < wave) before += sWave[v];
    uint32_t pos = block_off[blockIdx.x] + before + incl - c;
    for (; x; x &= x - 1u, ++pos)
        if (pos < cap) elig[pos] = (w << 5) + (uint32_t)__builtin_ctz(x);   // (pos < E <= cap by construction; checked all the same)
}

uint32_t sparse_list_blocks(uint32_t n_rows) { return (((n_rows + 31u) >> 5) + SPL_THREADS - 1) / SPL_THREADS; }
void launch_sparse_count(const uint32_t* rowmask, uint32_t n_rows, uint32_t* block_cnt, uint32_t* block_off, uint32_t* total, hipStream_t s) {
    const uint32_t n_words = (n_rows + 31u) >> 5, n_blocks = sparse_list_blocks(n_rows);
    if (n_blocks) hipLaunchKernelGGL(sparse_count_kernel, dim3(n_blocks), dim3(SPL_THREADS), 0, s, rowmask, n_rows, n_words, block_cnt);
    hipLaunchKernelGGL(sparse_scan_kernel, dim3(1), dim3(SPL_THREADS), 0, s, block_cnt, n_blocks, block_off, total);
}
void launch_sparse_scatter(const uint32_t* rowmask, uint32_t n_rows, const uint32_t* block_off, uint32_t* elig, uint32_t cap, hipStream_t s) {
    const uint32_t n_words = (n_rows + 31u) >> 5, n_blocks = sparse_list_blocks(n_rows);
    if (!n_blocks || !cap) return;
    hipLaunchKernelGGL(sparse_scatter_kernel, dim3(n_blocks), dim3(SPL_THREADS), 0, s, rowmask, n_rows, n_words, block_off, elig, cap);
}

// ---------------------------------------------------------------------------------------------
// The scan: one tile (kernels_sparse_tile.h, kernels_sparse_tile_body.h) per workgroup, blockIdx.x over the list, blockIdx.y
// over the queries of the pass.
// ---------------------------------------------------------------------------------------------
template <bool EUC>
__global__ __launch_bounds__(256) void sparse_scan_kernel_t(SparseScanParams p) {
#define SPARSE_TILE_J0 (blockIdx.x * SP_TR)
#define SPARSE_TILE_Q0 (blockIdx.y * SP_TQ)
#include "kernels_sparse_tile_body.h"
#undef SPARSE_TILE_J0
#undef SPARSE_TILE_Q0
}

void launch_sparse_scan(const SparseScanParams& p, hipStream_t s) {
    if (!p.n_elig || !p.nq) return;
    const dim3 grid((p.n_elig + SP_TR - 1) / SP_TR, (p.nq + SP_TQ - 1) / SP_TQ);
    if (p.metric == EUCLID) hipLaunchKernelGGL(sparse_scan_kernel_t<true>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(sparse_scan_kernel_t<false>, grid, dim3(256), 0, s, p);
}

}  // namespace vdb
