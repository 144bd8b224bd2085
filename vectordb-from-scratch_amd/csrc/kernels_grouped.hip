// kernels_grouped.hip -- the grouped route of the flat index (vdb_flat_search_batch_grouped): one batch, a
// filter per query.  The queries that share a filter form a GROUP; every group gets the eligible-row scan of the sparse-filter
// route (kernels_sparse.hip), and all groups get it in ONE launch chain:
//   1. grouped_rowmask_kernel: rowmask[g][w] = live AND mask_g[row_ids] for every group; a row's id and live bit are loaded once
//      and tested against all masks.
//   2. grouped_count_kernel / grouped_offsets_kernel: per-group popcounts per block of 256 mask words, their exclusive scan and
//      the totals E_g -- which the host reads in one copy.
//   3. grouped_scatter_kernel: all groups' ascending eligible-row lists side by side, group g at its list offset.
//   4. grouped_scan_kernel_t: the tile of the sparse scan (kernels_sparse_tile_body.h, the SAME statements) over a tile table the
//      host planned: every tile is 64 list positions x up to 64 queries of ONE group.
// Nothing read from device memory becomes an address before it passed its bound: a tile entry that does not fit the pass is
// skipped, a group or list range out of bounds leaves the tile an empty list (zero chunks staged, EMPTY_KEY written), a row
// at or above n_rows is masked by the tile itself.
// gfx950 only.  Built with -ffp-contract=off.
#include "kernels_sparse_tile.h"

#pragma clang fp contract(off)

namespace vdb {

// ---------------------------------------------------------------------------------------------
// Row masks of all groups.  256 threads = 256 rows = 8 mask words; the grid runs over the row words.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void grouped_rowmask_kernel(const uint64_t* __restrict__ row_ids, const uint32_t* __restrict__ livemask,
                                                              const GroupedMask* __restrict__ masks, uint32_t n_groups, uint32_t n_rows,
                                                              uint32_t n_words, uint32_t* __restrict__ out) {
    const uint32_t row = blockIdx.x * 256 + threadIdx.x;
    bool live = false;
    uint64_t id = 0;
    if (row < n_rows) {                                            // loaded ONCE, whatever the number of groups
        live = livemask ? ((livemask[row >> 5] >> (row & 31)) & 1u) : true;
        id = row_ids[row];
    }
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t w0 = (blockIdx.x * 256 + (threadIdx.x & ~63u)) >> 5;
    for (uint32_t g = 0; g < n_groups; ++g) {
        const GroupedMask m = masks[g];                            // (workgroup-uniform)
        const bool ok = live && id < m.bits && ((m.words[id >> 6] >> (id & 63)) & 1ull);
        const unsigned long long b = __ballot(ok);                 // rows at or above n_rows: bit clear
        uint32_t* o = out + (size_t)g * n_words;
        if (lane == 0 && w0 < n_words) o[w0] = (uint32_t)b;
        if (lane == 1 && w0 + 1 < n_words) o[w0 + 1] = (uint32_t)(b >> 32);
    }
}

// ---------------------------------------------------------------------------------------------
// Counts and lists: the three list kernels of the sparse route with the group in blockIdx.y.  block_cnt / block_off:
// [n_groups][n_blocks]; total: [n_groups].
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SPL_THREADS) void grouped_count_kernel(const uint32_t* __restrict__ rowmask, uint32_t n_rows, uint32_t n_words,
                                                                    uint32_t n_blocks, uint32_t* __restrict__ block_cnt) {
    __shared__ uint32_t sRed[4];
    const uint32_t g = blockIdx.y;
    const uint32_t w = blockIdx.x * SPL_THREADS + threadIdx.x;
    const uint32_t c = __popc(sparse_mask_word(rowmask + (size_t)g * n_words, w, n_words, n_rows));
    const uint32_t total = sparse_block_sum(c, sRed);
    if (threadIdx.x == 0) block_cnt[(size_t)g * n_blocks + blockIdx.x] = total;
}

// one workgroup per group: block_off[g][b] = sum of block_cnt[g][0..b), total[g] = E_g
__global__ __launch_bounds__(SPL_THREADS) void grouped_offsets_kernel(const uint32_t* __restrict__ block_cnt, uint32_t n_blocks,
                                                                      uint32_t* __restrict__ block_off, uint32_t* __restrict__ total) {
    __shared__ uint32_t sWave[4];
    const uint32_t g = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t* cnt = block_cnt + (size_t)g * n_blocks;
    uint32_t* off = block_off + (size_t)g * n_blocks;
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += SPL_THREADS) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t c = b < n_blocks ? cnt[b] : 0u;
        uint32_t incl = c;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if ((int)lane >= o) incl += t; }
        if (lane == 63) sWave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t v = 0; v < 4; ++v) { const uint32_t t = sWave[v]; if (v < wave) before += t; all += t; }
        if (b < n_blocks) off[b] = carry + before + incl - c;
        carry += all;
        __syncthreads();                                           // sWave is rewritten by the next round
    }
    if (threadIdx.x == 0) total[g] = carry;
}

// glist[g] = {list offset, list length}: a group that is not scanned has length 0 and writes nothing
__global__ __launch_bounds__(SPL_THREADS) void grouped_scatter_kernel(const uint32_t* __restrict__ rowmask, uint32_t n_rows, uint32_t n_words,
                                                                      uint32_t n_blocks, const uint32_t* __restrict__ block_off,
                                                                      const uint32_t* __restrict__ glist, uint32_t* __restrict__ lists,
                                                                      uint32_t lists_cap) {
    __shared__ uint32_t sWave[4];
    const uint32_t g = blockIdx.y;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t w = blockIdx.x * SPL_THREADS + threadIdx.x;
    const uint32_t off = glist[2 * g], len = glist[2 * g + 1];
    const bool fits = off <= lists_cap && len <= lists_cap - off;  // (by construction; checked all the same)
    uint32_t x = fits && len ? sparse_mask_word(rowmask + (size_t)g * n_words, w, n_words, n_rows) : 0u;
    const uint32_t c = __popc(x);
    uint32_t incl = c;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if ((int)lane >= o) incl += t; }
    if (lane == 63) sWave[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (uint32_t v = 0; v < 4; ++v) if (v < wave) before += sWave[v];
    uint32_t pos = block_off[(size_t)g * n_blocks + blockIdx.x] + before + incl - c;
    for (; x; x &= x - 1u, ++pos)
        if (pos < len) lists[off + pos] = (w << 5) + (uint32_t)__builtin_ctz(x);
}

void launch_grouped_rowmasks(const uint64_t* row_ids, const uint32_t* livemask, const GroupedMask* masks, uint32_t n_groups, uint32_t n_rows,
                             uint32_t* rowmasks, hipStream_t s) {
    if (!n_rows || !n_groups) return;
    hipLaunchKernelGGL(grouped_rowmask_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, s, row_ids, livemask, masks, n_groups, n_rows,
                       (n_rows + 31u) >> 5, rowmasks);
}
void launch_grouped_count(const uint32_t* rowmasks, uint32_t n_groups, uint32_t n_rows, uint32_t* block_cnt, uint32_t* block_off,
                          uint32_t* totals, hipStream_t s) {
    const uint32_t n_words = (n_rows + 31u) >> 5, n_blocks = sparse_list_blocks(n_rows);
    if (!n_groups) return;
    if (n_blocks) hipLaunchKernelGGL(grouped_count_kernel, dim3(n_blocks, n_groups), dim3(SPL_THREADS), 0, s, rowmasks, n_rows, n_words, n_blocks, block_cnt);
    hipLaunchKernelGGL(grouped_offsets_kernel, dim3(n_groups), dim3(SPL_THREADS), 0, s, block_cnt, n_blocks, block_off, totals);
}
void launch_grouped_scatter(const uint32_t* rowmasks, uint32_t n_groups, uint32_t n_rows, const uint32_t* block_off, const uint32_t* glist,
                            uint32_t* lists, uint32_t lists_cap, hipStream_t s) {
    const uint32_t n_words = (n_rows + 31u) >> 5, n_blocks = sparse_list_blocks(n_rows);
    if (!n_blocks || !n_groups || !lists_cap) return;
    hipLaunchKernelGGL(grouped_scatter_kernel, dim3(n_blocks, n_groups), dim3(SPL_THREADS), 0, s, rowmasks, n_rows, n_words, n_blocks, block_off,
                       glist, lists, lists_cap);
}

// ---------------------------------------------------------------------------------------------
// The scan.  One workgroup per entry of the tile table; the tile itself is the sparse scan's.
// ---------------------------------------------------------------------------------------------
template <bool EUC>
__global__ __launch_bounds__(256) void grouped_scan_kernel_t(GroupedScanParams gp) {
    const uint32_t* tile = gp.tiles + 4 * (size_t)blockIdx.x;
    const uint32_t t_group = tile[0], t_j0 = tile[1], t_q = tile[2], t_n = tile[3];
    // the tile's queries must lie inside the pass and its list positions inside the key rows: a tile that does not is skipped
    // (workgroup-uniform; nothing was addressed with its fields)
    if (t_q < gp.q_base) return;
    const uint32_t t_q0 = t_q - gp.q_base;
    if (t_q0 >= gp.scan.nq || t_n == 0 || t_n > SP_TQ || t_n > gp.scan.nq - t_q0) return;
    if (t_j0 % SP_TR || t_j0 >= gp.scan.key_stride) return;
    // the tile's view of the scan: its group's list, and no query beyond its own.  A group or a list range out of bounds leaves
    // an empty list -- every row of the tile masked
    SparseScanParams p = gp.scan;
    p.nq = t_q0 + t_n;
    p.n_elig = 0;
    if (t_group < gp.n_groups) {
        const uint32_t off = gp.glist[2 * t_group], len = gp.glist[2 * t_group + 1];
        if (off <= gp.scan.n_elig && len <= gp.scan.n_elig - off) { p.elig = gp.scan.elig + off; p.n_elig = len; }
    }
#define SPARSE_TILE_J0 t_j0
#define SPARSE_TILE_Q0 t_q0
#include "kernels_sparse_tile_body.h"
#undef SPARSE_TILE_J0
#undef SPARSE_TILE_Q0
}

void launch_grouped_scan(const GroupedScanParams& p, hipStream_t s) {
    if (!p.n_tiles || !p.scan.nq) return;
    if (p.scan.metric == EUCLID) hipLaunchKernelGGL(grouped_scan_kernel_t<true>, dim3(p.n_tiles), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(grouped_scan_kernel_t<false>, dim3(p.n_tiles), dim3(256), 0, s, p);
}

}  // namespace vdb
