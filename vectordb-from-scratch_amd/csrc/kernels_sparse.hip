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
#include "kernels.h"

#pragma clang fp contract(off)

namespace vdb {

// ---------------------------------------------------------------------------------------------
// Eligible-row list
// ---------------------------------------------------------------------------------------------
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

template <bool EUC>
__global__ __launch_bounds__(256) void sparse_scan_kernel_t(SparseScanParams p) {
    __shared__ __attribute__((aligned(16))) float sImg[2 * SP_IMG];
    __shared__ uint32_t sRow[SP_TR];

    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t j0 = blockIdx.x * SP_TR;                        // first list position of the tile
    const uint32_t q0 = blockIdx.y * SP_TQ;                        // first query (of this pass) of the tile
    if (tid < SP_TR) {
        const uint32_t j = j0 + tid;
        uint32_t row = 0xffffffffu;
        if (j < p.n_elig) { row = p.elig[j]; if (row >= p.n_rows) row = 0xffffffffu; }   // an entry out of range is skipped
        sRow[tid] = row;
    }
    __syncthreads();

    // staging: float4 f = tid + 256 u of a [64][32] chunk -> tile row f >> 3, 16-byte column f & 7 (8 threads = one 128-byte segment)
    const uint32_t st_r = tid >> 3, st_c = (tid & 7u) << 2;
    // sources: rows st_r, st_r + 32, queries st_r, st_r + 32.  A masked row or query reads the zero chunk instead (and does not
    // advance): no address is ever formed from an index that failed its check
    const uint32_t row_a = sRow[st_r], row_b = sRow[st_r + 32];
    const uint32_t q_a = q0 + st_r, q_b = q_a + 32;
    const bool ok0 = row_a != 0xffffffffu, ok1 = row_b != 0xffffffffu, ok2 = q_a < p.nq, ok3 = q_b < p.nq;
    const float* src0 = (ok0 ? p.rows + (size_t)row_a * p.ld : sparse_zero_chunk) + st_c;
    const float* src1 = (ok1 ? p.rows + (size_t)row_b * p.ld : sparse_zero_chunk) + st_c;
    const float* src2 = (ok2 ? p.qp + (size_t)q_a * p.ld : sparse_zero_chunk) + st_c;
    const float* src3 = (ok3 ? p.qp + (size_t)q_b * p.ld : sparse_zero_chunk) + st_c;
    const uint32_t step0 = ok0 ? KSTAGE : 0, step1 = ok1 ? KSTAGE : 0, step2 = ok2 ? KSTAGE : 0, step3 = ok3 ? KSTAGE : 0;
    const uint32_t off0 = st_r * SP_LD + st_c, off1 = off0 + 32 * SP_LD, off2 = off0 + SP_TR * SP_LD, off3 = off2 + 32 * SP_LD;
    const uint32_t n_chunks = (p.dim + KSTAGE - 1) / KSTAGE;       // (ld >= dim rounded up to KSTAGE; [dim, ld) reads as zero on both sides)
    float4 stg0 = *reinterpret_cast<const float4*>(src0);
    float4 stg1 = *reinterpret_cast<const float4*>(src1);
    float4 stg2 = *reinterpret_cast<const float4*>(src2);
    float4 stg3 = *reinterpret_cast<const float4*>(src3);
    *reinterpret_cast<float4*>(sImg + off0) = stg0;
    *reinterpret_cast<float4*>(sImg + off1) = stg1;
    *reinterpret_cast<float4*>(sImg + off2) = stg2;
    *reinterpret_cast<float4*>(sImg + off3) = stg3;
    __syncthreads();

    const uint32_t tr = lane >> 2, tq = wave * 16 + (lane & 3u) * 4;
    const bool wave_active = q0 + wave * 16 < p.nq;                // wave-uniform
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;

    for (uint32_t c = 0; c < n_chunks; ++c) {
        const bool more = c + 1 < n_chunks;
        if (more) {
            src0 += step0; src1 += step1; src2 += step2; src3 += step3;
            stg0 = *reinterpret_cast<const float4*>(src0);
            stg1 = *reinterpret_cast<const float4*>(src1);
            stg2 = *reinterpret_cast<const float4*>(src2);
            stg3 = *reinterpret_cast<const float4*>(src3);
        }
        if (wave_active) {
            const float* img = sImg + (c & 1u) * SP_IMG;
            // quads of this chunk that hold elements of the vectors (the rest is padding: +0 products, which leave the sums as they are)
            const uint32_t left = p.dim - c * KSTAGE;
            const uint32_t n_quads = left >= KSTAGE ? KSTAGE / 4 : (left + 3) / 4;
            for (uint32_t kq = 0; kq < n_quads; ++kq) {
                float4 x[4], q[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) x[i] = *reinterpret_cast<const float4*>(img + (tr + 16 * i) * SP_LD + 4 * kq);
#pragma unroll
                for (int j = 0; j < 4; ++j) q[j] = *reinterpret_cast<const float4*>(img + (SP_TR + tq + j) * SP_LD + 4 * kq);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float xv = e == 0 ? x[i].x : e == 1 ? x[i].y : e == 2 ? x[i].z : x[i].w;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float qv = e == 0 ? q[j].x : e == 1 ? q[j].y : e == 2 ? q[j].z : q[j].w;
                            if (EUC) { const float t = __fsub_rn(qv, xv); acc[i][j] = __fadd_rn(acc[i][j], __fmul_rn(t, t)); }
                            else acc[i][j] = __fadd_rn(acc[i][j], __fmul_rn(qv, xv));
                        }
                    }
                }
            }
        }
        if (more) {
            float* nxt = sImg + ((c + 1) & 1u) * SP_IMG;           // last read in round c - 1, before that round's barrier
            *reinterpret_cast<float4*>(nxt + off0) = stg0;
            *reinterpret_cast<float4*>(nxt + off1) = stg1;
            *reinterpret_cast<float4*>(nxt + off2) = stg2;
            *reinterpret_cast<float4*>(nxt + off3) = stg3;
        }
        __syncthreads();
    }

    // ---- epilogue: distance -> key, through LDS (every read of the images is behind the loop's last barrier)
    uint64_t* sKey = reinterpret_cast<uint64_t*>(sImg);           // [SP_TQ][SP_TR]
    if (wave_active) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t row = sRow[tr + 16 * i];
            const bool row_ok = row != 0xffffffffu;
            const float xn = (row_ok && p.metric == COSINE) ? p.nd[row] : 0.0f;
            const uint32_t rk = row_ok ? (p.idrank ? p.idrank[row] : row) : 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t q = q0 + tq + j;
                uint64_t key = EMPTY_KEY;
                if (row_ok && q < p.nq) {
                    const float s = acc[i][j];
                    float dist;
                    if (EUC) dist = __builtin_sqrtf(s);
                    else if (p.metric == DOT) dist = -s;
                    else {
                        float sim = __fdiv_rn(s, __fmul_rn(p.qnorm[q], xn));   // distance.rs:58
                        if (sim < -1.0f) sim = -1.0f;                         // f32::clamp keeps NaN
                        if (sim > 1.0f) sim = 1.0f;
                        dist = __fsub_rn(1.0f, sim);
                    }
                    if (dist != dist) atomicOr(p.status, ST_NAN);
                    key = ((uint64_t)f32_to_ordered(dist) << 32) | rk;
                }
                sKey[(tq + j) * SP_TR + tr + 16 * i] = key;
            }
        }
    }
    __syncthreads();
    // keys[q * key_stride + j]: one query's 64 keys are 512 contiguous bytes.  key_stride is a multiple of SPARSE_TILE_R, so the
    // whole tile is inside the buffer; the positions past the end of the list carry EMPTY_KEY
    for (uint32_t f = tid; f < SP_TQ * SP_TR; f += 256) {
        const uint32_t ql = f / SP_TR, r = f % SP_TR;
        const uint32_t q = q0 + ql;
        if (q < p.nq && j0 + r < p.key_stride) p.keys[(size_t)q * p.key_stride + j0 + r] = sKey[f];
    }
}

void launch_sparse_scan(const SparseScanParams& p, hipStream_t s) {
    if (!p.n_elig || !p.nq) return;
    const dim3 grid((p.n_elig + SP_TR - 1) / SP_TR, (p.nq + SP_TQ - 1) / SP_TQ);
    if (p.metric == EUCLID) hipLaunchKernelGGL(sparse_scan_kernel_t<true>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(sparse_scan_kernel_t<false>, grid, dim3(256), 0, s, p);
}

}  // namespace vdb
