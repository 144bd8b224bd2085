// kernels_i8.hip -- the int8 flat index (include/vdb_flat.h "Int8 vectors"): exact top-k on the integer matrix
// cores of gfx950.  v_mfma_i32_16x16x64_i8 accumulates in i32 without rounding, so ONE pass over 1 B/element rows yields the exact
// integer score of every (query, row) pair: no screen, no certificate, no re-rank.
//
//   score   ONE workgroup of 512 threads (8 waves) per (segment of R consecutive rows, tile of QT queries).  The query tile's int8
//           image lies in LDS -- the whole query where the select buffers leave room for it (dim 768 up to k = 124 does), else kc
//           bytes of every query at a time, re-staged per round -- at a row stride of kc + 16 bytes (the 16 lanes of one
//           ds_read_b128 group then hit 64 distinct banks).  A wave owns 32 rows of a round of 256: two A operands, each lane
//           loading 16 consecutive bytes of row (lane & 15) at K offset 16 * (lane >> 4) straight from global memory into the
//           operand registers -- a row is contiguous along K, so four lanes cover the 64 bytes of a K step and nothing is staged or
//           transposed.  The B operand is the same 16 bytes of query (lane & 15) from LDS: both operands use one K mapping, so the
//           sum is over matching elements whatever order the unit takes them in.  2 x QT/16 independent i32 accumulator tiles per
//           wave; the K loop runs in batches of four steps, double-buffered: the eight 16-byte row loads of the next batch are
//           in flight under the MFMAs of this one.  Workgroup ids are re-ordered so that the tiles of a segment share an XCD's L2.
//           Epilogue: accumulator r of lane l is (row 4 (l >> 4) + r, query l & 15).  The metric's f32 distance from the three
//           integer sums, the monotone key (ordered distance bits, id rank), the live bit, the id mask, then an offer into the
//           query's select buffer in LDS: threshold, bounded fill (an offer that finds the buffer full stays pending), prune to k
//           (a workgroup-wide bitonic network over every buffer above its k) and retry.  The workgroup writes its min(k, found) smallest
//           keys of every query to part[query][segment][.].
//   merge   one workgroup per query streams the segments' partial lists through the select of kernels_spv_select.h; keys are
//           unique (the id rank is), so the k smallest of the union are the answer.
// Compiled with -ffp-contract=off; every f32 operation of a distance is one correctly rounded IEEE operation.
#include "kernels.h"
#include "kernels_i8.h"
#include "kernels_spv_select.h"

#pragma clang fp contract(off)

namespace vdb {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr uint32_t I8_WAVES = I8_THREADS / 64;

template <int METRIC> __device__ __forceinline__ float i8_distance(int32_t s, int32_t nq, int32_t nx) {
    if (METRIC == EUCLID) return __builtin_sqrtf((float)(nq + nx - 2 * s));
    if (METRIC != COSINE) return -(float)s;
    const float den = __fmul_rn(__builtin_sqrtf((float)nq), __builtin_sqrtf((float)nx));
    float sim = __fdiv_rn((float)s, den);
    if (sim < -1.0f) sim = -1.0f;
    if (sim > 1.0f) sim = 1.0f;
    return __fsub_rn(1.0f, sim);
}

// ---- the norms of added rows: one wave per row
__global__ __launch_bounds__(256) void i8_row_norms_kernel(const int8_t* __restrict__ rows, uint32_t ld, uint32_t row_begin, uint32_t row_end,
                                                           int32_t* __restrict__ nx) {
    const uint32_t lane = threadIdx.x & 63, row = row_begin + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= row_end) return;                      // (whole waves leave: no barrier follows)
    const int8_t* __restrict__ x = rows + (size_t)row * ld;
    int32_t sum = 0;
    for (uint32_t off = lane * 16; off < ld; off += 64 * 16) {        // ld is a multiple of 64: a piece is inside the row
        const v4i v = *reinterpret_cast<const v4i*>(x + off);
        for (int w = 0; w < 4; ++w)
            for (int b = 0; b < 4; ++b) {
                const int32_t e = (int32_t)(int8_t)(v[w] >> (8 * b));
                sum += e * e;
            }
    }
    for (uint32_t d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    if (lane == 0) nx[row] = sum;
}

__global__ __launch_bounds__(256) void i8_zero_rows_kernel(const int32_t* __restrict__ nx, const uint32_t* __restrict__ live, uint32_t n_rows,
                                                           uint32_t* __restrict__ count) {
    uint32_t mine = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += gridDim.x * blockDim.x)
        mine += ((live[r >> 5] >> (r & 31)) & 1u) && nx[r] == 0;
    for (uint32_t d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, mine);
}

__global__ __launch_bounds__(256) void i8_fill_kernel(uint32_t* __restrict__ words, size_t n, uint32_t value) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) words[i] = value;
}

// ---- the select of a query tile.  EVERY buffer above its k -- not the full one alone: a prune costs the workgroup its barriers
// whatever the number of buffers, and 64 queries that fill up at 64 different times would pay them 64 times -- is sorted ascending
// by ONE bitonic network whose comparators all point upwards -- slots at and above a buffer's fill count as +inf and never move, so
// a buffer needs no power-of-two room -- and cut to its k smallest keys; the k-th becomes the threshold.  Called by the whole
// workgroup.
template <uint32_t QT>
__device__ inline void i8_prune(uint64_t* s_keys, uint64_t* s_thr, uint32_t* s_cnt, const uint32_t* s_kq, uint32_t* s_need, uint32_t cap,
                                uint32_t P) {
    const uint32_t tid = threadIdx.x;
    if (tid < QT) {
        const uint32_t kq = s_kq[tid], capq = min(cap, i8_select_cap(kq)), n = min(s_cnt[tid], capq);
        s_cnt[tid] = n;                              // (offers that found no room counted themselves in)
        s_need[tid] = n > kq;
    }
    __syncthreads();
    const uint32_t half = P >> 1, lh = __ffs(half) - 1;   // every size here is a power of two: shifts and masks, no division
    for (uint32_t k2 = 2; k2 <= P; k2 <<= 1)
        for (uint32_t j = k2 >> 1, lj = __ffs(j) - 1; j > 0; j >>= 1, --lj) {
            for (uint32_t item = tid; item < QT * half; item += I8_THREADS) {
                const uint32_t q = item >> lh, pi = item & (half - 1);
                if (!s_need[q]) continue;
                const uint32_t blk = pi >> lj, off = pi & (j - 1);
                uint32_t i, o;
                if (j == (k2 >> 1)) { i = blk * k2 + off; o = i + k2 - 1 - 2 * off; }   // the mirror step of a merge
                else { i = blk * 2 * j + off; o = i + j; }
                if (o < s_cnt[q]) {
                    uint64_t* kk = s_keys + (size_t)q * cap;
                    const uint64_t x = kk[i], y = kk[o];
                    if (x > y) { kk[i] = y; kk[o] = x; }
                }
            }
            __syncthreads();
        }
    if (tid < QT && s_need[tid]) {
        const uint32_t kq = s_kq[tid], n = s_cnt[tid];
        s_cnt[tid] = min(n, kq);
        s_thr[tid] = (kq && n >= kq) ? s_keys[(size_t)tid * cap + kq - 1] : EMPTY_KEY;
    }
    __syncthreads();
}

// U K steps of 64 bytes: the 2 U row loads of the lane first, so that they are in flight together, then U x 2 x QB MFMAs, each
// query operand read once from LDS for both row blocks
template <int U>
__device__ __forceinline__ void i8_load(const int8_t* __restrict__ a0p, const int8_t* __restrict__ a1p, v4i (&a)[U][2]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        a[u][0] = *reinterpret_cast<const v4i*>(a0p + 64 * u);
        a[u][1] = *reinterpret_cast<const v4i*>(a1p + 64 * u);
    }
}
template <int QB, int U>
__device__ __forceinline__ void i8_mma(const v4i (&a)[U][2], const unsigned char* bp, uint32_t stride, v4i (&acc)[2][QB]) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            const v4i b = *reinterpret_cast<const v4i*>(bp + qb * 16 * stride + 64 * u);
            acc[0][qb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[u][0], b, acc[0][qb], 0, 0, 0);
            acc[1][qb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[u][1], b, acc[1][qb], 0, 0, 0);
        }
}

// ---- score + select; the metric is a template parameter: the epilogue evaluates 8 x QT/16 distances per lane and round, and a
// run-time metric made each of them carry the square roots and the division of all three
template <int QB, int METRIC>
__global__ __launch_bounds__(I8_THREADS) void i8_score_kernel(I8SearchParams p) {
    constexpr uint32_t QT = 16 * QB;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_img[];   // [QT][stride]
    const uint32_t stride = p.kc + 16;               // bytes between two queries of the image: 4 (odd) dwords, no bank shared by 16 queries
    uint64_t* s_keys = reinterpret_cast<uint64_t*>(s_img + QT * stride);      // [QT][cap]
    uint64_t* s_thr = s_keys + (size_t)QT * p.cap;
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_thr + QT);
    uint32_t* s_kq = s_cnt + QT;
    uint32_t* s_need = s_kq + QT;
    int32_t* s_nq = reinterpret_cast<int32_t*>(s_need + QT);
    uint32_t* s_kmax = reinterpret_cast<uint32_t*>(s_nq + QT);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
    // Workgroup ids go round the 8 XCDs; this order gives every XCD a run of consecutive (segment, tile) pairs, so that the tiles of
    // one segment meet its rows in one L2.  The grid is padded to a multiple of 8: the surplus leaves here.
    const uint32_t tiles = (p.n_q + QT - 1) / QT, wg = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    if (wg >= p.segs * tiles) return;
    const uint32_t seg = wg / tiles, y0 = (wg - seg * tiles) * QT;
    const uint32_t r0 = seg * p.seg_rows, nr = min(p.seg_rows, p.n_rows - r0);      // seg < segs = ceil(n_rows / seg_rows)
    const uint32_t ld = p.ld, cap = p.cap;
    if (tid == 0) *s_kmax = 0;
    __syncthreads();
    if (tid < QT) {
        const bool valid = y0 + tid < p.n_q;
        const uint32_t kq = valid ? min(p.ks[p.q0 + y0 + tid], min(p.kout, I8_MAX_K)) : 0;
        s_kq[tid] = kq; s_cnt[tid] = 0; s_thr[tid] = EMPTY_KEY;
        s_nq[tid] = valid ? p.nq[p.q0 + y0 + tid] : 1;
        atomicMax(s_kmax, kq);
    }
    __syncthreads();
    uint32_t P = 2;                                  // the network's size: the largest buffer of the tile
    while (P < min(cap, i8_select_cap(*s_kmax))) P <<= 1;

    const uint32_t chunks = (ld + p.kc - 1) / p.kc, rounds = (nr + I8_ROUND_ROWS - 1) / I8_ROUND_ROWS;
    for (uint32_t it = 0; it < rounds; ++it) {
        const uint32_t base = r0 + it * I8_ROUND_ROWS + wave * 32;
        // the lane's two operand rows; a row beyond the store is read as the last row and never offered
        const int8_t* __restrict__ a0p = p.rows + (size_t)min(base + c, p.n_rows - 1) * ld + 16 * g;
        const int8_t* __restrict__ a1p = p.rows + (size_t)min(base + 16 + c, p.n_rows - 1) * ld + 16 * g;
        // what the epilogue needs of the lane's 8 result rows (base + 16 rb + 4 g + r), asked for now: it arrives under the K loop
        int32_t nx[8];
        uint32_t rk[8], okm = 0;
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
            const uint32_t row = base + 16 * (rr >> 2) + 4 * g + (rr & 3);
            bool ok = row < r0 + nr;
            nx[rr] = 1; rk[rr] = 0;
            if (ok) {
                ok = (p.live[row >> 5] >> (row & 31)) & 1u;
                if (ok && p.id_mask) {
                    const uint64_t id = p.row_ids[row];
                    ok = id < p.mask_bits && ((p.id_mask[id >> 6] >> (id & 63)) & 1ull);
                }
                nx[rr] = p.nx[row]; rk[rr] = p.rank[row];
            }
            okm |= (uint32_t)ok << rr;
        }
        v4i acc[2][QB];
        for (int rb = 0; rb < 2; ++rb)
            for (int qb = 0; qb < QB; ++qb) acc[rb][qb] = v4i{0, 0, 0, 0};
        for (uint32_t ch = 0; ch < chunks; ++ch) {
            const uint32_t kc0 = ch * p.kc, kc_len = min(p.kc, ld - kc0);           // a multiple of 64
            if (chunks > 1 || it == 0) {             // (uniform) the image: once where a query fits, else per round and chunk
                __syncthreads();                     // nobody reads the chunk before any more
                const uint32_t pieces = kc_len >> 4;
                for (uint32_t i = tid; i < QT * pieces; i += I8_THREADS) {
                    const uint32_t q = i / pieces, pc = i - q * pieces;
                    v4i v = v4i{0, 0, 0, 0};
                    if (y0 + q < p.n_q) v = *reinterpret_cast<const v4i*>(p.q + (size_t)(p.q0 + y0 + q) * ld + kc0 + 16 * pc);
                    *reinterpret_cast<v4i*>(s_img + q * stride + 16 * pc) = v;
                }
                __syncthreads();
            }
            // batches of 4 K steps, double-buffered: the 8 row loads of the next batch are in flight under the MFMAs of this one
            const unsigned char* bp = s_img + c * stride + 16 * g;
            const int8_t* __restrict__ x0 = a0p + kc0;
            const int8_t* __restrict__ x1 = a1p + kc0;
            const uint32_t steps = kc_len >> 6, nb = steps >> 2;
            v4i a[2][4][2];
            if (nb) i8_load<4>(x0, x1, a[0]);
            for (uint32_t b = 0; b < nb; b += 2) {
                if (b + 1 < nb) i8_load<4>(x0 + 256 * (b + 1), x1 + 256 * (b + 1), a[1]);
                i8_mma<QB, 4>(a[0], bp + 256 * b, stride, acc);
                if (b + 1 < nb) {
                    if (b + 2 < nb) i8_load<4>(x0 + 256 * (b + 2), x1 + 256 * (b + 2), a[0]);
                    i8_mma<QB, 4>(a[1], bp + 256 * (b + 1), stride, acc);
                }
            }
            for (uint32_t ks = 4 * nb; ks < steps; ++ks) {
                v4i t[1][2];
                i8_load<1>(x0 + 64 * ks, x1 + 64 * ks, t);
                i8_mma<QB, 1>(t, bp + 64 * ks, stride, acc);
            }
        }

        // ---- epilogue: the lane holds rows base + 16 rb + 4 g + r against queries 16 qb + c
        uint32_t pending = 0;
#pragma unroll
        for (int rr = 0; rr < 8; ++rr)
            if ((okm >> rr) & 1u) {
#pragma unroll
                for (int qb = 0; qb < QB; ++qb)
                    if (s_kq[16 * qb + c]) pending |= 1u << (rr * QB + qb);
            }
        for (;;) {
            uint32_t still = 0;
#pragma unroll
            for (int rr = 0; rr < 8; ++rr)
#pragma unroll
                for (int qb = 0; qb < QB; ++qb) {
                    const uint32_t bit = 1u << (rr * QB + qb);
                    if (pending & bit) {
                        const uint32_t q = 16 * qb + c;
                        const uint64_t key = make_key(i8_distance<METRIC>(acc[rr >> 2][qb][rr & 3], s_nq[q], nx[rr]), rk[rr]);
                        if (key < s_thr[q]) {
                            const uint32_t slot = atomicAdd(&s_cnt[q], 1u);
                            if (slot < min(cap, i8_select_cap(s_kq[q]))) s_keys[(size_t)q * cap + slot] = key;
                            else still |= bit;       // the buffer is full: pruned below, offered again
                        }
                    }
                }
            pending = still;
            if (!__syncthreads_or(pending != 0)) break;
            i8_prune<QT>(s_keys, s_thr, s_cnt, s_kq, s_need, cap, P);
        }
    }
    __syncthreads();
    i8_prune<QT>(s_keys, s_thr, s_cnt, s_kq, s_need, cap, P);
    for (uint32_t q = wave; q < QT; q += I8_WAVES) {
        if (y0 + q >= p.n_q) continue;               // (uniform in the wave)
        const size_t slot = (size_t)(y0 + q) * p.segs + seg;
        const uint32_t cnt = s_cnt[q];               // <= k of the query <= kout
        for (uint32_t i = lane; i < cnt; i += 64) p.part[slot * p.kout + i] = s_keys[(size_t)q * cap + i];
        if (lane == 0) p.part_cnt[slot] = cnt;
    }
    if (tid < 64) {
        uint32_t v = (tid < QT && y0 + tid < p.n_q) ? s_cnt[tid] : 0;
        for (uint32_t d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
        if (tid == 0 && v) atomicAdd(&p.counters[0], (unsigned long long)v);
    }
}

// ---- merge (spv_seg_merge_kernel's shape: one workgroup of SPV_THREADS per query)
__global__ __launch_bounds__(SPV_THREADS) void i8_merge_kernel(I8SearchParams p) {
    __shared__ uint64_t s_keys[SPV_SELECT_CAP];
    __shared__ uint64_t s_thr;
    __shared__ uint32_t s_cnt;
    const uint32_t tid = threadIdx.x, y = blockIdx.x, b = p.q0 + y;
    if (tid == 0) { s_cnt = 0; s_thr = EMPTY_KEY; }
    __syncthreads();
    const uint32_t kq = min(p.ks[b], min(p.kout, I8_MAX_K));
    const uint64_t* __restrict__ part = p.part + (size_t)y * p.segs * p.kout;
    const uint32_t* __restrict__ part_cnt = p.part_cnt + (size_t)y * p.segs;
    const uint64_t total = (uint64_t)p.segs * p.kout;
    uint32_t bound = 0;
    for (uint64_t j = tid; j - tid < total; j += SPV_THREADS) {
        if (bound + SPV_THREADS > SPV_SELECT_CAP) bound = spv_prune(s_keys, &s_cnt, &s_thr, kq);
        int pushed = 0;
        if (j < total) {
            const uint64_t seg = j / p.kout;
            if ((uint32_t)(j - seg * p.kout) < part_cnt[seg]) {      // a slot its workgroup has written
                const uint64_t key = part[j];
                pushed = key < s_thr;
                spv_offer(s_keys, &s_cnt, &s_thr, key);               // below bound + SPV_THREADS <= SPV_SELECT_CAP
            }
        }
        bound += (uint32_t)__syncthreads_count(pushed);
    }
    const uint32_t cnt = spv_prune(s_keys, &s_cnt, &s_thr, kq);
    for (uint32_t i = tid; i < cnt; i += SPV_THREADS) {
        const uint64_t key = s_keys[i];
        p.out_ids[(size_t)b * p.kout + i] = p.sorted_ids[(uint32_t)key];
        p.out_dists[(size_t)b * p.kout + i] = ordered_to_f32((uint32_t)(key >> 32));
    }
    if (tid == 0) p.out_counts[b] = cnt;
}

template <int QB> void launch_score(const I8SearchParams& p, uint32_t grid, size_t lds, hipStream_t s) {
    if (p.metric == EUCLID) hipLaunchKernelGGL((i8_score_kernel<QB, EUCLID>), dim3(grid), dim3(I8_THREADS), lds, s, p);
    else if (p.metric == COSINE) hipLaunchKernelGGL((i8_score_kernel<QB, COSINE>), dim3(grid), dim3(I8_THREADS), lds, s, p);
    else hipLaunchKernelGGL((i8_score_kernel<QB, DOT>), dim3(grid), dim3(I8_THREADS), lds, s, p);
}

size_t score_lds(size_t qt, uint32_t kc, uint32_t cap) { return qt * (kc + 16) + qt * (size_t)cap * 8 + qt * (8 + 4 * 4) + 16; }

}  // namespace

void launch_i8_row_norms(const int8_t* rows, uint32_t ld, uint32_t row_begin, uint32_t row_end, int32_t* nx, hipStream_t s) {
    if (row_end <= row_begin) return;
    hipLaunchKernelGGL(i8_row_norms_kernel, dim3((row_end - row_begin + 3) / 4), dim3(256), 0, s, rows, ld, row_begin, row_end, nx);
}

void launch_i8_zero_rows(const int32_t* nx, const uint32_t* live, uint32_t n_rows, uint32_t* count, hipStream_t s) {
    if (!n_rows) return;
    hipLaunchKernelGGL(i8_zero_rows_kernel, dim3(std::min((n_rows + 255) / 256, 2048u)), dim3(256), 0, s, nx, live, n_rows, count);
}

void launch_i8_fill(uint32_t* words, size_t n, uint32_t value, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(i8_fill_kernel, dim3((uint32_t)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, s, words, n, value);
}

void launch_i8_score(const I8SearchParams& p, hipStream_t s) {
    if (!p.n_q || !p.segs) return;
    const uint32_t tiles = (p.n_q + p.qt - 1) / p.qt;                 // the host keeps segs * tiles below 2^31
    // the image holds as much of every query as the select buffers leave of the LDS budget, at most the whole query
    I8SearchParams q = p;
    q.kc = std::min<uint32_t>(p.ld, (uint32_t)((I8_LDS_BUDGET - score_lds(p.qt, 0, p.cap)) / p.qt) / 64 * 64);
    const uint32_t grid = (p.segs * tiles + 7) / 8 * 8;
    const size_t lds = score_lds(p.qt, q.kc, p.cap);
    if (p.qt == I8_QT) launch_score<I8_QT / 16>(q, grid, lds, s);
    else launch_score<I8_QT_LARGE_K / 16>(q, grid, lds, s);
}

void launch_i8_merge(const I8SearchParams& p, hipStream_t s) {
    if (!p.n_q) return;
    hipLaunchKernelGGL(i8_merge_kernel, dim3(p.n_q), dim3(SPV_THREADS), 0, s, p);
}

}  // namespace vdb
