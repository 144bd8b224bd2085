// kernels_discover.hip -- the device steps of discovery search (vdb_flat_discover_batch, include/vdb_flat.h "DISCOVERY SEARCH",
// DESIGN.md 4.18): request b names a target t and pairs (p_i, n_i) of stored ids; every eligible row x has
//   rank(x) = the number of pairs with d(p_i, x) < d(n_i, x)    (IEEE <: a tie or a NaN does not count),
// and the answer is the eligible rows by (rank descending, ordered d(t, x) ascending, id ascending).  A request's examples lie
// side by side on the device: the target first, then p_1 n_1 p_2 n_2 ...  Three kernels:
//   - discover_rank_kernel (the list route): one workgroup per request takes its candidates -- the front of the ranking of the
//     eligible rows by (d(t, x), id), exact distances, from ONE certified search, the examples struck -- finds the device row of
//     every candidate id (binary search in id order, the live row among equal ids), folds it against the 2P examples' stored rows
//     eight at a time (fold_multi, the norms of both sides from the store) and counts the satisfied pairs.  The request is
//     ANSWERED when k_b candidates have rank P -- no row outside the list has a higher rank or sorts in front, so the first k_b
//     of them in list order are the answer -- or when the list is complete (it holds every eligible row): then the answer is
//     its stable sort by rank descending.  Both are one loop: the rank levels from P downwards, each compacted in list order.
//   - discover_scan_kernel (the exact scan): one thread per row, the row folded against the target and the 2P examples; one key
//     ((P - rank) << 59 | ordered d(t, x) << 27 | id rank) per eligible row, EMPTY_KEY for every other -- ascending keys are the
//     answer's order, every distance bit is kept, and the store has fewer than 2^27 rows (the host refuses a larger one).  A NaN
//     d(t, x) at any row the mask admits raises ST_NAN before the strike.
//   - discover_emit_kernel: the first k_b keys of the full-scan select, taken apart into id, distance and rank.
// Plain C++ throughout; gfx950 only.
#include "kernels_exact.h"

#pragma clang fp contract(off)

namespace vdb {

constexpr uint32_t DISC_THREADS = 256, DISC_WAVES = DISC_THREADS / 64;
constexpr uint32_t DISC_NO_RANK = 0xffu;                                   // rank byte of a candidate without a live row

// the first `nthis` of eight example rows as wave-uniform values (the row numbers live in memory every lane reads alike)
__device__ __forceinline__ void disc_rows8(const uint32_t* src, uint32_t nthis, uint32_t (&q8)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) q8[j] = j < (int)nthis ? (uint32_t)__builtin_amdgcn_readfirstlane((int)src[j]) : 0u;
}

// the live device row that holds `id`: binary search in id order, then along the rows of that id
__device__ __forceinline__ uint32_t disc_row_of(const DiscoverRankParams& p, uint64_t id) {
    uint32_t lo = 0, hi = p.n_rows;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint32_t r = p.rank2row ? p.rank2row[mid] : mid;
        if (r < p.n_rows && p.row_ids[r] < id) lo = mid + 1; else hi = mid;
    }
    for (; lo < p.n_rows; ++lo) {
        const uint32_t r = p.rank2row ? p.rank2row[lo] : lo;
        if (r >= p.n_rows || p.row_ids[r] != id) break;
        if ((p.live[r >> 5] >> (r & 31)) & 1u) return r;
    }
    return NO_ROW;
}

// ---------------------------------------------------------------------------------------------
// the list route: ranks of the candidates, the answered rule, the answer
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DISC_THREADS) void discover_rank_kernel(DiscoverRankParams p) {
    __shared__ uint8_t sRank[DISCOVER_MAX_LIST];
    __shared__ uint32_t sEx[2 * DISCOVER_MAX_PAIRS + 8];
    __shared__ uint32_t sWave[DISC_WAVES];
    __shared__ uint32_t sFull;
    const uint32_t j = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t b = p.sel ? p.sel[j] : j;
    const uint32_t o0 = p.R.offs[b], m0 = p.R.offs[b + 1] - o0;
    const uint32_t ne = m0 ? ((m0 - 1 < 2 * DISCOVER_MAX_PAIRS ? m0 - 1 : 2 * DISCOVER_MAX_PAIRS) & ~1u) : 0u;   // (the host refused a longer request)
    const uint32_t P = ne / 2;
    const uint32_t kb = p.R.ks[b] < p.kout ? p.R.ks[b] : p.kout;
    const uint32_t cap = p.cand_stride < DISCOVER_MAX_LIST ? p.cand_stride : DISCOVER_MAX_LIST;
    const uint32_t count = p.cand_cnt[j] < cap ? p.cand_cnt[j] : cap;
    if (tid < 2 * DISCOVER_MAX_PAIRS + 8) {
        const uint32_t r = tid < ne ? p.R.rows[o0 + 1 + tid] : 0u;
        sEx[tid] = r < p.n_rows ? r : 0u;                                  // (the host resolved every example: never outside the store)
    }
    if (tid == 0) sFull = 0;
    __syncthreads();
    const uint64_t* ids = p.cand_ids + (size_t)j * p.cand_stride;
    const float* dts = p.cand_dists + (size_t)j * p.cand_stride;
    uint32_t full = 0;
    for (uint32_t base = 0; base < count; base += DISC_THREADS) {
        const uint32_t i = base + tid;
        if (i >= count) continue;
        const uint32_t row = disc_row_of(p, ids[i]);
        if (row == NO_ROW) { atomicOr(p.status, 2u); sRank[i] = (uint8_t)DISC_NO_RANK; continue; }
        const float* x = p.rows + (size_t)row * p.ld;
        const float xn = p.nd[row];
        uint32_t rank = 0;
        float dpos = 0.0f;
        for (uint32_t c = 0; c < ne; c += 8) {
            const uint32_t nthis = ne - c < 8 ? ne - c : 8;
            uint32_t q8[8];
            disc_rows8(sEx + c, nthis, q8);
            float s[8];
            fold_multi<8>(p.metric, x, p.dim, p.rows, p.ld, q8, nthis, s);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (u < (int)nthis) {
                    const float d = distance_from_fold(p.metric, s[u], p.nd[q8[u]], xn);
                    if (u & 1) rank += dpos < d ? 1u : 0u;                 // a tie or a NaN is "not satisfied"
                    else dpos = d;
                }
            }
        }
        sRank[i] = (uint8_t)rank;
        full += rank == P ? 1u : 0u;
    }
    if (full) atomicAdd(&sFull, full);
    __syncthreads();
    const bool complete = p.exhaustive || p.raw_cnt[j] < p.depth;
    const bool answered = sFull >= kb || complete;
    if (tid == 0 && p.answered) p.answered[j] = answered ? 1u : 0u;
    if (!answered) return;                                                 // (the same in every lane)
    uint64_t* oi = p.out_ids + (size_t)b * p.kout;
    float* od = p.out_dists + (size_t)b * p.kout;
    uint32_t* orank = p.out_ranks + (size_t)b * p.kout;
    uint32_t kept = 0;                                                     // the same in every lane
    for (uint32_t level = P + 1; level-- > 0 && kept < kb;) {
        for (uint32_t base = 0; base < count && kept < kb; base += DISC_THREADS) {
            const uint32_t i = base + tid;
            const bool keep = i < count && sRank[i] == level;
            const unsigned long long kbits = __ballot(keep);
            if (lane == 0) sWave[wave] = (uint32_t)__popcll(kbits);
            __syncthreads();
            uint32_t before = kept, total = 0;
            for (uint32_t w = 0; w < DISC_WAVES; ++w) {
                if (w < wave) before += sWave[w];
                total += sWave[w];
            }
            const uint32_t pos = before + (uint32_t)__popcll(kbits & ((1ull << lane) - 1ull));
            if (keep && pos < kb) { oi[pos] = ids[i]; od[pos] = dts[i]; orank[pos] = level; }
            kept += total;
            __syncthreads();                                               // sWave is rewritten by the next chunk
        }
    }
    if (tid == 0) p.out_counts[b] = kept < kb ? kept : kb;
}

void launch_discover_rank(const DiscoverRankParams& p, uint32_t n_req, hipStream_t s) {
    if (!n_req) return;
    hipLaunchKernelGGL(discover_rank_kernel, dim3(n_req), dim3(DISC_THREADS), 0, s, p);
}

// ---------------------------------------------------------------------------------------------
// the exact scan
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DISC_THREADS) void discover_scan_kernel(DiscoverScanParams p) {
    const uint32_t row = blockIdx.x * DISC_THREADS + threadIdx.x;
    if (row >= p.n_rows) return;
    uint64_t* out = p.keys + (size_t)blockIdx.y * p.key_stride + row;
    const bool ok = p.rowmask ? ((p.rowmask[row >> 5] >> (row & 31)) & 1u) : true;
    if (!ok) { *out = EMPTY_KEY; return; }
    const uint32_t b = p.sel[blockIdx.y];
    const uint32_t o0 = p.R.offs[b], m0 = p.R.offs[b + 1] - o0;
    const uint32_t m = m0 ? (((m0 - 1 < 2 * DISCOVER_MAX_PAIRS ? m0 - 1 : 2 * DISCOVER_MAX_PAIRS) & ~1u) + 1) : 0u;   // target + 2P
    const uint32_t P = m / 2;
    const float* x = p.rows + (size_t)row * p.ld;
    const float xn = p.nd[row];
    float dt = 0.0f, dpos = 0.0f;
    uint32_t rank = 0;
    bool struck = false;
    for (uint32_t c = 0; c < m; c += 8) {
        const uint32_t nthis = m - c < 8 ? m - c : 8;
        uint32_t q8[8];
        disc_rows8(p.R.rows + o0 + c, nthis, q8);
        float s[8];
        fold_multi<8>(p.metric, x, p.dim, p.rows, p.ld, q8, nthis, s);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < (int)nthis) {
                const float d = distance_from_fold(p.metric, s[j], p.nd[q8[j]], xn);
                struck = struck || q8[j] == row;
                // (eight is even: entry c + j is a positive exactly when j is odd, the target is entry 0)
                if (c + j == 0) dt = d;
                else if (j & 1) dpos = d;
                else rank += dpos < d ? 1u : 0u;
            }
        }
    }
    const bool nan = dt != dt;
    if (nan) atomicOr(p.status, ST_NAN);
    const uint32_t rk = p.idrank ? p.idrank[row] : row;
    *out = (!struck && !nan && m) ? (((uint64_t)(P - rank) << DISCOVER_KEY_LEVEL_SHIFT) | ((uint64_t)f32_to_ordered(dt) << DISCOVER_KEY_ID_BITS) | rk)
                                  : EMPTY_KEY;
}

void launch_discover_scan(const DiscoverScanParams& p, uint32_t n_req, hipStream_t s) {
    if (!p.n_rows || !n_req) return;
    hipLaunchKernelGGL(discover_scan_kernel, dim3((p.n_rows + DISC_THREADS - 1) / DISC_THREADS, n_req), dim3(DISC_THREADS), 0, s, p);
}

__global__ __launch_bounds__(DISC_THREADS) void discover_emit_kernel(DiscoverEmitParams p) {
    const uint32_t y = blockIdx.x, b = p.sel[y];
    const uint32_t o0 = p.R.offs[b], m0 = p.R.offs[b + 1] - o0;
    const uint32_t P = m0 ? (m0 - 1 < 2 * DISCOVER_MAX_PAIRS ? m0 - 1 : 2 * DISCOVER_MAX_PAIRS) / 2 : 0u;
    const uint32_t kb = p.R.ks[b] < p.kout ? p.R.ks[b] : p.kout;
    const uint32_t have = p.key_cnt[y] < p.key_stride ? p.key_cnt[y] : p.key_stride;
    const uint32_t count = have < kb ? have : kb;
    const uint64_t* keys = p.keys + (size_t)y * p.key_stride;
    for (uint32_t i = threadIdx.x; i < count; i += DISC_THREADS) {
        const uint64_t key = keys[i];
        const uint32_t rk = (uint32_t)(key & ((1ull << DISCOVER_KEY_ID_BITS) - 1ull));
        const uint32_t row = rk < p.n_rows ? (p.rank2row ? p.rank2row[rk] : rk) : NO_ROW;
        const uint32_t level = (uint32_t)(key >> DISCOVER_KEY_LEVEL_SHIFT);
        const size_t o = (size_t)b * p.kout + i;
        if (row < p.n_rows && level <= P) {
            p.out_ids[o] = p.row_ids[row];
            p.out_dists[o] = ordered_to_f32((uint32_t)(key >> DISCOVER_KEY_ID_BITS));
            p.out_ranks[o] = P - level;
        } else {
            atomicOr(p.status, 2u);                                        // (an empty key among the first count: never)
            p.out_ids[o] = ~0ull; p.out_dists[o] = __uint_as_float(0x7fc00000u); p.out_ranks[o] = 0;
        }
    }
    if (threadIdx.x == 0) p.out_counts[b] = count;
}

void launch_discover_emit(const DiscoverEmitParams& p, uint32_t n_req, hipStream_t s) {
    if (!n_req) return;
    hipLaunchKernelGGL(discover_emit_kernel, dim3(n_req), dim3(DISC_THREADS), 0, s, p);
}

}  // namespace vdb
