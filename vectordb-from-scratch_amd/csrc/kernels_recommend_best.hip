// kernels_recommend_best.hip -- the device steps of "recommend by best score" (vdb_flat_recommend_best_batch, include/vdb_flat.h
// "RECOMMEND BY BEST SCORE"): every candidate row x is scored against every example on its own,
//   dp(x) = the smallest d(p_i, x) over the positives (left fold in list order with the IEEE <, the earlier positive's bits on a tie),
//   kept  iff dp(x) < d(n_j, x) for EVERY negative (a tie or a NaN is a veto),    dn(x) = the same fold over the negatives,
// and the answer is the kept rows ascending by (ordered dp, id).  Three kernels:
//   - rb_merge_kernel (the list route): the ranked lists of a request's positives -- one certified search each, ascending
//     (distance, id), exact distances -- are merged under the frontier proof.  A list with `depth` entries ends at its frontier; F
//     is the smallest frontier of the request; an entry with d < F is SETTLED: a row missing from list i has d(p_i, x) >= last_i
//     >= F, so the smallest distance seen for a settled row is its dp.  Because every list is sorted, the settled entries of a
//     list are a prefix of it (binary search).  At most RB_MAX_ENTRIES entries fit the sort area in LDS: when the settled
//     prefixes hold more, a bisection on the ordered distance finds the largest value t with "entries at or below t" within the
//     capacity (a binary search per list and step) -- that only lowers the frontier to just above t, the proof is the same.  The
//     entries are gathered, sorted by (id, distance, list) so that the first entry of every id is its fold, the examples (by
//     64-bit equality against the request's set) and the later entries of an id are dropped, the rest is sorted by (ordered
//     distance, id) and the first RB_MAX_ROWS rows leave as the request's candidates.  open[j] says whether rows may exist behind
//     them (a list that was not complete, or a walk that was cut).
//   - rb_scan_kernel (the exact scan): one thread per row, the row folded against the request's examples eight at a time
//     (fold_multi), positives first; one key (ordered dp, id rank) per kept row, EMPTY_KEY for every other -- the full-scan
//     select then emits the first k.  A NaN d(p_i, x) at any eligible row raises ST_NAN before the strike.
//   - rb_veto_kernel (both routes): for a request's candidates in order, the device row of each id (binary search in id order,
//     the live row among equal ids), the exact d(n_j, x) against every negative's stored row -- fold_multi again, the norms of
//     both sides from the store --, the kept rule, the dn fold, and the first k kept rows compacted in order.
// Plain C++ throughout; gfx950 only.
#include "kernels_exact.h"

#pragma clang fp contract(off)

namespace vdb {

constexpr uint32_t RB_THREADS = 256, RB_WAVES = RB_THREADS / 64;
constexpr uint32_t RB_DEAD = 0xffu;                                        // list byte of an entry that left the walk
constexpr float RB_INF = __builtin_huge_valf();

// the first `nthis` of eight example rows as wave-uniform values (the row numbers live in memory every lane reads alike)
__device__ __forceinline__ void rb_rows8(const uint32_t* src, uint32_t nthis, uint32_t (&q8)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) q8[j] = j < (int)nthis ? (uint32_t)__builtin_amdgcn_readfirstlane((int)src[j]) : 0u;
}

// ---------------------------------------------------------------------------------------------
// the exact scan
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RB_THREADS) void rb_scan_kernel(RbScanParams p) {
    const uint32_t row = blockIdx.x * RB_THREADS + threadIdx.x;
    if (row >= p.n_rows) return;
    uint64_t* out = p.keys + (size_t)blockIdx.y * p.key_stride + row;
    const bool ok = p.rowmask ? ((p.rowmask[row >> 5] >> (row & 31)) & 1u) : true;
    if (!ok) { *out = EMPTY_KEY; return; }
    const uint32_t b = p.sel[blockIdx.y];
    const uint32_t o0 = p.R.offs[b], m = p.R.offs[b + 1] - o0, np = p.R.n_pos[b];
    const float* x = p.rows + (size_t)row * p.ld;
    const float xn = p.nd[row];
    float dp = 0.0f;
    bool kept = true, nan = false, struck = false;
    for (uint32_t c = 0; c < m; c += 8) {
        const uint32_t nthis = m - c < 8 ? m - c : 8;
        uint32_t q8[8];
        rb_rows8(p.R.rows + o0 + c, nthis, q8);
        float s[8];
        fold_multi<8>(p.metric, x, p.dim, p.rows, p.ld, q8, nthis, s);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < (int)nthis) {
                const float d = distance_from_fold(p.metric, s[j], p.nd[q8[j]], xn);
                struck = struck || q8[j] == row;
                if (c + j < np) {
                    nan = nan || d != d;
                    if (c + j == 0 || d < dp) dp = d;
                } else kept = kept && dp < d;                              // (every positive has been folded: they come first)
            }
        }
    }
    if (nan) atomicOr(p.status, ST_NAN);
    const uint32_t rk = p.idrank ? p.idrank[row] : row;
    *out = (kept && !struck && !nan) ? (((uint64_t)f32_to_ordered(dp) << 32) | rk) : EMPTY_KEY;
}

void launch_rb_scan(const RbScanParams& p, uint32_t n_req, hipStream_t s) {
    if (!p.n_rows || !n_req) return;
    hipLaunchKernelGGL(rb_scan_kernel, dim3((p.n_rows + RB_THREADS - 1) / RB_THREADS, n_req), dim3(RB_THREADS), 0, s, p);
}

// ---------------------------------------------------------------------------------------------
// the merge of the ranked lists
// ---------------------------------------------------------------------------------------------
// entries of a sorted list (ordered distances) below `bound` (a 33-bit value: 1 << 32 admits everything)
__device__ __forceinline__ uint32_t rb_count_below(const float* d, uint32_t n, uint64_t bound) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint64_t)f32_to_ordered(d[mid]) < bound) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Bitonic sort of the triples (sD[i], sId[i], sL[i]), i < P (a power of two), ascending by `less`.  Ends with a barrier.
template <typename Less>
__device__ __forceinline__ void rb_sort(uint32_t* sD, uint64_t* sId, uint8_t* sL, uint32_t P, uint32_t tid, Less less) {
    for (uint32_t size = 2; size <= P; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t t = tid; t < P / 2; t += RB_THREADS) {
                const uint32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool up = ((lo & size) == 0);
                const uint32_t da = sD[lo], db = sD[hi];
                const uint64_t ia = sId[lo], ib = sId[hi];
                const uint8_t la = sL[lo], lb = sL[hi];
                const bool gt = less(db, ib, lb, da, ia, la);
                if (gt == up) { sD[lo] = db; sD[hi] = da; sId[lo] = ib; sId[hi] = ia; sL[lo] = lb; sL[hi] = la; }
            }
            __syncthreads();
        }
}

// +0.0 and -0.0 compare equal in the fold: both take the ordered value of +0.0 where the fold's order is wanted
__device__ __forceinline__ uint32_t rb_canon(uint32_t od) { return od == 0x7fffffffu ? 0x80000000u : od; }

__global__ __launch_bounds__(RB_THREADS) void rb_merge_kernel(RbMergeParams p) {
    __shared__ uint32_t sD[RB_MAX_ENTRIES];
    __shared__ __attribute__((aligned(16))) uint64_t sId[RB_MAX_ENTRIES];
    __shared__ uint8_t sL[RB_MAX_ENTRIES];
    __shared__ uint64_t sSet[RECOMMEND_MAX_EXAMPLES];
    __shared__ uint32_t sTake[RECOMMEND_MAX_EXAMPLES], sStart[RECOMMEND_MAX_EXAMPLES + 1];
    __shared__ uint32_t sFront, sOpen, sTotal;
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    const uint32_t b = p.sel ? p.sel[j] : j;
    const uint32_t o0 = p.R.offs[b], m0 = p.R.offs[b + 1] - o0;
    const uint32_t m = m0 < RECOMMEND_MAX_EXAMPLES ? m0 : RECOMMEND_MAX_EXAMPLES;      // (the host refused a longer request)
    const uint32_t np = p.R.n_pos[b] < m ? p.R.n_pos[b] : m;
    const uint32_t l0 = p.list0[j];
    if (tid < m) sSet[tid] = p.R.ids[o0 + tid];
    if (tid == 0) { sFront = 0xffffffffu; sOpen = 0; sTotal = 0; }
    __syncthreads();
    // ---- the frontier: the smallest last distance of the lists that came back full
    uint32_t cnt = 0;
    const float* dl = nullptr;
    if (tid < np) {
        dl = p.dists + (size_t)(l0 + tid) * p.depth;
        cnt = p.counts[l0 + tid] < p.depth ? p.counts[l0 + tid] : p.depth;
        if (cnt == p.depth && cnt) {
            const float f = dl[cnt - 1];
            // (IEEE "d < F": with F = +-0.0 neither zero is below it)
            atomicMin(&sFront, f == 0.0f ? 0x7fffffffu : f32_to_ordered(f));
            sOpen = 1;
        }
    }
    __syncthreads();
    uint64_t bound = sOpen ? (uint64_t)sFront : (1ull << 32);
    if (tid < np) { sTake[tid] = rb_count_below(dl, cnt, bound); atomicAdd(&sTotal, sTake[tid]); }
    __syncthreads();
    if (sTotal > RB_MAX_ENTRIES) {
        // ---- the largest ordered distance t with "entries at or below t" within the capacity; the frontier comes down to t + 1
        uint32_t t = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = t | (1u << bit);
            __syncthreads();
            if (tid == 0) sTotal = 0;
            __syncthreads();
            if (tid < np) {
                const uint64_t cb = (uint64_t)cand + 1 < bound ? (uint64_t)cand + 1 : bound;
                atomicAdd(&sTotal, rb_count_below(dl, cnt, cb));
            }
            __syncthreads();
            if (sTotal <= RB_MAX_ENTRIES) t = cand;
        }
        __syncthreads();
        bound = (uint64_t)t + 1 < bound ? (uint64_t)t + 1 : bound;
        if (tid < np) sTake[tid] = rb_count_below(dl, cnt, bound);
        if (tid == 0) sOpen = 1;                                           // the walk was cut
        __syncthreads();
    }
    if (tid == 0) {
        uint32_t at = 0;
        for (uint32_t i = 0; i < np; ++i) { sStart[i] = at; at += sTake[i]; }
        sStart[np] = at;
    }
    __syncthreads();
    const uint32_t total = sStart[np] < RB_MAX_ENTRIES ? sStart[np] : RB_MAX_ENTRIES;
    uint32_t P = 2;
    while (P < total) P <<= 1;
    // ---- gather
    for (uint32_t i = 0; i < np; ++i) {
        const uint32_t n = sTake[i], at = sStart[i];
        const float* d = p.dists + (size_t)(l0 + i) * p.depth;
        const uint64_t* id = p.ids + (size_t)(l0 + i) * p.depth;
        for (uint32_t e = tid; e < n && at + e < RB_MAX_ENTRIES; e += RB_THREADS) {
            sD[at + e] = f32_to_ordered(d[e]); sId[at + e] = id[e]; sL[at + e] = (uint8_t)i;
        }
    }
    for (uint32_t e = total + tid; e < P; e += RB_THREADS) { sD[e] = 0xffffffffu; sId[e] = ~0ull; sL[e] = RB_DEAD; }
    __syncthreads();
    // ---- by (id, distance as the fold compares it, list): the first entry of an id is its dp, bits included
    rb_sort(sD, sId, sL, P, tid, [](uint32_t da, uint64_t ia, uint8_t la, uint32_t db, uint64_t ib, uint8_t lb) {
        const bool xa = la == RB_DEAD, xb = lb == RB_DEAD;
        if (xa != xb) return xb;
        if (ia != ib) return ia < ib;
        const uint32_t ca = rb_canon(da), cb = rb_canon(db);
        if (ca != cb) return ca < cb;
        return la < lb;
    });
    // (a thread reads its left neighbour before anybody rewrites a list byte)
    bool drop[RB_MAX_ENTRIES / RB_THREADS];
#pragma unroll
    for (uint32_t u = 0; u < RB_MAX_ENTRIES / RB_THREADS; ++u) {
        const uint32_t e = u * RB_THREADS + tid;
        drop[u] = false;
        if (e < total) {
            const uint64_t id = sId[e];
            bool d = e > 0 && sId[e - 1] == id;
            for (uint32_t x = 0; x < m; ++x) d = d || id == sSet[x];
            drop[u] = d;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < RB_MAX_ENTRIES / RB_THREADS; ++u)
        if (drop[u]) sL[u * RB_THREADS + tid] = RB_DEAD;
    __syncthreads();
    // ---- by (ordered distance, id), the dropped entries behind
    rb_sort(sD, sId, sL, P, tid, [](uint32_t da, uint64_t ia, uint8_t la, uint32_t db, uint64_t ib, uint8_t lb) {
        const bool xa = la == RB_DEAD, xb = lb == RB_DEAD;
        if (xa != xb) return xb;
        if (da != db) return da < db;
        return ia < ib;
    });
    // the rows of the walk: the entries in front of the first dropped one
    uint32_t lo = 0, hi = total;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sL[mid] != RB_DEAD) lo = mid + 1; else hi = mid;
    }
    const uint32_t cap = p.cand_stride < RB_MAX_ROWS ? p.cand_stride : RB_MAX_ROWS;
    const uint32_t rows = lo < cap ? lo : cap;
    for (uint32_t e = tid; e < rows; e += RB_THREADS) {
        p.cand_ids[(size_t)j * p.cand_stride + e] = sId[e];
        p.cand_dists[(size_t)j * p.cand_stride + e] = ordered_to_f32(sD[e]);
    }
    if (tid == 0) { p.cand_cnt[j] = rows; p.open[j] = (sOpen || lo > cap) ? 1u : 0u; }
}

void launch_rb_merge(const RbMergeParams& p, uint32_t n_req, hipStream_t s) {
    if (!n_req) return;
    hipLaunchKernelGGL(rb_merge_kernel, dim3(n_req), dim3(RB_THREADS), 0, s, p);
}

// ---------------------------------------------------------------------------------------------
// the veto
// ---------------------------------------------------------------------------------------------
// the live device row that holds `id`: binary search in id order, then along the rows of that id
__device__ __forceinline__ uint32_t rb_row_of(const RbVetoParams& p, uint64_t id) {
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

__global__ __launch_bounds__(RB_THREADS) void rb_veto_kernel(RbVetoParams p) {
    __shared__ uint32_t sNeg[RECOMMEND_MAX_EXAMPLES + 8];
    __shared__ uint32_t sWave[RB_WAVES];
    const uint32_t j = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t b = p.sel ? p.sel[j] : j;
    const uint32_t o0 = p.R.offs[b], m0 = p.R.offs[b + 1] - o0;
    const uint32_t m = m0 < RECOMMEND_MAX_EXAMPLES ? m0 : RECOMMEND_MAX_EXAMPLES;
    const uint32_t np = p.R.n_pos[b] < m ? p.R.n_pos[b] : m, nn = m - np;
    const uint32_t kb = p.R.ks[b] < p.kout ? p.R.ks[b] : p.kout;
    const uint32_t count = p.cand_cnt[j] < p.cand_stride ? p.cand_cnt[j] : p.cand_stride;
    if (tid < RECOMMEND_MAX_EXAMPLES + 8) {
        uint32_t r = tid < nn ? p.R.rows[o0 + np + tid] : 0u;
        sNeg[tid] = r < p.n_rows ? r : 0u;                                 // (the host resolved every example: never outside the store)
    }
    __syncthreads();
    const uint64_t* ids = p.cand_ids + (size_t)j * p.cand_stride;
    const float* dps = p.cand_dists + (size_t)j * p.cand_stride;
    uint64_t* oi = p.out_ids + (size_t)b * p.kout;
    float* od = p.out_dists + (size_t)b * p.kout;
    float* on = p.out_neg + (size_t)b * p.kout;
    uint32_t kept = 0;                                                     // the same in every lane
    for (uint32_t base = 0; base < count && kept < kb; base += RB_THREADS) {
        const uint32_t i = base + tid;
        uint64_t id = 0;
        float dp = 0.0f, dn = RB_INF;
        uint32_t row = NO_ROW;
        if (i < count) {
            id = ids[i]; dp = dps[i];
            row = rb_row_of(p, id);
            if (row == NO_ROW) atomicOr(p.status, 2u);
        }
        bool keep = row != NO_ROW;
        if (keep && nn) {
            const float* x = p.rows + (size_t)row * p.ld;
            const float xn = p.nd[row];
            for (uint32_t c = 0; c < nn; c += 8) {
                const uint32_t nthis = nn - c < 8 ? nn - c : 8;
                uint32_t q8[8];
                rb_rows8(sNeg + c, nthis, q8);
                float s[8];
                fold_multi<8>(p.metric, x, p.dim, p.rows, p.ld, q8, nthis, s);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (u < (int)nthis) {
                        const float d = distance_from_fold(p.metric, s[u], p.nd[q8[u]], xn);
                        keep = keep && dp < d;                             // a tie or a NaN is a veto
                        if (c + u == 0 || d < dn) dn = d;
                    }
                }
            }
        }
        const unsigned long long kbits = __ballot(keep);
        if (lane == 0) sWave[wave] = (uint32_t)__popcll(kbits);
        __syncthreads();
        uint32_t before = kept, total = 0;
        for (uint32_t w = 0; w < RB_WAVES; ++w) {
            if (w < wave) before += sWave[w];
            total += sWave[w];
        }
        const uint32_t pos = before + (uint32_t)__popcll(kbits & ((1ull << lane) - 1ull));
        if (keep && pos < kb) { oi[pos] = id; od[pos] = dp; on[pos] = dn; }
        kept += total;
        __syncthreads();                                                   // sWave is rewritten by the next chunk
    }
    if (tid == 0) {
        p.out_counts[b] = kept < kb ? kept : kb;
        if (p.answered) p.answered[j] = (kept >= kb || !(p.open && p.open[j])) ? 1u : 0u;
    }
}

void launch_rb_veto(const RbVetoParams& p, uint32_t n_req, hipStream_t s) {
    if (!n_req) return;
    hipLaunchKernelGGL(rb_veto_kernel, dim3(n_req), dim3(RB_THREADS), 0, s, p);
}

}  // namespace vdb
