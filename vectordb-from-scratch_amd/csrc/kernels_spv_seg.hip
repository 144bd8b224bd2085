// kernels_spv_seg.hip -- the SEGMENTED inverted walk of the sparse-vector index (include/vdb_flat.h vdb_spv_set_segmented, DESIGN.md
// 4.20.2): many workgroups per query, for requests of a few queries, and no accumulator traffic outside LDS.
//
// The rows are cut into segments of R = 2^seg_shift consecutive CSR rows and the inverted file is ordered by (index, segment):
// sub_ptr[index * segs + segment] starts that segment's slice of the index's posting list (kernels_spv.hip builds it with the keyed
// histogram and scatter; the scan over the vocab * segs keys is here, many workgroups wide).
//
//   score   ONE workgroup of 1024 threads per (segment, query).  The segment's R accumulators live in LDS, filled with the
//           "untouched" pattern.  The query's table holds the SLICE (value, start, length) of every dimension; a workgroup whose
//           slices are all empty writes count 0 and leaves.  The fold is that of kernels_spv.hip -- dimensions ascending, threads
//           striding over the slice, load - add - store on acc[row - segment * R], a barrier between dimensions -- so every row
//           receives its products in ascending index order: the sequential f32 fold of the definition.  The emit is a linear pass
//           over the LDS accumulators, 1024 rows a round: no second walk and no atomics on the accumulators.  A touched row tests
//           the live bit and the id mask and offers (-score, id rank) to the select of kernels_spv_select.h; the workgroup writes
//           its min(k, found) smallest keys to part[query][segment][.].
//   merge   one workgroup per query streams the segs * kout partial slots through the same select.  Keys are unique (the id rank
//           is), so the k smallest of the union are the k smallest of everything: exact.  It writes ids, distances and counts as
//           the one-workgroup walk does.
// Compiled like kernels_spv.hip: no packed-f32 instructions, -ffp-contract=off.
#include "kernels.h"
#include "kernels_spv.h"
#include "kernels_spv_select.h"

namespace vdb {

namespace {

constexpr uint32_t SCAN_ITEMS = SPV_SEG_SCAN_TILE / SPV_THREADS;     // consecutive keys of one thread

__device__ inline bool live_row(const uint32_t* live, uint32_t row) { return (live[row >> 5] >> (row & 31)) & 1u; }

// ---- the scan over the keys: tile sums, their scan (spv_scan_kernel of kernels_spv.hip, one workgroup), then every tile on its own
__global__ __launch_bounds__(SPV_THREADS) void spv_seg_tile_sum_kernel(const uint32_t* __restrict__ counts, uint32_t n_keys,
                                                                       uint32_t* __restrict__ tile_sum) {
    __shared__ uint32_t s_wave[SPV_THREADS / 64];
    const uint32_t tid = threadIdx.x, base = blockIdx.x * SPV_SEG_SCAN_TILE;
    uint32_t sum = 0;
    for (uint32_t j = 0; j < SCAN_ITEMS; ++j) {
        const uint32_t i = base + j * SPV_THREADS + tid;
        if (i < n_keys) sum += counts[i];
    }
    for (uint32_t d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    if ((tid & 63) == 0) s_wave[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < SPV_THREADS / 64; ++w) all += s_wave[w];
        tile_sum[blockIdx.x] = all;
    }
}

// thread t owns the keys [base + 4 t, base + 4 t + 4): their sums are scanned in LDS (Hillis - Steele), tile_off[tile] comes on top
__global__ __launch_bounds__(SPV_THREADS) void spv_seg_scan_kernel(uint32_t* __restrict__ counts, uint32_t* __restrict__ sub_ptr, uint32_t n_keys,
                                                                   const uint32_t* __restrict__ tile_off, uint32_t n_tiles) {
    __shared__ uint32_t s_sum[SPV_THREADS];
    const uint32_t tid = threadIdx.x, i0 = blockIdx.x * SPV_SEG_SCAN_TILE + tid * SCAN_ITEMS;
    uint32_t c[SCAN_ITEMS], sum = 0;
    for (uint32_t j = 0; j < SCAN_ITEMS; ++j) {
        c[j] = i0 + j < n_keys ? counts[i0 + j] : 0;
        sum += c[j];
    }
    s_sum[tid] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < SPV_THREADS; off <<= 1) {
        const uint32_t v = tid >= off ? s_sum[tid - off] : 0;
        __syncthreads();
        s_sum[tid] += v;
        __syncthreads();
    }
    uint32_t run = tile_off[blockIdx.x] + s_sum[tid] - sum;
    for (uint32_t j = 0; j < SCAN_ITEMS; ++j)
        if (i0 + j < n_keys) {
            sub_ptr[i0 + j] = run;
            counts[i0 + j] = 0;
            run += c[j];
        }
    if (blockIdx.x == 0 && tid == 0) sub_ptr[n_keys] = tile_off[n_tiles];
}

__global__ __launch_bounds__(256) void spv_seg_lists_kernel(const uint32_t* __restrict__ sub_ptr, uint32_t segs, uint32_t vocab,
                                                            uint32_t* __restrict__ list_ptr) {
    for (uint32_t d = blockIdx.x * blockDim.x + threadIdx.x; d <= vocab; d += gridDim.x * blockDim.x) list_ptr[d] = sub_ptr[(size_t)d * segs];
}

// ---- scoring
__global__ __launch_bounds__(SPV_THREADS) void spv_seg_score_kernel(SpvSegParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_acc[];   // [R]: f32 bits, SPV_UNTOUCHED where nobody has added
    __shared__ float s_val[SPV_MAX_QUERY_NNZ];
    __shared__ uint32_t s_ptr[SPV_MAX_QUERY_NNZ], s_len[SPV_MAX_QUERY_NNZ];
    __shared__ uint64_t s_keys[SPV_SELECT_CAP];
    __shared__ uint64_t s_thr;
    __shared__ uint32_t s_cnt, s_offered, s_nan, s_any;
    const SpvSearchParams& q = p.q;
    const uint32_t tid = threadIdx.x, seg = blockIdx.x, y = blockIdx.y, b = q.q0 + y;
    const uint32_t R = 1u << p.seg_shift, r0 = seg << p.seg_shift, nr = min(R, q.n_rows - r0);   // seg < segs = ceil(n_rows / R)
    const uint32_t o0 = q.q_off[b], nt = q.q_off[b + 1] - o0;         // <= SPV_MAX_QUERY_NNZ (the host refuses longer queries)
    const size_t slot = (size_t)y * p.segs + seg;
    if (tid == 0) { s_cnt = 0; s_offered = 0; s_nan = 0; s_any = 0; s_thr = EMPTY_KEY; }
    __syncthreads();
    // the query's table: this segment's slice of every dimension's list.  A dimension at or above the vocabulary bound has none.
    if (tid < nt) {
        const uint32_t d = q.q_idx[o0 + tid];
        uint32_t a = 0, len = 0;
        if (d < q.vocab) {
            const uint32_t* sp = p.sub_ptr + (size_t)d * p.segs + seg;    // sp[1]: the next key, or the table's last word
            a = sp[0]; len = sp[1] - a;
        }
        s_val[tid] = q.q_val[o0 + tid]; s_ptr[tid] = a; s_len[tid] = len;
        if (len) s_any = 1;
    }
    for (uint32_t r = tid; r < R; r += SPV_THREADS) s_acc[r] = SPV_UNTOUCHED;
    __syncthreads();
    if (!s_any) {                                      // (uniform) no posting of the query lies in this segment
        if (tid == 0) p.part_cnt[slot] = 0;
        return;
    }

    // ---- fold: dimension after dimension, ascending
    for (uint32_t t = 0; t < nt; ++t) {
        const uint32_t len = s_len[t];
        if (len == 0) continue;                        // (uniform: nobody wrote, no barrier is owed)
        const SpvEntry* __restrict__ list = q.entries + s_ptr[t];
        const float qv = s_val[t];
        for (uint32_t i = tid; i < len; i += SPV_THREADS) {
            const SpvEntry e = list[i];
            const uint32_t r = e.row - r0;             // < R: the scatter keyed this entry by row >> seg_shift = seg
            const uint32_t old = s_acc[r];
            float s = (old == SPV_UNTOUCHED) ? 0.0f : __uint_as_float(old);
            const float prod = qv * e.val;
            s = s + prod;
            s_acc[r] = (s != s) ? 0x7fc00000u : __float_as_uint(s);   // (never SPV_UNTOUCHED, whatever payload came in)
        }
        __syncthreads();                               // the next dimension may meet the same rows
    }

    // ---- emit + select: the accumulators, 1024 rows a round
    const uint32_t kq = min(q.ks[b], min(q.kout, SPV_MAX_K));
    uint32_t bound = 0, offered = 0;                   // bound = s_cnt, the same in every thread
    for (uint32_t r = tid; r - tid < nr; r += SPV_THREADS) {
        if (bound + SPV_THREADS > SPV_SELECT_CAP) bound = spv_prune(s_keys, &s_cnt, &s_thr, kq);
        const uint32_t cur = r < nr ? s_acc[r] : SPV_UNTOUCHED;
        int pushed = 0;
        if (cur != SPV_UNTOUCHED) {
            const uint32_t row = r0 + r;
            bool ok = live_row(q.live, row);
            if (ok && q.id_mask) {
                const uint64_t id = q.row_ids[row];
                ok = id < q.mask_bits && ((q.id_mask[id >> 6] >> (id & 63)) & 1ull);
            }
            if (ok) {
                const float s = __uint_as_float(cur);
                ++offered;
                if (s != s) s_nan = 1;
                if (kq) {
                    const uint64_t key = make_key(-s, q.rank[row]);
                    pushed = key < s_thr;
                    spv_offer(s_keys, &s_cnt, &s_thr, key);   // below bound + SPV_THREADS <= SPV_SELECT_CAP
                }
            }
        }
        bound += (uint32_t)__syncthreads_count(pushed);
    }
    if (offered) atomicAdd(&s_offered, offered);
    const uint32_t cnt = spv_prune(s_keys, &s_cnt, &s_thr, kq);       // <= kq <= kout
    uint64_t* __restrict__ part = p.part + slot * q.kout;
    for (uint32_t i = tid; i < cnt; i += SPV_THREADS) part[i] = s_keys[i];
    if (tid == 0) {
        p.part_cnt[slot] = cnt;
        if (s_nan) atomicOr(q.status, (uint32_t)ST_NAN);
        unsigned long long walked = 0;
        for (uint32_t t = 0; t < nt; ++t) walked += s_len[t];
        atomicAdd(&q.counters[0], walked);
        atomicAdd(&q.counters[1], (unsigned long long)s_offered);
        atomicAdd(&q.counters[2], 1ull);
    }
}

// ---- merge
__global__ __launch_bounds__(SPV_THREADS) void spv_seg_merge_kernel(SpvSegParams p) {
    __shared__ uint64_t s_keys[SPV_SELECT_CAP];
    __shared__ uint64_t s_thr;
    __shared__ uint32_t s_cnt;
    const SpvSearchParams& q = p.q;
    const uint32_t tid = threadIdx.x, y = blockIdx.x, b = q.q0 + y;
    if (tid == 0) { s_cnt = 0; s_thr = EMPTY_KEY; }
    __syncthreads();
    const uint32_t kq = min(q.ks[b], min(q.kout, SPV_MAX_K));
    const uint64_t* __restrict__ part = p.part + (size_t)y * p.segs * q.kout;
    const uint32_t* __restrict__ part_cnt = p.part_cnt + (size_t)y * p.segs;
    const uint64_t total = (uint64_t)p.segs * q.kout;
    uint32_t bound = 0;
    for (uint64_t j = tid; j - tid < total; j += SPV_THREADS) {
        if (bound + SPV_THREADS > SPV_SELECT_CAP) bound = spv_prune(s_keys, &s_cnt, &s_thr, kq);
        int pushed = 0;
        if (j < total) {
            const uint64_t seg = j / q.kout;
            if ((uint32_t)(j - seg * q.kout) < part_cnt[seg]) {      // a slot its workgroup has written
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
        q.out_ids[(size_t)b * q.kout + i] = q.sorted_ids[(uint32_t)key];
        q.out_dists[(size_t)b * q.kout + i] = ordered_to_f32((uint32_t)(key >> 32));
    }
    if (tid == 0) q.out_counts[b] = cnt;
}

}  // namespace

void launch_spv_seg_scan(uint32_t* counts, uint32_t* sub_ptr, uint32_t n_keys, uint32_t* tiles, hipStream_t s) {
    const uint32_t n_tiles = (n_keys + SPV_SEG_SCAN_TILE - 1) / SPV_SEG_SCAN_TILE;
    hipLaunchKernelGGL(spv_seg_tile_sum_kernel, dim3(n_tiles), dim3(SPV_THREADS), 0, s, counts, n_keys, tiles);
    SpvBuildParams t{};                                // the tile sums' own scan: tiles[n_tiles + b] = the keys in front of tile b
    t.vocab = n_tiles; t.counts = tiles; t.list_ptr = tiles + n_tiles;
    launch_spv_scan(t, s);
    hipLaunchKernelGGL(spv_seg_scan_kernel, dim3(n_tiles), dim3(SPV_THREADS), 0, s, counts, sub_ptr, n_keys, tiles + n_tiles, n_tiles);
}

void launch_spv_seg_lists(const uint32_t* sub_ptr, uint32_t segs, uint32_t vocab, uint32_t* list_ptr, hipStream_t s) {
    hipLaunchKernelGGL(spv_seg_lists_kernel, dim3(std::min(vocab / 256 + 1, 4096u)), dim3(256), 0, s, sub_ptr, segs, vocab, list_ptr);
}

void launch_spv_seg_score(const SpvSegParams& p, uint32_t nq, hipStream_t s) {
    if (!nq) return;
    hipLaunchKernelGGL(spv_seg_score_kernel, dim3(p.segs, nq), dim3(SPV_THREADS), sizeof(uint32_t) << p.seg_shift, s, p);
}

void launch_spv_seg_merge(const SpvSegParams& p, uint32_t nq, hipStream_t s) {
    if (!nq) return;
    hipLaunchKernelGGL(spv_seg_merge_kernel, dim3(nq), dim3(SPV_THREADS), 0, s, p);
}

}  // namespace vdb
