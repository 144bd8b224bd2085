// kernels_spv.hip -- the sparse-VECTOR index on the device (include/vdb_flat.h "Sparse vectors").
//
// Building the inverted file (after a mutation): a histogram of the live rows' indices, an exclusive scan into list_ptr, a
// scatter of (row, value) postings.  A row occurs at most once per list and the position inside a list carries no meaning, so the
// scatter takes its slots with an atomic add on a per-list cursor.
//
// Searching: ONE workgroup of 1024 threads per query.
//   fold    the query's dimensions are walked in ASCENDING order; inside one dimension the threads stride over its posting list
//           and do a plain load - add - store on acc[row] (a row is in the list once: no two threads meet); a barrier separates
//           the dimensions.  Row x therefore receives its products q_d * x_d one dimension after the other, ascending in d: the
//           sequential f32 fold of the definition, with no per-row merge of two index lists.
//   emit    the same lists are walked again.  The thread whose atomic exchange takes a score OUT of acc[row] (and leaves the
//           "untouched" pattern there) owns the row: it tests the live bit and the id mask and offers (-score, id rank) to the
//           select.  Every touched row is offered once, and the accumulators are clean again without a memset.
//   select  an LDS buffer of SPV_SELECT_CAP 64-bit keys.  A round of the emit walk adds at most 1024 keys; before a round that
//           might not fit, the buffer is sorted (bitonic) and cut to its k smallest, and the k-th becomes a threshold later
//           offers must beat.  The k smallest of everything offered so far are always in the buffer: exact for any number of
//           candidates.
// Compiled without packed-f32 instructions (Makefile); -ffp-contract=off keeps the multiply and the add apart.
#include "kernels.h"
#include "kernels_spv.h"
#include "kernels_spv_select.h"

namespace vdb {

namespace {

constexpr uint32_t WAVE = 64;
constexpr uint32_t BUILD_THREADS = 256;
constexpr uint32_t MAX_GRID = 1u << 20;

__global__ __launch_bounds__(256) void spv_fill_kernel(uint32_t* __restrict__ words, size_t n, uint32_t value) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) words[i] = value;
}

__device__ inline bool live_row(const uint32_t* live, uint32_t row) { return (live[row >> 5] >> (row & 31)) & 1u; }
// the list an entry goes to: its index, or (index, segment of the row) in a segmented file
__device__ inline uint32_t list_key(const SpvBuildParams& p, uint32_t d, uint32_t row) {
    return p.segs > 1 ? d * p.segs + (row >> p.seg_shift) : d;
}

// one wave per row: its lanes stride over the row's entries
__global__ __launch_bounds__(BUILD_THREADS) void spv_histogram_kernel(SpvBuildParams p) {
    const uint32_t lane = threadIdx.x & (WAVE - 1), waves = gridDim.x * (BUILD_THREADS / WAVE);
    for (uint32_t row = blockIdx.x * (BUILD_THREADS / WAVE) + threadIdx.x / WAVE; row < p.n_rows; row += waves) {
        if (!live_row(p.live, row)) continue;
        const uint32_t e1 = p.row_ptr[row + 1];
        for (uint32_t e = p.row_ptr[row] + lane; e < e1; e += WAVE) atomicAdd(&p.counts[list_key(p, p.idx[e], row)], 1u);
    }
}

// list_ptr = exclusive scan of counts, by ONE workgroup: thread t owns a contiguous chunk, the chunk sums are scanned in LDS.
// counts is left zero: the scatter's cursors.
__global__ __launch_bounds__(SPV_THREADS) void spv_scan_kernel(SpvBuildParams p) {
    __shared__ uint32_t s_sum[SPV_THREADS];
    const uint32_t tid = threadIdx.x;
    const uint32_t chunk = (p.vocab + SPV_THREADS - 1) / SPV_THREADS;
    const uint32_t a = min(tid * chunk, p.vocab), b = min(a + chunk, p.vocab);
    uint32_t sum = 0;
    for (uint32_t d = a; d < b; ++d) sum += p.counts[d];
    s_sum[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (uint32_t t = 0; t < SPV_THREADS; ++t) { const uint32_t c = s_sum[t]; s_sum[t] = run; run += c; }
        p.list_ptr[p.vocab] = run;
    }
    __syncthreads();
    uint32_t run = s_sum[tid];
    for (uint32_t d = a; d < b; ++d) {
        const uint32_t c = p.counts[d];
        p.list_ptr[d] = run;
        p.counts[d] = 0;
        run += c;
    }
}

__global__ __launch_bounds__(BUILD_THREADS) void spv_scatter_kernel(SpvBuildParams p) {
    const uint32_t lane = threadIdx.x & (WAVE - 1), waves = gridDim.x * (BUILD_THREADS / WAVE);
    for (uint32_t row = blockIdx.x * (BUILD_THREADS / WAVE) + threadIdx.x / WAVE; row < p.n_rows; row += waves) {
        if (!live_row(p.live, row)) continue;
        const uint32_t e1 = p.row_ptr[row + 1];
        for (uint32_t e = p.row_ptr[row] + lane; e < e1; e += WAVE) {
            const uint32_t d = list_key(p, p.idx[e], row);
            // below list_ptr[d + 1]: the histogram counted exactly the entries that come here
            const uint32_t slot = p.list_ptr[d] + atomicAdd(&p.counts[d], 1u);
            p.entries[slot] = SpvEntry{row, p.val[e]};
        }
    }
}

__global__ __launch_bounds__(SPV_THREADS) void spv_search_kernel(SpvSearchParams p) {
    __shared__ float s_val[SPV_MAX_QUERY_NNZ];
    __shared__ uint32_t s_ptr[SPV_MAX_QUERY_NNZ], s_len[SPV_MAX_QUERY_NNZ];
    __shared__ uint64_t s_keys[SPV_SELECT_CAP];
    __shared__ uint64_t s_thr;
    __shared__ uint32_t s_cnt, s_offered, s_nan;
    const uint32_t tid = threadIdx.x, y = blockIdx.x, b = p.q0 + y;
    const uint32_t o0 = p.q_off[b], nt = p.q_off[b + 1] - o0;   // <= SPV_MAX_QUERY_NNZ (the host refuses longer queries)
    // the query's table: (value, list start, list length) per dimension, through LDS.  A dimension at or above the vocabulary
    // bound has no list.
    if (tid < nt) {
        const uint32_t d = p.q_idx[o0 + tid];
        uint32_t a = 0, len = 0;
        if (d < p.vocab) { a = p.list_ptr[d]; len = p.list_ptr[d + 1] - a; }
        s_val[tid] = p.q_val[o0 + tid]; s_ptr[tid] = a; s_len[tid] = len;
    }
    if (tid == 0) { s_cnt = 0; s_offered = 0; s_nan = 0; s_thr = EMPTY_KEY; }
    __syncthreads();
    float* __restrict__ acc = p.acc + (size_t)y * p.n_rows;

    // ---- fold: dimension after dimension, ascending
    for (uint32_t t = 0; t < nt; ++t) {
        const uint32_t len = s_len[t];
        if (len == 0) continue;
        const SpvEntry* __restrict__ list = p.entries + s_ptr[t];
        const float qv = s_val[t];
        for (uint32_t i = tid; i < len; i += SPV_THREADS) {
            const SpvEntry e = list[i];
            const float old = acc[e.row];
            float s = (__float_as_uint(old) == SPV_UNTOUCHED) ? 0.0f : old;
            const float prod = qv * e.val;
            s = s + prod;
            if (s != s) s = __uint_as_float(0x7fc00000u);   // (never SPV_UNTOUCHED, whatever payload came in)
            acc[e.row] = s;
        }
        __syncthreads();                               // the next dimension may meet the same rows
    }

    // ---- emit + select
    const uint32_t kq = min(p.ks[b], min(p.kout, SPV_MAX_K));
    uint32_t bound = 0;                                // >= s_cnt, the same in every thread
    for (uint32_t t = 0; t < nt; ++t) {
        const uint32_t len = s_len[t];
        const SpvEntry* __restrict__ list = p.entries + s_ptr[t];
        for (uint32_t i0 = 0; i0 < len; i0 += SPV_THREADS) {
            const uint32_t m = min(SPV_THREADS, len - i0);
            if (bound + m > SPV_SELECT_CAP) bound = spv_prune(s_keys, &s_cnt, &s_thr, kq);
            bound += m;
            if (tid < m) {
                const uint32_t row = list[i0 + tid].row;
                const uint32_t bits = atomicExch(reinterpret_cast<uint32_t*>(acc + row), SPV_UNTOUCHED);
                if (bits != SPV_UNTOUCHED) {           // this thread took the row's score: nobody else will
                    bool ok = live_row(p.live, row);
                    if (ok && p.id_mask) {
                        const uint64_t id = p.row_ids[row];
                        ok = id < p.mask_bits && ((p.id_mask[id >> 6] >> (id & 63)) & 1ull);
                    }
                    if (ok) {
                        const float s = __uint_as_float(bits);
                        atomicAdd(&s_offered, 1u);
                        if (s != s) s_nan = 1;
                        if (kq) {
                            const uint64_t key = make_key(-s, p.rank[row]);
                            spv_offer(s_keys, &s_cnt, &s_thr, key);            // below bound <= SPV_SELECT_CAP
                        }
                    }
                }
            }
        }
    }
    const uint32_t cnt = spv_prune(s_keys, &s_cnt, &s_thr, kq);
    for (uint32_t i = tid; i < cnt; i += SPV_THREADS) {
        const uint64_t key = s_keys[i];
        p.out_ids[(size_t)b * p.kout + i] = p.sorted_ids[(uint32_t)key];
        p.out_dists[(size_t)b * p.kout + i] = ordered_to_f32((uint32_t)(key >> 32));
    }
    if (tid == 0) {
        p.out_counts[b] = cnt;
        if (s_nan) atomicOr(p.status, (uint32_t)ST_NAN);
        unsigned long long walked = 0;
        for (uint32_t t = 0; t < nt; ++t) walked += s_len[t];
        atomicAdd(&p.counters[0], walked);
        atomicAdd(&p.counters[1], (unsigned long long)s_offered);
    }
}

uint32_t build_grid(uint32_t n_rows) {
    const uint32_t per = BUILD_THREADS / WAVE;
    return (uint32_t)std::min<uint64_t>(((uint64_t)n_rows + per - 1) / per, MAX_GRID);
}

}  // namespace

void launch_spv_fill(uint32_t* words, size_t n, uint32_t value, hipStream_t s) {
    if (!n) return;
    const uint32_t grid = (uint32_t)std::min<size_t>((n + 255) / 256, MAX_GRID);
    hipLaunchKernelGGL(spv_fill_kernel, dim3(grid), dim3(256), 0, s, words, n, value);
}

void launch_spv_histogram(const SpvBuildParams& p, hipStream_t s) {
    if (!p.n_rows) return;
    hipLaunchKernelGGL(spv_histogram_kernel, dim3(build_grid(p.n_rows)), dim3(BUILD_THREADS), 0, s, p);
}

void launch_spv_scan(const SpvBuildParams& p, hipStream_t s) {
    hipLaunchKernelGGL(spv_scan_kernel, dim3(1), dim3(SPV_THREADS), 0, s, p);
}

void launch_spv_scatter(const SpvBuildParams& p, hipStream_t s) {
    if (!p.n_rows) return;
    hipLaunchKernelGGL(spv_scatter_kernel, dim3(build_grid(p.n_rows)), dim3(BUILD_THREADS), 0, s, p);
}

void launch_spv_search(const SpvSearchParams& p, uint32_t nq, hipStream_t s) {
    if (!nq) return;
    hipLaunchKernelGGL(spv_search_kernel, dim3(nq), dim3(SPV_THREADS), 0, s, p);
}

}  // namespace vdb
