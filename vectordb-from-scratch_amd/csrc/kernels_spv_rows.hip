// kernels_spv_rows.hip -- the ROW-MAJOR route of the sparse-vector index (include/vdb_flat.h "Sparse vectors"):
// document-at-a-time scoring for batches whose queries hold the frequent words, where the inverted walk of kernels_spv.hip makes
// every query walk a large part of the store.  The CSR rows the inverted file is built from are read once per tile of 64 queries.
//
// A pass (vdb_spv.cpp) serves up to `tiles` x 64 queries:
//   table   the pass's queries densified over the distinct dimensions U they hold: table[u][query], query-minor, SPV_ABSENT where
//           a query does not hold U[u]; dim_slot[U[u]] = u maps a stored index to its table row (SPV_NO_SLOT elsewhere).  One
//           further row, u = |U|, stays SPV_ABSENT: the row of every stored index no query holds, so the fold has no branch on it.
//   fold    ONE WAVE per (tile of 64 consecutive rows, tile of 64 queries); a LANE IS A QUERY and keeps its running sum in a
//           register.  The row tile's entries are one contiguous CSR range.  The wave takes it 64 entries at a time: lane i loads
//           entry i (index, value) and looks its table row up; entry j's row and value are then wave-uniform, so they are
//           broadcast from lane j's registers into scalar registers (v_readlane) rather than staged through LDS, and the 64 table
//           loads -- one coalesced 256-B read each, scalar base + lane -- are all issued before the first add.  The adds follow in
//           entry order, which inside a row is ascending index order: the sequential f32 fold of the definition.  At a row's end
//           the lane parks its sum (or SPV_UNTOUCHED) in the wave's own LDS tile [query][row]; at the tile's end the wave writes
//           the tile out transposed, 64 consecutive rows of one query as one 256-B run of acc[query][row].  No workgroup barrier:
//           the four waves of a workgroup share nothing but the L1 lines of the rows they read together.
//   emit    one workgroup per query streams acc[query][0, n_rows), 1024 rows a round, puts SPV_UNTOUCHED back, tests the id mask
//           and offers (-s, id rank) to the select of kernels_spv_select.h.
// Compiled like kernels_spv.hip: no packed-f32 instructions, -ffp-contract=off.
#include "kernels.h"
#include "kernels_spv.h"
#include "kernels_spv_select.h"

namespace vdb {

namespace {

constexpr uint32_t T = SPV_ROWS_TILE;
constexpr uint32_t FOLD_WAVES = 4;
constexpr uint32_t MAX_GRID = 1u << 20;
constexpr uint32_t QNAN = 0x7fc00000u;

__device__ inline bool live_row(const uint32_t* live, uint32_t row) { return (live[row >> 5] >> (row & 31)) & 1u; }
__device__ inline uint32_t lane_u32(uint32_t v, uint32_t lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane); }

__global__ __launch_bounds__(256) void spv_rows_slots_kernel(SpvRowsParams p, bool set) {
    for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < p.n_u; u += gridDim.x * blockDim.x)
        p.dim_slot[p.udims[u]] = set ? u : SPV_NO_SLOT;   // udims[u] < vocab <= the size of dim_slot (the host's table of the pass)
}

// one wave per query of the pass: its pairs into the query's column
__global__ __launch_bounds__(256) void spv_rows_table_kernel(SpvRowsParams p) {
    const uint32_t lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= p.nq) return;
    const size_t stride = (size_t)p.tiles * T;
    const uint32_t i1 = p.q_off[p.qa + q + 1];
    for (uint32_t i = p.q_off[p.qa + q] + lane; i < i1; i += 64) {
        const uint32_t slot = p.q_slot[i];                // < n_u, or SPV_NO_SLOT for an index at or above vocab
        if (slot == SPV_NO_SLOT) continue;
        const float v = p.q_val[i];
        p.table[slot * stride + q] = (v != v) ? QNAN : __float_as_uint(v);
    }
}

__global__ __launch_bounds__(FOLD_WAVES * 64) void spv_rows_fold_kernel(SpvRowsParams p) {
    __shared__ uint32_t s_tile[FOLD_WAVES][T * T];       // [query][(row + query) & 63]: both the parking and the read-out hit 64 banks
    const uint32_t lane = threadIdx.x & 63, w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t g = (uint64_t)blockIdx.x * FOLD_WAVES + w;
    const uint32_t n_rt = (p.n_rows + T - 1) / T;
    if (g >= (uint64_t)n_rt * p.tiles) return;
    const uint32_t rt = (uint32_t)(g / p.tiles), qt = (uint32_t)(g % p.tiles);
    const uint32_t r0 = rt * T, nr = min(T, p.n_rows - r0);
    const size_t stride = (size_t)p.tiles * T;
    const uint32_t* __restrict__ col = p.table + (size_t)qt * T + lane;
    uint32_t* tile = s_tile[w];

    const uint32_t my_end = p.row_ptr[r0 + min(lane, nr - 1) + 1];   // lane r: where row r0 + r ends
    const uint32_t e0 = p.row_ptr[r0], e1 = lane_u32(my_end, nr - 1);
    uint32_t row = 0, rend = lane_u32(my_end, 0);       // wave-uniform: the row being folded, and its end
    float s = 0.0f;
    bool touched = false;
    uint32_t steps = 0;
    unsigned long long total = 0;

    auto park = [&]() {
        uint32_t out = SPV_UNTOUCHED;
        if (live_row(p.live, r0 + row)) {                // a dead row is in no list: no candidate, and its steps do not count
            total += steps;
            if (touched) out = (s != s) ? QNAN : __float_as_uint(s);
        }
        tile[lane * T + ((row + lane) & (T - 1))] = out;
        s = 0.0f; touched = false; steps = 0;
        ++row;
        rend = lane_u32(my_end, min(row, T - 1));
    };

    for (uint32_t b = e0; b < e1; b += 64) {            // (e1 < 2^32 - 64 is not promised: the loop ends on b >= e1 or on wrap)
        const uint32_t e = b + lane;
        uint32_t u = p.n_u;
        float x = 0.0f;
        if (e >= b && e < e1) {
            x = p.val[e];
            u = min(p.dim_slot[p.idx[e]], p.n_u);        // idx[e] < vocab; no slot -> the ABSENT row
        }
        uint32_t q[64];
#pragma unroll
        for (uint32_t j = 0; j < 64; ++j) q[j] = col[lane_u32(u, j) * stride];
#pragma unroll
        for (uint32_t j = 0; j < 64; ++j) {
            const uint32_t ej = b + j;
            if (ej < b || ej >= e1) break;
            while (ej == rend) park();                   // ej < e1 = the end of row nr - 1: this stops at a row below nr
            const float xj = __uint_as_float(lane_u32(__float_as_uint(x), j));
            if (q[j] != SPV_ABSENT) {
                const float prod = __uint_as_float(q[j]) * xj;
                s = s + prod;
                touched = true;
                ++steps;
            }
        }
        if (b + 64 < b) break;
    }
    while (row < nr) park();

    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the tile is the wave's own: its LDS operations complete in order
    const uint32_t nqt = min(T, p.nq - qt * T);
    for (uint32_t y = 0; y < nqt; ++y) {
        const uint32_t v = lane < nr ? tile[y * T + ((lane + y) & (T - 1))] : SPV_UNTOUCHED;
        // acc is SPV_UNTOUCHED already: a run nobody touched is not written
        if (__ballot(v != SPV_UNTOUCHED) && lane < nr) reinterpret_cast<uint32_t*>(p.acc)[(size_t)(qt * T + y) * p.n_rows + r0 + lane] = v;
    }
    for (uint32_t d = 32; d > 0; d >>= 1) total += __shfl_xor(total, d);
    if (lane == 0 && total) atomicAdd(&p.counters[0], total);
}

__global__ __launch_bounds__(SPV_THREADS) void spv_rows_emit_kernel(SpvRowsParams p) {
    __shared__ uint64_t s_keys[SPV_SELECT_CAP];
    __shared__ uint64_t s_thr;
    __shared__ uint32_t s_cnt, s_offered, s_nan;
    const uint32_t tid = threadIdx.x, y = blockIdx.x, b = p.qa + y;
    if (tid == 0) { s_cnt = 0; s_offered = 0; s_nan = 0; s_thr = EMPTY_KEY; }
    __syncthreads();
    uint32_t* __restrict__ acc = reinterpret_cast<uint32_t*>(p.acc) + (size_t)y * p.n_rows;
    const uint32_t kq = min(p.ks[b], min(p.kout, SPV_MAX_K));
    uint32_t bound = 0, offered = 0;                    // bound = s_cnt, the same in every thread
    uint32_t cur = tid < p.n_rows ? acc[tid] : SPV_UNTOUCHED;
    for (uint64_t row = tid; row - tid < p.n_rows; row += SPV_THREADS) {
        if (bound + SPV_THREADS > SPV_SELECT_CAP) bound = spv_prune(s_keys, &s_cnt, &s_thr, kq);
        const uint32_t nxt = row + SPV_THREADS < p.n_rows ? acc[row + SPV_THREADS] : SPV_UNTOUCHED;   // in flight over this round
        int pushed = 0;
        if (cur != SPV_UNTOUCHED) {                     // a live row that shares an index with the query (row < n_rows)
            acc[row] = SPV_UNTOUCHED;                   // this workgroup owns the slot
            bool ok = true;
            if (p.id_mask) {
                const uint64_t id = p.row_ids[row];
                ok = id < p.mask_bits && ((p.id_mask[id >> 6] >> (id & 63)) & 1ull);
            }
            if (ok) {
                const float s = __uint_as_float(cur);
                ++offered;
                if (s != s) s_nan = 1;
                if (kq) {
                    const uint64_t key = make_key(-s, p.rank[row]);
                    pushed = key < s_thr;
                    spv_offer(s_keys, &s_cnt, &s_thr, key);   // below bound + SPV_THREADS <= SPV_SELECT_CAP
                }
            }
        }
        bound += (uint32_t)__syncthreads_count(pushed);
        cur = nxt;
    }
    if (offered) atomicAdd(&s_offered, offered);
    const uint32_t cnt = spv_prune(s_keys, &s_cnt, &s_thr, kq);
    for (uint32_t i = tid; i < cnt; i += SPV_THREADS) {
        const uint64_t key = s_keys[i];
        p.out_ids[(size_t)b * p.kout + i] = p.sorted_ids[(uint32_t)key];
        p.out_dists[(size_t)b * p.kout + i] = ordered_to_f32((uint32_t)(key >> 32));
    }
    if (tid == 0) {
        p.out_counts[b] = cnt;
        if (s_nan) atomicOr(p.status, (uint32_t)ST_NAN);
        atomicAdd(&p.counters[1], (unsigned long long)s_offered);
    }
}

}  // namespace

void launch_spv_rows_slots(const SpvRowsParams& p, bool set, hipStream_t s) {
    if (!p.n_u) return;
    hipLaunchKernelGGL(spv_rows_slots_kernel, dim3((p.n_u + 255) / 256), dim3(256), 0, s, p, set);
}

void launch_spv_rows_table(const SpvRowsParams& p, hipStream_t s) {
    launch_spv_fill(p.table, ((size_t)p.n_u + 1) * p.tiles * T, SPV_ABSENT, s);
    if (!p.nq) return;
    hipLaunchKernelGGL(spv_rows_table_kernel, dim3((p.nq + 3) / 4), dim3(256), 0, s, p);
}

void launch_spv_rows_fold(const SpvRowsParams& p, hipStream_t s) {
    const uint64_t waves = (uint64_t)((p.n_rows + T - 1) / T) * p.tiles;
    if (!waves) return;
    hipLaunchKernelGGL(spv_rows_fold_kernel, dim3((uint32_t)((waves + FOLD_WAVES - 1) / FOLD_WAVES)), dim3(FOLD_WAVES * 64), 0, s, p);
}

void launch_spv_rows_emit(const SpvRowsParams& p, hipStream_t s) {
    if (!p.nq) return;
    hipLaunchKernelGGL(spv_rows_emit_kernel, dim3(p.nq), dim3(SPV_THREADS), 0, s, p);
}

}  // namespace vdb
