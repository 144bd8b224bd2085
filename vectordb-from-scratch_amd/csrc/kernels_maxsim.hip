// kernels_maxsim.hip -- the device steps of late-interaction search (vdb_flat_search_batch_maxsim, include/vdb_flat.h
// "LATE-INTERACTION SEARCH"): query b is T_b token vectors, a document is a code c >= 0 of a metadata column with
// at least one eligible row, and
//   m(t, c)  = the minimum, by the ordered-f32 comparison, of d(t, x) over the eligible rows x with code c,
//   score(c) = ((m(t_1, c) + m(t_2, c)) + m(t_3, c)) + ...          an f32 left fold that STARTS from the first term.
// Three kernels:
//   - maxsim_scan_kernel: one thread per row, grid.y = the queries of the chunk.  The row is read ONCE per query, 16 floats at a
//     time, and folded against all T_b tokens in that pass: up to 32 independent accumulator chains in VGPRs (fold_multi<32>, the
//     reference's operation order per chain), the token elements through wave-uniform scalar loads.  The T distances become
//     ordered integers and go into table[query][code][token] by atomicMin -- the minimum of integers is exact and order-free, so
//     the table does not depend on how the atomics land.  In front of the atomics a wave combines neighbouring lanes that hold
//     the same code: a segmented prefix minimum over runs of equal codes (log steps of __shfl_up, each lane bounded by the first
//     lane of its run), after which the LAST lane of a run holds the run's minima and is the only one that issues atomics.  A
//     document of 16 adjacent rows then costs one atomic per token, not 16; a store of one-row documents skips the step.  The
//     table is the same with or without it.  Lanes without an eligible row read no row; they stay in the wave for the shuffles.
//     maxsim_scan_marked_kernel is the same body for the screened route (kernels_maxsim_screen.hip): a row takes part only when
//     its code's bit is set in the query's candidate bitmap, and the rows folded are counted for every query.
//   - maxsim_fold_kernel: one thread per (query, code).  An entry whose token 0 is untouched (all ones: no distance maps there,
//     a NaN raises ST_NAN in the scan) is no document and gives EMPTY_KEY; else the T minima are folded left in token order and
//     the key is ordered(score) << 32 | code: ascending keys are the answer's order, ties go to the lower code.
//   - maxsim_emit_kernel: the first min(k_b, count) keys of the select, taken apart into code and score.
// Everything read from device memory is checked before an address is formed from it: an id against the column's length, a code
// against n_codes (status[3] bit 0 otherwise), a count against its stride.  Plain C++ throughout, no packed-f32 operations (the
// file is built with them switched off); gfx950 only.
#include "kernels_exact.h"

#pragma clang fp contract(off)

namespace vdb {

constexpr uint32_t MS_THREADS = 256;
constexpr uint32_t MS_NO_CODE = 0xffffffffu;                               // a lane without an eligible row of a document
constexpr uint32_t MS_UNTOUCHED = 0xffffffffu;                             // a table entry no row has reached

__device__ __forceinline__ uint32_t ms_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// ---------------------------------------------------------------------------------------------
// the row scan
// ---------------------------------------------------------------------------------------------
// (CAND: the candidate instance of the screened route -- a row takes part only when its code's bit is set in the query's bitmap)
template <bool CAND>
__device__ __forceinline__ void maxsim_scan_body(const MaxsimScanParams& p, const uint32_t* marked, uint32_t mark_words) {
    const uint32_t row = blockIdx.x * MS_THREADS + threadIdx.x, lane = threadIdx.x & 63u, y = blockIdx.y;
    const uint32_t t0 = ms_uniform(p.offs[p.q0 + y]);
    const uint32_t T0 = ms_uniform(p.offs[p.q0 + y + 1]) - t0;
    const uint32_t T = T0 < MAXSIM_MAX_TOKENS ? T0 : MAXSIM_MAX_TOKENS;    // (the host refused a longer query)

    // ---- the row's document: live, admitted, a code in [0, n_codes)
    uint32_t code = MS_NO_CODE;
    bool beyond = false;                                                   // a code at or above n_codes
    if (row < p.n_rows && (p.rowmask ? ((p.rowmask[row >> 5] >> (row & 31)) & 1u) : true)) {
        const uint64_t id = p.row_ids[row];
        if (id < p.codes_len) {
            const int32_t c = p.codes[id];
            if (c >= 0) {
                if ((uint32_t)c < p.n_codes) code = (uint32_t)c;
                else beyond = true;
            }
        }
    }
    if (CAND && code != MS_NO_CODE && !((marked[(size_t)y * mark_words + (code >> 5)] >> (code & 31u)) & 1u)) code = MS_NO_CODE;
    const bool mine = code != MS_NO_CODE;
    const unsigned long long active = __ballot(mine);
    // (every atomic of this kernel stands BEHIND the fold: a store in front of it would make the token loads vector loads)
    if (!active) {                                                         // (the whole wave: nothing below runs with a lane missing)
        if (beyond) atomicOr(p.status + 3, 1u);
        return;
    }

    // ---- T distances from one pass over the row
    uint32_t o[MAXSIM_MAX_TOKENS];
    bool nan = false;
#pragma unroll
    for (int j = 0; j < (int)MAXSIM_MAX_TOKENS; ++j) o[j] = MS_UNTOUCHED;
    if (mine) {
        // (token j is row j of the query's block: constant indices, so every token address is a uniform expression)
        const uint32_t tok[MAXSIM_MAX_TOKENS] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15,
                                                 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31};
        float s[MAXSIM_MAX_TOKENS];
        fold_multi<(int)MAXSIM_MAX_TOKENS>(p.metric, p.rows + (size_t)row * p.ld, p.dim, p.qp + (size_t)t0 * p.ld, p.ld, tok, T, s);
        const float xn = p.nd[row];
#pragma unroll
        for (int j = 0; j < (int)MAXSIM_MAX_TOKENS; ++j) {
            if (j < (int)T) {                                              // wave-uniform
                const float d = distance_from_fold(p.metric, s[j], p.qnorm[t0 + j], xn);
                nan = nan || d != d;
                o[j] = f32_to_ordered(d);
            }
        }
    }
    if (nan) atomicOr(p.status, ST_NAN);
    if (beyond) atomicOr(p.status + 3, 1u);
    if ((CAND || y == 0) && lane == 0) atomicAdd(p.rows_scanned, (unsigned long long)__popcll(active));

    // ---- one set of minima per run of equal codes: a segmented prefix minimum, lane by lane towards the run's last lane
    const uint32_t before = __shfl_up(code, 1u);
    const unsigned long long starts = __ballot(lane == 0 || before != code);
    const uint32_t head = 63u - (uint32_t)__clzll(starts & (~0ull >> (63u - lane)));   // the first lane of this lane's run
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const bool reach = lane >= head + off;                             // lane - off lies inside the run
        if (!__ballot(reach)) break;                                       // (uniform: no run is longer than off)
#pragma unroll
        for (int j = 0; j < (int)MAXSIM_MAX_TOKENS; ++j) {
            if (j < (int)T) {
                const uint32_t v = __shfl_up(o[j], off);
                if (reach && v < o[j]) o[j] = v;
            }
        }
    }
    const bool last = lane == 63 || ((starts >> (lane + 1)) & 1ull);
    if (mine && last) {
        uint32_t* e = p.table + ((size_t)y * p.n_codes + code) * MAXSIM_MAX_TOKENS;
#pragma unroll
        for (int j = 0; j < (int)MAXSIM_MAX_TOKENS; ++j)
            if (j < (int)T) atomicMin(e + j, o[j]);
    }
}

__global__ __launch_bounds__(MS_THREADS) void maxsim_scan_kernel(MaxsimScanParams p) { maxsim_scan_body<false>(p, nullptr, 0); }
__global__ __launch_bounds__(MS_THREADS) void maxsim_scan_marked_kernel(MaxsimScanParams p, const uint32_t* marked, uint32_t mark_words) {
    maxsim_scan_body<true>(p, marked, mark_words);
}

void launch_maxsim_scan_marked(const MaxsimScanParams& p, const uint32_t* marked, uint32_t mark_words, uint32_t n_queries, hipStream_t s) {
    if (!p.n_rows || !n_queries) return;
    hipLaunchKernelGGL(maxsim_scan_marked_kernel, dim3((p.n_rows + MS_THREADS - 1) / MS_THREADS, n_queries), dim3(MS_THREADS), 0, s, p,
                       marked, mark_words);
}

void launch_maxsim_scan(const MaxsimScanParams& p, uint32_t n_queries, hipStream_t s) {
    if (!p.n_rows || !n_queries) return;
    hipLaunchKernelGGL(maxsim_scan_kernel, dim3((p.n_rows + MS_THREADS - 1) / MS_THREADS, n_queries), dim3(MS_THREADS), 0, s, p);
}

// ---------------------------------------------------------------------------------------------
// the per-document fold into select keys
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MS_THREADS) void maxsim_fold_kernel(MaxsimFoldParams p) {
    const uint32_t c = blockIdx.x * MS_THREADS + threadIdx.x, y = blockIdx.y;
    const uint32_t t0 = ms_uniform(p.offs[p.q0 + y]);
    const uint32_t T0 = ms_uniform(p.offs[p.q0 + y + 1]) - t0;
    const uint32_t T = T0 < MAXSIM_MAX_TOKENS ? T0 : MAXSIM_MAX_TOKENS;
    bool doc = false;
    if (c < p.n_codes) {
        const uint32_t* e = p.table + ((size_t)y * p.n_codes + c) * MAXSIM_MAX_TOKENS;
        uint64_t key = EMPTY_KEY;
        const uint4 first = *reinterpret_cast<const uint4*>(e);
        if (first.x != MS_UNTOUCHED) {
            doc = true;
            float score = ordered_to_f32(first.x);                         // the fold starts FROM the first term: T = 1 keeps its bits
            const uint32_t w[3] = {first.y, first.z, first.w};
#pragma unroll
            for (int u = 0; u < 3; ++u)
                if (1 + u < (int)T) score = __fadd_rn(score, ordered_to_f32(w[u]));
            for (uint32_t j = 4; j < T; j += 4) {                          // (T is wave-uniform)
                const uint4 v = *reinterpret_cast<const uint4*>(e + j);
                const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (j + u < T) score = __fadd_rn(score, ordered_to_f32(x[u]));
            }
            if (score != score) atomicOr(p.status, ST_NAN);                // +inf and -inf met
            key = ((uint64_t)f32_to_ordered(score) << 32) | c;
        }
        p.keys[(size_t)y * p.n_codes + c] = key;
    }
    const unsigned long long docs = __ballot(doc);
    if (docs && (threadIdx.x & 63u) == 0) atomicAdd(p.docs_seen, (unsigned long long)__popcll(docs));
}

void launch_maxsim_fold(const MaxsimFoldParams& p, uint32_t n_queries, hipStream_t s) {
    if (!p.n_codes || !n_queries) return;
    hipLaunchKernelGGL(maxsim_fold_kernel, dim3((p.n_codes + MS_THREADS - 1) / MS_THREADS, n_queries), dim3(MS_THREADS), 0, s, p);
}

// ---------------------------------------------------------------------------------------------
// the answer
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MS_THREADS) void maxsim_emit_kernel(MaxsimEmitParams p) {
    const uint32_t y = blockIdx.x, b = p.q0 + y;
    const uint32_t kb = p.ks[b] < p.kout ? p.ks[b] : p.kout;
    const uint32_t have = p.key_cnt[y] < p.key_stride ? p.key_cnt[y] : p.key_stride;
    const uint32_t count = have < kb ? have : kb;
    const uint64_t* keys = p.keys + (size_t)y * p.key_stride;
    for (uint32_t i = threadIdx.x; i < count; i += MS_THREADS) {
        const uint64_t key = keys[i];
        const size_t o = (size_t)b * p.kout + i;
        if (key == EMPTY_KEY) atomicOr(p.status + 3, 2u);                  // (an empty key among the first count: never)
        p.out_codes[o] = key == EMPTY_KEY ? -1 : (int32_t)(uint32_t)key;
        p.out_scores[o] = key == EMPTY_KEY ? __uint_as_float(0x7fc00000u) : ordered_to_f32((uint32_t)(key >> 32));
    }
    if (threadIdx.x == 0) p.out_counts[b] = count;
}

void launch_maxsim_emit(const MaxsimEmitParams& p, uint32_t n_queries, hipStream_t s) {
    if (!n_queries) return;
    hipLaunchKernelGGL(maxsim_emit_kernel, dim3(n_queries), dim3(MS_THREADS), 0, s, p);
}

}  // namespace vdb
