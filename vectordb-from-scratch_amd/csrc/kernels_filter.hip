// kernels_filter.hip -- a MetadataFilter (src/storage.rs:45-71) evaluated for every internal id at once, on the device, from the
// metadata columns the store keeps resident (vdb_meta.cpp).  The output is the id bitmask the searches take as
// `d_id_mask`: bit i of word i >> 6 = id i is present and matches.
//   - one lane per id, one wave per 64-bit word: the wave's __ballot of the lanes' verdicts IS the word; it is ANDed with the
//     presence word of the same index and written by lane 0 with an ordinary store;
//   - the program is the same for every lane: it is copied to LDS once per workgroup and walked with a uniform index, so there
//     is no divergence; a lane's evaluation stack is the bits of one register (a leaf or a constant shifts a bit in, AND / OR
//     combine the two lowest bits);
//   - a leaf reads codes[id] (consecutive lanes, consecutive words: coalesced) only when id < the column's length and
//     id < mask_bits; every other lane sees -1 without touching memory;
//   - the workgroups stride over the words; no workgroup waits for another.  The eligible count is one atomic add per workgroup.
// Leaf semantics are MetadataFilter::matches' (storage.rs:60-71): Eq code == c, Ne code != c (a row without the field
// matches), Exists code >= 0.  A numeric leaf (Lt / Le / Gt / Ge) reads the same code and then the column's f64
// table: v = lut[c] only when 0 <= c < lut_len -- a column may hold ANY int32, so this check stands in front of every lut
// access -- else NaN; the verdict is the plain IEEE comparison with the leaf's constant, which NaN fails four times out of
// four.  A numeric leaf's lut, length and constant sit in a second LDS array behind the ops (nums[op.code]), so a program
// without one keeps its 24 bytes of LDS per op.
// gfx950 only.
#include "kernels.h"

namespace vdb {

static_assert(sizeof(FilterOp) == 24 && sizeof(FilterNum) == 24 && FILTER_MAX_OPS * (sizeof(FilterOp) + sizeof(FilterNum)) <= 64 * 1024,
              "the longest program, all numeric leaves, fits the default dynamic LDS of a launch");

constexpr uint32_t FLT_THREADS = 256, FLT_WAVES = FLT_THREADS / 64;

__global__ __launch_bounds__(FLT_THREADS) void filter_compile_kernel(FilterParams p, uint64_t n_words) {
    extern __shared__ FilterOp sOps[];
    __shared__ uint32_t sCnt[FLT_WAVES];
    FilterNum* sNums = reinterpret_cast<FilterNum*>(sOps + p.n_ops);       // (both records are 24 bytes, 8-byte aligned)
    for (uint32_t i = threadIdx.x; i < p.n_ops; i += FLT_THREADS) sOps[i] = p.ops[i];
    for (uint32_t i = threadIdx.x; i < p.n_nums; i += FLT_THREADS) sNums[i] = p.nums[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t found = 0;                                                    // set bits of this wave's words (the same in every lane)
    for (uint64_t w = (uint64_t)blockIdx.x * FLT_WAVES + wave; w < n_words; w += (uint64_t)gridDim.x * FLT_WAVES) {
        const uint64_t id = w * 64u + lane;
        const bool in_range = id < p.mask_bits;
        uint32_t st = 0;
        for (uint32_t i = 0; i < p.n_ops; ++i) {
            const FilterOp op = sOps[i];                                   // uniform address: an LDS broadcast
            if (op.op <= FOP_EXISTS) {
                int32_t c = -1;
                if (in_range && id < op.len) c = op.codes[id];
                const bool v = op.op == FOP_EQ ? c == op.code : (op.op == FOP_NE ? c != op.code : c >= 0);
                st = (st << 1) | (v ? 1u : 0u);
            } else if (op.op == FOP_CONST) {
                st = (st << 1) | (op.code ? 1u : 0u);
            } else if (op.op == FOP_AND) {
                st = (st >> 1) & (st | ~1u);
            } else if (op.op == FOP_OR) {
                st = (st >> 1) | (st & 1u);
            } else {                                                       // FOP_LT .. FOP_GE
                const FilterNum x = sNums[op.code];                        // uniform address again
                int32_t c = -1;
                if (in_range && id < op.len) c = op.codes[id];
                double v = __builtin_nan("");
                if (c >= 0 && (uint64_t)(uint32_t)c < x.lut_len) v = x.lut[c];
                const bool r = op.op == FOP_LT ? v < x.c : (op.op == FOP_LE ? v <= x.c : (op.op == FOP_GT ? v > x.c : v >= x.c));
                st = (st << 1) | (r ? 1u : 0u);
            }
        }
        uint64_t word = __ballot(in_range && (st & 1u));
        word &= w < p.present_words ? p.present[w] : 0ull;
        if (lane == 0) p.mask[w] = word;
        found += (uint32_t)__popcll(word);
    }
    if (lane == 0) sCnt[wave] = found;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        for (uint32_t i = 0; i < FLT_WAVES; ++i) total += sCnt[i];
        if (total) atomicAdd(p.count, total);
    }
}

void launch_filter_compile(const FilterParams& p, uint32_t n_cu, hipStream_t s) {
    const uint64_t n_words = (p.mask_bits + 63) / 64;
    if (n_words == 0) return;
    const uint64_t want = (n_words + FLT_WAVES - 1) / FLT_WAVES;
    const uint32_t grid = (uint32_t)(want < (uint64_t)n_cu * 8 ? want : (uint64_t)n_cu * 8);
    hipLaunchKernelGGL(filter_compile_kernel, dim3(grid), dim3(FLT_THREADS), p.n_ops * sizeof(FilterOp) + p.n_nums * sizeof(FilterNum), s, p, n_words);
}

}  // namespace vdb
