// fused_bf16_common.h -- what the kernels of the bf16 SCREENING tier share: kernels_fused_bf16.hip (sample
// pass; unpipelined filter pass in the diagnostics build), kernels_fused_bf16p.hip (filter pass), kernels_fused_bf16w.hip
// (512-query filter pass) and kernels_fused_s16.hip (filter and sample pass over the bf16 shadow rows).  Each of those files
// holds what is different about its kernel -- tile shape, DMA plan, the interleaving of MFMAs, LDS reads and DMA issue --
// and everything they must agree on, bit for bit, is defined ONCE, here or (where host code and other kernels need it too:
// the sub-pool index and the sample mapping) in kernels.h.
//
// THE METHOD.  Ranking scores of every row against a block of queries on the bf16 matrix cores
// (v_mfma_f32_32x32x16_bf16): rows are rounded to bf16 in registers (v_cvt_pk_bf16_f32, RNE; the shadow rows hold exactly
// those roundings), queries were rounded once per batch by query_prep.  A K stage of rows and queries is brought into an
// LDS ring by LDS-DMA, every wave owns a block of 32 x 32 MFMA tiles, and the epilogue of a tile turns the accumulators
// into scores fma(dot, alpha_row, beta_row) and
//   * FILTER: appends (score, row) of every eligible row with score <= thr[q] to the lane's private candidate sub-pool
//     (fused_bf16_subpool), or
//   * SAMPLE: keeps the smallest eligible score per (tile, row half, lane half) and query over the S sample rows
//     (screen_sample_row); the kp-th smallest of a query's group minima is a threshold that at least kp rows meet.
// Every accumulator sees the same operands in the same MFMA order in all kernels, so their scores agree bit for bit and
// the sample's threshold is valid for every filter kernel.  The scores only RANK rows: the re-rank recomputes exact f32
// distances and certifies that no excluded row can enter the top k (kernels_aux.hip cert_test).
// MARGIN instances (Dot / Euclid) rank by the LOWER-BOUND score fma(-g_q, margin_row, score), see FusedBf16Params.
#pragma once
#include "kernels.h"

#include <type_traits>

namespace vdb {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

namespace {
#ifdef VDB_DIAG
constexpr bool kDiag = true;                     // the ablate bits tested with kDiag exist in the diagnostics build only
#else
constexpr bool kDiag = false;
#endif
constexpr int A_ROWB = 128;                      // bytes of a row in a stage image (32 f32, or 64 bf16 of a shadow row)
constexpr int B_ROWB = 64;                       // bytes of a query in a stage image (32 bf16)

__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {
    f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));   // v_cvt_pk_bf16_f32 (RNE)
}
// THE SPLIT LAYOUT'S ROUNDING (row_split.h).  Over a store in the SPLIT layout kernels_fused_s16.hip reads the hi word of an
// element in the place of pk_bf16's result: hi = upper16(x) + bit 15 of x, the element rounded to bf16 HALF UP IN MAGNITUDE.
// It equals the RNE value except where the low half is exactly 0x8000 (a tie), and there it is the other neighbour of the
// tie, so |x - hi| <= half a bf16 ulp of x for every finite x, exactly the bound RNE gives -- and where RNE overflows to
// +-inf so does hi (upper 0x7f7f, lo >= 0x8000), nowhere else.  Every constant of the certificate (vdb_cert.cpp) and every
// per-row margin and error maximum of launch_row_stats is derived from that half-ulp bound per element (|e_d| <= 2^-9 |d|
// relative, |x - bf16(x)| absolute as an UPPER bound on what a reader may see), never from the direction of a tie: a tie's
// two neighbours are equally far away, so the stored |x - bf16(x)| is the same number for both.  They stay valid unchanged.
// The scores of a tie element differ between the layouts; the results do not, because scores only rank (THE METHOD above).
// The compact sample copy keeps RNE values: any threshold is valid for the filter, it only has to let enough rows pass.
// Non-finite elements never reach the hi plane: the forward conversion reports them and the index stays F32.
__device__ __forceinline__ bf16x8 cvt8(const float4& lo, const float4& hi) {
    u32x4 r = {pk_bf16(lo.x, lo.y), pk_bf16(lo.z, lo.w), pk_bf16(hi.x, hi.y), pk_bf16(hi.z, hi.w)};
    return __builtin_bit_cast(bf16x8, r);
}

// the named constant of VDB_LOOSEN below
constexpr float kThpSlack = 6.0e-7f;
}  // namespace

// The shared pieces of the kernel bodies are MACROS, not functions, where the function form was tried and changed the
// generated code (tools/isa_diff.py): these kernels sit at the 256-VGPR limit, and an instruction order that differs by
// one inlined call changes the register allocation of the whole stage loop.  Each expands in the kernel's own scope and
// names what it takes from it.

// ---- fragment reads of the f32-row kernels (scope: MT, QT, a_row_off, b_row_off, ra[], rb[]): a row fragment is two
// 16-byte halves of f32 (the second at ra ^ 16 in the swizzled image) rounded to bf16, a query fragment 16 bytes of bf16
#define VDB_READ_B(FB, IMG, T_)                                                                        \
    _Pragma("unroll") for (int j_ = 0; j_ < QT; ++j_) {                                                \
        const u32x4 raw_ = *reinterpret_cast<const u32x4*>((IMG) + b_row_off + j_ * 32 * B_ROWB + rb[T_]); \
        FB[j_] = __builtin_bit_cast(bf16x8, raw_);                                                     \
    }
#define VDB_LOAD_FRAGS(FA, FB, IMG, T_)                                                                \
    {                                                                                                  \
        _Pragma("unroll") for (int i_ = 0; i_ < MT; ++i_) {                                            \
            const float4 lo_ = *reinterpret_cast<const float4*>((IMG) + a_row_off + i_ * 32 * A_ROWB + ra[T_]); \
            const float4 hi_ = *reinterpret_cast<const float4*>((IMG) + a_row_off + i_ * 32 * A_ROWB + (ra[T_] ^ 16u)); \
            FA[i_] = cvt8(lo_, hi_);                                                                   \
        }                                                                                              \
        VDB_READ_B(FB, IMG, T_)                                                                        \
    }

// ---- the three-image ring: stage index mod 3 == image index.  RUN(st, image tag, steady tag) computes stage st; STEADY
// promises that the stages the kernel looks ahead to exist (st + TAIL - 2 < TOTAL), so its waits and DMA issues are
// unconditional; the last one to TAIL (4 or 5) stages run with conditional issue.  (Not a micro-optimisation: with a
// conditional issue hipcc's waitcnt pass sees a path on which nothing follows the previous fill of the image about to be
// read and puts a vmcnt(0) in front of the first ds_read of every third stage, which drains the DMA pipeline.)
#define VDB_RING3(RUN, TOTAL, TAIL)                                                                    \
    {                                                                                                  \
        using B0 = std::integral_constant<int, 0>;                                                     \
        using B1 = std::integral_constant<int, 1>;                                                     \
        using B2 = std::integral_constant<int, 2>;                                                     \
        uint32_t st = 0;                                                                               \
        for (; st + (TAIL) < (TOTAL); st += 3) {                                                       \
            RUN(st, B0{}, std::true_type{});                                                           \
            RUN(st + 1, B1{}, std::true_type{});                                                       \
            RUN(st + 2, B2{}, std::true_type{});                                                       \
        }                                                                                              \
        if (st < (TOTAL)) { RUN(st, B0{}, std::false_type{}); ++st; }                                  \
        if (st < (TOTAL)) { RUN(st, B1{}, std::false_type{}); ++st; }                                  \
        if (st < (TOTAL)) { RUN(st, B2{}, std::false_type{}); ++st; }                                  \
        if (st < (TOTAL)) { RUN(st, B0{}, std::false_type{}); ++st; }                                  \
        if ((TAIL) == 5 && st < (TOTAL)) { RUN(st, B1{}, std::false_type{}); ++st; }                   \
    }

// ---- MARGIN pre-test.  The filter is  lb = fma(-g_q, margin_row, score) <= thr.  Since margin_row <= mmax (the largest
// margin of the wave's rows of this tile), lb <= thr implies score <= thr + g_q mmax =: thp -- so the COMMON path compares
// the plain score with a per-tile loosened threshold (two fmas per lane and tile instead of one packed fma and one more LDS
// read per pair of elements), and only the rare path computes lb and applies the exact test (VDB_APPEND).
// kThpSlack covers the f32 roundings on both sides of that implication -- of thp itself and of lb in the exact test, each
// at most 2^-24 relative to |thr| + g mmax -- with a factor of five to spare, so no row with lb <= thr can fail the
// pre-test.  It is part of the certificate's soundness argument: looser is safe, tighter is not.
// VDB_WAVE_MAX: MM (the lane's largest margin) becomes the wave's.  +inf margins (norm overflow) open the tile; NaN rows
// carry NaN scores anyway.
#define VDB_WAVE_MAX(MM) for (int o = 32; o > 0; o >>= 1) MM = fmaxf(MM, __shfl_xor(MM, o));
#define VDB_LOOSEN(THP, THR, G, MMAX) THP = fmaf(G, MMAX, THR); THP += (fabsf(THR) + G * MMAX) * kThpSlack;

// ---- the filter test of four rows x one query (S01, S23: their scores, two per f32x2).  Hits are rare (about 0.1 % of
// the elements), so it is ONE compare: the smallest of the four scores against the (loosened) threshold, its lane mask
// straight into a not-taken branch; the append code is out of line.  v_min_f32 drops a NaN operand and a NaN score must
// pass (flat_index.rs:62) -- so the minimum stands alone only when no score of the launch can be NaN (fused_no_nan);
// otherwise the kernels OR in VDB_HITS_NAN4 of a NaN-propagating sum of the four (inf - inf gives a false alarm, which the
// per-row test of VDB_APPEND sorts out).
// The pieces are expressions, so that a kernel can order the tests of its queries as its register budget needs:
//   N = VDB_MIN4(S01, S23);  M = VDB_HITS_MIN4(N, THP);   U = VDB_SUM4(S01, S23);  T = U.x + U.y;  M |= VDB_HITS_NAN4(T);
#define VDB_MIN4(S01, S23) __builtin_elementwise_min(S01, S23)
#define VDB_HITS_MIN4(N, THP) __builtin_amdgcn_ballot_w64(!(fminf((N).x, (N).y) > (THP)))
#define VDB_SUM4(S01, S23) ((S01) + (S23))
#define VDB_HITS_NAN4(T) __builtin_amdgcn_ballot_w64((T) != (T))

// ---- the append (scope: p, MARGIN).  It is what the epilogue costs (with thresholds that let nothing pass the kernels are
// as fast as without an epilogue), so it is kept short: one 4-bit hit mask per lane -- S0..S3 against THP, AND the rows'
// eligibility bits ELIG4 -- then a loop over its set bits, typically one lane, one iteration.  MARGIN: the exact test, on
// the lower-bound score fma(NG, MG[MGI + e], s), NG = -g_q, against the unloosened THR.  Keys beyond the sub-pool's
// capacity are counted, not stored (a count above capl tells the select that the pool overflowed).  ROW0: device row of S0.
#define VDB_APPEND(S0, S1, S2, S3, ELIG4, THP, THR, NG, MG, MGI, POOL, PCNT, ROW0)                     \
    {                                                                                                  \
        uint32_t hm_ = (!((S0) > (THP)) ? 1u : 0u) | (!((S1) > (THP)) ? 2u : 0u) | (!((S2) > (THP)) ? 4u : 0u) | (!((S3) > (THP)) ? 8u : 0u); \
        hm_ &= (ELIG4) & 0xfu;                                                                         \
        while (hm_) {                                                                                  \
            const uint32_t e_ = (uint32_t)__builtin_ctz(hm_);                                          \
            hm_ &= hm_ - 1u;                                                                           \
            float sc_ = e_ == 0 ? (S0) : e_ == 1 ? (S1) : e_ == 2 ? (S2) : (S3);                       \
            if (MARGIN) {                                              /* the exact test, on the lower-bound score */ \
                sc_ = fmaf((NG), (MG)[(MGI) + e_], sc_);                                               \
                if (sc_ > (THR)) continue;                                                             \
            }                                                                                          \
            if (!(kDiag && (p.ablate & 32u)) && PCNT < p.capl) POOL[PCNT] = make_raw_key(sc_, (ROW0) + e_); /* diag 32: count only */ \
            ++PCNT;                                                                                    \
        }                                                                                              \
    }

// ---- LDS-DMA.  Issued from inline asm, not through __builtin_amdgcn_global_load_lds: hipcc's waitcnt pass tracks the
// builtin as a pending LDS write and, at the loop header of a stage ring, cannot bound how many vector-memory operations
// followed the fill of the image about to be read -- it then puts a vmcnt(0) in front of that stage's first ds_read, which
// drains the DMA pipeline.  All ordering between the DMA and the LDS reads is done by hand in the kernels (counted
// s_waitcnt + s_barrier once per stage); compiler-inserted vmcnt waits for ordinary loads stay correct because not
// counting these instructions only makes them wait longer.  GP: per-lane global address; the LDS destination is
// M0 + lane * (bytes per lane).
#define VDB_DMA(GP, IMG, LOFF)                                                                         \
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off"                     \
                 :: "s"((uint32_t)(uintptr_t)(lds_ptr_t)((IMG) + (LOFF))), "v"((const void*)(GP)) : "memory", "m0")
// rows are read once per launch: non-temporal, so that they do not push the queries out of the L2
#define VDB_DMA_NT(GP, IMG, LOFF)                                                                      \
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt"                  \
                 :: "s"((uint32_t)(uintptr_t)(lds_ptr_t)((IMG) + (LOFF))), "v"((const void*)(GP)) : "memory", "m0")
// (the instruction's immediate offset applies to BOTH addresses -- the global source and the LDS destination M0 + offset +
// lane * 16 -- so pieces that are IMM bytes apart on both sides share one source register AND one M0 value)
#define VDB_DMA_OFF(GP, IMG, LOFF, IMM)                                                                \
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off offset:%2"           \
                 :: "s"((uint32_t)(uintptr_t)(lds_ptr_t)((IMG) + (LOFF))), "v"((const void*)(GP)), "i"(IMM) : "memory", "m0")
// 4 bytes per lane: the per-row constants of a tile (alpha, beta, mask word, margin)
#define VDB_DMA4(GP, LP)                                                                               \
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, off"                        \
                 :: "s"((uint32_t)(uintptr_t)(lds_ptr_t)(LP)), "v"((const void*)(GP)) : "memory", "m0")

}  // namespace vdb
