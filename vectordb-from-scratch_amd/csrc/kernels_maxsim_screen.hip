// kernels_maxsim_screen.hip -- the device steps of the SCREENED route of late-interaction search (vdb_flat_set_maxsim_screen,
// DESIGN.md 4.19 "screened route").  The matrix cores rank every (token, row) pair in bf16, a certificate turns the smallest
// ranking score of a (token, document) into a LOWER BOUND of the exact minimum m(t, c), and the exact scan of kernels_maxsim.hip
// is spent only on the documents whose bound can still reach the k-th exact score.
//   - maxsim_cert_kernel: the certificate constants of every token (cert_consts, f64), once per call.
//   - maxsim_screen_kernel: the GEMM.  A workgroup of 4 waves owns a tile of 128 rows x 256 token columns: rows on the M side,
//     tokens on the N side of v_mfma_f32_32x32x16_bf16, so a lane's 16 accumulators of a 32 x 32 block are 16 rows of ONE token.
//     The rows come f32 from HBM, are rounded to bf16 in registers (cvt8, RNE) and stored as bf16 in LDS (64 bytes a row and K
//     stage); the token columns are the image query_prep wrote (16 KB per pass and K stage, contiguous).  Two LDS stages, the
//     global loads of stage s + 1 in flight over the MFMAs of stage s, one barrier per stage.  Wave w owns columns 64 w .. 64 w + 63
//     against all 128 rows: 8 accumulator blocks.  Epilogue, per 32 columns: the scores become ordered integers, the two lanes
//     that hold one column exchange halves so that each holds 64 CONSECUTIVE rows of its column in registers, and one pass in
//     row order keeps a running minimum that is flushed by one global atomicMin at the end of every run of equal codes -- one
//     atomic per (run inside a half tile of 64 rows, token), none for unused columns.
//   - maxsim_bound_kernel: per (query, code) the per-token bounds cert_lower_bound, folded left in f32 like the score.
//   - maxsim_mark_kernel<1 | 2>: the candidate bitmaps of the two rounds.
// Everything read from device memory is checked before an address is formed from it.  No packed-f32 operations; gfx950 only.
#include "fused_bf16_common.h"
#include "kernels_exact.h"

#pragma clang fp contract(off)

namespace vdb {

namespace {
constexpr uint32_t SC_ROWS = 128, SC_COLS = 256, SC_THREADS = 256, SC_HALF = 64;
constexpr uint32_t SC_A_BYTES = SC_ROWS * 64, SC_B_BYTES = SC_COLS * 64;   // one K stage: 32 bf16 a row, 32 bf16 a column
constexpr uint32_t SC_NO_CODE = 0xffffffffu, SC_UNTOUCHED = 0xffffffffu;
constexpr float SC_MAX_NORM = 1099511627776.0f;                            // 2^40: no product of the exact fold overflows below it
// byte offset of 16-byte chunk x (8 bf16) of row / column r inside a stage image: the swizzle of query_prep's image
__device__ __forceinline__ uint32_t sc_off(uint32_t r, uint32_t x) { return r * 64u + ((x ^ ((r >> 2) & 3u)) << 4); }
}  // namespace

// ---------------------------------------------------------------------------------------------
// certificate constants per token
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxsim_cert_kernel(MaxsimCertParams p) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.n_tokens) return;
    const float qn = p.qnorm[t];
    CertConsts c = cert_consts(p.cert_in, t, (double)qn);
    if (!(qn <= SC_MAX_NORM)) c.ok = 0;
    p.cert[t] = MaxsimTokenCert{c.a, c.b, c.tslack, c.lhs_scale, (uint32_t)c.square, (uint32_t)c.ok};
    const uint32_t q = p.colmap[t] >> 8;
    if (!c.ok && q < p.n_queries) atomicOr(p.unscreened + q, 1u);
}
void launch_maxsim_cert(const MaxsimCertParams& p, hipStream_t s) {
    if (!p.n_tokens) return;
    hipLaunchKernelGGL(maxsim_cert_kernel, dim3((p.n_tokens + 255) / 256), dim3(256), 0, s, p);
}

// ---------------------------------------------------------------------------------------------
// the screening GEMM
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_THREADS, 2) void maxsim_screen_kernel(MaxsimScreenParams p) {
    __shared__ __attribute__((aligned(16))) unsigned char sA[2][SC_A_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char sB[2][SC_B_BYTES];
    __shared__ __attribute__((aligned(16))) uint32_t sCode[SC_ROWS];
    __shared__ __attribute__((aligned(16))) float sAlpha[SC_ROWS];
    __shared__ __attribute__((aligned(16))) float sBeta[SC_ROWS];
    __shared__ __attribute__((aligned(16))) float sMargin[SC_ROWS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, col32 = lane & 31u, half = lane >> 5;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t row0 = blockIdx.x * SC_ROWS, pass = p.pass0 + blockIdx.y, nks = p.ld / KSTAGE;

    // ---- the tile's rows: code, alpha, beta, margin (threads 0..127); a tile without an eligible row is done
    bool mine = false;
    if (tid < SC_ROWS) {
        const uint32_t row = row0 + tid;
        uint32_t code = SC_NO_CODE;
        bool beyond = false;
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
        float al = 0.0f, be = 0.0f, ma = 0.0f;
        if (code != SC_NO_CODE) {
            al = p.alpha[row]; be = p.beta[row];
            if (p.margin) ma = p.margin[row];
            if (!(p.nd[row] <= SC_MAX_NORM)) al = __uint_as_float(0x7fc00000u);   // (its scores are NaN: the queries are not screened)
            mine = true;
        }
        if (beyond) atomicOr(p.status + 3, 1u);
        sCode[tid] = code; sAlpha[tid] = al; sBeta[tid] = be; sMargin[tid] = ma;
    }
    if (!__syncthreads_or(mine ? 1 : 0)) return;

    // ---- staging plan: thread t rounds row chunks t and t + 256 (row c >> 2, 8 floats at c & 3) and copies four 16-byte
    // pieces of the column image
    uint32_t a_off[2];
    const float* a_src[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const uint32_t c = tid + 256u * u, r = c >> 2, x = c & 3u;
        a_off[u] = sc_off(r, x);
        a_src[u] = sCode[r] != SC_NO_CODE ? p.rows + (size_t)(row0 + r) * p.ld + x * 8u : nullptr;   // (a row that is not eligible is never read)
    }
    const uint4* b_src = reinterpret_cast<const uint4*>(p.qb) + (size_t)pass * nks * (SC_B_BYTES / 16) + tid;
    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    // ---- iteration ks fetches stage ks into registers, multiplies stage ks - 1 out of LDS image (ks - 1) & 1 while those loads
    // are in flight, then rounds and stores stage ks into image ks & 1; one barrier per stage
    for (uint32_t ks = 0; ks <= nks; ++ks) {
        const bool more = ks < nks;
        const float4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
        float4 ra0 = z4, ra1 = z4, ra2 = z4, ra3 = z4;
        uint4 rb0 = {0, 0, 0, 0}, rb1 = rb0, rb2 = rb0, rb3 = rb0;
        if (more) {
            if (a_src[0]) { const float4* g = reinterpret_cast<const float4*>(a_src[0] + (size_t)ks * KSTAGE); ra0 = g[0]; ra1 = g[1]; }
            if (a_src[1]) { const float4* g = reinterpret_cast<const float4*>(a_src[1] + (size_t)ks * KSTAGE); ra2 = g[0]; ra3 = g[1]; }
            const uint4* g = b_src + (size_t)ks * (SC_B_BYTES / 16);
            rb0 = g[0]; rb1 = g[256]; rb2 = g[512]; rb3 = g[768];
        }
        if (ks) {
            const unsigned char* imgA = sA[(ks - 1) & 1u];
            const unsigned char* imgB = sB[(ks - 1) & 1u];
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2) {
                const uint32_t x = 2u * k2 + half;
                bf16x8 fa[4], fb[2];
#pragma unroll
                for (int i = 0; i < 4; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(imgA + sc_off(32u * i + col32, x));
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const bf16x8*>(imgB + sc_off(wave * 64u + 32u * j + col32, x));
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
            }
        }
        if (more) {
            unsigned char* imgA = sA[ks & 1u];
            unsigned char* imgB = sB[ks & 1u];
            *reinterpret_cast<bf16x8*>(imgA + a_off[0]) = cvt8(ra0, ra1);
            *reinterpret_cast<bf16x8*>(imgA + a_off[1]) = cvt8(ra2, ra3);
            *reinterpret_cast<uint4*>(imgB + tid * 16u) = rb0;
            *reinterpret_cast<uint4*>(imgB + (tid + 256u) * 16u) = rb1;
            *reinterpret_cast<uint4*>(imgB + (tid + 512u) * 16u) = rb2;
            *reinterpret_cast<uint4*>(imgB + (tid + 768u) * 16u) = rb3;
        }
        __syncthreads();
    }

    // ---- epilogue, 32 columns at a time: accumulator e of block i is row 32 i + 8 (e >> 2) + 4 half + (e & 3) of column col32
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t t = pass * SC_COLS + wave * 64u + 32u * j + col32;  // (the column map and qg are padded to whole passes)
        const uint32_t cm = p.colmap[t];
        const uint32_t q = cm >> 8, slot = cm & 255u;
        const bool valid = cm != 0xffffffffu && q >= p.q0 && q - p.q0 < p.nq && slot < MAXSIM_MAX_TOKENS;
        const float g = p.qg ? p.qg[t] : 0.0f;
        uint32_t* dst = p.table + ((size_t)(valid ? q - p.q0 : 0u) * p.n_codes) * MAXSIM_MAX_TOKENS + (valid ? slot : 0u);
        bool bad = false;
        uint32_t cur = SC_UNTOUCHED, c = sCode[SC_HALF * half];
        // 32 rows of each half tile at a time (blocks b and 2 + b): scores -> ordered integers, then the lanes col32 and col32 + 32,
        // which hold the column, exchange so that lane half h holds rows 64 h + 32 b .. + 31 in order, then one pass in row order:
        // the running minimum of a run of equal codes goes out at the run's last row
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            uint32_t o[2][16];
#pragma unroll
            for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                for (int e4 = 0; e4 < 4; ++e4) {
                    const int i = 2 * ii + b;
                    const uint32_t r = 32u * i + 8u * e4 + 4u * half;
                    const uint4 c4 = *reinterpret_cast<const uint4*>(sCode + r);
                    const float4 a4 = *reinterpret_cast<const float4*>(sAlpha + r), b4 = *reinterpret_cast<const float4*>(sBeta + r);
                    const float4 m4 = *reinterpret_cast<const float4*>(sMargin + r);
                    const uint32_t cc[4] = {c4.x, c4.y, c4.z, c4.w};
                    const float aa[4] = {a4.x, a4.y, a4.z, a4.w}, bb[4] = {b4.x, b4.y, b4.z, b4.w}, mm[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        float sc = __builtin_fmaf(acc[i][j][4 * e4 + u], aa[u], bb[u]);
                        if (p.margin) sc = __builtin_fmaf(-g, mm[u], sc);  // the lower-bound score of FusedBf16Params
                        const bool el = cc[u] != SC_NO_CODE, fin = __builtin_fabsf(sc) < __builtin_inff();
                        bad = bad || (el && !fin);
                        o[ii][4 * e4 + u] = !el ? SC_UNTOUCHED : (fin ? f32_to_ordered(sc) : 0u);
                    }
                }
            uint32_t v[32];
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = 4 * e4 + u;
                    const uint32_t own = half ? o[1][e] : o[0][e], send = half ? o[0][e] : o[1][e];
                    const uint32_t recv = (uint32_t)__shfl_xor((int)send, 32);
                    v[8 * e4 + u] = half ? recv : own;
                    v[8 * e4 + 4 + u] = half ? own : recv;
                }
#pragma unroll
            for (int s = 0; s < 32; ++s) {
                const int at = 32 * b + s;
                const uint32_t cn = at + 1 < (int)SC_HALF ? sCode[SC_HALF * half + at + 1] : SC_NO_CODE;
                cur = v[s] < cur ? v[s] : cur;
                if (at + 1 == (int)SC_HALF || cn != c) {
                    if (c != SC_NO_CODE && valid) atomicMin(dst + (size_t)c * MAXSIM_MAX_TOKENS, cur);   // (c < n_codes: checked above)
                    cur = SC_UNTOUCHED;
                }
                c = cn;
            }
        }
        if (bad && valid) atomicOr(p.unscreened + q, 1u);
    }
}

void launch_maxsim_screen(const MaxsimScreenParams& p, uint32_t n_pass, hipStream_t s) {
    if (!p.n_rows || !n_pass || !p.nq) return;
    hipLaunchKernelGGL(maxsim_screen_kernel, dim3((p.n_rows + SC_ROWS - 1) / SC_ROWS, n_pass), dim3(SC_THREADS), 0, s, p);
}

// ---------------------------------------------------------------------------------------------
// the per-document lower bound
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxsim_bound_kernel(MaxsimBoundParams p) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const uint32_t t0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.offs[p.q0 + y]);
    const uint32_t T0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.offs[p.q0 + y + 1]) - t0;
    const uint32_t T = T0 < MAXSIM_MAX_TOKENS ? T0 : MAXSIM_MAX_TOKENS;
    bool doc = false;
    if (c < p.n_codes) {
        const uint32_t* e = p.table + ((size_t)y * p.n_codes + c) * MAXSIM_MAX_TOKENS;
        uint32_t lo = SC_UNTOUCHED;
        if (e[0] != SC_UNTOUCHED) {
            doc = true;
            float L = 0.0f;
            for (uint32_t j = 0; j < T; ++j) {                              // (T is wave-uniform, the constants come by scalar loads)
                const MaxsimTokenCert& k = p.cert[t0 + j];
                const CertConsts cc{k.a, k.b, k.tslack, k.lhs_scale, (int)k.square, (int)k.ok};
                const float b = cert_lower_bound(cc, p.metric, ordered_to_f32(e[j]));
                L = j ? __fadd_rn(L, b) : b;                                // the score's fold: from the first term
            }
            if (L != L) L = __uint_as_float(0xff800000u);                  // a NaN bound bounds nothing: -inf
            lo = f32_to_ordered(L);
        }
        p.lb[(size_t)(p.q0 + y) * p.n_codes + c] = lo;
        p.keys[(size_t)y * p.n_codes + c] = doc ? ((uint64_t)lo << 32) | c : EMPTY_KEY;
    }
    const unsigned long long docs = __ballot(doc);
    if (docs && (threadIdx.x & 63u) == 0) atomicAdd(p.docs_seen, (unsigned long long)__popcll(docs));
}
void launch_maxsim_bound(const MaxsimBoundParams& p, uint32_t n_queries, hipStream_t s) {
    if (!p.n_codes || !n_queries) return;
    hipLaunchKernelGGL(maxsim_bound_kernel, dim3((p.n_codes + 255) / 256, n_queries), dim3(256), 0, s, p);
}

// ---------------------------------------------------------------------------------------------
// the candidate bitmaps
// ---------------------------------------------------------------------------------------------
template <int ROUND>
__global__ __launch_bounds__(256) void maxsim_mark_kernel(MaxsimMarkParams p) {
    const uint32_t y = blockIdx.y, b = p.q0 + y;
    const bool screened = p.unscreened[b] == 0u;
    const uint32_t have = p.sel_cnt[y] < p.sel_stride ? p.sel_cnt[y] : p.sel_stride;
    const uint64_t* sel = p.sel + (size_t)y * p.sel_stride;
    uint32_t* marked = p.marked + (size_t)y * p.mark_words;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    uint32_t n = 0;
    if (ROUND == 1) {
        if (!screened) {
            if (i < p.mark_words) marked[i] = 0xffffffffu;                  // (the scan tests a code against n_codes before its bit)
        } else if (i < have && i < p.kk) {
            const uint32_t c = (uint32_t)sel[i];
            if (sel[i] != EMPTY_KEY && c < p.n_codes) { atomicOr(marked + (c >> 5), 1u << (c & 31u)); n = 1; }
        }
    } else if (i < p.mark_words) {
        uint32_t bits = 0;
        if (screened) {
            const uint32_t ek = (p.kk && have >= p.kk) ? (uint32_t)(sel[p.kk - 1] >> 32) : 0xffffffffu;
            const uint32_t* lb = p.lb + (size_t)b * p.n_codes;
            for (uint32_t u = 0; u < 32; ++u) {
                const uint32_t c = 32u * i + u;
                if (c < p.n_codes) {
                    const uint32_t l = lb[c];
                    if (l != SC_UNTOUCHED && l <= ek) bits |= 1u << u;
                }
            }
            bits &= ~marked[i];
        }
        marked[i] = bits;
        n = (uint32_t)__popc(bits);
    }
    for (int o = 32; o > 0; o >>= 1) n += (uint32_t)__shfl_xor((int)n, o);
    if (n && (threadIdx.x & 63u) == 0) atomicAdd(p.rescored, (unsigned long long)n);
}
void launch_maxsim_mark(const MaxsimMarkParams& p, int round, uint32_t n_queries, hipStream_t s) {
    if (!n_queries || !p.mark_words) return;
    const uint32_t work = round == 1 ? (p.mark_words > p.kk ? p.mark_words : p.kk) : p.mark_words;
    const dim3 grid((work + 255) / 256, n_queries);
    if (round == 1) hipLaunchKernelGGL(maxsim_mark_kernel<1>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(maxsim_mark_kernel<2>, grid, dim3(256), 0, s, p);
}

}  // namespace vdb
