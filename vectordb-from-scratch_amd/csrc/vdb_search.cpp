// vdb_search.cpp -- the tier scheduler of the batched search: bf16 screening pass, re-threshold pass,
// f32-input MFMA tier, exact scan.  Each tier either PROVES its answer is the oracle's or hands the query on; results never
// depend on which tier answered.  Reference: FlatIndex::search (src/flat_index.rs:52-65) driven by
// VectorStore::search_batch (src/storage.rs:302-310).
#include <cmath>
#include <cstdio>
#include <limits>

#include "vdb_index.h"

namespace vdbi {

// The filter pass of the screening tier: over the bf16 shadow rows when the index keeps them (vdb_flat_set_shadow) and the
// row pitch allows whole 128-byte row requests, else over the f32 rows.  Same scores either way, bit for bit.  A store in the
// SPLIT layout (row_split.h) is its own shadow: the same kernel streams the hi piece of every row at the store's pitch (scores
// differ from the other two only where an element lies exactly between two bf16 values, fused_bf16_common.h; results never).
bool shadow_usable(const Index* ix) { return ix->d_rows16 && ix->ld % 64 == 0; }
void launch_filter_pass(Index* ix, vdb::FusedBf16Params& fp, hipStream_t s) {
    if (shadow_usable(ix)) { fp.rows16 = ix->d_rows16; vdb::launch_fused_s16(fp, s); return; }
    if (ix->layout == vdb::LAYOUT_SPLIT) {
        fp.rows16 = reinterpret_cast<const uint16_t*>(ix->d_rows_store.p); fp.rows16_pitch = 2 * ix->ld;
        vdb::launch_fused_s16(fp, s);
        return;
    }
#ifdef VDB_DIAG
    if (!ix->kn.fused_pipe) { vdb::launch_fused_bf16(fp, s); return; }
#endif
    vdb::launch_fused_bf16p(fp, s);
}

// ------------------------------------------------------------------ parameter blocks shared by the tiers
// grid of a screening pass: one workgroup per CU, at most one per row tile
static uint32_t screen_grid(const Index* ix, uint32_t tile_rows) {
    return std::min<uint32_t>((uint32_t)ix->n_cu, (ix->n_uploaded + tile_rows - 1) / tile_rows);
}
// A screening launch: everything that comes from the index and the pass-local workspace W.  The caller adds the query
// block (screen_queries) and what its pass differs in.
static vdb::FusedBf16Params screen_params(const Index* ix, const Workspace& W, const uint32_t* d_rowmask, uint32_t* d_status,
                                          uint32_t capl, uint32_t n_wg) {
    vdb::FusedBf16Params fp{};
    fp.rows = ix->d_rows_store; fp.ld = ix->ld; fp.n_rows = ix->n_uploaded;      // (in the layout of the moment: launch_filter_pass)
    fp.alpha = ix->d_alpha; fp.beta = ix->d_beta; fp.rowmask = d_rowmask ? d_rowmask : ix->d_live;
    fp.margin = ix->d_margin;
    fp.pool = W.w_pool.p; fp.pool_cnt = W.w_subcnt.p; fp.capl = capl; fp.n_wg = n_wg;
    fp.scalars = ix->d_scalars; fp.qmax_bits = status_qmax(d_status);
    return fp;
}
// ... its queries: the 256-query block (512 for the wide kernel) that starts at q0 of the bf16 images / g_q / thresholds
static void screen_queries(vdb::FusedBf16Params& fp, const Index* ix, const uint16_t* qb, const float* qg, const float* thr, uint32_t q0) {
    fp.qb = qb + (size_t)q0 * ix->ld; fp.qg = ix->d_margin ? qg + q0 : nullptr; fp.thr = thr + q0;
}
// An exact re-rank of the candidate lists cand[q * kp ..] (cand_cnt[q] of them): everything but the query block, the
// outputs and the certificate inputs of the tier.
static vdb::RerankParams rerank_params(const Index* ix, const uint32_t* d_rowmask, uint32_t* d_status, size_t k, const uint64_t* cand,
                                       uint32_t kp, const uint32_t* cand_cnt) {
    vdb::RerankParams rp{};
    rp.rows = ix->d_rows_store; rp.split = ix->layout == vdb::LAYOUT_SPLIT ? 1u : 0u;
    rp.ld = ix->ld; rp.dim = ix->dim; rp.n_rows = ix->n_uploaded;
    rp.nd = ix->d_nd; rp.row_ids = ix->d_row_ids; rp.rowmask = d_rowmask;
    rp.cand = cand; rp.cand_stride = kp; rp.cand_cnt = cand_cnt; rp.kp = kp;
    rp.metric = ix->metric; rp.k = (uint32_t)k; rp.nd2max_bits = ix->d_scalars;
    rp.out_stride = (uint32_t)k; rp.status = d_status;
    return rp;
}
// ... its queries (padded rows / norms of a block that starts at q0) and where their results and certificates go
static void rerank_io(vdb::RerankParams& rp, const Index* ix, const float* qp, const float* qnorm, uint64_t* out_ids, float* out_dists,
                      uint32_t* out_counts, uint32_t* cert, uint32_t q0) {
    rp.qp = qp + (size_t)q0 * ix->ld; rp.qnorm = qnorm + q0;
    rp.out_ids = out_ids + (size_t)q0 * rp.k; rp.out_dists = out_dists + (size_t)q0 * rp.k;
    rp.out_counts = out_counts + q0; rp.cert = cert + q0;
}

// ------------------------------------------------------------------ steps shared by the routes
// The eligibility mask of a search: tombstones, optionally AND the caller's id filter (built into W.w_rowmask on s).  Null: every row.
static int eligibility_mask(Index* ix, Workspace& W, hipStream_t s, const uint64_t* d_idmask, size_t mask_bits, const uint32_t** out) {
    int rc;
    const uint32_t n = ix->n_uploaded;
    *out = (ix->n_live == n) ? nullptr : ix->d_live.p;
    if (d_idmask) {
        if ((rc = W.w_rowmask.ensure((n + 31) / 32))) return rc;
        vdb::launch_build_rowmask(ix->d_row_ids, *out, d_idmask, mask_bits, n, W.w_rowmask.p, s);
        *out = W.w_rowmask.p;
    }
    return VDB_OK;
}

// What a search of a non-empty store checks before any device work, in the order its errors win: the dimension, a live zero-norm
// row under Cosine, the batch size (the caller's verdict: the limits differ per entry point), the dimension limit.
static int pre_device_checks(Index* ix, size_t dim, bool batch_too_large) {
    int rc;
    if ((rc = query_dim_check(ix, dim))) return rc;
    if (ix->metric == vdb::COSINE) {
        if ((rc = ensure_zero_count(ix))) return rc;
        if (ix->zero_live) return fail_zero_vector();   // distance.rs:51-55 aborts the whole search (flat_index.rs:57-60)
    }
    if (batch_too_large) return fail(VDB_ERR_INVALID_ARGUMENT, "batch too large");
    if (ix->dim > 16384) return fail(VDB_ERR_INVALID_ARGUMENT, "dimension %u exceeds the supported 16384", ix->dim);
    return VDB_OK;
}

// A select in EMIT mode -- the k smallest keys written as final ids, distances and counts -- through W's sort area: everything
// but the keys (keys / stride / counts / n_fixed / cap) and the output slice (emit_ids / emit_dists / emit_counts).
static vdb::SelectParams emit_select_params(const Index* ix, Workspace& W, size_t k) {
    vdb::SelectParams mp{};
    mp.kk = (uint32_t)k; mp.out_keys = W.w_exsel.p; mp.out_stride = MAX_SELECT; mp.out_cnt = W.w_cnt.p;
    mp.emit_stride = (uint32_t)k;
    mp.emit_rank2row = ix->ids_monotone ? nullptr : ix->d_rank2row.p; mp.emit_row_ids = ix->d_row_ids;
    return mp;
}

// The queries of an exact route (sparse, grouped): the zero-padded block and the exact-order norms in W, the status block cleared
// in front; query_prep raises ST_ZERO_QUERY.  No bf16 image and no per-query flags.
static int prep_exact_queries(Index* ix, Workspace& W, hipStream_t s, const float* d_q, uint32_t nq, size_t dim) {
    int rc;
    const uint32_t ld = ix->ld, bp_all = round_up(nq, SUPER);
    if ((rc = W.w_qp.ensure((size_t)bp_all * ld)) || (rc = W.w_qnorm.ensure(bp_all)) || (rc = W.w_thr.ensure(bp_all)) ||
        (rc = W.w_flags.ensure(SearchFlags::words(nq))))
        return rc;
    uint32_t* d_status = SearchFlags(W.w_flags.p, nq).status;
    HIP_TRY(hipMemsetAsync(d_status, 0, STATUS_BYTES, s));
    W.status_dirty = true;                                         // (the tiers' bookkeeping: the block is cleared again before its next use)
    vdb::QueryPrepParams qp{d_q, (uint32_t)dim, nq, W.w_qp.p, ld, bp_all, W.w_qnorm.p, W.w_thr.p, ix->metric, d_status,
                            nullptr, nullptr, nullptr, 0.0f, nullptr, nullptr};
    vdb::launch_query_prep(qp, s);
    return VDB_OK;
}

// The cut pass (re-threshold pass, screened range search): the filter pass of one block of up to SUPER queries whose thresholds are
// score cuts, then the select of EVERY key that passed -- up to CUT_KMAX per query, truncation flagged in d_ovf -- into W.w2_cand
// (counts: cand_counts(W)).  cut_pass_setup: the grid and the buffers, once per call.
constexpr uint32_t CUT_KMAX = MAX_SELECT, CUT_CAPL = 256;
struct CutGrid { uint32_t n_wg, n_sub; };
static uint32_t* cand_counts(Workspace& W) { return W.w_cnt.p + 2 * SUPER; }
static int cut_pass_setup(const Index* ix, Workspace& W, CutGrid* g) {
    int rc;
    g->n_wg = screen_grid(ix, vdb::fused_bf16_tile_rows());
    g->n_sub = vdb::fused_bf16_subpools_per_query(g->n_wg);
    if ((rc = W.w2_cand.ensure((size_t)SUPER * CUT_KMAX))) return rc;
    if ((rc = W.w_pool.ensure((size_t)SUPER * g->n_sub * CUT_CAPL))) return rc;
    return W.w_subcnt.ensure((size_t)SUPER * g->n_sub);
}
static void cut_pass(Index* ix, Workspace& W, hipStream_t s, const CutGrid& g, const uint32_t* d_rowmask, uint32_t* d_status,
                     const uint16_t* qb, const float* qg, const float* thr, uint32_t q0, uint32_t nb, uint32_t* d_ovf) {
    vdb::FusedBf16Params fp = screen_params(ix, W, d_rowmask, d_status, CUT_CAPL, g.n_wg);
    screen_queries(fp, ix, qb, qg, thr, q0);
    launch_filter_pass(ix, fp, s);
    vdb::SelectParams mp{};
    mp.keys = W.w_pool.p; mp.sub_counts = W.w_subcnt.p; mp.n_sub = g.n_sub; mp.capl = CUT_CAPL; mp.wg_major = 1;
    mp.kk = CUT_KMAX; mp.out_keys = W.w2_cand.p; mp.out_stride = CUT_KMAX; mp.out_cnt = cand_counts(W);
    mp.ovf = d_ovf + q0; mp.summary = nullptr; mp.flag_truncation = 1;
    vdb::launch_select(mp, nb, s);
}

// The compact re-run block of the queries `todo` (batch indices) that a tier could not certify: the w2_* buffers for
// them, the index list on the device, their padded rows and norms gathered (thresholds: -inf in the padding).
static int gather_compact(Index* ix, Workspace& W, hipStream_t s, const std::vector<uint32_t>& todo, size_t k, bool zero_flags) {
    int rc;
    
    const uint32_t nf = (uint32_t)todo.size(), nfp = round_up(nf, SUPER), ld = ix->ld;
    if ((rc = W.w2_qp.ensure((size_t)nfp * ld))) return rc;
    if ((rc = W.w2_qnorm.ensure(nfp))) return rc;
    if ((rc = W.w2_thr.ensure(nfp))) return rc;
    if ((rc = W.w2_outi.ensure((size_t)nf * k))) return rc;
    if ((rc = W.w2_outd.ensure((size_t)nf * k))) return rc;
    if ((rc = W.w2_outc.ensure(nf))) return rc;
    if ((rc = W.w2_flags.ensure(2 * (size_t)nf))) return rc;
    if ((rc = W.w2_qidx.ensure(nf))) return rc;
    HIP_TRY(hipMemcpyAsync(W.w2_qidx.p, todo.data(), (size_t)nf * 4, hipMemcpyHostToDevice, s));
    if (zero_flags) HIP_TRY(hipMemsetAsync(W.w2_flags.p, 0, 2 * (size_t)nf * 4, s));
    vdb::launch_gather_queries(W.w_qp.p, W.w_qnorm.p, ld, W.w2_qidx.p, nf, nfp, W.w2_qp.p, W.w2_qnorm.p, W.w2_thr.p, s);
    return VDB_OK;
}

// diagnostics (kn.rr_depth): the re-rank depth each query of the block ended at and its phase stamps, printed
static int dump_rerank_depth(Workspace& W, hipStream_t s, uint32_t nb, uint32_t kp_first) {
    std::vector<uint32_t> dep((size_t)SUPER * 17);
    HIP_TRY(hipMemcpyAsync(dep.data(), W.w_depth.p, dep.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // phase stamps (s_memrealtime, 100 MHz): 0 start, 1 query row in LDS, 2 round 1 staged+folded, 3 sorted, 4 depth decided, 5 last round folded, 6 end
    const uint64_t* st64 = reinterpret_cast<const uint64_t*>(dep.data() + SUPER);
    uint64_t t0 = ~0ull;
    for (uint32_t q = 0; q < nb; ++q) t0 = std::min(t0, st64[(size_t)q * 8]);
    for (int ph = 0; ph < 7; ++ph) {
        std::vector<double> v(nb);
        for (uint32_t q = 0; q < nb; ++q) v[q] = (double)(st64[(size_t)q * 8 + ph] - t0) * 0.01;
        std::sort(v.begin(), v.end());
        fprintf(stderr, "[vdb] re-rank phase %d at us: min %.2f median %.2f p90 %.2f max %.2f\n", ph, v[0], v[nb / 2], v[(size_t)nb * 9 / 10], v[nb - 1]);
    }
    std::sort(dep.begin(), dep.begin() + nb);
    fprintf(stderr, "[vdb] re-rank depth of %u queries: min %u  p25 %u  median %u  p75 %u  p95 %u  max %u  (first round %u)\n", nb,
            dep[0], dep[nb / 4], dep[nb / 2], dep[(size_t)nb * 3 / 4], dep[(size_t)nb * 95 / 100], dep[nb - 1], kp_first);
    return VDB_OK;
}

// ------------------------------------------------------------------ exact path for one query
int exact_one(Index* ix, Workspace& W, hipStream_t s, uint32_t q, size_t k, const uint32_t* d_rowmask, uint64_t* d_out_ids,
              float* d_out_dists, uint32_t* d_out_count) {
    int rc;
    uint32_t n = ix->n_uploaded;
    if ((rc = ensure_ranks(ix))) return rc;
    if ((rc = W.w_exact.ensure(n))) return rc;
    if ((rc = W.w_exsel.ensure(MAX_SELECT + 8))) return rc;
    if ((rc = W.w_cnt.ensure(4 * SUPER + 16))) return rc;
    vdb::ExactScanParams ep{rows_f32(ix), ix->ld, ix->dim, n, W.w_qp.p + (size_t)q * ix->ld, W.w_qnorm.p + q, ix->d_nd,
                            d_rowmask, ix->ids_monotone ? nullptr : ix->d_idrank.p, ix->metric, W.w_exact.p,
                            W.w_flags.p};
    vdb::launch_exact_scan(ep, s);
    uint32_t* cnt = W.w_cnt.p + 4 * SUPER;
    uint64_t* last = W.w_exsel.p + MAX_SELECT;      // largest key emitted so far (one u64 after the sort area)
    // k may be as large as the index: emit in chunks of MAX_SELECT, each chunk = the smallest keys
    // strictly above the previous chunk's last key
    for (size_t done = 0; done < k; done += MAX_SELECT) {
        uint32_t kk = (uint32_t)std::min<size_t>(MAX_SELECT, k - done);
        vdb::SelectParams sp{};
        sp.keys = W.w_exact.p; sp.stride = 0; sp.counts = nullptr; sp.n_fixed = n; sp.cap = n;
        sp.kk = kk; sp.out_keys = W.w_exsel.p; sp.out_stride = MAX_SELECT; sp.out_cnt = cnt;
        sp.out_thr = nullptr; sp.ovf = nullptr;
        sp.lo_excl = done ? last : nullptr; sp.out_last = last;
        vdb::launch_select(sp, 1, s);
        vdb::EmitParams em{W.w_exsel.p, MAX_SELECT, cnt, ix->ids_monotone ? nullptr : ix->d_rank2row.p,
                           ix->d_row_ids, d_out_ids + done, d_out_dists + done, d_out_count, kk, done ? 1u : 0u, n};
        vdb::launch_emit(em, s);
    }
    HIP_TRY(hipGetLastError());
    return VDB_OK;
}

// ------------------------------------------------------------------ the bounded exact scan, eight queries per pass over the rows
// The queries of `todo` (batch indices into the workspace's prepared queries) through launch_bounded_scan: a row survives for a
// query only if its exact distance passes the query's bound -- d_radii[q] if d_radii is given (the range scan), else the k-th
// exact distance the re-rank left in d_out_dists / d_out_counts (the kNN fallback).  The kk smallest survivors of query q go to
// d_out_*[q * kk ..], the survivor count to d_out_totals[q] if given.  `dense` receives the queries with more survivors than
// the key buffer holds (e.g. every row ties with the bound): their outputs are not valid, the caller runs exact_one for them.
constexpr uint32_t SCAN_CAP = 32768;                               // keys per query of a bounded pass
static int bounded_scan_queries(Index* ix, Workspace& W, hipStream_t s, const std::vector<uint32_t>& todo, uint32_t kk, const float* d_radii,
                                const uint32_t* d_rowmask, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                                uint64_t* d_out_totals, uint32_t* d_status, std::vector<uint32_t>& dense) {
    int rc;
    
    const uint32_t n = ix->n_uploaded;
    if ((rc = ensure_ranks(ix))) return rc;
    if ((rc = W.w_exact.ensure(std::max<size_t>((size_t)8 * SCAN_CAP, n)))) return rc;
    if ((rc = W.w_exsel.ensure((size_t)8 * MAX_SELECT + 8))) return rc;
    uint32_t* d_cnt8 = W.w_cnt.p + 3 * SUPER;                     // [8] survivors per query, [8..16) select counts
    for (size_t g0 = 0; g0 < todo.size(); g0 += 8) {
        const uint32_t nqf = (uint32_t)std::min<size_t>(8, todo.size() - g0);
        HIP_TRY(hipMemsetAsync(d_cnt8, 0, 16 * 4, s));
        vdb::BoundedScanParams ep{};
        ep.rows = rows_f32(ix); ep.ld = ix->ld; ep.dim = ix->dim; ep.n_rows = n; ep.qp = W.w_qp.p; ep.qnorm = W.w_qnorm.p;
        ep.nd = ix->d_nd; ep.rowmask = d_rowmask; ep.idrank = ix->ids_monotone ? nullptr : ix->d_idrank.p;
        ep.metric = ix->metric; ep.nqf = nqf;
        for (uint32_t j = 0; j < nqf; ++j) ep.qidx[j] = todo[g0 + j];
        if (d_radii) ep.radii = d_radii;
        else { ep.prev_dists = d_out_dists; ep.prev_counts = d_out_counts; ep.k = kk; }
        ep.keys = W.w_exact.p; ep.cap = SCAN_CAP; ep.cnt = d_cnt8; ep.status = d_status;
        vdb::launch_bounded_scan(ep, s);
        uint32_t h_cnt[8];
        HIP_TRY(hipMemcpyAsync(h_cnt, d_cnt8, nqf * 4, hipMemcpyDeviceToHost, s));
        vdb::SelectParams sp{};
        sp.keys = W.w_exact.p; sp.stride = SCAN_CAP; sp.counts = d_cnt8; sp.n_fixed = 0; sp.cap = SCAN_CAP; sp.kk = kk;
        sp.out_keys = W.w_exsel.p; sp.out_stride = MAX_SELECT; sp.out_cnt = d_cnt8 + 8;
        vdb::launch_select(sp, nqf, s);
        vdb::EmitMultiParams em{};
        em.keys = W.w_exsel.p; em.key_stride = MAX_SELECT; em.cnt = d_cnt8 + 8;
        em.survivors = d_cnt8; em.out_totals = d_out_totals;
        em.rank2row = ix->ids_monotone ? nullptr : ix->d_rank2row.p; em.row_ids = ix->d_row_ids; em.n_rows = n;
        em.out_ids = d_out_ids; em.out_dists = d_out_dists; em.out_count = d_out_counts; em.k = kk; em.nqf = nqf;
        for (uint32_t j = 0; j < nqf; ++j) em.qidx[j] = todo[g0 + j];
        vdb::launch_emit_multi(em, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
        for (uint32_t j = 0; j < nqf; ++j)
            if (h_cnt[j] > SCAN_CAP) dense.push_back(todo[g0 + j]);
    }
    return VDB_OK;
}

// ------------------------------------------------------------------ tier: f32 MFMA scores + certified re-rank
// Runs the f32 pipeline for the nq queries whose padded rows start at qp (stride ld; the block
// must be readable and zero up to a multiple of 256 rows, thr = -inf in the padding), writing results for query j
// at out_*[j*k ..] and the certification / pool-overflow flags at d_cert[j] / d_ovf[j].
// first_tier: no screening tier ran in front, so the sample, k' and the profiled kernel time the counters report are this tier's.
int pass_f32(Index* ix, Workspace& W, hipStream_t s, const float* qp, const float* qnorm, float* thr, uint32_t nq, size_t k, uint32_t kp,
             const uint32_t* d_rowmask, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_cert,
             uint32_t* d_ovf, uint32_t* d_status, bool first_tier) {
    int rc;
    const uint32_t n = ix->n_uploaded, ld = ix->ld;
    const bool small = n <= SMALL_N;
    (void)rows_f32(ix);                                              // this tier reads f32 rows, its re-rank included
    // Threshold sample size S: the fused pass keeps about n*kp/S keys per query, spread over 512 private
    // sub-pools of 64 slots and gathered into 16384 LDS slots by the select.  S is chosen so that this
    // expectation stays near 8000 or below (mean sub-pool fill <= 16), and the sample costs <= ~3 % of the
    // fused pass for k = 10.
    uint32_t S = n;
    if (!small) {
        uint64_t want = std::max<uint64_t>(n / 256u, (uint64_t)n * kp / 8000u);
        S = (uint32_t)std::min<uint64_t>(65536u, std::max<uint64_t>(2048u, pow2_ceil(want)));
        if (ix->kn.sample) S = std::min<uint32_t>(n, std::max(64u, ix->kn.sample));
    }
    // candidate pools: one private sub-pool per (query, row range, row part, lane half) of the fused kernel
    const uint32_t capl = 64;
    // sub-pools in one pass = queries * row ranges * row parts * 2 = 512 * n_cu for every kernel shape
    const size_t pass_subs = 512u * (size_t)ix->n_cu;
    if ((rc = W.w_dense.ensure((size_t)SUPER * S))) return rc;
    if ((rc = W.w_cand.ensure((size_t)SUPER * kp))) return rc;
    if (!small) {
        if ((rc = W.w_samp.ensure((size_t)SUPER * kp))) return rc;
        if ((rc = W.w_pool.ensure(pass_subs * capl))) return rc;
        if ((rc = W.w_subcnt.ensure(pass_subs))) return rc;
    }
    uint32_t* d_cnt_a = W.w_cnt.p;               // sample select counts
    uint32_t* d_cand_cnt = W.w_cnt.p + 2 * SUPER;
    if (first_tier) { W.stats[STAT_SAMPLE] = S; W.stats[STAT_KP] = kp; }
    const float eps = eps_coef(ix);

    for (uint32_t q0 = 0; q0 < nq; q0 += SUPER) {
        const uint32_t nb = std::min(SUPER, nq - q0);
        const uint32_t tiles = (nb + 31) / 32;
        // fused-kernel shape: 32 / 64 / 128 queries per workgroup; 2 workgroups per CU in flight
        const bool shape8 = !ix->kn.shape4;   // default: ONE 8-wave workgroup per CU, 256 queries share each fetched row tile (diagnostics: two 4-wave workgroups of 128 queries)
        const int nqt = (shape8 && tiles > 4) ? 8 : tiles > 2 ? 4 : (int)tiles;
        const uint32_t n_super = (tiles + nqt - 1) / nqt;          // workgroups along the query axis (1 or 2)
        const float* qp0 = qp + (size_t)q0 * ld;

        vdb::DenseParams dp{rows_f32(ix), ld, n, qp0, round_up(nb, 32), ix->d_alpha, ix->d_beta, d_rowmask, S,
                            W.w_dense.p, S};
        vdb::launch_dense_scores(dp, s);

        vdb::SelectParams sp{};
        sp.keys = W.w_dense.p; sp.stride = S; sp.counts = nullptr; sp.n_fixed = S; sp.cap = S; sp.kk = kp;
        sp.out_stride = kp;
        if (small) {
            sp.out_keys = W.w_cand.p; sp.out_cnt = d_cand_cnt; sp.out_thr = nullptr; sp.ovf = nullptr;
            vdb::launch_select(sp, nb, s);
        } else {
            // thresholds: the sample's kp-th score (padding queries were given -inf by query_prep)
            sp.out_keys = W.w_samp.p; sp.out_cnt = d_cnt_a; sp.out_thr = thr + q0; sp.ovf = nullptr;
            vdb::launch_select(sp, nb, s);
            const uint32_t n_wg = std::min<uint32_t>((nqt == 8 ? 1u : 2u) * (uint32_t)ix->n_cu / n_super, (n + 31) / 32);
            const uint32_t n_sub = vdb::fused_subpools_per_query(nqt, n_wg);
            vdb::FusedParams fp{rows_f32(ix), ld, n, qp, q0, ix->d_alpha, ix->d_beta, d_rowmask ? d_rowmask : ix->d_live,
                                thr, W.w_pool.p - (size_t)q0 * n_sub * capl,
                                W.w_subcnt.p - (size_t)q0 * n_sub, capl, n_wg,
                                ix->kn.fused_ablate};
            const bool prof = ix->profile && first_tier;          // with the screening tier on, ITS kernel is the one timed
            if (prof) HIP_TRY(hipEventRecord(ix->ev0, s));
            // 256-query passes: LDS-DMA staging, 3-image ring with the barrier in mid-stage; smaller batches: the
            // register-staged 128/64/32-query shapes.  (Diagnostics build: the 2-image and register-staged A/B variants.)
#ifdef VDB_DIAG
            if (nqt == 8 && ix->kn.regstage) vdb::launch_fused(fp, nqt, n_super, s);
            else if (nqt == 8 && ix->kn.dma2) vdb::launch_fused_dma(fp, n_super, s);
            else
#endif
            if (nqt == 8) vdb::launch_fused_dma3(fp, n_super, s);
            else vdb::launch_fused(fp, nqt, n_super, s);
            if (prof) {
                // one super-tile per event pair: wait here so the pair can be reused (profiling mode only)
                HIP_TRY(hipEventRecord(ix->ev1, s));
                HIP_TRY(hipEventSynchronize(ix->ev1));
                float ms = 0.f;
                HIP_TRY(hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
                W.stats[STAT_KERNEL_NS] += (uint64_t)((double)ms * 1e6);
            }
            W.stats[STAT_ROWS_SCANNED] += n;
            vdb::SelectParams mp{};
            mp.keys = W.w_pool.p; mp.stride = 0; mp.counts = nullptr; mp.n_fixed = 0; mp.cap = 0;
            mp.sub_counts = W.w_subcnt.p; mp.n_sub = n_sub; mp.capl = capl;
            mp.kk = kp; mp.out_keys = W.w_cand.p; mp.out_stride = kp; mp.out_cnt = d_cand_cnt;
            mp.out_thr = nullptr; mp.ovf = d_ovf + q0; mp.summary = status_summary(d_status);
            vdb::launch_select(mp, nb, s);
        }
        vdb::RerankParams rp = rerank_params(ix, d_rowmask, d_status, k, W.w_cand.p, kp, d_cand_cnt);
        rerank_io(rp, ix, qp, qnorm, d_out_ids, d_out_dists, d_out_counts, d_cert, q0);
        rp.eps_coef = eps;
        rp.thr = small ? nullptr : thr + q0;
        vdb::launch_rerank(rp, nb, s);
    }
    return VDB_OK;
}

// ------------------------------------------------------------------ tier: bf16 screening + certified re-rank
// Same structure, with the scores of the HBM-bound bf16 kernels (fused_bf16_common.h): group minima of a row
// sample -> per-query threshold -> one pass over all rows keeping the keys under the threshold -> the kp smallest
// keys -> exact re-rank, certified with the bf16 error bound.  Queries come from W0.w_qp / w_qb / w_qnorm: W0 is the search's
// workspace, W below the pass-local buffers of one pass (W0's, or the other workspace's for every second pass).
int pass_bf16(Index* ix, Workspace& W0, hipStream_t s, uint32_t nq, size_t k, const Bf16Plan& pl, const uint32_t* d_rowmask,
              uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_cert, uint32_t* d_ovf,
              uint32_t* d_status, float* d_thr_next, bool allow_alt) {
    int rc;
    const uint32_t n = ix->n_uploaded, ld = ix->ld;
    const uint32_t S = pl.S, kp = pl.kp, KT = pl.kt;
    const uint32_t M = vdb::fused_bf16_sample_groups(S);
    // private sub-pools of 256 slots: when the rows near a query are stored next to each other (data ordered by
    // cluster) most of the ~N*kt/S keys that pass land in ONE workgroup's four sub-pools; 4 x 256 slots hold about twice
    // the expected total, so that case stays on this tier instead of overflowing into the next.  The gather reads
    // counts and keys, never empty slots, so the capacity costs address space only (0.5 GB of workspace at 1M rows).
    const uint32_t capl = 256;
    const uint32_t n_wg = screen_grid(ix, vdb::fused_bf16_tile_rows());
    // ---- the layout of the rows.  A search can run over SPLIT rows if the filter pass may use the shadow-row
    // kernel at the store's pitch (ld % 64, no shadow of its own, the production kernel) and the sample pass has its compact
    // copy: that copy is made from f32 rows, so a stale one sends the rows back to F32 first.  A batch above 256 queries on a
    // SPLIT index runs as 256-query passes of that kernel (the wide kernel reads f32 rows), as over the shadow.
    Workspace& other = other_workspace(ix, W0);
    const bool split_able = ix->split_mode != 0 && !shadow_usable(ix) && ld % 64 == 0 && ix->sample_cache && !ix->kn.sample_block &&
                            ix->kn.fused_pipe && !ix->kn.bf16_ablate;
    if (ix->layout == vdb::LAYOUT_SPLIT && (!split_able || ix->sample16_n != n || ix->sample16_S != S)) (void)rows_f32(ix);
    const bool go_split = ix->layout == vdb::LAYOUT_SPLIT;
    // Batches above 256 queries: the WIDE filter kernel (kernels_fused_bf16w.hip, 128 rows x 512 queries per workgroup) serves
    // two 256-query blocks per fetch of the rows -- BASELINE config 3 (B = 1024) reads its shard twice per batch instead of
    // four times.  Not over the opt-in bf16 shadow rows (their kernel has the one shape); vdb_flat_set_wide(h, 0) turns it off.
    const bool use_wide = ix->wide && nq > SUPER && !shadow_usable(ix) && !go_split
#ifdef VDB_DIAG
                          && ix->kn.fused_pipe
#endif
        ;
    const uint32_t n_wg_w = screen_grid(ix, vdb::fused_bf16w_tile_rows());
    const uint32_t n_sub = vdb::fused_bf16_subpools_per_query(std::max(n_wg, use_wide ? n_wg_w : 0u));   // (both kernels write the 4-sub-pool layout)
    const size_t pool_block = (size_t)SUPER * n_sub * capl, cnt_block = (size_t)SUPER * n_sub;
    // A batch above 256 queries takes several passes.  They are independent, so they ALTERNATE between
    // this context and the handle's other workspace and stream when that one is idle: the latency-bound tail of pass i (its
    // slowest re-rank workgroups, a few CUs) then runs beside the head of pass i+1 instead of in front of it.  The per-query
    // arrays (queries, thresholds, flags, outputs) are indexed by q0 and shared; only the pass-local buffers are doubled.
    Workspace* alt = nullptr;
    if (allow_alt && nq > (use_wide ? 2 * SUPER : SUPER) && !ix->profile && !ix->kn.rr_depth) {
        if (!other.busy) alt = &other;
    }
    Workspace* const Wv[2] = {&W0, alt ? alt : &W0};
    const hipStream_t Sv[2] = {s, alt ? alt->stream : s};
    for (int t = 0; t < (alt ? 2 : 1); ++t) {
        Workspace* w = Wv[t];
        if ((rc = w->w_dense.ensure((size_t)SUPER * M))) return rc;
        if ((rc = w->w_cand.ensure((size_t)SUPER * kp))) return rc;
        if ((rc = w->w_samp.ensure((size_t)SUPER * std::max(kp, KT)))) return rc;
        if ((rc = w->w_pool.ensure((use_wide ? 2 : 1) * pool_block))) return rc;
        if ((rc = w->w_subcnt.ensure((use_wide ? 2 : 1) * cnt_block))) return rc;
        if ((rc = w->w_cnt.ensure(4 * SUPER + 16))) return rc;
    }
    // the sample pass runs over the compact bf16 copy of the sample rows when the row pitch allows (rebuilt here, before the
    // passes fork onto two streams, when rows were added since it was made -- mutators are refused while a search is in flight,
    // so nobody else is reading it; with ANOTHER search in flight and a different key this one keeps the f32 gather)
    bool sample_copy = ix->sample_cache && ld % 64 == 0 && !ix->kn.sample_block;
    if (sample_copy && (ix->sample16_n != n || ix->sample16_S != S)) {
        if (other.busy) sample_copy = false;
        else {
            const size_t need = (size_t)S * ld;
            if (ix->d_sample16.n < need) {
                if (ix->d_sample16) HIP_TRY(hipDeviceSynchronize());
                if (ix->d_sample16.alloc(need) != hipSuccess) { (void)hipGetLastError(); sample_copy = false; }   // no memory for the optional copy: f32 gather
            }
            if (sample_copy) {
                vdb::launch_sample_to_bf16(rows_f32(ix), ld, n, S, pl.shift, ix->d_sample16, s);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipStreamSynchronize(s));                    // once per change of the rows: later searches on OTHER streams read it
                ix->sample16_n = n; ix->sample16_S = S;
            }
        }
    }
    // the adaptive rule: consecutive searches that could run over SPLIT rows are counted (rows_f32 and every mutation reset the
    // count); after split_after of them the next one converts first -- under the handle mutex, and only while no other search of
    // this handle is in flight (its kernels read the rows), else not this time.  Mode 2 converts before the next such search.
    if (split_able && sample_copy && nq <= SUPER) {
        if (!go_split && !ix->split_refused && !other.busy && (ix->split_mode == 2 || ix->split_streak >= ix->split_after)) {
            if ((rc = rows_to_split(ix))) return rc;
        }
        ++ix->split_streak;
    }
    if (alt) {                                                   // the other stream starts behind query_prep and the row mask
        if ((rc = ix->ev_pass[0].create(hipEventDisableTiming)) || (rc = ix->ev_pass[1].create(hipEventDisableTiming))) return rc;
        HIP_TRY(hipEventRecord(ix->ev_pass[0], s));
        HIP_TRY(hipStreamWaitEvent(Sv[1], ix->ev_pass[0], 0));
    }
    W0.stats[STAT_SAMPLE] = S;
    const float eps = eps_coef(ix);
    // thresholds: sample pass + threshold select per 256-query block.  A batch of several passes computes ALL of them first, on the
    // caller's stream: left to their own pass, the second stream's small kernels queue up behind the first pass's filter kernel
    // (which owns every CU for a millisecond) and the second filter pass starts late.
    // a launch of this tier over pass-local buffers W: sample geometry and the diagnostics' ablation on top of screen_params
    auto pass_params = [&](Workspace& W) {
        vdb::FusedBf16Params fp = screen_params(ix, W, d_rowmask, d_status, capl, n_wg);
        fp.ablate = ix->kn.bf16_ablate;
        fp.n_sample = S; fp.sample_shift = pl.shift;
        fp.sample_block = ix->kn.sample_block ? (n / (S / 256u)) : 0u; fp.minkeys = W.w_dense.p; fp.minkey_stride = M;
        return fp;
    };
    auto thresholds_of = [&](Workspace& W, hipStream_t st, uint32_t qb0) {
        const uint32_t nb = std::min(SUPER, nq - qb0);
        vdb::FusedBf16Params fp = pass_params(W);
        screen_queries(fp, ix, W0.w_qb.p, W0.w_qg.p, W0.w_thr.p, qb0);
        if (sample_copy) {
            vdb::FusedBf16Params sp16 = fp;
            sp16.rows16 = ix->d_sample16;
            vdb::launch_sample_s16(sp16, st);
        } else vdb::launch_sample_bf16(fp, st);
        vdb::SelectParams sp{};
        sp.keys = W.w_dense.p; sp.stride = M; sp.counts = nullptr; sp.n_fixed = M; sp.cap = M; sp.kk = KT;
        sp.out_stride = KT; sp.out_keys = W.w_samp.p; sp.out_cnt = W.w_cnt.p; sp.out_thr = W0.w_thr.p + qb0; sp.ovf = nullptr;
        if (ix->d_margin) { sp.shift_g = W0.w_qg.p + qb0; sp.shift_m_bits = ix->d_scalars + 4; }   // plain-score sample -> lower-bound units
        vdb::launch_thr_select(sp, nb, st);
    };
    // (measured at config 3's shape: four 256-query passes 3.26 -> 3.09 ms with the thresholds first; the two 512-query passes
    // are better off with their own -- 2.75 against 2.84 ms: the second pass's thresholds then run beside the first pass's tail)
    const uint32_t n_passes = use_wide ? (nq + 2 * SUPER - 1) / (2 * SUPER) : (nq + SUPER - 1) / SUPER;
    const bool thr_first = alt != nullptr && n_passes > 2;
    if (thr_first) {
        for (uint32_t qb0 = 0; qb0 < nq; qb0 += SUPER) thresholds_of(W0, s, qb0);
        HIP_TRY(hipEventRecord(ix->ev_pass[0], s));               // (re-recorded: the other stream starts behind the thresholds)
        HIP_TRY(hipStreamWaitEvent(Sv[1], ix->ev_pass[0], 0));
    }
    for (uint32_t q0 = 0, pass = 0; q0 < nq; ++pass) {
        const bool wide = use_wide && nq - q0 > SUPER;            // two 256-query blocks share this pass's fetch of the rows
        const uint32_t n_blocks = wide ? 2u : 1u;
        Workspace& W = *Wv[pass & 1];                             // pass-local buffers
        const hipStream_t s = Sv[pass & 1];                       // (shadows the caller's stream inside the loop)
        uint32_t* d_cand_cnt = W.w_cnt.p + 2 * SUPER;
        vdb::FusedBf16Params fp = pass_params(W);
        // ---- thresholds of the pass's blocks (unless they were all computed up front)
        if (!thr_first)
            for (uint32_t b = 0; b < n_blocks; ++b) thresholds_of(W, s, q0 + b * SUPER);
        // ---- ONE pass over the rows for all of them
        screen_queries(fp, ix, W0.w_qb.p, W0.w_qg.p, W0.w_thr.p, q0);
        if (ix->profile) HIP_TRY(hipEventRecord(ix->ev0, s));
        if (wide) {
            fp.n_wg = n_wg_w; fp.pool_block_stride = pool_block; fp.cnt_block_stride = cnt_block;
            vdb::launch_fused_bf16w(fp, s);
        } else launch_filter_pass(ix, fp, s);
        if (ix->profile) {
            HIP_TRY(hipEventRecord(ix->ev1, s));
            HIP_TRY(hipEventSynchronize(ix->ev1));
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
            W0.stats[STAT_KERNEL_NS] += (uint64_t)((double)ms * 1e6);
        }
#ifdef VDB_DIAG
        // An ablated launch leaves wrong pools behind; if the step went on with them every query would fall through to the
        // slower tiers, and the extra milliseconds of f32 MFMA work change the clock the NEXT timed launch runs at (ablation
        // arms with broken results read 10-25 us low for that reason alone).  So the ablated launch is the timed one, and an
        // unablated launch (untimed) overwrites its pools: every arm of an A/B then runs the same step around the kernel.
        if (fp.ablate) {
            fp.ablate = 0;
            if (wide) vdb::launch_fused_bf16w(fp, s); else launch_filter_pass(ix, fp, s);
            W0.stats[STAT_ROWS_SCANNED] += n;
        }
#endif
        W0.stats[STAT_ROWS_SCANNED] += n;

        // ---- per block: the smallest pooled keys, then the exact re-rank
        for (uint32_t b = 0; b < n_blocks; ++b) {
            const uint32_t qb0 = q0 + b * SUPER, nb = std::min(SUPER, nq - qb0);
            vdb::SelectParams mp{};
            mp.keys = W.w_pool.p + (size_t)b * pool_block; mp.stride = 0; mp.counts = nullptr; mp.n_fixed = 0; mp.cap = 0;
            mp.sub_counts = W.w_subcnt.p + (size_t)b * cnt_block; mp.n_sub = vdb::fused_bf16_subpools_per_query(wide ? n_wg_w : n_wg);
            mp.capl = capl; mp.wg_major = 1;
            mp.kk = kp; mp.out_keys = W.w_cand.p; mp.out_stride = kp; mp.out_cnt = d_cand_cnt;
            mp.out_thr = nullptr; mp.ovf = d_ovf + qb0; mp.summary = status_summary(d_status);
            vdb::launch_select(mp, nb, s);

            vdb::RerankParams rp = rerank_params(ix, d_rowmask, d_status, k, W.w_cand.p, kp, d_cand_cnt);
            rerank_io(rp, ix, W0.w_qp.p, W0.w_qnorm.p, d_out_ids, d_out_dists, d_out_counts, d_cert, qb0);
            rp.eps_coef = eps;
            rp.thr = W0.w_thr.p + qb0;
            rp.qerr = W0.w_qerr.p + qb0; rp.c_acc = c_acc_bf16(ix); rp.lb_scores = ix->d_margin ? 1u : 0u;
            rp.kp_first = round_up((uint32_t)k + 38u, 16u); rp.kp_step = 32;
            rp.thr_next = d_thr_next ? d_thr_next + qb0 : nullptr;
            rp.cut_always = force_rethreshold(ix->tiers) ? 1u : 0u;
            // diagnostics build: the first re-rank round overridden, the depth each query ended at printed
            if (ix->kn.kp_first) rp.kp_first = ix->kn.kp_first;
            const bool dump_depth = ix->kn.rr_depth;
            if (dump_depth) {
                if ((rc = W.w_depth.ensure(SUPER * 17))) return rc;      // depth[q], then 8 x 64-bit phase stamps per query
                rp.depth = W.w_depth.p;
            }
            if (pl.large) {
                // 112 < k <= 1024: the large-k re-rank (first round k + k/8, at least k + 38; then as deep as the certificate asks)
                rp.kp_first = round_up((uint32_t)k + std::max<uint32_t>(38u, (uint32_t)k / 8u), 16u); rp.kp_step = 64;
                if (ix->kn.kp_first) rp.kp_first = ix->kn.kp_first;
                vdb::launch_rerank_large(rp, nb, s);
            } else vdb::launch_rerank(rp, nb, s);
            if (dump_depth && (rc = dump_rerank_depth(W, s, nb, rp.kp_first))) return rc;
        }
        q0 += n_blocks * SUPER;
    }
    if (alt) {                                                   // the caller's stream continues behind BOTH chains
        HIP_TRY(hipEventRecord(ix->ev_pass[1], Sv[1]));
        HIP_TRY(hipStreamWaitEvent(s, ix->ev_pass[1], 0));
    }
    return VDB_OK;
}

// ------------------------------------------------------------------ the batched search
// ------------------------------------------------------------------ tier 0b: the re-threshold pass
// For queries the screening tier re-ranked to its depth limit without a certificate, the k-th exact distance found so
// far still bounds the answer: rerank_kernel turned it into a score cut above which no row can enter the top k.  The
// queries are gathered into a compact block, the HBM-bound filter pass runs once more with those cuts as thresholds,
// and EVERY key that passes (up to 2048 per query) is re-ranked exactly: by rerank_all_kernel for k <= 112, by the exhaustive
// form of the large-k re-rank above that (k <= 1024).  Exact by construction; a query whose list does not fit (pool overflow,
// more than 2048 keys) keeps its flag and goes on to the next tier.
// todo: batch indices; cuts: their score cuts.  On return flags2 (host) holds cert / overflow per compact query.
int pass_rethreshold(Index* ix, Workspace& W, hipStream_t s, const std::vector<uint32_t>& todo, const std::vector<float>& cuts, size_t k,
                     const uint32_t* d_rowmask, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                     uint32_t* d_status, std::vector<uint32_t>& flags2) {
    int rc;
    const uint32_t n = ix->n_uploaded, ld = ix->ld;
    const uint32_t nf = (uint32_t)todo.size(), nfp = round_up(nf, SUPER);
    CutGrid grid;
    if ((rc = W.w2_qerr.ensure(nfp))) return rc;
    if ((rc = W.w2_qg.ensure(nfp))) return rc;
    if ((rc = W.w2_qb.ensure((size_t)nfp * ld))) return rc;
    if ((rc = cut_pass_setup(ix, W, &grid))) return rc;
    if ((rc = gather_compact(ix, W, s, todo, k, false))) return rc;          // (query_prep below zeroes the flags)
    uint32_t* d_cert2 = W.w2_flags.p;
    uint32_t* d_ovf2 = W.w2_flags.p + nf;
    // bf16 image, |q - bf16(q)| and zeroed flags of the compact block (the rows are already padded: dim = ld)
    vdb::QueryPrepParams qp{W.w2_qp.p, ld, nf, W.w2_qp.p, ld, nfp, W.w2_qnorm.p, W.w2_thr.p, vdb::EUCLID, d_status,
                            W.w2_qb.p, W.w2_qerr.p, ix->d_margin ? W.w2_qg.p : nullptr, margin_plan(ix).kappa, d_cert2, d_ovf2};
    vdb::launch_query_prep(qp, s);
    HIP_TRY(hipMemcpyAsync(W.w2_thr.p, cuts.data(), (size_t)nf * 4, hipMemcpyHostToDevice, s));   // padding queries keep -inf
    for (uint32_t q0 = 0; q0 < nf; q0 += SUPER) {
        const uint32_t nb = std::min(SUPER, nf - q0);
        cut_pass(ix, W, s, grid, d_rowmask, d_status, W.w2_qb.p, W.w2_qg.p, W.w2_thr.p, q0, nb, d_ovf2);
        W.stats[STAT_ROWS_SCANNED] += n;
        vdb::RerankParams rp = rerank_params(ix, d_rowmask, d_status, k, W.w2_cand.p, CUT_KMAX, cand_counts(W));
        rerank_io(rp, ix, W.w2_qp.p, W.w2_qnorm.p, W.w2_outi.p, W.w2_outd.p, W.w2_outc.p, d_cert2, q0);
        if (k <= BF16_MAX_K) vdb::launch_rerank_all(rp, nb, s);
        else vdb::launch_rerank_all_large(rp, nb, s);
    }
    HIP_TRY(hipGetLastError());
    flags2.assign(2 * (size_t)nf, 0u);
    HIP_TRY(hipMemcpyAsync(flags2.data(), W.w2_flags.p, 2 * (size_t)nf * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // only the queries this pass answered completely are written back
    std::vector<uint32_t> good;
    for (uint32_t j = 0; j < nf; ++j) if (flags2[j] && !flags2[nf + j]) good.push_back(j);
    if (!good.empty()) {
        // scatter compact results j -> batch position todo[j] (the scatter kernel walks a (source, destination) list)
        std::vector<uint32_t> src_dst(2 * good.size());
        for (size_t i = 0; i < good.size(); ++i) { src_dst[i] = good[i]; src_dst[good.size() + i] = todo[good[i]]; }
        if ((rc = W.w2_qidx.ensure(2 * good.size()))) return rc;
        HIP_TRY(hipMemcpyAsync(W.w2_qidx.p, src_dst.data(), src_dst.size() * 4, hipMemcpyHostToDevice, s));
        vdb::launch_scatter_results_list(W.w2_outi.p, W.w2_outd.p, W.w2_outc.p, W.w2_qidx.p, W.w2_qidx.p + good.size(),
                                         (uint32_t)good.size(), (uint32_t)k, d_out_ids, d_out_dists, d_out_counts, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
    }
    return VDB_OK;
}

// ------------------------------------------------------------------ the direct path of small indexes
// Index::search as it stands (flat_index.rs:52-65) -- every row's exact distance, the k smallest by (distance, id) -- for an
// index of at most 16384 rows and a batch of at most DIRECT_MAX_Q queries: BASELINE configs[0] (benches/search_bench.rs:18-33:
// 10k x 128, ONE query).  At that size the tiered pipeline is five launches of latency (query preparation, dense MFMA scores,
// select, re-rank, flag copy: ~90 us per call); here it is TWO kernels and one stream synchronisation -- small_scan_kernel reads
// the raw queries (from wherever they are: the host-pointer entry point hands over MAPPED host memory, so no copy is enqueued at
// all) and writes one exact key per row, select_kernel in EMIT mode writes ids, distances, counts and the status word straight
// into the caller's buffers (mapped host memory again for the host-pointer entry point).  Exact by construction: no certificate.
bool direct_eligible(const Index* ix, size_t n_rows, size_t nq, size_t k) {
    return !(ix->tiers & VDB_TIERS_NO_DIRECT) && n_rows > 0 && n_rows <= SMALL_N && nq > 0 && nq <= DIRECT_MAX_Q && k > 0 && k <= MAX_SELECT;
}

int ensure_host_io(Workspace& W, size_t bytes) {
    return W.h_io.ensure(std::max<size_t>(bytes, 1u << 16));
}

static int search_direct(Index* ix, Workspace& W, hipStream_t s, const float* d_q, uint32_t nq, size_t k, const uint32_t* d_rowmask,
                         uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts) {
    int rc;
    
    const uint32_t n = ix->n_uploaded;
    if ((rc = ensure_ranks(ix))) return rc;
    // every workgroup of the scan keeps its k smallest keys only (k < 256): the select ranks n/256 * k keys instead of n
    const uint32_t keep = k < 256 ? (uint32_t)k : 0u;
    const uint32_t n_keys = keep ? vdb::small_scan_groups(n) * keep : n;
    if ((rc = W.w_exact.ensure((size_t)nq * std::max(n_keys, n)))) return rc;
    if ((rc = W.w_exsel.ensure((size_t)nq * MAX_SELECT + 8))) return rc;
    if ((rc = W.w_cnt.ensure(4 * SUPER + 16))) return rc;
    if (!W.dstat_ready) {
        if ((rc = W.w_dstat.ensure(4))) return rc;
        if ((rc = W.h_dstat.ensure(16))) return rc;
        HIP_TRY(hipMemsetAsync(W.w_dstat.p, 0, 16, s));
        W.dstat_ready = true;
    }
    vdb::SmallScanParams sp{rows_f32(ix), ix->ld, ix->dim, n, d_q, nq, ix->d_nd, d_rowmask, ix->ids_monotone ? nullptr : ix->d_idrank.p,
                            ix->metric, W.w_exact.p, n_keys, keep, W.w_dstat.p};
    vdb::launch_small_scan(sp, s);
    vdb::SelectParams mp = emit_select_params(ix, W, k);
    mp.keys = W.w_exact.p; mp.stride = n_keys; mp.counts = nullptr; mp.n_fixed = n_keys; mp.cap = n_keys;
    mp.emit_ids = d_out_ids; mp.emit_dists = d_out_dists; mp.emit_counts = d_out_counts;
    mp.emit_status_in = W.w_dstat.p; mp.emit_status = W.h_dstat.d;
    vdb::launch_select(mp, nq, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    uint32_t status = 0;
    for (uint32_t q = 0; q < nq; ++q) status |= W.h_dstat[q];
    W.stats[STAT_EXACT] = nq;                                      // answered by an exact scan
    if (status) {                                                  // (rare: leave the device word clean for the next search)
        HIP_TRY(hipMemsetAsync(W.w_dstat.p, 0, 16, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (status & vdb::ST_ZERO_QUERY) return fail_zero_vector();
    if (status & vdb::ST_NAN) return fail_nan();
    return VDB_OK;
}

// ------------------------------------------------------------------ the sparse-filter route (vdb_flat_set_sparse_filter)
// A masked search whose filter leaves few rows eligible reads ONLY those rows: the set bits of the row mask become an ascending
// list of device rows (kernels_sparse.hip: popcount per block, one-workgroup scan, scatter -- the host reads E, 4 bytes, in
// between), sparse_scan_kernel computes the reference distance of every (query, eligible row) pair, select_kernel in EMIT mode
// writes the k smallest by (distance, id) as final results.  Exact by construction, like the direct path: no certificate.
//
// The automatic mode (2) takes the route when E * nq * dim <= C * n_rows * ld: the pair arithmetic of the scan against the one
// HBM pass over the store that the tiers make.  C is a MEASUREMENT (tools/sparse_filter_bench.py), not an
// estimate; until the grid has been measured it is 0 and mode 2 never sends a non-empty list to the route.
constexpr double SPARSE_AUTO_C = 0.0;
size_t sparse_limit(size_t n_rows, size_t ld, size_t dim, size_t nq) {
    if (!n_rows) return 0;
    const size_t cap = std::min<size_t>(n_rows, SPARSE_MAX_E);
    const double per_row = (double)std::max<size_t>(nq, 1) * (double)std::max<size_t>(dim, 1);
    const double e = SPARSE_AUTO_C * (double)n_rows * (double)std::max<size_t>(ld, 1) / per_row;
    return e >= (double)cap ? cap : (size_t)e;
}

// E = set bits of the row mask below n_uploaded, read back to the host (one synchronisation)
int eligible_count(Index* ix, Workspace& W, hipStream_t s, const uint32_t* d_rowmask, uint32_t* out_E) {
    int rc;
    const uint32_t n = ix->n_uploaded, nb = vdb::sparse_list_blocks(n);
    if ((rc = W.w_eligblk.ensure(2 * (size_t)nb + 4))) return rc;
    uint32_t* blk = W.w_eligblk.p;
    vdb::launch_sparse_count(d_rowmask, n, blk, blk + nb, blk + 2 * (size_t)nb, s);
    HIP_TRY(hipGetLastError());
    uint32_t E = 0;
    HIP_TRY(hipMemcpyAsync(&E, blk + 2 * (size_t)nb, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (E > n) return fail(VDB_ERR_DEVICE, "eligible-row count %u exceeds the %u rows of the store", E, n);
    *out_E = E;
    return VDB_OK;
}
// ... and the list itself, w_elig[0..E), from the block offsets eligible_count left behind
int eligible_list(Index* ix, Workspace& W, hipStream_t s, const uint32_t* d_rowmask, uint32_t E) {
    int rc;
    const uint32_t n = ix->n_uploaded, nb = vdb::sparse_list_blocks(n);
    if ((rc = W.w_elig.ensure(std::max<size_t>(E, 1)))) return rc;
    vdb::launch_sparse_scatter(d_rowmask, n, W.w_eligblk.p + nb, W.w_elig.p, E, s);
    HIP_TRY(hipGetLastError());
    return VDB_OK;
}

static int search_sparse(Index* ix, Workspace& W, hipStream_t s, const float* d_q, uint32_t nq, size_t dim, size_t k, uint32_t E,
                         const uint32_t* d_rowmask, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts) {
    int rc;
    
    const uint32_t n = ix->n_uploaded, ld = ix->ld;
    // (ST_ZERO_QUERY is raised also when nothing is eligible)
    if ((rc = prep_exact_queries(ix, W, s, d_q, nq, dim))) return rc;
    uint32_t* d_status = SearchFlags(W.w_flags.p, nq).status;
    if (E == 0) HIP_TRY(hipMemsetAsync(d_out_counts, 0, (size_t)nq * 4, s));
    else {
        if ((rc = ensure_ranks(ix))) return rc;
        if ((rc = eligible_list(ix, W, s, d_rowmask, E))) return rc;
        const uint32_t stride = round_up(E, vdb::SPARSE_TILE_R);
        if ((rc = W.w_exact.ensure((size_t)std::min(nq, SUPER) * stride))) return rc;
        if ((rc = W.w_exsel.ensure((size_t)SUPER * MAX_SELECT + 8))) return rc;
        if ((rc = W.w_cnt.ensure(4 * SUPER + 16))) return rc;
        for (uint32_t q0 = 0; q0 < nq; q0 += SUPER) {              // passes of SUPER queries: the key buffer stays bounded
            const uint32_t nb = std::min(SUPER, nq - q0);
            vdb::SparseScanParams sp{rows_f32(ix), ld, ix->dim, n, W.w_elig.p, E, W.w_qp.p + (size_t)q0 * ld, W.w_qnorm.p + q0, nb,
                                     ix->d_nd, ix->ids_monotone ? nullptr : ix->d_idrank.p, ix->metric, W.w_exact.p, stride, d_status};
            vdb::launch_sparse_scan(sp, s);
            vdb::SelectParams mp = emit_select_params(ix, W, k);
            mp.keys = W.w_exact.p; mp.stride = stride; mp.counts = nullptr; mp.n_fixed = stride; mp.cap = stride;
            mp.emit_ids = d_out_ids + (size_t)q0 * k; mp.emit_dists = d_out_dists + (size_t)q0 * k; mp.emit_counts = d_out_counts + q0;
            vdb::launch_select(mp, nb, s);
        }
    }
    HIP_TRY(hipGetLastError());
    uint32_t st[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(st, d_status, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    W.stats[STAT_EXACT] = nq;                                      // answered by an exact scan
    ix->sparse_last = 1; ++ix->sparse_count;
    if (st[0] & vdb::ST_ZERO_QUERY) return fail_zero_vector();
    if (st[0] & vdb::ST_NAN) return fail_nan();
    return VDB_OK;
}

// distance.rs:21-26: the first row whose dimension differs from the query's fails the search
int query_dim_check(const Index* ix, size_t dim) {
    if (ix->n_live && ix->dim != dim) return fail_dim(dim, ix->dim);
    for (auto& kv : ix->misfits)
        if (kv.second.size() != dim) return fail_dim(dim, kv.second.size());
    if (!ix->misfits.empty()) {
        // every stored row has the query's dimension but none is on the device (zero-length rows)
        return fail(VDB_ERR_INVALID_ARGUMENT, "zero-dimensional vectors are not searchable");
    }
    return VDB_OK;
}

// Part 1: checks, workspace, and the FIRST tier enqueued on the stream -- no host synchronisation unless the search is
// one of the cases answered completely here (empty store, k = 0, k too large for the MFMA tiers).
int search_part1(Index* ix, Workspace& W, const float* d_q, size_t nq, size_t dim, size_t k, const uint64_t* d_idmask,
                 size_t mask_bits, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                 hipStream_t user_stream, bool allow_alt) {
    int rc;
    W.ctx.pending = false;
    ix->sparse_last = 0;
    if ((rc = set_device(ix))) return rc;
    if ((rc = flush(ix))) return rc;
    if (nq == 0) return VDB_OK;
    // all launches of this search go to the caller's stream when one is given (so that the caller's
    // events bracket them); the workspace is protected by the handle mutex and the final sync
    hipStream_t s = user_stream ? user_stream : W.stream;
    memset(W.stats, 0, sizeof(W.stats));
    W.stats[STAT_SHADOW] = shadow_usable(ix) ? 1u : 0u;   // the screening pass reads the bf16 shadow rows
    W.stats[STAT_DIAG] = ix->kn.any ? 1u : 0u;            // diagnostics build with a knob set: the run is NOT covered by the exactness guarantee
    const auto t_entry = std::chrono::steady_clock::now();
    auto since = [&]() { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_entry).count(); };
    size_t total_rows = ix->n_live + ix->misfits.size();
    if (total_rows == 0 || k == 0) {   // storage.rs:218-220: empty store -> Ok(vec![]) before any check
        HIP_TRY(hipMemsetAsync(d_out_counts, 0, nq * 4, s));
        HIP_TRY(hipStreamSynchronize(s));
        return VDB_OK;
    }
    if ((rc = pre_device_checks(ix, dim, nq > 0x7fffffffull / 2 || k > 0x7fffffffull))) return rc;

    const uint32_t n = ix->n_uploaded;
    const uint32_t ld = ix->ld;
    const uint32_t nq32 = (uint32_t)nq;
    const uint32_t bp_all = round_up(nq32, SUPER);
    const uint32_t kp = pick_kp(k);

    // ---- sparse-filter route (off by default): a masked search scans only the rows its filter leaves eligible.  Mode 1 takes it
    // whenever the select can hold k and the list fits; mode 2 also asks the measured cost limit and leaves small indexes to the
    // direct path.  Answered completely here, like the direct path; otherwise the search goes on below as if nothing had happened.
    if (ix->sparse_mode && d_idmask) {
        const uint32_t* d_rowmask;
        if ((rc = eligibility_mask(ix, W, s, d_idmask, mask_bits, &d_rowmask))) return rc;
        uint32_t E = 0;
        if ((rc = eligible_count(ix, W, s, d_rowmask, &E))) return rc;
        ix->sparse_E = E;
        bool take = k <= MAX_SELECT && E <= SPARSE_MAX_E;
        if (ix->sparse_mode == 2) take = take && !direct_eligible(ix, n, nq, k) && E <= sparse_limit(n, ld, ix->dim, nq);
        if (take) {
            rc = search_sparse(ix, W, s, d_q, nq32, dim, k, E, d_rowmask, d_out_ids, d_out_dists, d_out_counts);
            W.stats[STAT_ENQUEUED_NS] = W.stats[STAT_FLAGS_NS] = W.stats[STAT_TOTAL_NS] = since();
            return rc;
        }
    }

    // ---- small index, a few queries: the direct exact path (two kernels, answered completely here)
    if (direct_eligible(ix, n, nq, k)) {
        const uint32_t* d_rowmask;
        if ((rc = eligibility_mask(ix, W, s, d_idmask, mask_bits, &d_rowmask))) return rc;
        rc = search_direct(ix, W, s, d_q, nq32, k, d_rowmask, d_out_ids, d_out_dists, d_out_counts);
        W.stats[STAT_ENQUEUED_NS] = W.stats[STAT_FLAGS_NS] = W.stats[STAT_TOTAL_NS] = since();
        return rc;
    }

    // ---- workspace
    if ((rc = W.w_qp.ensure((size_t)bp_all * ld))) return rc;
    if ((rc = W.w_qnorm.ensure(bp_all))) return rc;
    if ((rc = W.w_thr.ensure(bp_all))) return rc;
    const size_t flag_words = SearchFlags::words(nq32);           // status block | cert | overflow | score cut per query
    if ((rc = W.w_flags.ensure(flag_words))) return rc;
    if ((rc = W.h_flags.ensure(flag_words))) return rc;
    const SearchFlags df(W.w_flags.p, nq32);
    uint32_t* const d_status = df.status;
    // the per-query flags are zeroed by query_prep; the 16-byte status block only needs a memset when the last
    // search left it set (or the buffer is new) -- one launch less at the head of every search
    const bool flags_by_prep = kp != 0 || (ix->screen && plan_bf16(ix, n, k).kp);
    if (!flags_by_prep) HIP_TRY(hipMemsetAsync(W.w_flags.p, 0, flag_words * 4, s));
    else if (W.status_dirty || W.w_flags.p != W.status_buf) {
        HIP_TRY(hipMemsetAsync(d_status, 0, STATUS_BYTES, s));
        W.status_buf = W.w_flags.p;
    }
    W.status_dirty = true;                               // until a clean status word has been read back

    const uint32_t* d_rowmask;
    if ((rc = eligibility_mask(ix, W, s, d_idmask, mask_bits, &d_rowmask))) return rc;

    // ---- queries: zero-padded copy + exact-order norms
    {
        uint16_t* qb = nullptr;
        if (ix->screen && plan_bf16(ix, n, k).kp) {
            if ((rc = W.w_qb.ensure((size_t)bp_all * ld))) return rc;
            if ((rc = W.w_qerr.ensure(bp_all))) return rc;
            if ((rc = W.w_qg.ensure(bp_all))) return rc;
            qb = W.w_qb.p;
        }
        vdb::QueryPrepParams qp{d_q, (uint32_t)dim, nq32, W.w_qp.p, ld, bp_all, W.w_qnorm.p, W.w_thr.p, ix->metric, d_status, qb,
                                W.w_qerr.p, (qb && ix->d_margin) ? W.w_qg.p : nullptr, margin_plan(ix).kappa,
                                flags_by_prep ? df.cert : nullptr, flags_by_prep ? df.ovf : nullptr};
        vdb::launch_query_prep(qp, s);
    }

    if (kp == 0 && !(ix->screen && plan_bf16(ix, n, k).kp)) {
        // large k: exact scan for every query
        const SearchFlags hf(W.h_flags, nq32);
        HIP_TRY(hipMemcpyAsync(hf.status, d_status, STATUS_BYTES, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (hf.status[0] & vdb::ST_ZERO_QUERY)
            return fail_zero_vector();
        for (uint32_t q = 0; q < nq32; ++q) {
            if ((rc = exact_one(ix, W, s, q, k, d_rowmask, d_out_ids + (size_t)q * k, d_out_dists + (size_t)q * k,
                                d_out_counts + q)))
                return rc;
        }
        W.stats[STAT_EXACT] = nq32;
        HIP_TRY(hipMemcpyAsync(hf.status, d_status, STATUS_BYTES, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (hf.status[0] & vdb::ST_NAN) return fail_nan();
        return VDB_OK;
    }

    // ---- tiers.  Large indexes: the bf16 screening tier first (HBM-bound pass), the queries it cannot certify
    // are re-run as a compact block by the f32 MFMA tier; whatever that cannot certify goes to the exact scan.
    const Bf16Plan pl16 = ix->screen ? plan_bf16(ix, n, k) : Bf16Plan{};
    const uint32_t kp16 = pl16.kp;
    if ((rc = W.w_cnt.ensure(4 * SUPER + 16))) return rc;
    if (kp16) {
        W.stats[STAT_SCREENED] = 1;
        W.stats[STAT_KP] = kp16;
        if ((rc = pass_bf16(ix, W, s, nq32, k, pl16, d_rowmask, d_out_ids, d_out_dists, d_out_counts, df.cert, df.ovf, d_status,
                            df.cut, allow_alt)))
            return rc;
    } else {
        if ((rc = pass_f32(ix, W, s, W.w_qp.p, W.w_qnorm.p, W.w_thr.p, nq32, k, kp, d_rowmask, d_out_ids, d_out_dists,
                           d_out_counts, df.cert, df.ovf, d_status, true)))
            return rc;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(W.h_flags, W.w_flags.p, flag_words * 4, hipMemcpyDeviceToHost, s));
    W.stats[STAT_ENQUEUED_NS] = since();                      // host time until everything of the first tier is enqueued, ns
    Workspace::SearchCtx& c = W.ctx;
    c.pending = true; c.nq32 = nq32; c.kp = kp; c.kp16 = kp16; c.k = k; c.s = s; c.d_rowmask = d_rowmask;
    c.d_out_ids = d_out_ids; c.d_out_dists = d_out_dists; c.d_out_counts = d_out_counts; c.t_entry = t_entry;
    return VDB_OK;
}

// Part 2: wait for the first tier, read its flags, run the fallback tiers for the queries it could not certify.
// *changed (may be null) tells whether outputs were rewritten after part 1's pass.
int search_part2(Index* ix, Workspace& W, int* changed) {
    if (changed) *changed = 0;
    Workspace::SearchCtx& c = W.ctx;
    if (!c.pending) return VDB_OK;
    c.pending = false;
    int rc;
    const uint32_t nq32 = c.nq32, kp = c.kp, kp16 = c.kp16;
    const size_t k = c.k;
    hipStream_t s = c.s;
    const uint32_t* d_rowmask = c.d_rowmask;
    uint64_t* d_out_ids = c.d_out_ids; float* d_out_dists = c.d_out_dists; uint32_t* d_out_counts = c.d_out_counts;
    uint32_t* d_status = SearchFlags(W.w_flags.p, nq32).status;
    const SearchFlags hf(W.h_flags, nq32);                        // the first tier's flags, once the stream has been waited for
    const auto t_entry = c.t_entry;
    auto since = [&]() { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_entry).count(); };
    HIP_TRY(hipStreamSynchronize(s));
    W.stats[STAT_FLAGS_NS] = since();            // ... until the first tier's flags are on the host, ns
    uint32_t status = hf.status[0];
    if (status & vdb::ST_ZERO_QUERY) return fail_zero_vector();
    // the hand-over (vdb_flags.h): who is settled, who takes the re-threshold pass.  vdb_flat_set_tiers forces it (tests); every
    // tier returns the same results
    TierTriage tri = tier_triage(hf.cert, hf.ovf, hf.cut, nq32, ix->tiers, kp16, kp);
    W.stats[STAT_OVERFLOW] += tri.n_overflow;
    W.stats[STAT_UNCERTIFIED] += tri.n_uncertified;
    if (changed && !tri.todo.empty()) *changed = 1;
    std::vector<uint32_t> todo;
    if (tri.rethreshold) {
        // ---- tier 0b: queries with a known score cut get one more HBM-bound pass with that cut as the threshold
        if (!tri.sel.empty()) {
            std::vector<uint32_t> fl;
            if ((rc = pass_rethreshold(ix, W, s, tri.sel, tri.cuts, k, d_rowmask, d_out_ids, d_out_dists, d_out_counts, d_status, fl))) return rc;
            W.stats[STAT_RETHRESHOLD] += after_rethreshold(tri.sel, fl, tri.rest, &W.stats[STAT_OVERFLOW]);
        }
        todo.swap(tri.rest);
    } else todo.swap(tri.todo);
    if (kp16 && !todo.empty()) {
        // ---- second tier: the uncertified queries as one compact block through the f32 MFMA pipeline
        const uint32_t nf = (uint32_t)todo.size();
        W.stats[STAT_TO_F32] = nf;
        if ((rc = gather_compact(ix, W, s, todo, k, true))) return rc;
        if (!tri.f32_tier) {
            // k too large for the f32 tier (the large-k screening tier's uncertified queries): straight to the exact scan (flags stay 0)
        } else {
            if ((rc = pass_f32(ix, W, s, W.w2_qp.p, W.w2_qnorm.p, W.w2_thr.p, nf, k, kp, d_rowmask, W.w2_outi.p,
                               W.w2_outd.p, W.w2_outc.p, W.w2_flags.p, W.w2_flags.p + nf, d_status, false)))
                return rc;
            vdb::launch_scatter_results(W.w2_outi.p, W.w2_outd.p, W.w2_outc.p, W.w2_qidx.p, nf, (uint32_t)k,
                                        d_out_ids, d_out_dists, d_out_counts, s);
        }
        HIP_TRY(hipGetLastError());
        std::vector<uint32_t> f2(2 * (size_t)nf + STATUS_WORDS);   // cert | overflow of the compact block | the status block
        HIP_TRY(hipMemcpyAsync(f2.data(), W.w2_flags.p, 2 * (size_t)nf * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(f2.data() + 2 * (size_t)nf, d_status, STATUS_BYTES, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        status |= f2[2 * (size_t)nf];
        if (status & vdb::ST_ZERO_QUERY)
            return fail_zero_vector();
        todo = after_f32(todo, f2.data(), ix->tiers, &W.stats[STAT_OVERFLOW]);
    }
    // ---- exact fallback for the queries the MFMA tiers could not certify.  Up to 8 of them share one pass
    // over the rows; a row survives for a query only if its exact distance is <= the k-th exact distance
    // the re-rank already found (a valid upper bound), so each query is left with a handful of keys.
    const uint32_t n_fallback = (uint32_t)todo.size();
    if (!todo.empty()) {
        std::vector<uint32_t> dense;                             // queries whose bounded pass overflowed
        if ((rc = bounded_scan_queries(ix, W, s, todo, (uint32_t)k, nullptr, d_rowmask, d_out_ids, d_out_dists, d_out_counts, nullptr,
                                       d_status, dense)))
            return rc;
        for (uint32_t q : dense)
            if ((rc = exact_one(ix, W, s, q, k, d_rowmask, d_out_ids + (size_t)q * k, d_out_dists + (size_t)q * k,
                                d_out_counts + q)))
                return rc;
    }
    W.stats[STAT_TOTAL_NS] = since();            // whole call, ns
    W.stats[STAT_MFMA] = nq32 - n_fallback;
    W.stats[STAT_EXACT] = n_fallback;
    uint32_t st2 = status;
    if (n_fallback) {
        HIP_TRY(hipMemcpyAsync(hf.status, d_status, STATUS_BYTES, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        st2 |= hf.status[0];
    }
    // status bits, the summary word, or a query norm beyond the kernels' no-NaN domain (word 2 is a running maximum: tame
    // values may stay, a wild one must not outlive its search)
    W.status_dirty = st2 != 0 || W.stats[STAT_UNCERTIFIED] != 0 || W.stats[STAT_OVERFLOW] != 0 || *status_qmax(hf.status) > 0x53800000u;
    if (st2 & vdb::ST_NAN)
        return fail_nan();
    return VDB_OK;
}

// ------------------------------------------------------------------ the exact range search
// Every eligible row with reference distance d <= radius, ascending by (distance, id): the first min(total, max_results) and
// the total per query.  No reference counterpart; the machinery is the re-threshold pass's with the radius in the place of the
// k-th exact distance:
//   1. screened route (screening tier on, n >= BF16_MIN_ROWS): query_prep, range_cut_kernel (threshold = score_cut(radius): every
//      row scoring above it lies strictly beyond the radius), the bf16 filter pass per 256 queries, the select of up to 2048 keys
//      with truncation flagged, range_rerank_kernel -- every key evaluated exactly.  No sample pass.
//   2. exact range scan, eight queries per pass over the rows: everything route 1 does not serve or could not finish (pool or
//      select overflow, no finite cut, a NaN-score key).
//   3. dense fallback: more than 32768 survivors -> exact_one for the first max_results (all within the radius); the total is
//      route 2's counter.
// (the caller checked the radii: none is NaN)
static int range_search_run(Index* ix, Workspace& W, const float* d_q, size_t nq, size_t dim, const float* d_radii,
                            const uint64_t* d_idmask, size_t mask_bits, size_t max_results, uint64_t* d_out_ids, float* d_out_dists,
                            uint32_t* d_out_counts, uint64_t* d_out_totals, hipStream_t s, uint64_t* st) {
    int rc;
    
    const size_t total_rows = ix->n_live + ix->misfits.size();
    if (total_rows == 0) {                                         // as the searches: an empty store answers before any check
        HIP_TRY(hipMemsetAsync(d_out_counts, 0, nq * 4, s));
        if (d_out_totals) HIP_TRY(hipMemsetAsync(d_out_totals, 0, nq * 8, s));
        HIP_TRY(hipStreamSynchronize(s));
        return VDB_OK;
    }
    if ((rc = pre_device_checks(ix, dim, nq > 0x7fffffffull / 2))) return rc;

    const uint32_t n = ix->n_uploaded, ld = ix->ld, nq32 = (uint32_t)nq, bp_all = round_up(nq32, SUPER);
    const uint32_t mr = (uint32_t)max_results;
    (void)rows_f32(ix);                                            // both routes read f32 rows (range_rerank_kernel, the range scan)
    const bool screened = ix->screen && n >= BF16_MIN_ROWS;

    // ---- workspace.  Flags: status block | overflow | no cut | complete | keys evaluated, per query; all zeroed here
    if ((rc = W.w_qp.ensure((size_t)bp_all * ld))) return rc;
    if ((rc = W.w_qnorm.ensure(bp_all))) return rc;
    if ((rc = W.w_thr.ensure(bp_all))) return rc;
    if ((rc = W.w_flags.ensure(RangeFlags::words(nq32)))) return rc;
    if ((rc = W.w_cnt.ensure(4 * SUPER + 16))) return rc;
    const RangeFlags df(W.w_flags.p, nq32);
    uint32_t* const d_status = df.status;
    HIP_TRY(hipMemsetAsync(W.w_flags.p, 0, RangeFlags::words(nq32) * 4, s));
    W.status_dirty = true;                                        // (the tiers' bookkeeping: the block is cleared again before its next use)

    const uint32_t* d_rowmask;
    if ((rc = eligibility_mask(ix, W, s, d_idmask, mask_bits, &d_rowmask))) return rc;

    // ---- queries: zero-padded copy, exact-order norms; for the screened route the bf16 image, |q - bf16(q)| and g_q as a search prepares them
    if (screened) {
        if ((rc = W.w_qb.ensure((size_t)bp_all * ld))) return rc;
        if ((rc = W.w_qerr.ensure(bp_all))) return rc;
        if ((rc = W.w_qg.ensure(bp_all))) return rc;
    }
    {
        vdb::QueryPrepParams qp{d_q, (uint32_t)dim, nq32, W.w_qp.p, ld, bp_all, W.w_qnorm.p, W.w_thr.p, ix->metric, d_status,
                                screened ? W.w_qb.p : nullptr, W.w_qerr.p, (screened && ix->d_margin) ? W.w_qg.p : nullptr,
                                margin_plan(ix).kappa, nullptr, nullptr};
        vdb::launch_query_prep(qp, s);
    }

    std::vector<uint32_t> todo;                                    // batch indices for the exact range scan
    if (screened) {
        CutGrid grid;
        if ((rc = cut_pass_setup(ix, W, &grid))) return rc;
        // thresholds: score_cut(radius) from the constants the re-rank hands to score_cut (pass_bf16)
        vdb::RangeCutParams cp{};
        cp.cert = rerank_params(ix, d_rowmask, d_status, mr, nullptr, CUT_KMAX, nullptr);
        cp.cert.qnorm = W.w_qnorm.p; cp.cert.eps_coef = eps_coef(ix);
        cp.cert.qerr = W.w_qerr.p; cp.cert.c_acc = c_acc_bf16(ix); cp.cert.lb_scores = ix->d_margin ? 1u : 0u;
        cp.radii = d_radii; cp.nq = nq32; cp.thr = W.w_thr.p; cp.nocut = df.nocut;
        vdb::launch_range_cut(cp, s);
        for (uint32_t q0 = 0; q0 < nq32; q0 += SUPER) {
            const uint32_t nb = std::min(SUPER, nq32 - q0);
            cut_pass(ix, W, s, grid, d_rowmask, d_status, W.w_qb.p, W.w_qg.p, W.w_thr.p, q0, nb, df.ovf);
            st[3] += n;
            vdb::RangeRerankParams rp{};
            rp.rows = rows_f32(ix); rp.ld = ld; rp.dim = ix->dim; rp.n_rows = n;
            rp.qp = W.w_qp.p + (size_t)q0 * ld; rp.qnorm = W.w_qnorm.p + q0; rp.nd = ix->d_nd;
            rp.row_ids = ix->d_row_ids; rp.rowmask = d_rowmask;
            rp.cand = W.w2_cand.p; rp.cand_stride = CUT_KMAX; rp.cand_cnt = cand_counts(W);
            rp.radii = d_radii + q0; rp.metric = ix->metric; rp.max_results = mr;
            rp.out_ids = d_out_ids + (size_t)q0 * mr; rp.out_dists = d_out_dists + (size_t)q0 * mr;
            rp.out_counts = d_out_counts + q0; rp.out_totals = d_out_totals ? d_out_totals + q0 : nullptr;
            rp.complete = df.complete + q0; rp.n_keys = df.n_keys + q0; rp.status = d_status;
            vdb::launch_range_rerank(rp, nb, s);
        }
        HIP_TRY(hipGetLastError());
    }
    std::vector<uint32_t> h_words(RangeFlags::words(nq32));
    const RangeFlags hf(h_words.data(), nq32);
    HIP_TRY(hipMemcpyAsync(h_words.data(), W.w_flags.p, h_words.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (hf.status[0] & vdb::ST_ZERO_QUERY) return fail_zero_vector();
    if (screened) {
        for (uint32_t q = 0; q < nq32; ++q) {
            if (hf.nocut[q]) ++st[6];
            else { if (hf.ovf[q]) ++st[5]; st[4] += hf.n_keys[q]; }
            if (hf.nocut[q] || hf.ovf[q] || !hf.complete[q]) todo.push_back(q);
        }
    } else {
        todo.resize(nq32);
        for (uint32_t q = 0; q < nq32; ++q) todo[q] = q;
    }

    // ---- exact range scan of the queries left; the dense fallback for those with more survivors than the key buffer holds
    uint32_t n_dense = 0;
    if (!todo.empty()) {
        std::vector<uint32_t> dense;
        if ((rc = bounded_scan_queries(ix, W, s, todo, mr, d_radii, d_rowmask, d_out_ids, d_out_dists, d_out_counts, d_out_totals,
                                       d_status, dense)))
            return rc;
        // (every one of the first max_results <= 2048 lies within the radius: more than 32768 rows do)
        for (uint32_t q : dense)
            if ((rc = exact_one(ix, W, s, q, mr, d_rowmask, d_out_ids + (size_t)q * mr, d_out_dists + (size_t)q * mr, d_out_counts + q)))
                return rc;
        n_dense = (uint32_t)dense.size();
    }
    st[0] = nq32 - todo.size(); st[1] = todo.size() - n_dense; st[2] = n_dense;
    uint32_t status = hf.status[0];
    if (!todo.empty()) {
        uint32_t st4[STATUS_WORDS] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpyAsync(st4, d_status, STATUS_BYTES, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        status |= st4[0];
    }
    if (status & vdb::ST_ZERO_QUERY) return fail_zero_vector();
    if (status & vdb::ST_NAN) return fail_nan();
    return VDB_OK;
}

int range_search_device(Index* ix, const float* d_q, size_t nq, size_t dim, const float* d_radii, const uint64_t* d_idmask,
                        size_t mask_bits, size_t max_results, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                        uint64_t* d_out_totals, hipStream_t user_stream) {
    int rc;
    if (max_results == 0 || max_results > MAX_SELECT)
        return fail(VDB_ERR_INVALID_ARGUMENT, "max_results %zu outside [1, %u]", max_results, MAX_SELECT);
    Workspace* W;
    if ((rc = idle_workspace(ix, &W))) return rc;
    if ((rc = set_device(ix))) return rc;
    hipStream_t s = user_stream ? user_stream : W->stream;
    // the radii on the host: a NaN radius is refused before anything is launched
    std::vector<float> h_radii(nq);
    if (nq) {
        HIP_TRY(hipMemcpyAsync(h_radii.data(), d_radii, nq * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    for (size_t b = 0; b < nq; ++b)
        if (h_radii[b] != h_radii[b]) return fail(VDB_ERR_INVALID_ARGUMENT, "the radius of query %zu is NaN", b);
    uint64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    rc = flush(ix);
    if (!rc && nq) rc = range_search_run(ix, *W, d_q, nq, dim, d_radii, d_idmask, mask_bits, max_results, d_out_ids, d_out_dists,
                                         d_out_counts, d_out_totals, s, st);
    memcpy(ix->range_stats, st, sizeof(st));
    return rc;
}

void publish_stats(Index* ix, const Workspace& W) { memcpy(ix->stats, W.stats, sizeof(ix->stats)); }

// A synchronous call takes the workspace no submitted search is using
int idle_workspace(Index* ix, Workspace** W) {
    *W = ix->wsv[0].busy ? &ix->wsv[1] : &ix->wsv[0];
    if ((*W)->busy) return fail(VDB_ERR_INVALID_ARGUMENT, "two submitted searches are in flight on this handle: wait for one first");
    return VDB_OK;
}
Workspace& other_workspace(Index* ix, Workspace& W) { return ix->wsv[&W == &ix->wsv[0] ? 1 : 0]; }

// searches submitted and not yet waited for (vdb_flat_search_batch_device_submit): the row store must not change under them
bool in_flight(const Index* ix) { return ix->wsv && (ix->wsv[0].busy || ix->wsv[1].busy); }
int refuse_in_flight() { return fail(VDB_ERR_INVALID_ARGUMENT, "a submitted search is still in flight on this handle: wait for it first"); }

// ---------------------------------------------------------------------------------------------
// One nearest row per group (vdb_flat_search_batch_distinct).  The answer of a query is defined on its FULL
// ranking; a search returns a prefix of it, so the driver only decides how deep it has to look, in three stages that are all exact:
//   A  one search of the whole batch at depth dA, each list collapsed on the device (distinct_first_kernel).  The collapse of a
//      prefix is a prefix of the collapse of the ranking: a query whose list kept k rows, or came back short, is complete.
//   B  the incomplete queries, gathered into a dense block, at depth dB = min(len, 1024), collapsed from scratch into their places.
//   C  a query still incomplete has one group owning its whole list.  Exclusion rounds: a mask without the groups (and the
//      group-less rows) already answered, one search of that query under it, the list appended.  The ranking under "mask minus
//      those rows" is the ranking with those rows deleted, and a deleted row could only have been dropped by the walk, so the
//      concatenation is the walk of the full ranking.  Every round adds a group or comes back short: at most k rounds.
// One host read of the flags per stage and per round; ids, distances and codes stay on the device until the end.
// ---------------------------------------------------------------------------------------------
int distinct_drive(Index* H, hipStream_t s, const DistinctSearch& search, const DistinctArgs& a) {
    int rc;
    if ((rc = distinct_groups(H, s, search, a))) return rc;
    // ---- the answers come down (a kept count is clamped to the answers' stride)
    DistinctWs& W = H->dws;
    size_t emitted = 0;
    if ((rc = copy_out(Lists{W.ai.p, W.ad.p, W.kept.p, W.ac.p, a.kmax}, a.r, s, &emitted))) return rc;
    H->distinct_stats[7] += emitted;
    return VDB_OK;
}

int distinct_groups(Index* H, hipStream_t s, const DistinctSearch& search, const DistinctArgs& a, const uint64_t** d_mask_out) {
    DistinctWs& W = H->dws;
    uint64_t* st = H->distinct_stats;
    const size_t nq = a.r.nq, dim = a.r.dim, kmax = a.kmax;
    const size_t dA = vdb_flat_distinct_depth(kmax, a.len, 0), dB = vdb_flat_distinct_depth(kmax, a.len, 1);
    st[0] = nq; st[5] = dA; st[6] = dB;
    int rc;
    if ((rc = W.q.ensure(nq * std::max<size_t>(dim, 1))) || (rc = W.li.ensure(nq * dA)) || (rc = W.ld.ensure(nq * dA)) || (rc = W.lc.ensure(nq)) ||
        (rc = W.ai.ensure(nq * kmax)) || (rc = W.ad.ensure(nq * kmax)) || (rc = W.ac.ensure(nq * kmax)) || (rc = W.kept.ensure(nq)) ||
        (rc = W.complete.ensure(nq)) || (rc = W.sel.ensure(nq)))
        return rc;
    if (dim) HIP_TRY(hipMemcpyAsync(W.q.p, a.r.queries, nq * dim * sizeof(float), hipMemcpyHostToDevice, s));
    const uint64_t* d_mask;
    const size_t mask_bits = a.r.mask_bits;
    if ((rc = stage_mask(W.mask_in, mask_src(a.r), s, &d_mask))) return rc;
    if (d_mask_out) *d_mask_out = d_mask;
    vdb::DistinctFirstParams fp{};
    fp.ids = W.li.p; fp.dists = W.ld.p; fp.counts = W.lc.p;
    fp.codes = a.d_codes; fp.codes_len = a.codes_len; fp.n_answers = (uint32_t)nq; fp.k = (uint32_t)kmax; fp.kstride = (uint32_t)kmax;
    fp.out_ids = W.ai.p; fp.out_dists = W.ad.p; fp.out_codes = W.ac.p; fp.kept = W.kept.p; fp.complete = W.complete.p;
    std::vector<uint32_t> flag(nq), pending;
    // the incomplete queries after a collapse (one host read of the flags)
    auto read_pending = [&]() -> int {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(flag.data(), W.complete.p, nq * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        pending.clear();
        for (size_t b = 0; b < nq; ++b) if (!flag[b]) pending.push_back((uint32_t)b);
        return VDB_OK;
    };

    // ---- stage A
    if ((rc = search(W.q.p, nq, dA, d_mask, mask_bits, W.li.p, W.ld.p, W.lc.p))) return rc;
    fp.stride = fp.depth = (uint32_t)dA; fp.exhaustive = dA >= a.len; fp.dest = nullptr; fp.append = 0;
    vdb::launch_distinct_first(fp, (uint32_t)nq, s);
    if ((rc = read_pending())) return rc;
    st[1] = nq - pending.size();

    // ---- stage B
    if (!pending.empty()) HIP_TRY(hipMemcpyAsync(W.sel.p, pending.data(), pending.size() * 4, hipMemcpyHostToDevice, s));
    const std::vector<uint32_t> sel = pending;                     // W.sel[j] = sel[j] from here on
    if (!pending.empty() && dB > dA) {
        const size_t nB = pending.size();
        if ((rc = W.q2.ensure(nB * std::max<size_t>(dim, 1))) || (rc = W.li.ensure(nB * dB)) || (rc = W.ld.ensure(nB * dB))) return rc;
        vdb::launch_gather_rows(W.q.p, (uint32_t)dim, (uint32_t)dim, (uint32_t)nq, W.sel.p, (uint32_t)nB, W.q2.p, s);
        HIP_TRY(hipGetLastError());
        if ((rc = search(W.q2.p, nB, dB, d_mask, mask_bits, W.li.p, W.ld.p, W.lc.p))) return rc;
        fp.ids = W.li.p; fp.dists = W.ld.p;
        fp.stride = fp.depth = (uint32_t)dB; fp.exhaustive = dB >= a.len; fp.dest = W.sel.p; fp.append = 0;
        vdb::launch_distinct_first(fp, (uint32_t)nB, s);
        if ((rc = read_pending())) return rc;
        st[2] = nB - pending.size();
    }

    // ---- stage C
    if (!pending.empty()) {
        const uint64_t xbits = d_mask ? (uint64_t)mask_bits : a.id_bound;
        if ((rc = W.xmask.ensure(std::max<size_t>((xbits + 63) / 64, 1))) || (rc = W.li.ensure(dB)) || (rc = W.ld.ensure(dB))) return rc;
        fp.ids = W.li.p; fp.dists = W.ld.p;
        fp.stride = fp.depth = (uint32_t)dB; fp.exhaustive = dB >= a.len; fp.append = 1;
        vdb::ExcludeGroupsParams xp{d_mask, xbits, W.xmask.p, a.d_codes, a.codes_len, W.ai.p, W.ac.p, W.kept.p, (uint32_t)kmax, 0};
        size_t j = 0;
        for (uint32_t b : pending) {
            while (sel[j] != b) ++j;                               // (pending is a subsequence of sel)
            xp.answer = b;
            fp.dest = W.sel.p + j;
            uint32_t done = 0;
            for (size_t round = 0; !done; ++round) {
                if (round > kmax) return fail(VDB_ERR_DEVICE, "internal error: query %u needed more than %zu exclusion rounds", b, kmax);
                vdb::launch_exclude_groups(xp, a.n_cu, s);
                HIP_TRY(hipGetLastError());
                if ((rc = search(W.q.p + (size_t)b * dim, 1, dB, W.xmask.p, (size_t)xbits, W.li.p, W.ld.p, W.lc.p))) return rc;
                ++st[4];
                vdb::launch_distinct_first(fp, 1, s);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(&done, W.complete.p + b, 4, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
            }
            ++st[3];
        }
    }
    return VDB_OK;
}

// ---------------------------------------------------------------------------------------------
// Up to g rows of each of the k nearest groups (vdb_flat_search_batch_per_group).  The groups are the search by
// group's answers, left on the device; the members of a group with code c >= 0 are the first g rows of the full ranking whose
// code is c, so only the rows of the wanted codes are ever ranked:
//   1  distinct_groups; the codes and kept counts come down, the host sorts them into the table of wanted codes (per_group_plan)
//   2  one pass over the rows counts every wanted code's members, a host prefix sum, a second pass writes the member lists
//   3  a giant -- a code with more members than the fill takes -- gets the mask "caller's mask AND code == c" and one ordinary
//      search of the queries that want it, at depth g
//   4  every other pair with a code gets a workgroup of per_group_fill_kernel; pairs without a code keep the representative
//   5  one copy-out.  Nothing is written to the caller's arrays before every check has passed.
// Nothing survives the call: no list can go stale after an add, a remove, a compaction or a column write.
// ---------------------------------------------------------------------------------------------
void per_group_plan(const int32_t* codes, const uint32_t* kept, const size_t* ks, size_t nq, size_t kmax, std::vector<int32_t>* wanted,
                    std::vector<uint32_t>* index) {
    wanted->clear();
    index->assign(nq * kmax, 0xffffffffu);
    auto groups_of = [&](size_t b) { return std::min(std::min<size_t>(kept[b], kmax), ks ? ks[b] : kmax); };
    for (size_t b = 0; b < nq; ++b)
        for (size_t j = 0, c = groups_of(b); j < c; ++j)
            if (codes[b * kmax + j] >= 0) wanted->push_back(codes[b * kmax + j]);
    std::sort(wanted->begin(), wanted->end());
    wanted->erase(std::unique(wanted->begin(), wanted->end()), wanted->end());
    for (size_t b = 0; b < nq; ++b)
        for (size_t j = 0, c = groups_of(b); j < c; ++j) {
            const int32_t code = codes[b * kmax + j];
            if (code >= 0) (*index)[b * kmax + j] = (uint32_t)(std::lower_bound(wanted->begin(), wanted->end(), code) - wanted->begin());
        }
}

int per_group_drive(Index* ix, hipStream_t s, const DistinctSearch& search, const DistinctArgs& a, const PerGroupOut& o) {
    DistinctWs& W = ix->dws;
    PerGroupWs& G = ix->pgw;
    uint64_t* st = ix->per_group_stats;
    const size_t nq = a.r.nq, dim = a.r.dim, kmax = a.kmax, g = o.g, slots = nq * kmax;
    int rc;
    const uint64_t* d_mask = nullptr;
    if ((rc = distinct_groups(ix, s, search, a, &d_mask))) return rc;

    // ---- the plan
    std::vector<int32_t> h_codes(slots), wanted;
    std::vector<uint32_t> h_kept(nq), index, pairs, plan;
    // (the uploads below read host vectors of this frame: no return, early ones included, leaves one in flight)
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{s};
    HIP_TRY(hipMemcpyAsync(h_codes.data(), W.ac.p, slots * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_kept.data(), W.kept.p, nq * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    per_group_plan(h_codes.data(), h_kept.data(), a.r.ks, nq, kmax, &wanted, &index);
    const size_t U = wanted.size();
    st[4] = U;

    // ---- every pair starts as its representative alone
    if ((rc = G.oi.ensure(slots * g)) || (rc = G.od.ensure(slots * g)) || (rc = G.sizes.ensure(slots)) || (rc = G.stat.ensure(2))) return rc;
    HIP_TRY(hipMemsetAsync(G.stat.p, 0, 8, s));
    vdb::launch_per_group_init(vdb::PerGroupInitParams{W.ai.p, W.ad.p, W.kept.p, (uint32_t)nq, (uint32_t)kmax, (uint32_t)g, G.oi.p, G.od.p, G.sizes.p}, s);
    HIP_TRY(hipGetLastError());

    if (g > 1 && U) {
        // ---- member lists: count, prefix sum on the host, scatter
        const uint32_t n = ix->n_uploaded;
        const uint32_t cap = ix->per_group_scan_cap ? ix->per_group_scan_cap : SPARSE_MAX_E;
        if ((rc = G.wanted.ensure(U)) || (rc = G.cnt.ensure(U)) || (rc = G.plan.ensure(3 * U)) || (rc = G.list.ensure(std::max<size_t>(n, 1)))) return rc;
        HIP_TRY(hipMemcpyAsync(G.wanted.p, wanted.data(), U * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(G.cnt.p, 0, U * 4, s));
        vdb::PerGroupListParams lp{};
        lp.row_ids = ix->d_row_ids; lp.live = (ix->n_live == n) ? nullptr : ix->d_live.p; lp.n_rows = n;
        lp.mask = d_mask; lp.mask_bits = a.r.mask_bits;
        lp.codes = a.d_codes; lp.codes_len = a.codes_len;
        lp.wanted = G.wanted.p; lp.n_wanted = (uint32_t)U; lp.counts = G.cnt.p;
        lp.offs = G.plan.p; lp.lens = G.plan.p + U; lp.cursor = G.plan.p + 2 * U; lp.list = G.list.p; lp.list_cap = n;
        vdb::launch_per_group_list(lp, false, a.n_cu, s);
        HIP_TRY(hipGetLastError());
        std::vector<uint32_t> count(U);
        plan.assign(3 * U, 0);
        HIP_TRY(hipMemcpyAsync(count.data(), G.cnt.p, U * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        uint64_t listed = 0;
        for (size_t u = 0; u < U; ++u) {
            const uint32_t e = std::min(count[u], n);                      // (a count read from the device: clamped)
            const uint32_t len = (e > cap || listed + e > n) ? 0 : e;      // a giant is not listed
            plan[u] = (uint32_t)listed; plan[U + u] = len;
            listed += len;
        }
        st[5] = listed;
        HIP_TRY(hipMemcpyAsync(G.plan.p, plan.data(), 3 * U * 4, hipMemcpyHostToDevice, s));
        if (listed) {
            vdb::launch_per_group_list(lp, true, a.n_cu, s);
            HIP_TRY(hipGetLastError());
        }

        // ---- the pairs: those of a listed code for the fill, those of a giant by code
        std::vector<std::vector<uint32_t>> giant(U);
        for (size_t slot = 0; slot < slots; ++slot) {
            const uint32_t u = index[slot];
            if (u == 0xffffffffu) continue;
            if (plan[U + u]) { pairs.push_back((uint32_t)slot); pairs.push_back(u); st[6] += plan[U + u]; }
            else { giant[u].push_back((uint32_t)slot); ++st[3]; }
        }
        st[2] = pairs.size() / 2;

        // ---- giants: one masked search per code, at depth g
        if (st[3]) {
            const uint64_t xbits = std::min<uint64_t>(d_mask ? (uint64_t)a.r.mask_bits : a.id_bound, a.codes_len);
            const size_t depth = std::min(g, a.len);
            if ((rc = G.gmask.ensure(std::max<size_t>((xbits + 63) / 64, 1)))) return rc;
            for (size_t u = 0; u < U; ++u) {
                const size_t m = giant[u].size();
                if (!m) continue;
                std::vector<uint32_t> sel(m);
                for (size_t i = 0; i < m; ++i) sel[i] = giant[u][i] / (uint32_t)kmax;
                if ((rc = G.sel.ensure(m)) || (rc = G.dest.ensure(m)) || (rc = G.gq.ensure(m * std::max<size_t>(dim, 1))) || (rc = G.gi.ensure(m * depth)) ||
                    (rc = G.gd.ensure(m * depth)) || (rc = G.gc.ensure(m)))
                    return rc;
                HIP_TRY(hipMemcpyAsync(G.sel.p, sel.data(), m * 4, hipMemcpyHostToDevice, s));
                HIP_TRY(hipMemcpyAsync(G.dest.p, giant[u].data(), m * 4, hipMemcpyHostToDevice, s));
                vdb::launch_per_group_code_mask(vdb::PerGroupCodeMaskParams{d_mask, xbits, G.gmask.p, a.d_codes, a.codes_len, wanted[u]}, a.n_cu, s);
                vdb::launch_gather_rows(W.q.p, (uint32_t)dim, (uint32_t)dim, (uint32_t)nq, G.sel.p, (uint32_t)m, G.gq.p, s);
                HIP_TRY(hipGetLastError());
                if ((rc = search(G.gq.p, m, depth, G.gmask.p, (size_t)xbits, G.gi.p, G.gd.p, G.gc.p))) {
                    (void)hipStreamSynchronize(s);                         // (sel is a host vector of this frame)
                    return rc;
                }
                vdb::launch_per_group_place(vdb::PerGroupPlaceParams{G.gi.p, G.gd.p, G.gc.p, (uint32_t)depth, G.dest.p, (uint32_t)nq, (uint32_t)kmax, (uint32_t)g,
                                                                     W.ai.p, W.ad.p, G.oi.p, G.od.p, G.sizes.p, G.stat.p}, (uint32_t)m, s);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipStreamSynchronize(s));                          // (sel and the next round's buffers)
            }
        }

        // ---- the fill reads plain f32 rows, as every non-screening reader does
        if (!pairs.empty()) {
            const float* rows = rows_f32(ix);
            if (!rows) return fail(VDB_ERR_DEVICE, "internal error: no rows to rank");
            if ((rc = G.pairs.ensure(pairs.size()))) return rc;
            HIP_TRY(hipMemcpyAsync(G.pairs.p, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice, s));
            vdb::PerGroupFillParams fp{};
            fp.rows = rows; fp.ld = ix->ld; fp.dim = ix->dim; fp.n_rows = n; fp.nd = ix->d_nd; fp.row_ids = ix->d_row_ids; fp.metric = ix->metric;
            fp.q = W.q.p; fp.nq = (uint32_t)nq; fp.kmax = (uint32_t)kmax; fp.g = (uint32_t)g;
            fp.pairs = G.pairs.p; fp.offs = G.plan.p; fp.lens = G.plan.p + U; fp.n_wanted = (uint32_t)U; fp.list = G.list.p; fp.list_cap = n;
            fp.rep_ids = W.ai.p; fp.rep_dists = W.ad.p;
            fp.out_ids = G.oi.p; fp.out_dists = G.od.p; fp.out_sizes = G.sizes.p; fp.status = G.stat.p;
            vdb::launch_per_group_fill(fp, (uint32_t)(pairs.size() / 2), s);
            HIP_TRY(hipGetLastError());
        }
    }

    // ---- one copy-out; nothing reaches the caller's arrays before the status words are read
    std::vector<uint64_t> h_ids(slots * g);
    std::vector<float> h_dists(slots * g);
    std::vector<uint32_t> h_sizes(slots);
    uint32_t h_stat[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(h_ids.data(), G.oi.p, slots * g * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_dists.data(), G.od.p, slots * g * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_sizes.data(), G.sizes.p, slots * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_stat, G.stat.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h_stat[0] & vdb::ST_NAN) return fail_nan();
    st[7] = h_stat[1];
    if (h_stat[1]) return fail(VDB_ERR_DEVICE, "internal error: the first member of %u groups is not the group's representative", h_stat[1]);
    const Batch& r = a.r;
    for (size_t b = 0; b < nq; ++b) {
        const size_t c = std::min(std::min<size_t>(h_kept[b], kmax), r.ks ? r.ks[b] : r.k);
        r.counts[b] = c;
        st[1] += c;
        for (size_t j = 0; j < c; ++j) {
            const size_t from = b * kmax + j, to = b * r.kstride + j;
            const size_t size = std::min<size_t>(h_sizes[from], g);
            o.sizes[to] = (uint32_t)size;
            if (r.codes) r.codes[to] = h_codes[from];
            for (size_t m = 0; m < size; ++m) { r.ids[to * g + m] = h_ids[from * g + m]; r.dists[to * g + m] = h_dists[from * g + m]; }
        }
    }
    return VDB_OK;
}

// A synchronous search in the workspace its entry point picked (idle_workspace, or the first when nothing may be in flight)
int search_device(Index* ix, Workspace& W, const float* d_q, size_t nq, size_t dim, size_t k, const uint64_t* d_idmask,
                  size_t mask_bits, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                  hipStream_t user_stream) {
    // (the other workspace may serve the alternating passes of a large batch: the handle mutex is held until part 2 is done,
    // so no submit can claim it meanwhile)
    int rc = search_part1(ix, W, d_q, nq, dim, k, d_idmask, mask_bits, d_out_ids, d_out_dists, d_out_counts, user_stream, !in_flight(ix));
    if (rc) { W.ctx.pending = false; publish_stats(ix, W); return rc; }
    rc = search_part2(ix, W, nullptr);
    publish_stats(ix, W);
    return rc;
}

// ---------------------------------------------------------------------------------------------
// One batch, a filter per query (vdb_flat_search_batch_grouped).  The answer of a query is what the ordinary search
// returns for it alone under its mask; the queries that share a mask form a group, and the groups whose eligible rows fit get the
// sparse-filter route's scan in ONE launch chain: row masks of all groups, their counts (one host read: every E_g and the
// status of query_prep), the plan, all lists, then per pass of SUPER permuted queries one scan over the tile table and one
// select in EMIT mode, and one scatter back into the caller's order.  Exact by construction, like search_sparse: no certificate.
// ---------------------------------------------------------------------------------------------
bool group_plan(const uint32_t* group_of, size_t nq, const uint32_t* elig, size_t n_masks, bool can_scan, GroupPlan* out) {
    out->perm.clear(); out->tiles.clear(); out->passes.clear();
    out->n_scan = out->n_empty = out->n_over = out->n_none = 0;
    // kind of a query: 0 scanned, 1 nothing eligible, 2 beyond the scan's capacity, 3 unfiltered
    auto kind = [&](uint32_t g) -> int {
        if (g == VDB_GROUP_NONE) return 3;
        return elig[g] == 0 ? 1 : (can_scan && elig[g] <= SPARSE_MAX_E) ? 0 : 2;
    };
    std::vector<uint32_t> cnt(n_masks + 1, 0);                     // queries per group (the last: unfiltered)
    for (size_t b = 0; b < nq; ++b) {
        const uint32_t g = group_of[b];
        if (g != VDB_GROUP_NONE && g >= n_masks) return false;
        ++cnt[g == VDB_GROUP_NONE ? n_masks : g];
    }
    // a counting sort by (kind, group): stable, so a group's queries keep the caller's order
    std::vector<uint32_t> start(n_masks + 1, 0);
    uint32_t at = 0;
    for (int kd = 0; kd < 4; ++kd)
        for (size_t g = 0; g <= n_masks; ++g) {
            if (!cnt[g] || kind(g == n_masks ? VDB_GROUP_NONE : (uint32_t)g) != kd) continue;
            start[g] = at; at += cnt[g];
            (kd == 0 ? out->n_scan : kd == 1 ? out->n_empty : kd == 2 ? out->n_over : out->n_none) += cnt[g];
        }
    out->perm.resize(nq);
    std::vector<uint32_t> fill(start);
    for (size_t b = 0; b < nq; ++b) out->perm[fill[group_of[b] == VDB_GROUP_NONE ? n_masks : group_of[b]]++] = (uint32_t)b;
    // tiles: the scanned groups in the order of the permutation, cut at the pass boundaries
    for (uint32_t p0 = 0; p0 < out->n_scan; p0 += SUPER) out->passes.push_back(GroupPass{p0, std::min(SUPER, out->n_scan - p0), 0, 0, 0});
    for (size_t g = 0; g < n_masks; ++g) {
        if (!cnt[g] || kind((uint32_t)g) != 0) continue;
        const uint32_t a = start[g], b = a + cnt[g], E = elig[g];
        for (uint32_t q = a; q < b;) {
            GroupPass& P = out->passes[q / SUPER];
            const uint32_t nqt = std::min(std::min(b, P.q0 + P.nq) - q, vdb::SPARSE_TILE_Q);
            if (!P.n_tiles) P.tile0 = (uint32_t)out->tiles.size();
            for (uint32_t j0 = 0; j0 < E; j0 += vdb::SPARSE_TILE_R) out->tiles.push_back(GroupTile{(uint32_t)g, j0, q, nqt});
            P.n_tiles = (uint32_t)out->tiles.size() - P.tile0;
            P.stride = std::max(P.stride, round_up(E, vdb::SPARSE_TILE_R));
            q += nqt;
        }
    }
    return true;
}

// an ordinary search of the queries `idx` (caller's indices) under one mask or none, its results put into their places
static int grouped_ordinary(Index* ix, Workspace& W, hipStream_t s, const GroupedArgs& a, const std::vector<uint32_t>& idx, const vdb::GroupedMask* mask) {
    int rc;
    GroupedWs& G = ix->gws;
    const size_t m = idx.size(), k = a.k;
    if (!m) return VDB_OK;
    if ((rc = G.sel.ensure(m)) || (rc = G.q2.ensure(m * std::max<size_t>(a.dim, 1))) || (rc = G.si.ensure(m * k)) || (rc = G.sd.ensure(m * k)) ||
        (rc = G.sc.ensure(m)))
        return rc;
    HIP_TRY(hipMemcpyAsync(G.sel.p, idx.data(), m * 4, hipMemcpyHostToDevice, s));
    vdb::launch_gather_rows(a.d_q, (uint32_t)a.dim, (uint32_t)a.dim, (uint32_t)a.nq, G.sel.p, (uint32_t)m, G.q2.p, s);
    HIP_TRY(hipGetLastError());
    if ((rc = search_device(ix, W, G.q2.p, m, a.dim, k, mask ? mask->words : nullptr, mask ? (size_t)mask->bits : 0, G.si.p, G.sd.p, G.sc.p, nullptr)))
        return rc;
    vdb::launch_scatter_results(G.si.p, G.sd.p, G.sc.p, G.sel.p, (uint32_t)m, (uint32_t)k, a.d_out_ids, a.d_out_dists, a.d_out_counts, s);
    HIP_TRY(hipGetLastError());
    return VDB_OK;
}

int search_grouped(Index* ix, Workspace& W, hipStream_t s, const GroupedArgs& a) {
    int rc;
    GroupedWs& G = ix->gws;
    uint64_t* st = ix->grouped_stats;
    const size_t nq = a.nq, k = a.k, R = a.n_ref;
    const uint32_t nq32 = (uint32_t)nq;
    // the checks of a search, in its order (search_part1; the entry point has refused an oversized batch already)
    if ((rc = pre_device_checks(ix, a.dim, false))) return rc;
    const uint32_t n = ix->n_uploaded, ld = ix->ld;
    const uint32_t n_words = (n + 31) / 32, nb = vdb::sparse_list_blocks(n);

    // ---- row masks and counts of all referenced groups; the queries prepared (the whole batch: a zero-norm query anywhere fails
    // the call before any distance is looked at)
    HIP_TRY(hipMemsetAsync(a.d_out_counts, 0, nq * 4, s));
    if ((rc = prep_exact_queries(ix, W, s, a.d_q, nq32, a.dim))) return rc;
    uint32_t* d_status = SearchFlags(W.w_flags.p, nq32).status;
    uint32_t* d_blk = nullptr;                                     // [R][nb] counts | [R][nb] offsets | [R] totals
    if (R) {
        if ((rc = G.rowmask.ensure(R * std::max<size_t>(n_words, 1))) || (rc = G.blk.ensure(2 * R * (size_t)nb + R))) return rc;
        d_blk = G.blk.p;
        vdb::launch_grouped_rowmasks(ix->d_row_ids, (ix->n_live == n) ? nullptr : ix->d_live, a.d_desc, (uint32_t)R, n, G.rowmask.p, s);
        vdb::launch_grouped_count(G.rowmask.p, (uint32_t)R, n, d_blk, d_blk + R * (size_t)nb, d_blk + 2 * R * (size_t)nb, s);
    }
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> elig(R + 4, 0);                          // E of every referenced group | the status block
    if (R) HIP_TRY(hipMemcpyAsync(elig.data(), d_blk + 2 * R * (size_t)nb, R * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(elig.data() + R, d_status, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (elig[R] & vdb::ST_ZERO_QUERY) return fail_zero_vector();
    for (size_t g = 0; g < R; ++g)
        if (elig[g] > n) return fail(VDB_ERR_DEVICE, "eligible-row count %u exceeds the %u rows of the store", elig[g], n);

    // ---- the plan
    GroupPlan plan;
    if (!group_plan(a.slot, nq, elig.data(), R, k <= MAX_SELECT, &plan)) return fail(VDB_ERR_DEVICE, "internal error: a query's group is not among the referenced masks");
    st[2] = plan.n_scan; st[3] = plan.n_over; st[4] = plan.n_none; st[6] = plan.tiles.size(); st[7] = plan.passes.size();

    if (plan.n_scan) {
        // one block for the device: permutation | key count per permuted query | {list offset, length} per group | tiles
        const uint32_t ns = plan.n_scan, nt = (uint32_t)plan.tiles.size();
        std::vector<uint32_t> hp((size_t)2 * ns + 2 * R + 4 * (size_t)nt, 0);
        uint32_t* h_kcnt = hp.data() + ns; uint32_t* h_glist = h_kcnt + ns; uint32_t* h_tiles = h_glist + 2 * R;
        uint64_t lists_len = 0;
        for (uint32_t i = 0; i < ns; ++i) { hp[i] = plan.perm[i]; h_kcnt[i] = round_up(elig[a.slot[plan.perm[i]]], vdb::SPARSE_TILE_R); }
        for (uint32_t i = 0; i < ns;) {                             // (group by group: the scanned queries are sorted by group)
            const uint32_t g = a.slot[plan.perm[i]];
            h_glist[2 * g] = (uint32_t)lists_len; h_glist[2 * g + 1] = elig[g];
            lists_len += elig[g]; st[5] += elig[g];
            while (i < ns && a.slot[plan.perm[i]] == g) ++i;
        }
        if (lists_len > 0xfffffff0ull) return fail(VDB_ERR_INVALID_ARGUMENT, "the eligible-row lists of the batch hold %llu rows: too many for one call", (unsigned long long)lists_len);
        memcpy(h_tiles, plan.tiles.data(), (size_t)nt * 16);
        size_t key_rows = 0;
        for (const GroupPass& P : plan.passes) key_rows = std::max(key_rows, (size_t)P.nq * P.stride);
        if ((rc = ensure_ranks(ix))) return rc;
        if ((rc = G.plan.ensure(hp.size())) || (rc = G.lists.ensure(lists_len)) || (rc = W.w2_qp.ensure((size_t)ns * ld)) ||
            (rc = W.w2_qnorm.ensure(ns)) || (rc = W.w2_thr.ensure(ns)) || (rc = G.si.ensure((size_t)ns * k)) || (rc = G.sd.ensure((size_t)ns * k)) ||
            (rc = G.sc.ensure(ns)) || (rc = W.w_exact.ensure(key_rows)) || (rc = W.w_exsel.ensure((size_t)SUPER * MAX_SELECT + 8)) ||
            (rc = W.w_cnt.ensure(4 * SUPER + 16)))
            return rc;
        HIP_TRY(hipMemcpyAsync(G.plan.p, hp.data(), hp.size() * 4, hipMemcpyHostToDevice, s));
        const uint32_t* d_perm = G.plan.p; const uint32_t* d_kcnt = d_perm + ns; const uint32_t* d_glist = d_kcnt + ns;
        const uint32_t* d_tiles = d_glist + 2 * R;
        vdb::launch_grouped_scatter(G.rowmask.p, (uint32_t)R, n, d_blk + R * (size_t)nb, d_glist, G.lists.p, (uint32_t)lists_len, s);
        vdb::launch_gather_queries(W.w_qp.p, W.w_qnorm.p, ld, d_perm, ns, ns, W.w2_qp.p, W.w2_qnorm.p, W.w2_thr.p, s);
        for (const GroupPass& P : plan.passes) {
            vdb::GroupedScanParams gp{};
            gp.scan = vdb::SparseScanParams{rows_f32(ix), ld, ix->dim, n, G.lists.p, (uint32_t)lists_len, W.w2_qp.p + (size_t)P.q0 * ld,
                                            W.w2_qnorm.p + P.q0, P.nq, ix->d_nd, ix->ids_monotone ? nullptr : ix->d_idrank.p, ix->metric,
                                            W.w_exact.p, P.stride, d_status};
            gp.tiles = d_tiles + 4 * (size_t)P.tile0; gp.n_tiles = P.n_tiles; gp.glist = d_glist; gp.n_groups = (uint32_t)R; gp.q_base = P.q0;
            vdb::launch_grouped_scan(gp, s);
            vdb::SelectParams mp = emit_select_params(ix, W, k);
            mp.keys = W.w_exact.p; mp.stride = P.stride; mp.counts = d_kcnt + P.q0; mp.n_fixed = P.stride; mp.cap = P.stride;
            mp.emit_ids = G.si.p + (size_t)P.q0 * k; mp.emit_dists = G.sd.p + (size_t)P.q0 * k; mp.emit_counts = G.sc.p + P.q0;
            vdb::launch_select(mp, P.nq, s);
        }
        vdb::launch_scatter_results(G.si.p, G.sd.p, G.sc.p, d_perm, ns, (uint32_t)k, a.d_out_ids, a.d_out_dists, a.d_out_counts, s);
        HIP_TRY(hipGetLastError());
        uint32_t st4[STATUS_WORDS] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpyAsync(st4, d_status, STATUS_BYTES, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (st4[0] & vdb::ST_NAN) return fail_nan();
    }

    // ---- the queries not on the route, by the existing code: one ordinary masked search per group beyond the scan's capacity,
    // one unmasked search for all unfiltered queries
    std::vector<uint32_t> idx;
    for (uint32_t i = plan.n_scan + plan.n_empty; i < plan.n_scan + plan.n_empty + plan.n_over;) {
        const uint32_t g = a.slot[plan.perm[i]];
        idx.clear();
        for (; i < plan.n_scan + plan.n_empty + plan.n_over && a.slot[plan.perm[i]] == g; ++i) idx.push_back(plan.perm[i]);
        if ((rc = grouped_ordinary(ix, W, s, a, idx, &a.h_desc[g]))) return rc;
    }
    idx.assign(plan.perm.begin() + (nq - plan.n_none), plan.perm.end());
    if ((rc = grouped_ordinary(ix, W, s, a, idx, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return VDB_OK;
}

// ---------------------------------------------------------------------------------------------
// Recommend by best score (vdb_flat_recommend_best_batch).  The answer of a request is defined row by row (dp,
// the kept rule, dn); the driver only decides how it gets there, and every way is exact:
//   lists  the positives of the requests in hand become one query block (gathered on the device), ONE certified search ranks
//          them at depth D, rb_merge_kernel walks each request's lists under the frontier proof, rb_veto_kernel applies the
//          negatives and keeps the first k.  A request is answered when k rows were kept or nothing can lie behind its
//          candidates.  Stage 0 runs at vdb_flat_recommend_best_depth(.., 0), stage 1 -- the unanswered requests only -- at
//          (.., 1).
//   scan   what is still unanswered: rb_scan_kernel writes one key per kept row, the full-scan select emits the first k, the
//          same veto kernel adds dn.
// One host read of the flags per list stage; ids and distances stay on the device until the copy-out.
// ---------------------------------------------------------------------------------------------
constexpr size_t RB_SCAN_KEYS = (size_t)1 << 25;                   // keys of one scan pass (256 MiB)

int recommend_best_drive(Index* ix, const HostSearch& r, const RecommendReq& rec, const uint32_t* ex_rows, size_t kmax) {
    RecBestWs& B = ix->rbw;
    Workspace& W = ix->wsv[0];                                     // (nothing is in flight)
    hipStream_t s = ix->stream;
    uint64_t* st = ix->recommend_best_stats;
    const size_t nq = r.nq, total = rec.total, dim = ix->dim;
    const size_t len = ix->n_live + ix->misfits.size();
    const size_t kcut = std::min(kmax, len);
    int rc;
    if (kcut == 0) {
        for (size_t b = 0; b < nq; ++b) r.counts[b] = 0;
        return VDB_OK;
    }
    if (kcut > vdb::RB_MAX_ROWS)
        return fail(VDB_ERR_INVALID_ARGUMENT, "a recommend by best score returns at most %u rows per request, not %zu", vdb::RB_MAX_ROWS, kcut);
    if ((rc = pre_device_checks(ix, dim, false))) return rc;
    if ((rc = ensure_ranks(ix))) return rc;
    const uint32_t n = ix->n_uploaded;
    const size_t D0 = vdb_flat_recommend_best_depth(kcut, rec.mmax, len, 0), D1 = vdb_flat_recommend_best_depth(kcut, rec.mmax, len, 1);
    st[5] = D0;

    // ---- the requests go up: offsets [nq + 1] | n_pos [nq] | k [nq] | rows [total], and the ids
    const size_t o_np = nq + 1, o_k = o_np + nq, o_row = o_k + nq, words = o_row + total;
    std::vector<uint32_t> meta(words);
    for (size_t b = 0; b <= nq; ++b) meta[b] = (uint32_t)rec.offsets[b];
    for (size_t b = 0; b < nq; ++b) {
        meta[o_np + b] = rec.n_pos[b];
        meta[o_k + b] = (uint32_t)std::min(r.ks ? r.ks[b] : r.k, kcut);
    }
    memcpy(meta.data() + o_row, ex_rows, total * 4);
    const size_t no = nq * kcut;
    if ((rc = B.meta.ensure(words)) || (rc = B.ids.ensure(std::max<size_t>(total, 1))) || (rc = B.stat.ensure(2)) ||
        (rc = B.outi.ensure(no)) || (rc = B.outd.ensure(no)) || (rc = B.outn.ensure(no)) || (rc = B.outc.ensure(nq)))
        return rc;
    // (the uploads below read host vectors of this frame: no return, early ones included, leaves one in flight)
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{s};
    HIP_TRY(hipMemcpyAsync(B.meta.p, meta.data(), words * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(B.ids.p, rec.ids, total * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(B.stat.p, 0, 8, s));
    const vdb::RbRequests R{B.meta.p, B.meta.p + o_np, B.meta.p + o_k, B.meta.p + o_row, B.ids.p};
    const uint64_t* d_mask;
    if ((rc = stage_mask(B.mask_in, mask_src(r), s, &d_mask))) return rc;

    auto veto_params = [&]() {
        vdb::RbVetoParams vp{};
        vp.rows = rows_f32(ix); vp.ld = ix->ld; vp.dim = ix->dim; vp.n_rows = n; vp.metric = ix->metric; vp.nd = ix->d_nd;
        vp.row_ids = ix->d_row_ids; vp.rank2row = ix->ids_monotone ? nullptr : ix->d_rank2row.p; vp.live = ix->d_live;
        vp.R = R; vp.cand_ids = B.ci.p; vp.cand_dists = B.cd.p; vp.cand_cnt = B.cc.p;
        vp.out_ids = B.outi.p; vp.out_dists = B.outd.p; vp.out_neg = B.outn.p; vp.out_counts = B.outc.p; vp.kout = (uint32_t)kcut;
        vp.status = B.stat.p + 1;
        return vp;
    };

    // ---- a list stage for the requests `reqs` at depth D; *left receives those it could not answer
    auto run_lists = [&](const std::vector<uint32_t>& reqs, size_t D, std::vector<uint32_t>* left) -> int {
        const size_t nr = reqs.size();
        // requests [nr] | first list [nr] | positive rows [nl]
        std::vector<uint32_t> sel(2 * nr);
        for (size_t j = 0; j < nr; ++j) {
            const uint32_t b = reqs[j];
            sel[j] = b;
            sel[nr + j] = (uint32_t)(sel.size() - 2 * nr);
            sel.insert(sel.end(), ex_rows + rec.offsets[b], ex_rows + rec.offsets[b] + rec.n_pos[b]);
        }
        const size_t nl = sel.size() - 2 * nr;
        const size_t cs = vdb::RB_MAX_ROWS;
        if ((rc = B.sel.ensure(sel.size())) || (rc = B.q.ensure(nl * std::max<size_t>(dim, 1))) || (rc = B.li.ensure(nl * D)) ||
            (rc = B.ld.ensure(nl * D)) || (rc = B.lc.ensure(nl)) || (rc = B.ci.ensure(nr * cs)) || (rc = B.cd.ensure(nr * cs)) ||
            (rc = B.cc.ensure(nr)) || (rc = B.open.ensure(nr)) || (rc = B.answered.ensure(nr)))
            return rc;
        HIP_TRY(hipMemcpyAsync(B.sel.p, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, s));
        // only row numbers go up; the vectors never leave HBM
        vdb::launch_gather_rows(rows_f32(ix), ix->ld, ix->dim, n, B.sel.p + 2 * nr, (uint32_t)nl, B.q.p, s);
        HIP_TRY(hipGetLastError());
        if ((rc = search_device(ix, W, B.q.p, nl, dim, D, d_mask, r.mask_bits, B.li.p, B.ld.p, B.lc.p, nullptr))) return rc;
        st[6] += nl;
        vdb::RbMergeParams mp{R, B.sel.p, B.sel.p + nr, B.li.p, B.ld.p, B.lc.p, (uint32_t)D, B.ci.p, B.cd.p, B.cc.p, B.open.p, (uint32_t)cs};
        vdb::launch_rb_merge(mp, (uint32_t)nr, s);
        vdb::RbVetoParams vp = veto_params();
        vp.sel = B.sel.p; vp.open = B.open.p; vp.cand_stride = (uint32_t)cs; vp.answered = B.answered.p;
        vdb::launch_rb_veto(vp, (uint32_t)nr, s);
        HIP_TRY(hipGetLastError());
        std::vector<uint32_t> flag(nr);
        HIP_TRY(hipMemcpyAsync(flag.data(), B.answered.p, nr * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        left->clear();
        for (size_t j = 0; j < nr; ++j) if (!flag[j]) left->push_back(reqs[j]);
        return VDB_OK;
    };

    // ---- the exact scan for the requests `reqs`, as many per pass as the key buffer holds
    auto run_scan = [&](const std::vector<uint32_t>& reqs) -> int {
        const size_t nr = reqs.size();
        const uint32_t* d_rowmask;
        if ((rc = eligibility_mask(ix, W, s, d_mask, r.mask_bits, &d_rowmask))) return rc;
        const size_t G = std::min<size_t>(std::min<size_t>(nr, SUPER), std::max<size_t>(RB_SCAN_KEYS / std::max<uint32_t>(n, 1), 1));
        if ((rc = B.sel.ensure(nr)) || (rc = W.w_exact.ensure(G * n)) || (rc = W.w_exsel.ensure((size_t)SUPER * MAX_SELECT + 8)) ||
            (rc = W.w_cnt.ensure(4 * SUPER + 16)) || (rc = B.ci.ensure(G * kcut)) || (rc = B.cd.ensure(G * kcut)) || (rc = B.cc.ensure(G)))
            return rc;
        HIP_TRY(hipMemcpyAsync(B.sel.p, reqs.data(), nr * 4, hipMemcpyHostToDevice, s));
        for (size_t g0 = 0; g0 < nr; g0 += G) {
            const uint32_t g = (uint32_t)std::min(G, nr - g0);
            vdb::RbScanParams sp{rows_f32(ix), ix->ld, ix->dim, n, ix->metric, ix->d_nd, d_rowmask,
                                 ix->ids_monotone ? nullptr : ix->d_idrank.p, R, B.sel.p + g0, W.w_exact.p, n, B.stat.p};
            vdb::launch_rb_scan(sp, g, s);
            vdb::SelectParams mp = emit_select_params(ix, W, kcut);
            mp.keys = W.w_exact.p; mp.stride = n; mp.counts = nullptr; mp.n_fixed = n; mp.cap = n;
            mp.emit_ids = B.ci.p; mp.emit_dists = B.cd.p; mp.emit_counts = B.cc.p;
            vdb::launch_select(mp, g, s);
            vdb::RbVetoParams vp = veto_params();
            vp.sel = B.sel.p + g0; vp.open = nullptr; vp.cand_stride = (uint32_t)kcut; vp.answered = nullptr;
            vdb::launch_rb_veto(vp, g, s);
            HIP_TRY(hipGetLastError());
        }
        return VDB_OK;
    };

    std::vector<uint32_t> todo(nq), left;
    for (size_t b = 0; b < nq; ++b) todo[b] = (uint32_t)b;
    // (automatic: lists whose depth is the whole index are the expensive way to scan it)
    const bool lists = ix->rb_route == 1 || (ix->rb_route == 0 && D0 < len);
    if (lists) {
        if ((rc = run_lists(todo, D0, &left))) return rc;
        st[2] = todo.size() - left.size();
        todo.swap(left);
        if (!todo.empty() && D1 > D0) {
            if ((rc = run_lists(todo, D1, &left))) return rc;
            st[3] = todo.size() - left.size();
            todo.swap(left);
        }
    }
    if (!todo.empty()) {
        if ((rc = run_scan(todo))) return rc;
        st[4] = todo.size();
    }
    uint32_t status[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(status, B.stat.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (status[1] & 2u) return fail(VDB_ERR_DEVICE, "internal error: a candidate without a live row on the device");
    if (status[0] & vdb::ST_NAN) return fail_nan();
    return copy_out(Lists{B.outi.p, B.outd.p, B.outc.p, nullptr, kcut, B.outn.p}, r, s);
}

// ---------------------------------------------------------------------------------------------
// Discovery search (vdb_flat_discover_batch).  The answer of a request is defined row by row (rank, d(t, x));
// the driver only decides how it gets there, and every way is exact:
//   lists  the targets of the requests in hand become one query block (gathered on the device), ONE certified search ranks
//          the store for each at depth D, the set strike removes every request's examples, discover_rank_kernel counts the
//          satisfied pairs of every candidate and writes the answer of a request that has k rows of rank P or a complete
//          list.  Stage 0 runs at vdb_flat_discover_depth(.., 0), stage 1 -- the unanswered requests only -- at (.., 1).
//   scan   what is still unanswered: discover_scan_kernel writes one key per eligible row, the full-scan select sorts the first
//          k, discover_emit_kernel takes them apart.
// One host read of the flags per list stage; ids and distances stay on the device until the copy-out.
// ---------------------------------------------------------------------------------------------
int discover_drive(Index* ix, const HostSearch& r, const DiscoverReq& req, const uint64_t* ex_ids, const uint32_t* ex_rows, size_t kcut,
                   uint32_t* out_ranks) {
    DiscoverWs& B = ix->dcw;
    Workspace& W = ix->wsv[0];                                     // (nothing is in flight)
    hipStream_t s = ix->stream;
    uint64_t* st = ix->discover_stats;
    const size_t nq = r.nq, total = nq + 2 * req.pairs, dim = ix->dim;
    const size_t len = ix->n_live + ix->misfits.size();
    int rc;
    if (kcut == 0) {
        for (size_t b = 0; b < nq; ++b) r.counts[b] = 0;
        return VDB_OK;
    }
    if ((rc = pre_device_checks(ix, dim, false))) return rc;
    if ((rc = ensure_ranks(ix))) return rc;
    const uint32_t n = ix->n_uploaded;
    const size_t D0 = vdb_flat_discover_depth(kcut, req.pmax, len, 0), D1 = vdb_flat_discover_depth(kcut, req.pmax, len, 1);
    st[5] = D0;

    // ---- the requests go up: offsets [nq + 1] | k [nq] | rows [total], and the ids
    const size_t o_k = nq + 1, o_row = o_k + nq, words = o_row + total;
    std::vector<uint32_t> meta(words);
    for (size_t b = 0; b <= nq; ++b) meta[b] = (uint32_t)(b + 2 * req.offsets[b]);
    for (size_t b = 0; b < nq; ++b) meta[o_k + b] = (uint32_t)std::min(r.ks ? r.ks[b] : r.k, kcut);
    memcpy(meta.data() + o_row, ex_rows, total * 4);
    const size_t no = nq * kcut;
    if ((rc = B.meta.ensure(words)) || (rc = B.ids.ensure(total)) || (rc = B.stat.ensure(2)) || (rc = B.outi.ensure(no)) ||
        (rc = B.outd.ensure(no)) || (rc = B.outr.ensure(no)) || (rc = B.outc.ensure(nq)))
        return rc;
    // (the uploads below read host vectors of this frame: no return, early ones included, leaves one in flight)
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{s};
    HIP_TRY(hipMemcpyAsync(B.meta.p, meta.data(), words * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(B.ids.p, ex_ids, total * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(B.stat.p, 0, 8, s));
    const vdb::DiscoverRequests R{B.meta.p, B.meta.p + o_k, B.meta.p + o_row, B.ids.p};
    const uint64_t* d_mask;
    if ((rc = stage_mask(B.mask_in, mask_src(r), s, &d_mask))) return rc;
    const uint32_t* d_rank2row = ix->ids_monotone ? nullptr : ix->d_rank2row.p;

    // ---- a list stage for the requests `reqs` at depth D; *left receives those it could not answer
    auto run_lists = [&](const std::vector<uint32_t>& reqs, size_t D, std::vector<uint32_t>* left) -> int {
        const size_t nr = reqs.size();
        // requests [nr] | target rows [nr] | offsets of the stage's example sets [nr + 1]; the ids of those sets
        std::vector<uint32_t> sel(3 * nr + 1);
        std::vector<uint64_t> sids;
        for (size_t j = 0; j < nr; ++j) {
            const uint32_t b = reqs[j];
            sel[j] = b;
            sel[nr + j] = ex_rows[meta[b]];
            sel[2 * nr + j] = (uint32_t)sids.size();
            sids.insert(sids.end(), ex_ids + meta[b], ex_ids + meta[b + 1]);
        }
        sel[3 * nr] = (uint32_t)sids.size();
        if ((rc = B.sel.ensure(sel.size())) || (rc = B.sids.ensure(sids.size())) || (rc = B.q.ensure(nr * std::max<size_t>(dim, 1))) ||
            (rc = B.li.ensure(nr * D)) || (rc = B.ld.ensure(nr * D)) || (rc = B.lc.ensure(nr)) || (rc = B.raw.ensure(nr)) ||
            (rc = B.answered.ensure(nr)) || (rc = B.struck.ensure(1)))
            return rc;
        HIP_TRY(hipMemcpyAsync(B.sel.p, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(B.sids.p, sids.data(), sids.size() * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(B.struck.p, 0, 4, s));
        // only row numbers go up; the vectors never leave HBM
        vdb::launch_gather_rows(rows_f32(ix), ix->ld, ix->dim, n, B.sel.p + nr, (uint32_t)nr, B.q.p, s);
        HIP_TRY(hipGetLastError());
        if ((rc = search_device(ix, W, B.q.p, nr, dim, D, d_mask, r.mask_bits, B.li.p, B.ld.p, B.lc.p, nullptr))) return rc;
        st[6] += nr;
        // (the strike rewrites the counts: whether a list came back full is read from this copy)
        HIP_TRY(hipMemcpyAsync(B.raw.p, B.lc.p, nr * 4, hipMemcpyDeviceToDevice, s));
        vdb::StrikeSetParams sp{B.li.p, B.ld.p, B.lc.p, (uint32_t)D, B.sel.p + 2 * nr, B.sids.p, (uint32_t)D, B.struck.p};
        vdb::launch_strike_set(sp, (uint32_t)nr, s);
        vdb::DiscoverRankParams rp{};
        rp.rows = rows_f32(ix); rp.ld = ix->ld; rp.dim = ix->dim; rp.n_rows = n; rp.metric = ix->metric; rp.nd = ix->d_nd;
        rp.row_ids = ix->d_row_ids; rp.rank2row = d_rank2row; rp.live = ix->d_live;
        rp.R = R; rp.sel = B.sel.p;
        rp.cand_ids = B.li.p; rp.cand_dists = B.ld.p; rp.cand_cnt = B.lc.p; rp.raw_cnt = B.raw.p;
        rp.cand_stride = (uint32_t)D; rp.depth = (uint32_t)D; rp.exhaustive = D >= len ? 1u : 0u;
        rp.out_ids = B.outi.p; rp.out_dists = B.outd.p; rp.out_ranks = B.outr.p; rp.out_counts = B.outc.p; rp.kout = (uint32_t)kcut;
        rp.answered = B.answered.p; rp.status = B.stat.p + 1;
        vdb::launch_discover_rank(rp, (uint32_t)nr, s);
        HIP_TRY(hipGetLastError());
        std::vector<uint32_t> flag(nr);
        HIP_TRY(hipMemcpyAsync(flag.data(), B.answered.p, nr * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        left->clear();
        for (size_t j = 0; j < nr; ++j) if (!flag[j]) left->push_back(reqs[j]);
        return VDB_OK;
    };

    // ---- the exact scan for the requests `reqs`, as many per pass as the key buffer holds
    auto run_scan = [&](const std::vector<uint32_t>& reqs) -> int {
        const size_t nr = reqs.size();
        if (n >> vdb::DISCOVER_KEY_ID_BITS)
            return fail(VDB_ERR_INVALID_ARGUMENT, "the exact scan of a discovery search keys at most 2^%u - 1 rows, the store holds %u",
                        vdb::DISCOVER_KEY_ID_BITS, n);
        const uint32_t* d_rowmask;
        if ((rc = eligibility_mask(ix, W, s, d_mask, r.mask_bits, &d_rowmask))) return rc;
        const size_t G = std::min<size_t>(std::min<size_t>(nr, SUPER), std::max<size_t>(RB_SCAN_KEYS / std::max<uint32_t>(n, 1), 1));
        if ((rc = B.sel.ensure(nr)) || (rc = W.w_exact.ensure(G * n)) || (rc = W.w_exsel.ensure((size_t)SUPER * MAX_SELECT + 8)) ||
            (rc = W.w_cnt.ensure(4 * SUPER + 16)))
            return rc;
        HIP_TRY(hipMemcpyAsync(B.sel.p, reqs.data(), nr * 4, hipMemcpyHostToDevice, s));
        for (size_t g0 = 0; g0 < nr; g0 += G) {
            const uint32_t g = (uint32_t)std::min(G, nr - g0);
            vdb::DiscoverScanParams sp{rows_f32(ix), ix->ld, ix->dim, n, ix->metric, ix->d_nd, d_rowmask,
                                       ix->ids_monotone ? nullptr : ix->d_idrank.p, R, B.sel.p + g0, W.w_exact.p, n, B.stat.p};
            vdb::launch_discover_scan(sp, g, s);
            // (the keys are no (distance, id rank) pairs: the select only sorts them, discover_emit_kernel reads them)
            vdb::SelectParams mp{};
            mp.kk = (uint32_t)kcut; mp.out_keys = W.w_exsel.p; mp.out_stride = MAX_SELECT; mp.out_cnt = W.w_cnt.p;
            mp.keys = W.w_exact.p; mp.stride = n; mp.counts = nullptr; mp.n_fixed = n; mp.cap = n;
            vdb::launch_select(mp, g, s);
            vdb::DiscoverEmitParams ep{W.w_exsel.p, W.w_cnt.p, MAX_SELECT, R, B.sel.p + g0, d_rank2row, ix->d_row_ids, n,
                                       B.outi.p, B.outd.p, B.outr.p, B.outc.p, (uint32_t)kcut, B.stat.p + 1};
            vdb::launch_discover_emit(ep, g, s);
            HIP_TRY(hipGetLastError());
        }
        return VDB_OK;
    };

    std::vector<uint32_t> todo(nq), left;
    for (size_t b = 0; b < nq; ++b) todo[b] = (uint32_t)b;
    // (automatic: a list whose depth is the whole index is the expensive way to scan it)
    const bool lists = ix->discover_route == 1 || (ix->discover_route == 0 && D0 < len);
    if (lists) {
        if ((rc = run_lists(todo, D0, &left))) return rc;
        st[2] = todo.size() - left.size();
        todo.swap(left);
        if (!todo.empty() && D1 > D0) {
            if ((rc = run_lists(todo, D1, &left))) return rc;
            st[3] = todo.size() - left.size();
            todo.swap(left);
        }
    }
    if (!todo.empty()) {
        if ((rc = run_scan(todo))) return rc;
        st[4] = todo.size();
    }
    uint32_t status[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(status, B.stat.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (status[1] & 2u) return fail(VDB_ERR_DEVICE, "internal error: a candidate without a live row on the device");
    if (status[0] & vdb::ST_NAN) return fail_nan();
    // (the ranks travel in the copy-out's 32-bit column: the same bits, read back as uint32_t)
    Batch out = r;
    out.codes = reinterpret_cast<int32_t*>(out_ranks);
    return copy_out(Lists{B.outi.p, B.outd.p, B.outc.p, reinterpret_cast<const int32_t*>(B.outr.p), kcut}, out, s);
}

}  // namespace vdbi
