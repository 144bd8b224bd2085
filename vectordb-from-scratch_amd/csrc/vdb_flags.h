// vdb_flags.h -- the per-search flag blocks (Workspace::w_flags on the device, h_flags or a vector on the host) by name, and
// the tier hand-over that search_part2 decides from them.  Plain host arithmetic: nothing of HIP is included, so
// tests/cpp/tier_triage_test.cpp checks all of it on the CPU.  Not part of the C ABI.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/vdb_flat.h"

namespace vdbi {

// Both blocks start with the status block: [0] vdb::ST_* bits | [1] the selects' summary word | [2] running maximum of the query
// norms' bits | [3] unused.  The kernels take raw pointers; the layouts in memory are the ones below and nothing else.
constexpr size_t STATUS_WORDS = 4, STATUS_BYTES = 4 * STATUS_WORDS;
inline uint32_t* status_summary(uint32_t* status) { return status + 1; }
inline uint32_t* status_qmax(uint32_t* status) { return status + 2; }

// A kNN search: status[4] | cert[nq] | overflow[nq] | score cut[nq] (f32), over the device or the host copy at `base`.
struct SearchFlags {
    uint32_t *status, *cert, *ovf;
    float* cut;
    SearchFlags(uint32_t* base, size_t nq)
        : status(base), cert(base + STATUS_WORDS), ovf(cert + nq), cut(reinterpret_cast<float*>(ovf + nq)) {}
    static size_t words(size_t nq) { return STATUS_WORDS + 3 * nq; }
};

// A range search: status[4] | overflow[nq] | no cut[nq] | complete[nq] | keys evaluated[nq].
struct RangeFlags {
    uint32_t *status, *ovf, *nocut, *complete, *n_keys;
    RangeFlags(uint32_t* base, size_t nq)
        : status(base), ovf(base + STATUS_WORDS), nocut(ovf + nq), complete(nocut + nq), n_keys(complete + nq) {}
    static size_t words(size_t nq) { return STATUS_WORDS + 4 * nq; }
};

// VDB_TIERS_FORCE_RETHRESHOLD in effect: ignored together with FORCE_EXACT / FORCE_F32, and when the pass itself is switched off
inline bool force_rethreshold(uint32_t tiers) {
    return (tiers & VDB_TIERS_FORCE_RETHRESHOLD) && !(tiers & (VDB_TIERS_FORCE_EXACT | VDB_TIERS_FORCE_F32 | VDB_TIERS_NO_RETHRESHOLD));
}

// What the first tier's flags and the VDB_TIERS_* bits decide (kp16: the screening tier ran first; kp: the f32 tier can hold k).
struct TierTriage {
    std::vector<uint32_t> todo;           // the queries the first tier did not settle, ascending
    bool rethreshold = false;             // the re-threshold pass is on for this search: todo splits into sel and rest
    std::vector<uint32_t> sel;            // ... with a finite score cut and no pool overflow: the re-threshold pass's
    std::vector<float> cuts;              // ... their cuts
    std::vector<uint32_t> rest;           // ... the others
    bool f32_tier = false;                // what is still open behind the screening tier runs the f32 tier (else: the exact scan)
    uint64_t n_overflow = 0, n_uncertified = 0;
};
inline TierTriage tier_triage(const uint32_t* cert, const uint32_t* ovf, const float* cut, uint32_t nq, uint32_t tiers, uint32_t kp16, uint32_t kp) {
    TierTriage t;
    const bool force_exact = (tiers & VDB_TIERS_FORCE_EXACT) != 0, force_f32 = (tiers & VDB_TIERS_FORCE_F32) != 0;
    const bool force_rethr = kp16 && force_rethreshold(tiers);       // every query with a cut takes the re-threshold pass as well
    for (uint32_t q = 0; q < nq; ++q) {
        if (ovf[q]) ++t.n_overflow;
        if (!cert[q]) ++t.n_uncertified;
        if (cert[q] && !ovf[q] && !force_exact && !(kp16 && force_f32) && !force_rethr) continue;
        t.todo.push_back(q);
    }
    t.f32_tier = kp16 && kp;
    t.rethreshold = kp16 && !t.todo.empty() && !(tiers & VDB_TIERS_NO_RETHRESHOLD) && !force_exact && !force_f32;
    if (t.rethreshold)
        for (uint32_t q : t.todo) {
            const float c = cut[q];
            if (!ovf[q] && c == c && std::isfinite(c)) { t.sel.push_back(q); t.cuts.push_back(c); }
            else t.rest.push_back(q);
        }
    return t;
}

// After the re-threshold pass over `sel` (fl: its cert[nf] | overflow[nf]): the queries it did not answer completely join `rest`,
// which stays ascending.  Returns how many it answered; overflows are added to *n_overflow.
inline uint64_t after_rethreshold(const std::vector<uint32_t>& sel, const std::vector<uint32_t>& fl, std::vector<uint32_t>& rest, uint64_t* n_overflow) {
    const size_t nf = sel.size();
    uint64_t answered = 0;
    for (size_t j = 0; j < nf; ++j) {
        if (fl[j] && !fl[nf + j]) ++answered;
        else { rest.push_back(sel[j]); if (fl[nf + j]) ++*n_overflow; }
    }
    std::sort(rest.begin(), rest.end());
    return answered;
}

// After the f32 tier over the compact block `todo` (f2: its cert[nf] | overflow[nf]): the queries left for the exact scan.
inline std::vector<uint32_t> after_f32(const std::vector<uint32_t>& todo, const uint32_t* f2, uint32_t tiers, uint64_t* n_overflow) {
    const size_t nf = todo.size();
    std::vector<uint32_t> left;
    for (size_t j = 0; j < nf; ++j) {
        if (f2[nf + j]) ++*n_overflow;
        if (f2[j] && !f2[nf + j] && !(tiers & VDB_TIERS_FORCE_EXACT)) continue;
        left.push_back(todo[j]);
    }
    return left;
}

}  // namespace vdbi
