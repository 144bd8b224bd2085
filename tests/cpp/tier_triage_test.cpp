// The tier hand-over of a search (csrc/vdb_flags.h: tier_triage, after_rethreshold, after_f32) and the flag-block structs, on the
// CPU.  The header includes nothing of HIP; no runtime is linked and no GPU touched.  Built with -fsanitize=address,undefined by
// tests/test_tier_triage_cpu.py.
//   1. tier_triage for nq = 3: every combination of cert in {0,1}, overflow in {0,1}, cut in {finite, +inf, NaN} per query, crossed
//      with every subset of the five VDB_TIERS_* bits, kp16 in {0, nonzero} and kp in {0, nonzero}, against `restated` below: the
//      three loops as search_part2 had them before the function was lifted out, kept here word for word.
//   2. the two later filters against the same restatement, with every flag combination of the compact block.
//   3. SearchFlags / RangeFlags: for nq in {0, 1, 255, 256, 257} the fields lie base + 4, + nq, + nq ... apart, the word counts
//      are 4 + 3 nq and 4 + 4 nq, and a write through every field of the range block touches a word no other field touches.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../vectordb-from-scratch_amd/csrc/vdb_flags.h"

namespace {

int g_failed = 0;
long g_cases = 0;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

// ---- search_part2's hand-over as it stood: h_flags is status[4] | cert[nq] | ovf[nq] | cut[nq], stats the sixteen counters
struct Restated {
    std::vector<uint32_t> todo_first;     // after the first loop
    std::vector<uint32_t> sel, rest;      // what the second loop made (empty when the re-threshold block was not entered)
    std::vector<float> cuts;
    bool entered = false;                 // the re-threshold block was entered
    uint64_t stats2 = 0, stats6 = 0;
};
Restated restated(const uint32_t* h_flags, uint32_t nq32, uint32_t tiers, uint32_t kp16) {
    Restated r;
    const bool force_exact = (tiers & VDB_TIERS_FORCE_EXACT) != 0;
    const bool force_f32 = (tiers & VDB_TIERS_FORCE_F32) != 0;
    const bool no_rethr = (tiers & VDB_TIERS_NO_RETHRESHOLD) != 0;
    const bool force_rethr = kp16 && ((tiers & VDB_TIERS_FORCE_RETHRESHOLD) &&
                                      !(tiers & (VDB_TIERS_FORCE_EXACT | VDB_TIERS_FORCE_F32 | VDB_TIERS_NO_RETHRESHOLD)));
    std::vector<uint32_t> todo;
    for (uint32_t q = 0; q < nq32; ++q) {
        bool cert = h_flags[4 + q] != 0, ovf = h_flags[4 + nq32 + q] != 0;
        if (ovf) ++r.stats2;
        if (!cert) ++r.stats6;
        if (cert && !ovf && !force_exact && !(kp16 && force_f32) && !force_rethr) continue;
        todo.push_back(q);
    }
    r.todo_first = todo;
    if (kp16 && !todo.empty() && !no_rethr && !force_exact && !force_f32) {
        r.entered = true;
        const uint32_t* h_ovf = h_flags + 4 + nq32;
        const float* h_cut = reinterpret_cast<const float*>(h_flags + 4 + 2 * (size_t)nq32);
        for (uint32_t q : todo) {
            const float c = h_cut[q];
            if (!h_ovf[q] && c == c && std::isfinite(c)) { r.sel.push_back(q); r.cuts.push_back(c); }
            else r.rest.push_back(q);
        }
    }
    return r;
}
// ... the loop behind pass_rethreshold (fl: cert[nf] | overflow[nf]); returns stats[13]'s increment
uint64_t restated_after_rethreshold(const std::vector<uint32_t>& sel, const std::vector<uint32_t>& fl, std::vector<uint32_t>& rest, uint64_t* stats2) {
    uint64_t stats13 = 0;
    const uint32_t nf = (uint32_t)sel.size();
    for (uint32_t j = 0; j < nf; ++j) {
        if (fl[j] && !fl[nf + j]) ++stats13;
        else { rest.push_back(sel[j]); if (fl[nf + j]) ++*stats2; }
    }
    std::sort(rest.begin(), rest.end());
    return stats13;
}
// ... and the loop behind the f32 tier
std::vector<uint32_t> restated_after_f32(const std::vector<uint32_t>& todo, const std::vector<uint32_t>& f2, bool force_exact, uint64_t* stats2) {
    const uint32_t nf = (uint32_t)todo.size();
    std::vector<uint32_t> todo2;
    for (uint32_t j = 0; j < nf; ++j) {
        bool cert = f2[j] != 0, ovf = f2[nf + j] != 0;
        if (ovf) ++*stats2;
        if (cert && !ovf && !force_exact) continue;
        todo2.push_back(todo[j]);
    }
    return todo2;
}

void triage_cases() {
    constexpr uint32_t nq = 3;
    const float cut_kinds[3] = {1.5f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()};
    const uint32_t bits[5] = {VDB_TIERS_FORCE_EXACT, VDB_TIERS_FORCE_F32, VDB_TIERS_NO_RETHRESHOLD, VDB_TIERS_FORCE_RETHRESHOLD, VDB_TIERS_NO_DIRECT};
    std::vector<uint32_t> words(vdbi::SearchFlags::words(nq), 0);
    const vdbi::SearchFlags f(words.data(), nq);
    for (uint32_t combo = 0; combo < 12 * 12 * 12; ++combo) {                // 12 = 2 x 2 x 3 states per query
        for (uint32_t q = 0, c = combo; q < nq; ++q, c /= 12) {
            const uint32_t st = c % 12;
            f.cert[q] = st & 1; f.ovf[q] = (st >> 1) & 1; f.cut[q] = cut_kinds[st >> 2] + (float)q;   // (distinct finite cuts)
        }
        for (uint32_t subset = 0; subset < 32; ++subset) {
            uint32_t tiers = 0;
            for (int b = 0; b < 5; ++b) if (subset >> b & 1) tiers |= bits[b];
            for (uint32_t kp16 : {0u, 48u})
                for (uint32_t kp : {0u, 32u}) {
                    ++g_cases;
                    const Restated want = restated(words.data(), nq, tiers, kp16);
                    const vdbi::TierTriage got = vdbi::tier_triage(f.cert, f.ovf, f.cut, nq, tiers, kp16, kp);
                    bool ok = got.todo == want.todo_first && got.n_overflow == want.stats2 && got.n_uncertified == want.stats6 &&
                              got.rethreshold == want.entered && got.sel == want.sel && got.rest == want.rest &&
                              got.cuts.size() == want.cuts.size() && got.f32_tier == (kp16 != 0 && kp != 0);
                    for (size_t i = 0; ok && i < got.cuts.size(); ++i) ok = got.cuts[i] == want.cuts[i];   // (finite by construction)
                    if (!ok) { printf("FAILED triage: combo %u tiers %u kp16 %u kp %u\n", combo, tiers, kp16, kp); ++g_failed; }
                    // what search_part2 goes on with: rest when the block was entered, the first list otherwise
                    if (!want.entered) CHECK(got.sel.empty() && got.rest.empty() && got.cuts.empty());
                    // ---- the filter behind the re-threshold pass, for every flag combination of the compact block
                    const size_t nf = want.sel.size();
                    for (uint32_t fc = 0; nf && fc < (1u << (2 * nf)); ++fc) {
                        std::vector<uint32_t> fl(2 * nf);
                        for (size_t j = 0; j < 2 * nf; ++j) fl[j] = fc >> j & 1;
                        std::vector<uint32_t> rest_w = want.rest, rest_g = got.rest;
                        uint64_t s2w = 0, s2g = 0;
                        const uint64_t a_w = restated_after_rethreshold(want.sel, fl, rest_w, &s2w);
                        const uint64_t a_g = vdbi::after_rethreshold(got.sel, fl, rest_g, &s2g);
                        CHECK(a_w == a_g && s2w == s2g && rest_w == rest_g);
                    }
                }
        }
    }
    // ---- the filter behind the f32 tier: every subset of {0, 1, 2} as the compact block, every flag combination, both FORCE_EXACT states
    for (uint32_t members = 1; members < 8; ++members) {
        std::vector<uint32_t> todo;
        for (uint32_t q = 0; q < 3; ++q) if (members >> q & 1) todo.push_back(q);
        const size_t nf = todo.size();
        for (uint32_t fc = 0; fc < (1u << (2 * nf)); ++fc)
            for (uint32_t tiers : {0u, (uint32_t)VDB_TIERS_FORCE_EXACT, (uint32_t)(VDB_TIERS_FORCE_F32 | VDB_TIERS_NO_DIRECT)}) {
                std::vector<uint32_t> f2(2 * nf + 4, 0xdeadbeefu);           // (the status block behind the flags is not looked at)
                for (size_t j = 0; j < 2 * nf; ++j) f2[j] = fc >> j & 1;
                uint64_t s2w = 0, s2g = 0;
                ++g_cases;
                CHECK(restated_after_f32(todo, f2, (tiers & VDB_TIERS_FORCE_EXACT) != 0, &s2w) == vdbi::after_f32(todo, f2.data(), tiers, &s2g));
                CHECK(s2w == s2g);
            }
    }
}

void flag_blocks() {
    for (size_t nq : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257}) {
        CHECK(vdbi::SearchFlags::words(nq) == 4 + 3 * nq);
        CHECK(vdbi::RangeFlags::words(nq) == 4 + 4 * nq);
        std::vector<uint32_t> a(vdbi::SearchFlags::words(nq)), b(vdbi::RangeFlags::words(nq), 0);   // exactly the words: ASan sees an overrun
        const vdbi::SearchFlags s(a.data(), nq);
        CHECK(s.status == a.data() && s.cert == a.data() + 4 && s.ovf == s.cert + nq);
        CHECK(reinterpret_cast<uint32_t*>(s.cut) == s.ovf + nq);
        CHECK(reinterpret_cast<uint32_t*>(s.cut) + nq == a.data() + a.size());
        CHECK(vdbi::status_summary(s.status) == a.data() + 1 && vdbi::status_qmax(s.status) == a.data() + 2);
        const vdbi::RangeFlags r(b.data(), nq);
        CHECK(r.status == b.data() && r.ovf == b.data() + 4 && r.nocut == r.ovf + nq && r.complete == r.nocut + nq && r.n_keys == r.complete + nq);
        CHECK(r.n_keys + nq == b.data() + b.size());
        // no two fields share a word: every field writes its own tag everywhere, and every word ends up written exactly once
        for (size_t i = 0; i < vdbi::STATUS_WORDS; ++i) r.status[i] += 1;
        for (size_t q = 0; q < nq; ++q) { r.ovf[q] += 1; r.nocut[q] += 1; r.complete[q] += 1; r.n_keys[q] += 1; }
        bool once = true;
        for (uint32_t w : b) once = once && w == 1;
        CHECK(once);
    }
}

}  // namespace

int main() {
    triage_cases();
    flag_blocks();
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("tier triage ok: %ld cases\n", g_cases);
    return 0;
}
