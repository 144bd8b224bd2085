// The escalation ladder of the staged searches by stored examples (csrc/vdb_stages.h: run_stages, unanswered, scan_pass_width),
// on the CPU.  The header includes nothing of HIP; no runtime is linked and no GPU touched.  Built with
// -fsanitize=address,undefined by tests/test_stage_ladder_cpu.py.
//   1. run_stages against `restated` below: the tail of recommend_best_drive and discover_drive as both had it before the
//      function was lifted out, kept here word for word, with the loop that built `left` from the flags.  Over every route in
//      {0, 1, 2}, nq in {0, 1, 3}, D0 < len and D0 == len, D1 > D0 and D1 == D0, every subset of the requests answered by stage 0
//      and every subset of the rest answered by stage 1, and no error or an error code from the stage-0 lists, the stage-1 lists
//      or the scan.  Compared: the sequence of calls with their request lists and depths, all eight statistics words (only
//      [2..4] may change), the returned code.
//   2. scan_pass_width at n in {0, 1, 2^25 - 1, 2^25, 2^25 + 1} x nr in {1, SUPER, SUPER + 1} against the formula written out.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../vectordb-from-scratch_amd/csrc/vdb_stages.h"

namespace {

int g_failed = 0;
long g_cases = 0;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

constexpr size_t SUPER = 256;                  // queries per pipeline pass (vdb_index.h)
constexpr int ERR = 7;                         // the code an injected failure returns
constexpr uint64_t UNTOUCHED = 0xdead0000ull;  // + i: what statistics word i holds before the ladder runs

// ---- the drivers' tail as it stood (st: the eight counters; run_lists / run_scan: the drivers' lambdas)
template <class RunLists, class RunScan>
int restated(size_t nq, size_t D0, size_t D1, size_t len, int route, uint64_t* st, RunLists run_lists, RunScan run_scan) {
    int rc;
    std::vector<uint32_t> todo(nq), left;
    for (size_t b = 0; b < nq; ++b) todo[b] = (uint32_t)b;
    // (automatic: lists whose depth is the whole index are the expensive way to scan it)
    const bool lists = route == 1 || (route == 0 && D0 < len);
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
    return 0;
}

// ---- the callables of one case: list stage i answers the requests of answered[i]; callable `fail_at` (0: the stage-0 lists,
// 1: the stage-1 lists, 2: the scan; -1: none) returns ERR.  Every call is written down.
struct Call {
    int kind;                                  // 0: lists, 1: scan
    std::vector<uint32_t> reqs;
    size_t depth;
    bool operator==(const Call& o) const { return kind == o.kind && reqs == o.reqs && depth == o.depth; }
};
struct Script {
    uint32_t answered[2];
    int fail_at;
    bool use_header_filter;                    // build `left` with vdbi::unanswered, else with the loop as it stood
    std::vector<Call> calls;
    int list_calls = 0;

    int lists(const std::vector<uint32_t>& reqs, size_t D, std::vector<uint32_t>* left) {
        const int stage = list_calls++;
        calls.push_back(Call{0, reqs, D});
        if (stage > 1) { CHECK(!"a third list stage"); return ERR; }
        if (fail_at == stage) return ERR;
        const size_t nr = reqs.size();
        std::vector<uint32_t> flag(nr);
        for (size_t j = 0; j < nr; ++j) flag[j] = (answered[stage] >> reqs[j]) & 1u;
        if (use_header_filter) *left = vdbi::unanswered(reqs, flag.data());
        else {
            left->clear();
            for (size_t j = 0; j < nr; ++j) if (!flag[j]) left->push_back(reqs[j]);
        }
        return 0;
    }
    int scan(const std::vector<uint32_t>& reqs) {
        calls.push_back(Call{1, reqs, 0});
        return fail_at == 2 ? ERR : 0;
    }
};

void one_case(size_t nq, size_t D0, size_t D1, size_t len, int route, uint32_t a0, uint32_t a1, int fail_at) {
    ++g_cases;
    uint64_t st_old[8], st_new[8];
    for (int i = 0; i < 8; ++i) st_old[i] = st_new[i] = UNTOUCHED + i;
    Script so{{a0, a1}, fail_at, false, {}}, sn{{a0, a1}, fail_at, true, {}};
    const int rc_old = restated(nq, D0, D1, len, route, st_old,
                                [&](const std::vector<uint32_t>& r, size_t D, std::vector<uint32_t>* l) { return so.lists(r, D, l); },
                                [&](const std::vector<uint32_t>& r) { return so.scan(r); });
    const int rc_new = vdbi::run_stages(nq, D0, D1, len, route, st_new,
                                        [&](const std::vector<uint32_t>& r, size_t D, std::vector<uint32_t>* l) { return sn.lists(r, D, l); },
                                        [&](const std::vector<uint32_t>& r) { return sn.scan(r); });
    CHECK(rc_old == rc_new);
    CHECK(so.calls == sn.calls);
    for (int i = 0; i < 8; ++i) {
        CHECK(st_old[i] == st_new[i]);
        if (i < 2 || i > 4) CHECK(st_new[i] == UNTOUCHED + i);
    }
    // what the ladder promises, said once more without the restatement
    if (fail_at < 0) CHECK(rc_new == 0);
    else CHECK(rc_new == 0 || rc_new == ERR);
    const bool lists = route == 1 || (route == 0 && D0 < len);
    if (!lists) { CHECK(sn.list_calls == 0); CHECK(st_new[2] == UNTOUCHED + 2 && st_new[3] == UNTOUCHED + 3); }
    if (nq == 0) CHECK(sn.calls.size() == (lists ? 1u : 0u) && st_new[4] == UNTOUCHED + 4);
    if (D1 <= D0) CHECK(sn.list_calls <= 1);
    for (const Call& c : sn.calls) {
        if (&c != &sn.calls[0] || c.kind == 1) CHECK(!c.reqs.empty());            // only stage 0 may run on nothing
        CHECK(std::is_sorted(c.reqs.begin(), c.reqs.end()));
    }
    if (rc_new == ERR) {
        CHECK(!sn.calls.empty());
        const Call& last = sn.calls.back();
        CHECK(fail_at == (last.kind == 1 ? 2 : sn.list_calls - 1));               // nothing ran behind the failure
    }
}

void ladder() {
    const size_t len = 10;
    for (int route = 0; route <= 2; ++route)
        for (size_t nq : {(size_t)0, (size_t)1, (size_t)3})
            for (size_t D0 : {(size_t)5, len})
                for (size_t D1 : {D0, D0 + 2})
                    for (uint32_t a0 = 0; a0 < (1u << nq); ++a0)
                        for (uint32_t a1 = 0; a1 < (1u << nq); ++a1) {
                            if (a1 & a0) continue;                                 // stage 1 only sees what stage 0 left
                            for (int fail_at = -1; fail_at <= 2; ++fail_at) one_case(nq, D0, D1, len, route, a0, a1, fail_at);
                        }
}

void pass_width() {
    const uint32_t M = 1u << 25;
    for (uint32_t n : {0u, 1u, M - 1, M, M + 1})
        for (size_t nr : {(size_t)1, SUPER, SUPER + 1}) {
            ++g_cases;
            const size_t want = std::min<size_t>(std::min<size_t>(nr, SUPER), std::max<size_t>(((size_t)1 << 25) / std::max<uint32_t>(n, 1), 1));
            CHECK(vdbi::scan_pass_width(nr, n, SUPER) == want);
            CHECK(want >= 1 && want <= nr && want <= SUPER);
            if (n >= M - 1) CHECK(want == 1);                                      // a store of 2^25 - 1 rows or more: one request a pass
            if (n <= 1) CHECK(want == std::min(nr, SUPER));
        }
    CHECK(vdbi::SCAN_PASS_KEYS == (size_t)1 << 25);
    CHECK(vdbi::unanswered({}, nullptr).empty());
}

}  // namespace

int main() {
    ladder();
    pass_width();
    if (g_failed) { printf("%d checks failed in %ld cases\n", g_failed, g_cases); return 1; }
    printf("stage ladder ok: %ld cases\n", g_cases);
    return 0;
}
