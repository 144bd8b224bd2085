// vdb_stages.h -- the escalation ladder of the searches by stored examples (recommend by best score, discovery: DESIGN.md 4.17 "The staged driver"),
// the pass width of their exact scan, and the filter from a stage's answered flags to the requests it leaves over.  Plain host
// arithmetic: nothing of HIP is included, so tests/cpp/stage_ladder_test.cpp checks all of it on the CPU.  Not part of the C ABI.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vdbi {

// The requests of `reqs` whose flag a list stage left at zero (flags[j] belongs to reqs[j]), in order.
inline std::vector<uint32_t> unanswered(const std::vector<uint32_t>& reqs, const uint32_t* flags) {
    std::vector<uint32_t> left;
    for (size_t j = 0; j < reqs.size(); ++j) if (!flags[j]) left.push_back(reqs[j]);
    return left;
}

// Requests per pass of the exact scan: one key per (request, row), SCAN_PASS_KEYS keys in the buffer, at most `super` requests.
constexpr size_t SCAN_PASS_KEYS = (size_t)1 << 25;                 // keys of one scan pass (256 MiB)
inline size_t scan_pass_width(size_t nr, uint32_t n, size_t super) {
    return std::min<size_t>(std::min<size_t>(nr, super), std::max<size_t>(SCAN_PASS_KEYS / std::max<uint32_t>(n, 1), 1));
}

// The ladder over requests 0 .. nq - 1.  run_lists(reqs, depth, &left) -> int answers what it can of reqs from ranked lists of
// that depth and leaves the others in *left; run_scan(reqs) -> int answers all of reqs by the exact scan.  route 1 forces the
// lists, 2 goes straight to the scan, 0 is automatic: lists whose depth is the whole index are the expensive way to scan it.
// Stage 0 at depth D0; stage 1 at D1 for what is left, when that is deeper; the scan for what is still left.  st[2], st[3], st[4]
// receive the requests answered by stage 0, by stage 1 and by the scan (a stage that did not run leaves its word alone); the
// first non-zero code of a callable is returned at once.
template <class RunLists, class RunScan>
int run_stages(size_t nq, size_t D0, size_t D1, size_t len, int route, uint64_t* st, RunLists&& run_lists, RunScan&& run_scan) {
    std::vector<uint32_t> todo(nq), left;
    for (size_t b = 0; b < nq; ++b) todo[b] = (uint32_t)b;
    int rc;
    if (route == 1 || (route == 0 && D0 < len)) {
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

}  // namespace vdbi
