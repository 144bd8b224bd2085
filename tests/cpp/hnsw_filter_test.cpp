// The C++ host mirror's pre-filtered HNSW search (GpuHnswIndex::search_batch_masked, vdb_host.hpp) against the C ABI it wraps:
// the same results as vdb_hnsw_search_batch_masked, only eligible ids, k of them, and an all-ones mask equal to search_batch.
// Needs an MI355X; exits non-zero on the first failed check.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "vdb_host.hpp"
using namespace vdb_host;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

int main() {
    const size_t n = 400, dim = 8, k = 10;
    std::mt19937 rng(7);
    std::normal_distribution<float> nd(0.f, 1.f);
    auto rand_vec = [&]() { std::vector<float> v(dim); for (auto& x : v) x = nd(rng); return Vector(v); };
    GpuHnswIndex ix(DistanceMetric::Euclidean, HnswParams::make(8, 64, 50), 3);
    for (size_t i = 0; i < n; ++i) ix.add(i, rand_vec());
    std::vector<std::pair<Vector, size_t>> qs;
    for (int b = 0; b < 5; ++b) qs.emplace_back(rand_vec(), k);

    std::vector<uint64_t> even((n + 63) / 64, 0), ones((n + 63) / 64, 0);
    for (size_t i = 0; i < n; ++i) { ones[i / 64] |= 1ull << (i % 64); if (i % 2 == 0) even[i / 64] |= 1ull << (i % 64); }

    auto got = ix.search_batch_masked(qs, even.data(), n);
    CHECK(got.size() == qs.size());
    for (size_t b = 0; b < qs.size(); ++b) {
        CHECK(got[b].size() == k);
        for (auto& r : got[b]) CHECK(r.first % 2 == 0);
        std::vector<uint64_t> ids(k); std::vector<float> ds(k); size_t cnt = 0;
        CHECK(vdb_hnsw_search_batch_masked(ix.handle(), qs[b].first.as_slice().data(), 1, dim, k, 50, even.data(), n, ids.data(), ds.data(), &cnt) == VDB_OK);
        CHECK(cnt == got[b].size());
        for (size_t i = 0; i < cnt; ++i) CHECK(ids[i] == got[b][i].first && ds[i] == got[b][i].second);
    }
    auto all = ix.search_batch_masked(qs, ones.data(), n);
    auto plain = ix.search_batch(qs);
    CHECK(all == plain);
    auto none = ix.search_batch_masked(qs, even.data(), 0);                  // mask_bits = 0: nothing is eligible
    for (auto& r : none) CHECK(r.empty());
    std::printf("hnsw filter ok\n");
    return 0;
}
