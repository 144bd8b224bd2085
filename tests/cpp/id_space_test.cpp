// Ids from each family of tests/id_families.py through the C++ host mirror (vdb_host.hpp) and the C ABI: add, len,
// get_vector, search of one tie group (every row equal: the order is the id's alone), remove, search again.  Prints
//   <family> <phase> <id> <id> ...
// lines in decimal; tests/test_gpu_id_space.py compares them with the families computed in Python.  Needs an MI355X.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "vdb_host.hpp"
using namespace vdb_host;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static std::vector<uint64_t> family(const std::string& f, uint64_t n) {
    std::vector<uint64_t> v(n);
    for (uint64_t i = 0; i < n; ++i) {
        if (f == "control") v[i] = i;
        else if (f == "across32") v[i] = (1ull << 32) - n / 2 + i;
        else if (f == "across63") v[i] = (1ull << 63) - n / 2 + i;
        else if (f == "top") v[i] = (uint64_t)0 - n + i;
        else if (f == "high_word_only") v[i] = (i << 32) | 0x9e3779b9ull;
        else v[i] = (0xdeadbeefull << 32) | i;
    }
    return v;
}

static void print(const std::string& f, const char* phase, const std::vector<Neighbor>& r) {
    std::printf("%s %s", f.c_str(), phase);
    for (auto& x : r) std::printf(" %" PRIu64, (uint64_t)x.first);
    std::printf("\n");
}

int main() {
    static_assert(sizeof(size_t) == 8, "the mirror's ids are size_t: 64 bits");
    const uint64_t n = 48;
    for (const char* name : {"control", "across32", "across63", "top", "high_word_only", "low_word_only"}) {
        const std::string f = name;
        const auto ids = family(f, n);
        GpuFlatIndex ix(DistanceMetric::Euclidean);
        for (uint64_t i = 0; i < n; ++i) {                       // inserted in a scrambled order: the id rank decides, not the row
            const uint64_t j = (i * 29) % n;
            ix.add(ids[j], Vector{1.f, 2.f, 3.f});
        }
        CHECK(ix.len() == n);
        CHECK(ix.get_vector(ids[n - 1]) && ix.get_vector(ids[n / 2]) && !ix.get_vector(ids[n - 1] + 1) && !ix.get_vector(ids[0] - 1));
        const auto r = ix.search(Vector{0.f, 0.f, 0.f}, 20);
        CHECK(r.size() == 20);
        print(f, "first20", r);
        print(f, "all", ix.search(Vector{0.f, 0.f, 0.f}, n + 5));
        for (uint64_t i = 0; i < n; i += 3) ix.remove(ids[i]);  // every third id, the smallest included
        ix.remove(ids[n - 1]);                                   // and the largest
        CHECK(ix.len() == n - (n + 2) / 3 - 1 && !ix.get_vector(ids[n - 1]) && !ix.get_vector(ids[0]) && ix.get_vector(ids[1]));
        print(f, "after_remove", ix.search(Vector{0.f, 0.f, 0.f}, n));
        ix.add(ids[n - 1], Vector{0.f, 0.f, 0.f});               // the largest id again, now the nearest row
        const auto z = ix.search(Vector{0.f, 0.f, 0.f}, 1);
        CHECK(z.size() == 1 && z[0].first == ids[n - 1] && z[0].second == 0.f);
        print(f, "readd", z);
    }
    std::printf("id space ok\n");
    return 0;
}
