// numeric_filter_test.cpp -- the numeric range predicates of the C++ host mirror (host/vdb_host.hpp: parse_number,
// MetadataFilter::lt / le / gt / ge, VectorStore::compile_filter) on the host alone: no index handle is created and no device
// is touched, so the program runs anywhere and is built with -fsanitize=address,undefined (tests/test_numeric_filter_cpp.py).
//   numeric_filter_test tests/golden/numeric_strings.tsv
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <unordered_map>

#include "vdb_host.hpp"

using namespace vdb_host;

static int failures = 0;
#define CHECK(cond, ...)                                                    \
    do {                                                                    \
        if (!(cond)) {                                                      \
            ++failures;                                                     \
            std::printf("FAIL %s:%d  %s  ", __FILE__, __LINE__, #cond);     \
            std::printf(__VA_ARGS__);                                       \
            std::printf("\n");                                              \
        }                                                                   \
    } while (0)

static uint64_t bits_of(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}

// an Index with nothing behind it: the store's maps and metadata work, searches answer nothing
class FakeIndex : public Index {
public:
    void add(size_t id, Vector v) override { rows_[id] = std::move(v); }
    void remove(size_t id) override { rows_.erase(id); }
    std::vector<Neighbor> search(const Vector&, size_t) const override { return {}; }
    const Vector* get_vector(size_t id) const override {
        auto it = rows_.find(id);
        return it == rows_.end() ? nullptr : &it->second;
    }
    DistanceMetric metric() const override { return DistanceMetric::Euclidean; }
    size_t len() const override { return rows_.size(); }
private:
    std::unordered_map<size_t, Vector> rows_;
};

static size_t fixture(const char* path) {
    std::ifstream in(path, std::ios::binary);
    CHECK(in.good(), "cannot open %s", path);
    std::string line;
    size_t n = 0, numeric = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        const size_t tab = line.rfind('\t');
        CHECK(tab != std::string::npos, "no tab in line %zu", n);
        if (tab == std::string::npos) continue;
        const std::string s = line.substr(0, tab), want = line.substr(tab + 1);
        double v = -1234.5;
        const bool ok = parse_number(s, &v);
        if (want == "-") {
            CHECK(!ok, "\"%s\" parsed as %a", s.c_str(), v);
            CHECK(v == -1234.5, "\"%s\": *out written on refusal", s.c_str());
        } else {
            char got[17];
            std::snprintf(got, sizeof got, "%016llx", (unsigned long long)bits_of(v));
            CHECK(ok && want == got, "\"%s\": want %s, got %s (ok=%d)", s.c_str(), want.c_str(), got, (int)ok);
            ++numeric;
        }
        ++n;
    }
    CHECK(n >= 30 && numeric >= 12, "fixture too short: %zu lines, %zu numeric", n, numeric);
    return n;
}

static bool py(MetadataFilter::Op op, double a, double b) {
    return op == MetadataFilter::Lt ? a < b : (op == MetadataFilter::Le ? a <= b : (op == MetadataFilter::Gt ? a > b : a >= b));
}

static void truth_table() {
    const double inf = std::numeric_limits<double>::infinity();
    const MetadataFilter::Op ops[] = {MetadataFilter::Lt, MetadataFilter::Le, MetadataFilter::Gt, MetadataFilter::Ge};
    const std::pair<const char*, double> strings[] = {{"10", 10.0}, {"-3.5", -3.5}, {"0", 0.0}, {"-0", -0.0}, {"5e-324", 5e-324}, {"-5e-324", -5e-324},
                                                     {"1e3", 1000.0}, {"9007199254740993", 9007199254740992.0}, {"1.7976931348623157e308", 1.7976931348623157e308}};
    const double consts[] = {0.0, -0.0, 10.0, -3.5, 5e-324, inf, -inf, 9007199254740992.0, std::nextafter(10.0, 11.0), std::nextafter(10.0, 9.0)};
    const char* junk[] = {"n/a", "", " 1", "1 ", "1_0", "inf", "nan", "0x10", "1e", ".", "-"};
    for (auto op : ops)
        for (double c : consts) {
            const MetadataFilter f = MetadataFilter::numeric(op, "n", c);
            for (auto& s : strings) {
                Metadata m;
                m.insert("n", s.first);
                CHECK(f.matches(m) == py(op, s.second, c), "op %d \"%s\" against %a", (int)op, s.first, c);
            }
            for (const char* s : junk) {
                Metadata m;
                m.insert("n", s);
                CHECK(!f.matches(m), "op %d matched the non-numeric \"%s\"", (int)op, s);
            }
            Metadata other;
            other.insert("other", "1");
            CHECK(!f.matches(other) && !f.matches(Metadata()), "op %d matched a row without the field", (int)op);
        }
    Metadata neg0, pos0, ten;
    neg0.insert("n", "-0");
    pos0.insert("n", "0");
    ten.insert("n", "10.0");
    CHECK(MetadataFilter::le("n", 0.0).matches(neg0) && MetadataFilter::ge("n", -0.0).matches(pos0), "-0 equals +0");
    CHECK(!MetadataFilter::lt("n", 0.0).matches(neg0) && !MetadataFilter::gt("n", -0.0).matches(pos0), "-0 equals +0");
    CHECK(!MetadataFilter::eq("n", "10").matches(ten) && MetadataFilter::ne("n", "10").matches(ten), "Eq / Ne stay string comparisons");
    CHECK(MetadataFilter::all({MetadataFilter::ge("n", 10), MetadataFilter::lt("n", 11)}).matches(ten), "10 <= 10.0 < 11");
    for (auto op : ops) {
        bool threw = false;
        try {
            MetadataFilter::numeric(op, "n", std::numeric_limits<double>::quiet_NaN());
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw, "op %d took a NaN constant", (int)op);
    }
}

static void compile_filter_over_a_store() {
    VectorStore<FakeIndex> st(std::make_unique<FakeIndex>());
    const char* prices[] = {"5", "50", "n/a", "7", nullptr, "70", "1e1", "25", "24.999", "-0"};
    const size_t n = sizeof prices / sizeof *prices;
    for (size_t i = 0; i < 70; ++i) {                                           // 70 rows: the mask has two words
        Metadata m;
        if (prices[i % n]) m.insert("price", prices[i % n]);
        m.insert("color", i % 3 ? "red" : "blue");
        st.insert_with_metadata("r" + std::to_string(i), Vector{(float)i, 0.0f}, m);
    }
    Metadata up;
    up.insert("price", "3");
    st.insert_with_metadata("r1", Vector{1.0f, 1.0f}, up);                      // an upsert: internal id 1 goes, 70 comes
    st.remove("r7");
    const double val[] = {5, 50, NAN, 7, NAN, 70, 10, 25, 24.999, -0.0};
    struct Case { MetadataFilter f; bool (*want)(double, bool red); };
    const Case cases[] = {
        {MetadataFilter::lt("price", 25), [](double p, bool) { return p < 25; }},
        {MetadataFilter::all({MetadataFilter::ge("price", 25), MetadataFilter::lt("price", 75), MetadataFilter::eq("color", "red")}),
         [](double p, bool red) { return p >= 25 && p < 75 && red; }},
        {MetadataFilter::any({MetadataFilter::gt("price", 50), MetadataFilter::le("price", 0)}), [](double p, bool) { return p > 50 || p <= 0; }},
        {MetadataFilter::gt("price", -std::numeric_limits<double>::infinity()), [](double p, bool) { return p == p; }},
        {MetadataFilter::lt("weight", 1e9), [](double, bool) { return false; }},
    };
    for (size_t c = 0; c < sizeof cases / sizeof *cases; ++c) {
        size_t bits = 0;
        const std::vector<uint64_t> mask = st.compile_filter(cases[c].f, &bits);
        CHECK(bits == 71 && mask.size() == 2, "case %zu: %zu bits, %zu words", c, bits, mask.size());
        if (mask.size() != 2) continue;
        for (size_t i = 0; i < 71; ++i) {
            bool want;
            if (i == 1 || i == 7) want = false;                                 // superseded, deleted
            else if (i == 70) want = cases[c].want(3.0, false);
            else want = cases[c].want(val[i % n], i % 3 != 0);
            CHECK((bool)((mask[i >> 6] >> (i & 63)) & 1) == want, "case %zu id %zu", c, i);
        }
        CHECK(mask[1] >> 7 == 0, "case %zu: tail bits set", c);
    }
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::printf("usage: numeric_filter_test numeric_strings.tsv\n");
        return 2;
    }
    const size_t lines = fixture(argv[1]);
    truth_table();
    compile_filter_over_a_store();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("numeric filter ok (%zu fixture lines)\n", lines);
    return 0;
}
