// tests/host/pooled_call.cpp -- a stand-alone host program (its own main, no GPU, no HIP header) over the host arithmetic of
// a pooled search call, cobs_amd/csrc/pooled_call.hpp: min_key, first_pool_cap, real_documents / real_ranges, cut_passes
// and hand_out_lists against values written out by hand.  Built and run with -fsanitize=address,undefined by
// tests/test_pooled_call_cpu.py:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       tests/host/pooled_call.cpp -o pooled_call
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "../../cobs_amd/csrc/pooled_call.hpp"

// the library's error text lives in engine.cpp; here the last one is kept for the checks
static std::string last_text;
namespace cobs_amd {
cobs_gpu_status fail(cobs_gpu_status st, const std::string& msg) {
    last_text = msg;
    return st;
}
}  // namespace cobs_amd

using namespace cobs_amd;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

// The plain search's rule as pass.cpp states it (threshold_for), written again here because that file needs the device
// runtime: ceil(t * T) in double, 0 where that is not > 0, clamped at 2^32 - 1.
static uint32_t plain_bound(double t, uint64_t terms) {
    const double v = std::ceil(t * (double)terms);
    if (!(v > 0)) return 0;
    if (v >= 4294967295.0) return 0xFFFFFFFFu;
    return (uint32_t)v;
}

static void test_min_key() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // a threshold that is not > 0: every document
    CHECK(min_key<uint32_t>(0.0, 100) == 0u);
    CHECK(min_key<uint32_t>(-0.0, 100) == 0u);
    CHECK(min_key<uint32_t>(-1.0, 100) == 0u);
    CHECK(min_key<uint32_t>(-inf, 100) == 0u);
    CHECK(min_key<uint32_t>(nan, 100) == 0u);
    CHECK(min_key<uint64_t>(0.0, 100) == 0ull);
    CHECK(min_key<uint64_t>(nan, 100) == 0ull);
    // the smallest threshold above 0: one position
    CHECK(min_key<uint32_t>(5e-324, 100) == 1u);
    CHECK(min_key<uint64_t>(5e-324, 100) == 1ull);
    // inf saturates; inf * 0 is NaN and counts as "at least 1"
    CHECK(min_key<uint32_t>(inf, 100) == 0xFFFFFFFFu);
    CHECK(min_key<uint64_t>(inf, 100) == ~0ull);
    CHECK(min_key<uint32_t>(inf, 0) == 1u);
    CHECK(min_key<uint64_t>(inf, 0) == 1ull);
    // P = 0
    CHECK(min_key<uint32_t>(0.5, 0) == 1u);
    CHECK(min_key<uint64_t>(0.5, 0) == 1ull);
    CHECK(min_key<uint32_t>(0.0, 0) == 0u);
    // a product exactly on an integer, and the threshold's double successor
    CHECK(min_key<uint32_t>(0.5, 100) == 50u);
    CHECK(min_key<uint32_t>(std::nextafter(0.5, 1.0), 100) == 51u);
    CHECK(min_key<uint64_t>(0.5, 100) == 50ull);
    CHECK(min_key<uint64_t>(std::nextafter(0.5, 1.0), 100) == 51ull);
    CHECK(min_key<uint32_t>(1.0, 100) == 100u);
    CHECK(min_key<uint32_t>(std::nextafter(1.0, 2.0), 100) == 101u);
    // the product is formed in double: 0.07 * 100 rounds up past 7
    CHECK(min_key<uint32_t>(0.07, 100) == 8u);
    // both saturations: 2^32 - 1 from 4294967295.0 on, 2^64 - 1 from the largest double below 2^64 on
    CHECK(min_key<uint32_t>(1.0, 4294967294ull) == 4294967294u);
    CHECK(min_key<uint32_t>(1.0, 4294967295ull) == 0xFFFFFFFFu);
    CHECK(min_key<uint32_t>(2.0, 4294967295ull) == 0xFFFFFFFFu);
    CHECK(min_key<uint32_t>(1e300, 7) == 0xFFFFFFFFu);
    CHECK(min_key<uint64_t>(2.0, 4294967295ull) == 8589934590ull);
    CHECK(min_key<uint64_t>(1.0, 18446744073709547520ull) == 18446744073709547520ull);     // 2^64 - 4096: a double
    CHECK(min_key<uint64_t>(1.0, 18446744073709549568ull) == ~0ull);                        // 2^64 - 2048: the last one
    CHECK(min_key<uint64_t>(1e300, 7) == ~0ull);
    // for every threshold > 0 it is the plain rule, at least 1
    const uint64_t Ps[] = {0, 1, 7, 255, 256, 65535, 4294967294ull};
    const double ts[] = {5e-324, 1e-300, 1e-9, 0.07, 0.25, 0.5, std::nextafter(0.5, 1.0), 0.999, 1.0, std::nextafter(1.0, 2.0), 2.0, 1e300, inf};
    for (uint64_t P : Ps)
        for (double t : ts) {
            const uint32_t plain = plain_bound(t, P);
            CHECK(min_key<uint32_t>(t, P) == (plain > 1u ? plain : 1u));
            if (plain < 0xFFFFFFFFu) CHECK(min_key<uint64_t>(t, P) == (plain > 1u ? plain : 1u));
        }
    // ... and where the threshold is not > 0 both say 0
    for (uint64_t P : Ps) {
        CHECK(min_key<uint32_t>(0.0, P) == 0u && plain_bound(0.0, P) == 0u);
        CHECK(min_key<uint32_t>(-1.0, P) == 0u && plain_bound(-1.0, P) == 0u);
        CHECK(min_key<uint32_t>(nan, P) == 0u && plain_bound(nan, P) == 0u);
    }
    // the one difference: a product that is 0 or NaN under a threshold > 0
    CHECK(plain_bound(0.5, 0) == 0u && min_key<uint32_t>(0.5, 0) == 1u);
    CHECK(plain_bound(inf, 0) == 0u && min_key<uint32_t>(inf, 0) == 1u);
}

static void test_first_pool_cap() {
    // every document comes back: every record
    CHECK(first_pool_cap(0, 0.0, 300, 5) == 1500);
    CHECK(first_pool_cap(0, -1.0, 300, 5) == 1500);
    CHECK(first_pool_cap(0, std::numeric_limits<double>::quiet_NaN(), 300, 5) == 1500);
    // a threshold: at most max(2^20, 1024 per list), never more than every record
    CHECK(first_pool_cap(0, 0.5, 300, 5) == 1500);
    CHECK(first_pool_cap(0, 0.5, 1000000, 5) == (1u << 20));
    CHECK(first_pool_cap(0, 0.5, 1000000, 2000) == 2000 * 1024);
    // hit_cap lowers it and never raises it
    CHECK(first_pool_cap(7, 0.5, 300, 5) == 7);
    CHECK(first_pool_cap(7, 0.0, 300, 5) == 7);
    CHECK(first_pool_cap(7, 0.0, 1, 5) == 5);
    // nothing to return: one record all the same
    CHECK(first_pool_cap(0, 0.0, 0, 5) == 1);
    CHECK(first_pool_cap(0, 0.5, 0, 5) == 1);
    CHECK(first_pool_cap(7, 0.5, 0, 5) == 1);
    CHECK(first_pool_cap(0, 0.5, 300, 0) == 1);
}

struct FakeMeta { std::vector<int> doc_names; };
struct FakePart { FakeMeta meta; uint64_t slot_begin, slot_count, local_offset; };
struct FakeIndex { std::vector<FakePart> parts; };
struct Range { uint32_t begin, end, doc0, file; };

static void test_real_documents() {
    FakeIndex ix;
    ix.parts.push_back(FakePart{{std::vector<int>(300)}, 0, 304, 0});        // the padding of the last byte is not real
    ix.parts.push_back(FakePart{{std::vector<int>(10)}, 16, 8, 304});        // a shard whose slots lie behind the documents
    ix.parts.push_back(FakePart{{std::vector<int>(100)}, 64, 64, 312});      // a shard that holds the file's tail: 36 real
    ix.parts.push_back(FakePart{{std::vector<int>(100)}, 0, 64, 376});       // ... and one that holds its head: all 64
    CHECK(real_documents_of(ix.parts[0]) == 300);
    CHECK(real_documents_of(ix.parts[1]) == 0);
    CHECK(real_documents_of(ix.parts[2]) == 36);
    CHECK(real_documents_of(ix.parts[3]) == 64);
    CHECK(real_documents(ix) == 400);
    const std::vector<Range> r = real_ranges<Range>(ix);
    CHECK(r.size() == 3);
    if (r.size() == 3) {
        CHECK(r[0].begin == 0 && r[0].end == 300 && r[0].doc0 == 0 && r[0].file == 0);
        CHECK(r[1].begin == 312 && r[1].end == 348 && r[1].doc0 == 64 && r[1].file == 2);
        CHECK(r[2].begin == 376 && r[2].end == 440 && r[2].doc0 == 0 && r[2].file == 3);
    }
    CHECK(real_documents(FakeIndex{}) == 0 && real_ranges<Range>(FakeIndex{}).empty());
}

typedef std::vector<std::pair<size_t, size_t>> Passes;

static Passes cut(const std::vector<uint64_t>& bytes, uint64_t limit, cobs_gpu_status* status = nullptr, size_t fail_at = ~(size_t)0) {
    Passes out;
    const cobs_gpu_status s = cut_passes(bytes.size(), limit, [&](size_t q) { return bytes[q]; }, [&](size_t a, size_t b) {
        out.emplace_back(a, b);
        return out.size() - 1 == fail_at ? COBS_GPU_ERR_HIP : COBS_GPU_OK;
    });
    if (status) *status = s;
    return out;
}

static void test_cut_passes() {
    // no query: one empty pass (no family comes here with it; the cutter keeps what its copies did)
    CHECK(cut({}, 100) == (Passes{{0, 0}}));
    // everything fits
    CHECK(cut({10, 20, 30}, 100) == (Passes{{0, 3}}));
    // the sum lands exactly on the limit | one byte more
    CHECK(cut({40, 60}, 100) == (Passes{{0, 2}}));
    CHECK(cut({40, 61}, 100) == (Passes{{0, 1}, {1, 2}}));
    CHECK(cut({40, 60, 1}, 100) == (Passes{{0, 2}, {2, 3}}));
    CHECK(cut({40, 60, 100, 1}, 100) == (Passes{{0, 2}, {2, 3}, {3, 4}}));
    // a limit below every query's bytes: one query per pass, no empty pass in front, between or behind
    CHECK(cut({50, 60, 70}, 10) == (Passes{{0, 1}, {1, 2}, {2, 3}}));
    CHECK(cut({50}, 10) == (Passes{{0, 1}}));
    CHECK(cut({5, 50, 5, 5}, 10) == (Passes{{0, 1}, {1, 2}, {2, 4}}));
    CHECK(cut({50, 60}, 0) == (Passes{{0, 1}, {1, 2}}));
    // the ranges partition [0, nq) in order, whatever the limit
    const std::vector<uint64_t> bytes = {7, 1, 9, 3, 3, 3, 12, 1, 1, 8, 2};
    for (uint64_t limit = 0; limit <= 60; ++limit) {
        const Passes p = cut(bytes, limit);
        size_t at = 0;
        for (const auto& r : p) {
            CHECK(r.first == at && r.second > r.first);
            uint64_t sum = 0;
            for (size_t q = r.first; q < r.second; ++q) sum += bytes[q];
            CHECK(sum <= limit || r.second - r.first == 1);
            // (greedy: the next query did not fit any more)
            if (r.second < bytes.size()) CHECK(sum + bytes[r.second] > limit);
            at = r.second;
        }
        CHECK(at == bytes.size());
    }
    // the first status that is not OK ends the call: in the middle | in the last pass
    cobs_gpu_status s = COBS_GPU_OK;
    CHECK(cut({50, 60, 70}, 10, &s, 1) == (Passes{{0, 1}, {1, 2}}) && s == COBS_GPU_ERR_HIP);
    CHECK(cut({50, 60, 70}, 10, &s, 2) == (Passes{{0, 1}, {1, 2}, {2, 3}}) && s == COBS_GPU_ERR_HIP);
    CHECK(cut({50, 60, 70}, 10, &s).size() == 3 && s == COBS_GPU_OK);
}

struct Rec { uint32_t list, score, file, doc; };
struct Hit { uint32_t file, doc, score; };
static bool operator==(const Hit& a, const Hit& b) { return a.file == b.file && a.doc == b.doc && a.score == b.score; }

static cobs_gpu_status hand_out(std::vector<Rec> recs, size_t n_lists, size_t num_results, std::vector<Hit>& hits, size_t cap, std::vector<size_t>& offs) {
    return hand_out_lists(recs, n_lists, [](const Rec& r) { return r.list; },
        [](const Rec& a, const Rec& b) {
            if (a.score != b.score) return a.score > b.score;
            if (a.file != b.file) return a.file < b.file;
            return a.doc < b.doc;
        }, num_results, hits.data(), cap, offs.data(), "nq", [](const Rec& r) { return Hit{r.file, r.doc, r.score}; });
}

static void test_hand_out_lists() {
    // three lists, the middle one empty; list 0 has four records with a tie in score that (file, document) decides
    const std::vector<Rec> recs = {
        {2, 5, 0, 9}, {0, 7, 1, 3}, {0, 9, 0, 4}, {2, 5, 0, 2}, {0, 7, 0, 8}, {0, 7, 1, 1}, {2, 6, 1, 0},
    };
    const Hit untouched{77, 77, 77};
    std::vector<Hit> hits(8, untouched);
    std::vector<size_t> offs(4, 99);
    // num_results = 0: whole lists
    CHECK(hand_out(recs, 3, 0, hits, 8, offs) == COBS_GPU_OK);
    CHECK((offs == std::vector<size_t>{0, 4, 4, 7}));
    CHECK((std::vector<Hit>(hits.begin(), hits.begin() + 7) ==
           std::vector<Hit>{{0, 4, 9}, {0, 8, 7}, {1, 1, 7}, {1, 3, 7}, {1, 0, 6}, {0, 2, 5}, {0, 9, 5}}));
    CHECK(hits[7] == untouched);
    // num_results = 1: the best of every list
    hits.assign(8, untouched);
    offs.assign(4, 99);
    CHECK(hand_out(recs, 3, 1, hits, 8, offs) == COBS_GPU_OK);
    CHECK((offs == std::vector<size_t>{0, 1, 1, 2}));
    CHECK((hits[0] == Hit{0, 4, 9}) && (hits[1] == Hit{1, 0, 6}) && hits[2] == untouched);
    // num_results = 3: cuts list 0, leaves list 2 whole; more than any list has: whole lists
    hits.assign(8, untouched);
    CHECK(hand_out(recs, 3, 3, hits, 8, offs) == COBS_GPU_OK);
    CHECK((offs == std::vector<size_t>{0, 3, 3, 6}));
    CHECK((hits[2] == Hit{1, 1, 7}) && (hits[3] == Hit{1, 0, 6}) && (hits[5] == Hit{0, 9, 5}) && hits[6] == untouched);
    CHECK(hand_out(recs, 3, 100, hits, 8, offs) == COBS_GPU_OK);
    CHECK((offs == std::vector<size_t>{0, 4, 4, 7}));
    // cap exactly what is used
    hits.assign(7, untouched);
    offs.assign(4, 99);
    CHECK(hand_out(recs, 3, 0, hits, 7, offs) == COBS_GPU_OK);
    CHECK((offs == std::vector<size_t>{0, 4, 4, 7}) && (hits[6] == Hit{0, 9, 5}));
    // ... and one less: ERR_CAPACITY, the offsets are all written (the last is the size needed), no hit is
    hits.assign(7, untouched);
    offs.assign(4, 99);
    last_text.clear();
    CHECK(hand_out(recs, 3, 0, hits, 6, offs) == COBS_GPU_ERR_CAPACITY);
    CHECK(last_text == "result buffer too small; hit_offsets[nq] holds the needed size");
    CHECK((offs == std::vector<size_t>{0, 4, 4, 7}));
    for (const Hit& h : hits) CHECK(h == untouched);
    // ... also with no buffer at all
    offs.assign(4, 99);
    std::vector<Rec> copy = recs;
    CHECK(hand_out_lists(copy, 3, [](const Rec& r) { return r.list; },
                         [](const Rec& a, const Rec& b) { return a.doc < b.doc; }, 2, (Hit*)nullptr, 0, offs.data(), "n_groups",
                         [](const Rec& r) { return Hit{r.file, r.doc, r.score}; }) == COBS_GPU_ERR_CAPACITY);
    CHECK(last_text == "result buffer too small; hit_offsets[n_groups] holds the needed size");
    CHECK((offs == std::vector<size_t>{0, 2, 2, 4}));
    // no record at all, and no list at all
    hits.assign(2, untouched);
    offs.assign(4, 99);
    CHECK(hand_out({}, 3, 0, hits, 0, offs) == COBS_GPU_OK);
    CHECK((offs == std::vector<size_t>{0, 0, 0, 0}) && hits[0] == untouched);
    offs.assign(1, 99);
    CHECK(hand_out({}, 0, 0, hits, 0, offs) == COBS_GPU_OK && offs[0] == 0);
}

int main() {
    test_min_key();
    test_first_pool_cap();
    test_real_documents();
    test_cut_passes();
    test_hand_out_lists();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("pooled_call ok");
    return 0;
}
