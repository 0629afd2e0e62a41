// tests/tools/abundance_collide.cpp -- the CPU search behind the constants of tests/abundance_table.py: k-mers whose
// keys in the min_count builder's counting table (cobs_amd/csrc/abundance_kernels.hip) share the 24-bit tag AND the
// home slot of the smallest table (1024 slots), 34 bits in all.  Stand-alone, host only, not part of the suite:
//
//     c++ -O2 -std=c++17 -pthread tests/tools/abundance_collide.cpp -o /tmp/abundance_collide && /tmp/abundance_collide [threads]
//
// prints Python literals; tests/test_abundance_table_cpu.py re-derives every property it claims from the plain-Python
// restatement, so a mistake here cannot reach the GPU tests unnoticed.
//
// The key, restated from the kernel: h = mix64(XXH64(canonical bytes, seed 0x5851F42D4C957F2D) ^ doc * 0x9E3779B97F4A7C15),
// mix64 = the splitmix64 finaliser (add the golden ratio first), tag = h >> 40, home = h & (cap - 1).  XXH64 is the public
// xxHash specification.  P1 .. P6 are birthday searches (two keys of ONE document), P7 runs over (k-mer, document pair)
// trials: the same k-mer in two documents of one batch.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace {

constexpr uint64_t P1 = 0x9E3779B185EBCA87ULL, P2 = 0xC2B2AE3D27D4EB4FULL, P3 = 0x165667B19E3779F9ULL,
                   P4 = 0x85EBCA77C2B2AE63ULL, P5 = 0x27D4EB2F165667C5ULL;
constexpr uint64_t kKeySeed = 0x5851F42D4C957F2DULL, kPhi = 0x9E3779B97F4A7C15ULL;

inline uint64_t rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
inline uint64_t rd64(const uint8_t* p) { uint64_t v; std::memcpy(&v, p, 8); return v; }
inline uint64_t rd32(const uint8_t* p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
inline uint64_t xround(uint64_t acc, uint64_t in) { return rotl(acc + in * P2, 31) * P1; }
inline uint64_t xmerge(uint64_t h, uint64_t v) { return (h ^ xround(0, v)) * P1 + P4; }

uint64_t xxh64(const uint8_t* p, size_t len, uint64_t seed) {
    const uint8_t* end = p + len;
    uint64_t h;
    if (len >= 32) {
        uint64_t v1 = seed + P1 + P2, v2 = seed + P2, v3 = seed, v4 = seed - P1;
        do {
            v1 = xround(v1, rd64(p)); v2 = xround(v2, rd64(p + 8)); v3 = xround(v3, rd64(p + 16)); v4 = xround(v4, rd64(p + 24));
            p += 32;
        } while (p + 32 <= end);
        h = rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
        h = xmerge(h, v1); h = xmerge(h, v2); h = xmerge(h, v3); h = xmerge(h, v4);
    } else {
        h = seed + P5;
    }
    h += (uint64_t)len;
    while (p + 8 <= end) { h ^= xround(0, rd64(p)); h = rotl(h, 27) * P1 + P4; p += 8; }
    if (p + 4 <= end) { h ^= rd32(p) * P1; h = rotl(h, 23) * P2 + P3; p += 4; }
    while (p < end) { h ^= (uint64_t)*p * P5; h = rotl(h, 11) * P1; ++p; }
    h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32;
    return h;
}

inline uint64_t mix64(uint64_t z) {
    z += kPhi;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

inline uint8_t fwd(uint8_t c) { return (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? c : 0; }
inline uint8_t comp(uint8_t c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 0; }

// the bytes handed to the hash function (canonicalize_kmer: invalid -> 0, the first strict difference among the first
// k / 2 positions picks the smaller of forward and reverse complement, ties keep the forward one)
std::string canonical(const std::string& t, bool canonicalize) {
    if (!canonicalize) return t;
    const size_t k = t.size();
    std::string f(k, 0), r(k, 0);
    for (size_t i = 0; i < k; ++i) { f[i] = (char)fwd((uint8_t)t[i]); r[i] = (char)comp((uint8_t)t[k - 1 - i]); }
    for (size_t s = 0; s < k / 2; ++s) {
        if ((uint8_t)f[s] < (uint8_t)r[s]) return f;
        if ((uint8_t)f[s] > (uint8_t)r[s]) return r;
    }
    return f;
}

inline uint64_t key_hash(const std::string& bytes, uint64_t doc) {
    return mix64(xxh64((const uint8_t*)bytes.data(), bytes.size(), kKeySeed) ^ (doc * kPhi));
}
inline uint64_t bits34(uint64_t h) { return ((h >> 40) << 10) | (h & 1023u); }     // tag, home slot at 1024 slots

struct Rng {
    uint64_t s;
    uint64_t next() { s += kPhi; uint64_t z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; return z ^ (z >> 31); }
};

std::string random_kmer(Rng& g, size_t k) {
    std::string t(k, 'A');
    uint64_t w = 0;
    for (size_t i = 0; i < k; ++i) {
        if (i % 32 == 0) w = g.next();
        t[i] = "ACGT"[w & 3];
        w >>= 2;
    }
    return t;
}

struct Cand { uint64_t v; uint32_t idx; };

// a birthday search over `n` candidates of doc 0; cls(i) in {0, 1} and a pair must have one of each class when `cross`
bool birthday(const char* name, size_t k, bool canonicalize, int invalid_a, int invalid_b, bool canonical_form, uint64_t seed, size_t n) {
    Rng g{seed};
    std::vector<std::string> raw(n), key(n);
    std::vector<Cand> c(n);
    const bool cross = invalid_a != invalid_b;
    for (size_t i = 0; i < n; ++i) {
        std::string t = random_kmer(g, k);
        const int inv = (cross && (i & 1)) ? invalid_b : invalid_a;
        if (inv) t[g.next() % k] = "NXn"[g.next() % 3];
        if (canonical_form) t = canonical(t, true);
        raw[i] = t;
        key[i] = canonical(t, canonicalize);
        c[i] = Cand{bits34(key_hash(key[i], 0)), (uint32_t)i};
    }
    std::sort(c.begin(), c.end(), [](const Cand& a, const Cand& b) { return a.v < b.v || (a.v == b.v && a.idx < b.idx); });
    for (size_t i = 0; i + 1 < n; ++i) {
        if (c[i].v != c[i + 1].v) continue;
        const uint32_t a = c[i].idx, b = c[i + 1].idx;
        if (key[a] == key[b]) continue;
        if (cross && ((a ^ b) & 1) == 0) continue;
        const uint32_t x = (cross && (a & 1)) ? b : a, y = x == a ? b : a;     // cross: x is the valid one
        std::printf("%s = (b\"%s\", b\"%s\")    # k = %zu, canonicalize = %d, tag 0x%06llx, home %llu\n", name, raw[x].c_str(),
                    raw[y].c_str(), k, (int)canonicalize, (unsigned long long)(c[i].v >> 10), (unsigned long long)(c[i].v & 1023));
        return true;
    }
    std::printf("# %s: no pair among %zu candidates\n", name, n);
    return false;
}

}  // namespace

int main(int argc, char** argv) {
    const unsigned threads = argc > 1 ? (unsigned)std::atoi(argv[1]) : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    const size_t n = (size_t)1 << 20;
    birthday("P1", 31, true, 0, 0, false, 101, n);
    birthday("P2", 31, false, 0, 0, false, 102, n);
    birthday("P3", 31, true, 0, 1, false, 103, n);
    birthday("P4", 31, true, 1, 1, false, 104, n);
    birthday("P5", 20, true, 0, 0, true, 105, n);
    birthday("P6", 40, true, 0, 0, true, 106, n);

    // keys needed by their home slot only: canonical-form 31-mers of document 0, four per slot 1020 .. 1023
    {
        Rng g{107};
        std::vector<std::vector<std::string>> by(4);
        size_t have = 0;
        while (have < 16) {
            const std::string t = canonical(random_kmer(g, 31), true);
            const uint64_t home = key_hash(t, 0) & 1023u;
            if (home >= 1020 && by[home - 1020].size() < 4) { by[home - 1020].push_back(t); ++have; }
        }
        std::printf("HOME_1024 = {\n");
        for (int s = 0; s < 4; ++s) {
            std::printf("    %d: (", 1020 + s);
            for (const auto& t : by[s]) std::printf("b\"%s\", ", t.c_str());
            std::printf("),\n");
        }
        std::printf("}\n");
    }

    // P7: one canonical-form 31-mer whose keys in two of the documents 0 .. 11 collide
    {
        constexpr int kDocs = 12;
        const auto t0 = std::chrono::steady_clock::now();
        std::atomic<bool> found{false};
        std::atomic<uint64_t> trials{0};
        std::mutex mu;
        std::string best;
        int da = 0, db = 0;
        uint64_t bv = 0;
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < threads; ++t)
            pool.emplace_back([&, t]() {
                Rng g{0x7000 + t};
                uint64_t v[kDocs], mine = 0;
                while (!found.load(std::memory_order_relaxed)) {
                    for (int rep = 0; rep < 4096; ++rep) {
                        const std::string x = canonical(random_kmer(g, 31), true);
                        const uint64_t xh = xxh64((const uint8_t*)x.data(), 31, kKeySeed);
                        for (int d = 0; d < kDocs; ++d) v[d] = bits34(mix64(xh ^ ((uint64_t)d * kPhi)));
                        for (int a = 0; a < kDocs; ++a)
                            for (int b = a + 1; b < kDocs; ++b)
                                if (v[a] == v[b]) {
                                    std::lock_guard<std::mutex> l(mu);
                                    if (!found.exchange(true)) { best = x; da = a; db = b; bv = v[a]; }
                                }
                    }
                    mine += 4096;
                    trials.fetch_add(4096, std::memory_order_relaxed);
                }
                (void)mine;
            });
        for (auto& th : pool) th.join();
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("P7 = (b\"%s\", %d, %d)    # tag 0x%06llx, home %llu; %.3g k-mers x 66 document pairs, %.1f s on %u threads\n",
                    best.c_str(), da, db, (unsigned long long)(bv >> 10), (unsigned long long)(bv & 1023),
                    (double)trials.load(), sec, threads);
    }
    return 0;
}
