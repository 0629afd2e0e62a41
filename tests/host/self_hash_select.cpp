// tests/host/self_hash_select.cpp -- a stand-alone host program (its own main, no GPU) over the shape-class selection of the
// self-hashing scan: all of geometry.cpp -- scan_geometry, tile_sub_indexes, self_hash_fits and the choice itself,
// self_hash_shape / pass_self_hash -- compiled into this program with the predicates of kernels.hpp it reads.
// Built and run with -fsanitize=address,undefined by tests/test_self_hash_select_cpu.py:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -D__HIP_PLATFORM_AMD__ -I<rocm>/include
//       -Icobs_amd/csrc -Iinclude tests/host/self_hash_select.cpp -o self_hash_select
// It walks every tile of a set of chunk layouts and counts the sub-indexes the tile really lies in, which
// tile_sub_indexes must bound (the kernel's LDS array is sized by that bound), checks the limits of self_hash_fits, and
// drives self_hash_shape / pass_self_hash over hand-built handles and batches: every condition that keeps a pass on the
// hash kernel's table, and the table-size rule of the default setting at its threshold.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cobs_amd/csrc/geometry.cpp"

// The program links no HIP runtime and none of the library's other translation units.  The handles below own no device
// memory, events or mappings, so what their destructors would release does not exist: the release calls and the
// out-of-line destructors are defined empty here.
extern "C" {
hipError_t hipFree(void*) { return hipSuccess; }
hipError_t hipHostFree(void*) { return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
}
namespace cobs_amd {
MappedFile::~MappedFile() {}
Part::~Part() {}
StreamBufs::~StreamBufs() {}
ResultArena::~ResultArena() {}
}  // namespace cobs_amd
cobs_gpu_index::~cobs_gpu_index() {}
cobs_gpu_batch::~cobs_gpu_batch() {}

using namespace cobs_amd;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static Chunk make_chunk(uint32_t npages, uint32_t cpp, uint64_t sig) {
    Chunk c;
    c.cpp = cpp;
    c.pitch = cpp * 16;
    c.total_chunks = npages * cpp;
    c.pages.resize(npages);
    c.vp.resize(npages);
    for (uint32_t p = 0; p < npages; ++p) { c.pages[p] = PageDev{}; c.pages[p].sig = sig + p; c.vp[p].fp = p; }
    return c;
}


// A handle of one compact file: `npages` whole sub-indexes of `cpp` 16-byte chunks per row, resident (one chunk).
static uint8_t resident_rows[16];
static void add_part(cobs_gpu_index& ix, uint32_t npages, uint32_t cpp, uint64_t sig) {
    ix.parts.emplace_back();
    Part& p = ix.parts.back();
    p.meta.kind = IndexKind::Compact;
    p.meta.term_size = 31;
    p.meta.canonicalize = 1;
    p.meta.num_hashes = 1;
    p.meta.header_page_size = cpp * 16ull;
    for (uint32_t k = 0; k < npages; ++k) p.meta.signature_sizes.push_back(sig + k);
    p.first_page = 0;
    p.end_page = npages;
    p.chunks.push_back(make_chunk(npages, cpp, sig));
    Chunk& c = p.chunks.back();
    c.d_data = resident_rows;
    for (VPage& v : c.vp) { v.col0 = 0; v.ncols = p.meta.page_row_bytes(); }
}

// The host side of a batch as set_queries leaves it: query lengths in terms -> block offsets per file, longest query, planes.
static void fill_batch(cobs_gpu_batch& b, cobs_gpu_index& ix, const std::vector<uint32_t>& terms) {
    b.ix = &ix;
    b.nq = terms.size();
    b.max_terms = 1;
    b.work.clear();
    b.work.resize(ix.parts.size());
    for (PartWork& w : b.work) {
        w.h_blk_off.assign(terms.size() + 1, 0);
        for (size_t q = 0; q < terms.size(); ++q) w.h_blk_off[q + 1] = w.h_blk_off[q] + (terms[q] + 7) / 8;
    }
    for (uint32_t t : terms) b.max_terms = std::max<uint64_t>(b.max_terms, t);
    b.planes = b.max_terms < 16 ? 4 : b.max_terms < 256 ? 8 : b.max_terms < 1024 ? 10 : 12;      // (scan_planes_for, to 2048 terms)
    b.elem_bytes = scan_score_bytes(b.planes);
    b.findere = ix.findere;
    b.invalid_bases = ix.invalid_bases;
    b.topk_k = 0;
    b.topk_direct = false;
}

static void selection_cases() {
    const std::vector<uint32_t> headline(3000, 1000);      // 3000 x 126 blocks x 32 B = 12 MB per sub-index
    {
        cobs_gpu_index ix;
        add_part(ix, 8, 104, 4000000);
        cobs_gpu_batch b;
        fill_batch(b, ix, headline);
        CHECK(ix.tune.scan_self_hash == 1);                // the shipped default
        CHECK(self_hash_shape(&b) && pass_self_hash(&b, 0.0) && pass_self_hash(&b, 0.8));
        // the switch
        ix.tune.scan_self_hash = 0;
        CHECK(!self_hash_shape(&b) && !pass_self_hash(&b, 0.0));
        ix.tune.scan_self_hash = 2;
        CHECK(self_hash_shape(&b));
        ix.tune.scan_self_hash = 1;
        // top-k runs keep the table (either form), the shape class itself does not change
        b.topk_k = 10;
        CHECK(self_hash_shape(&b) && !pass_self_hash(&b, 0.0));
        b.topk_k = 0; b.topk_direct = true;
        CHECK(!pass_self_hash(&b, 0.0));
        b.topk_direct = false;
        // invalid_bases = skip: thresholds come from K1's valid positions; without a threshold the scan records them
        b.invalid_bases = COBS_GPU_INVALID_SKIP;
        CHECK(pass_self_hash(&b, 0.0) && !pass_self_hash(&b, 0.8));
        b.invalid_bases = COBS_GPU_INVALID_MISS;
        CHECK(pass_self_hash(&b, 0.8));
        b.invalid_bases = COBS_GPU_INVALID_ERROR;
        // an HBM budget, findere, the LDS-staged variant
        ix.hbm_budget = 1ull << 30;
        CHECK(!self_hash_shape(&b));
        ix.hbm_budget = 0;
        b.findere = 1;
        CHECK(!self_hash_shape(&b));
        b.findere = 0;
        ix.tune.lds_staged = true;
        CHECK(!self_hash_shape(&b));
        ix.tune.lds_staged = false;
        // the file: three hash functions, another term size, 64-bit indices, streamed, row ranges, no chunk
        Part& p = ix.parts[0];
        p.meta.num_hashes = 3; CHECK(!self_hash_shape(&b)); p.meta.num_hashes = 1;
        p.meta.term_size = 21; CHECK(!self_hash_shape(&b)); p.meta.term_size = 31;
        p.idx64 = true; CHECK(!self_hash_shape(&b)); p.idx64 = false;
        p.streamed = true; CHECK(!self_hash_shape(&b)); p.streamed = false;
        p.has_row_ranges = true; CHECK(!self_hash_shape(&b)); p.has_row_ranges = false;
        // the chunk: not resident, a row range, a shard cut inside a sub-index (head columns, tail columns)
        Chunk& c = p.chunks[0];
        c.d_data = nullptr; CHECK(!self_hash_shape(&b)); c.d_data = resident_rows;
        c.row_range = true; CHECK(!self_hash_shape(&b)); c.row_range = false;
        c.vp[3].row0 = 1024; c.vp[3].nrows = 4096; CHECK(!self_hash_shape(&b)); c.vp[3].row0 = 0; c.vp[3].nrows = 0;
        c.vp[7].ncols -= 16; CHECK(!self_hash_shape(&b)); c.vp[7].ncols += 16;
        c.vp[0].col0 = 16; c.vp[0].ncols -= 16; CHECK(!self_hash_shape(&b)); c.vp[0].col0 = 0; c.vp[0].ncols += 16;
        CHECK(self_hash_shape(&b));
        std::vector<Chunk> none;
        p.chunks.swap(none); CHECK(!self_hash_shape(&b)); p.chunks.swap(none);
        // a second file that does not qualify keeps the whole pass on the table
        add_part(ix, 1, 80, 1021);
        fill_batch(b, ix, headline);
        CHECK(self_hash_shape(&b));
        ix.parts[1].meta.num_hashes = 2;
        CHECK(!self_hash_shape(&b));
        // no queries
        fill_batch(b, ix, {});
        CHECK(!self_hash_shape(&b) && !pass_self_hash(&b, 0.0));
    }
    {
        // the default's table rule: (blocks + one padding block per query) x 32 B of ONE sub-index must EXCEED 4 MiB.
        // 1024 queries of 127 blocks: exactly 4 MiB -- the table; one of them a block longer: 4 MiB + 32 -- self-hashing
        cobs_gpu_index ix;
        add_part(ix, 8, 104, 4000000);
        cobs_gpu_batch b;
        std::vector<uint32_t> terms(1024, 127 * 8);
        fill_batch(b, ix, terms);
        CHECK((b.work[0].h_blk_off[b.nq] + b.nq) * 32ull == kSelfHashMinTable);
        CHECK(!self_hash_shape(&b));
        ix.tune.scan_self_hash = 2;
        CHECK(self_hash_shape(&b));
        ix.tune.scan_self_hash = 1;
        terms[500] += 1;
        fill_batch(b, ix, terms);
        CHECK((b.work[0].h_blk_off[b.nq] + b.nq) * 32ull == kSelfHashMinTable + 32);
        CHECK(self_hash_shape(&b) && pass_self_hash(&b, 0.8));
        // the two measured batch sizes either side of it: 1000 and 3000 queries of 1000 terms
        fill_batch(b, ix, std::vector<uint32_t>(1000, 1000));
        CHECK(!self_hash_shape(&b));
        fill_batch(b, ix, std::vector<uint32_t>(3000, 1000));
        CHECK(self_hash_shape(&b));
    }
    {
        // the LDS array (2112 entries): 263 blocks and the padding block of a one-sub-index file fit, 264 do not;
        // short reads get the multi-query geometry, which has no self-hashing form
        cobs_gpu_index ix;
        add_part(ix, 1, 80, 1021);
        ix.tune.scan_self_hash = 2;
        cobs_gpu_batch b;
        fill_batch(b, ix, std::vector<uint32_t>(5, 2048));
        CHECK(self_hash_shape(&b));
        fill_batch(b, ix, std::vector<uint32_t>(5, 263 * 8));
        CHECK(self_hash_shape(&b));
        fill_batch(b, ix, std::vector<uint32_t>(5, 263 * 8 + 1));
        CHECK(!self_hash_shape(&b));
        fill_batch(b, ix, std::vector<uint32_t>(40, 70));
        CHECK(!self_hash_shape(&b));
        ix.tune.mq = 0;
        CHECK(self_hash_shape(&b));
        cobs_gpu_index narrow;
        add_part(narrow, 4, 13, 64);
        narrow.tune.scan_self_hash = 2;
        fill_batch(b, narrow, std::vector<uint32_t>(5, 2048));
        CHECK(!self_hash_shape(&b));
        // 13-chunk pages, 1000 terms: the geometry's own 16-chunk tiles lie in three sub-indexes (3 x 126 x 8 entries: the
        // table); 8-chunk tiles in two (2016 entries: self-hashing); 64-chunk tiles in all four
        fill_batch(b, narrow, std::vector<uint32_t>(5, 1000));
        CHECK(scan_geometry(narrow.parts[0].chunks[0], 125, 125, 1, 0, 10, false, narrow.tune).tile_w == 16);
        CHECK(!self_hash_shape(&b));
        narrow.tune.tile_w = 8;
        CHECK(self_hash_shape(&b));
        narrow.tune.tile_w = 64;
        CHECK(!self_hash_shape(&b));
    }
}

int main() {
    const uint32_t widths[] = {4, 8, 16, 32, 64};
    for (uint32_t npages : {1u, 2u, 4u, 8u, 245u})
        for (uint32_t cpp : {1u, 2u, 3u, 7u, 8u, 13u, 32u, 63u, 64u, 65u, 104u}) {
            const Chunk c = make_chunk(npages, cpp, 1000);
            for (uint32_t w : widths) {
                uint32_t worst = 0;
                for (uint32_t c0 = 0; c0 < c.total_chunks; c0 += w) {
                    const uint32_t c1 = std::min(c0 + w, c.total_chunks) - 1;
                    worst = std::max(worst, c1 / cpp - c0 / cpp + 1);
                }
                const uint32_t bound = tile_sub_indexes(c, w);
                CHECK(worst <= bound);
                CHECK(bound <= npages);
                if (npages == 1 || cpp % w == 0) CHECK(bound == 1);
                ScanGeom g{w, 4, false};
                for (uint64_t blocks : {1ull, 43ull, 44ull, 125ull, 131ull, 132ull, 256ull, 262ull, 263ull, 264ull, 100000ull}) {
                    const bool fits = self_hash_fits(c, g, blocks);
                    CHECK(fits == ((uint64_t)bound * (blocks + 1) * 8 <= kSelfHashEntries));
                    if (fits) CHECK((uint64_t)worst * (blocks + 1) * 8 <= kSelfHashEntries);      // what the kernel writes
                }
                g.multi_query = true;
                CHECK(!self_hash_fits(c, g, 1));
            }
        }
    // the limits the tests name: 2048 terms of one sub-index fit, of two they do not; 13-chunk pages under W = 8 and 64
    const Chunk narrow = make_chunk(4, 13, 64), wide = make_chunk(8, 104, 4000000), classic = make_chunk(1, 80, 1021);
    CHECK(tile_sub_indexes(narrow, 8) == 2 && tile_sub_indexes(narrow, 64) == 4 && tile_sub_indexes(wide, 8) == 1);
    CHECK(self_hash_fits(classic, ScanGeom{8, 4, false}, 256) && !self_hash_fits(narrow, ScanGeom{8, 4, false}, 256));
    CHECK(self_hash_fits(narrow, ScanGeom{8, 4, false}, 125) && !self_hash_fits(narrow, ScanGeom{64, 4, false}, 125));
    // the geometry the headline batch gets (125 blocks per query): 8-chunk tiles, four waves, one query per group
    Tuning tune;
    const ScanGeom g = scan_geometry(wide, 125, 125, 1, 0, 10, false, tune);
    CHECK(g.tile_w == 8 && g.nwaves == 4 && !g.multi_query && self_hash_fits(wide, g, 125));
    const ScanGeom reads = scan_geometry(wide, 9, 9, 1, 0, 8, false, tune);
    CHECK(reads.multi_query && !self_hash_fits(wide, reads, 9));
    selection_cases();
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::puts("self_hash_select ok");
    return 0;
}
