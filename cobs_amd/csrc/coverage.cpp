// cobs_amd/csrc/coverage.cpp -- cobs_gpu_search_coverage: a search whose score is the number of query BASES covered by
// the positions a document holds (a set position covers span = k + z bases), and cobs_gpu_covered_bases, the same count
// from one cobs_gpu_hit_positions bitmap on the host.  Per device pass (cut by the workspace limit, on the handle's
// scratch batch): K1 hashes the queries (unchanged: findere and the invalid-bases policy live in its table) and the
// coverage scan appends the documents that reach the query's threshold to a pool (coverage_kernels.hip).  The pass, the
// pool's retry and the hand-over are the shared ones (pooled_pass.hpp, pooled_call.hpp); what stands here is what coverage
// refuses, the threshold it stages per query (covered bases of the query's length) and its scan launches.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <string>
#include <vector>

#include "coverage_kernels.hpp"
#include "engine.hpp"
#include "pooled_pass.hpp"

namespace cobs_amd {

struct CoverageWork : ScanWork {            // thr: [nq]
    CoverageWork() : ScanWork("coverage: the hit pool") {}
};

void destroy_coverage_work(CoverageWork* w) { delete w; }

namespace {

// the scan of the pass's n queries (the longest has max_len characters) over every resident chunk, into the pool
cobs_gpu_status launch_scans(const ScanCall& c, CoverageWork* w, cobs_gpu_batch* b, size_t n, size_t max_len, uint64_t pool_cap,
                             hipStream_t st) {
    cobs_gpu_index* ix = c.ix;
    const int planes = coverage_planes_for(max_len);
    for (size_t f = 0; f < ix->parts.size(); ++f) {
        const Part& p = ix->parts[f];
        CoverageScanArgs sa{};
        sa.t = table_ref_for(b, f, p, c.z);
        sa.thr = w->thr.p;
        sa.pool = w->hits.pool.p;
        sa.fill = w->hits.fill.p;
        sa.cap = pool_cap;
        sa.nq = (uint32_t)n;
        sa.num_docs = (uint32_t)p.meta.doc_names.size();
        sa.file_no = (uint32_t)f;
        sa.span = p.meta.term_size + c.z;
        sa.seg = ix->tune.coverage_seg;      // (COBS_GPU_COVERAGE_SEG, read when the index was opened)
        cobs_gpu_status s = for_each_resident_chunk(p, [&](const Chunk& ch) -> cobs_gpu_status {
            sa.data = ch.d_data;
            sa.pages = ch.d_pages;
            sa.pitch = ch.pitch;
            sa.cpp = ch.cpp;
            sa.total_chunks = ch.total_chunks;
            sa.tile_w = coverage_tile_w(ch.total_chunks);
            HIP_TRY(launch_coverage_scan(sa, planes, st));
            return COBS_GPU_OK;
        });
        if (s != COBS_GPU_OK) return s;
    }
    return COBS_GPU_OK;
}

cobs_gpu_status search_coverage_impl(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                     double threshold, size_t num_results, cobs_gpu_hit* hits, size_t cap, size_t* hit_offsets,
                                     size_t* bad_query) {
    if (!ix || !hit_offsets) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if ((nq && (!queries || !lens)) || (cap && !hits)) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if (nq >= 0xFFFFFFF0ull) return fail(COBS_GPU_ERR_ARG, "too many queries");
    if (ix->hbm_budget != 0 || any_streamed(ix)) return fail(COBS_GPU_ERR_UNSUPPORTED, "coverage: not on a handle with an HBM budget (its rows are not all resident)");
    if (ix->shard_count > 1) return fail(COBS_GPU_ERR_UNSUPPORTED, "coverage: not on one shard of several (a shard answers its own documents only)");
    for (size_t q = 0; q <= nq; ++q) hit_offsets[q] = 0;
    const size_t nf = ix->parts.size();
    const uint32_t z = ix->findere;
    for (const Part& p : ix->parts)
        if (p.meta.term_size + z > kCoverageMaxSpan)
            return fail(COBS_GPU_ERR_UNSUPPORTED, "coverage: a position covers term size + findere z = " + std::to_string(p.meta.term_size + z) +
                        " bases; the countdown of the scan holds at most " + std::to_string(kCoverageMaxSpan));
    // everything the host can refuse is refused before anything is launched
    cobs_gpu_status refused = check_query_lengths(ix, queries, lens, nq, z, [&](size_t q) -> cobs_gpu_status {
        if (lens[q] >= kCoverageMaxLen)
            return fail(COBS_GPU_ERR_QUERY_TOO_LONG, "query too long: coverage search takes queries below " +
                        std::to_string(kCoverageMaxLen) + " characters (query " + std::to_string(q) + ")");
        return COBS_GPU_OK;
    }, bad_query);
    if (refused != COBS_GPU_OK) return refused;
    if (nq == 0 || nf == 0) return COBS_GPU_OK;

    if (!ix->coverage) ix->coverage = new CoverageWork;
    CoverageWork* w = ix->coverage;
    std::vector<HitDev> recs;
    const ScanCall call{ix, queries, lens, threshold, bad_query, z, real_documents(*ix), &recs};
    // passes: K1's tables, a threshold per query and -- when every document comes back -- the pool's records stay below
    // the search call's workspace limit
    const uint64_t terms_per_char = table_bytes_per_char(ix);
    const uint64_t pool_bytes = threshold > 0.0 ? 0 : call.real_total * sizeof(HitDev);
    cobs_gpu_status s = cut_passes(nq, ix->tune.pass_bytes,
        [&](size_t q) { return (uint64_t)(lens[q] + 16) * terms_per_char + pool_bytes + 4; },
        [&](size_t q0, size_t q1) {
            const size_t n = q1 - q0, max_len = *std::max_element(lens + q0, lens + q1);
            return run_scan_pass(call, w, q0, q1, n,
                // covered bases a document has to reach, of the query's length (0: every real document)
                [&](uint32_t* thr) { for (size_t q = q0; q < q1; ++q) thr[q - q0] = min_key<uint32_t>(threshold, lens[q]); },
                [&](cobs_gpu_batch* b, uint64_t pool_cap, hipStream_t st) { return launch_scans(call, w, b, n, max_len, pool_cap, st); });
        });
    if (s != COBS_GPU_OK) return s;
    return hand_out_hits(recs, nq, num_results, hits, cap, hit_offsets);
}

}  // namespace
}  // namespace cobs_amd

using namespace cobs_amd;

extern "C" {

uint64_t cobs_gpu_covered_bases(const uint64_t* words, size_t n, uint32_t span) {
    if (!words || n == 0) return 0;
    return covered_bases(words, n, span);
}

cobs_gpu_status cobs_gpu_search_coverage(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                         double threshold, size_t num_results, cobs_gpu_hit* hits, size_t cap,
                                         size_t* hit_offsets, size_t* bad_query) {
    return guarded([&]() {
        return search_coverage_impl(ix, queries, lens, nq, threshold, num_results, hits, cap, hit_offsets, bad_query);
    });
}

cobs_gpu_status cobs_gpu_coverage_ms(cobs_gpu_index* ix, double out[3]) {
    CoverageWork* w = ix ? ix->coverage : nullptr;
    return take_ms(ix, out, 2, w ? w->ms : nullptr, w ? &w->passes : nullptr);
}

}  // extern "C"
