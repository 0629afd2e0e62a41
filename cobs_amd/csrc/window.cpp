// cobs_amd/csrc/window.cpp -- cobs_gpu_search_window: a search whose score is the largest number of set positions in any
// window of w = min(window, the query's positions) consecutive positions of the query, and cobs_gpu_best_window, the same
// number (with the window's start) from one cobs_gpu_hit_positions bitmap on the host.  Per device pass (cut by the
// workspace limit, on the handle's scratch batch): K1 hashes the queries (unchanged: findere and the invalid-bases policy
// live in its table) and the window scan appends the documents that reach the query's threshold to a pool
// (window_kernels.hip).  The pass, the pool's retry and the hand-over are the shared ones (pooled_pass.hpp,
// pooled_call.hpp); what stands here is what the window search refuses, the threshold and the window it stages per
// (file, query) and its scan launches.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <string>
#include <vector>

#include "coverage_kernels.hpp"     // coverage_tile_w: the scans share their mapping
#include "engine.hpp"
#include "pooled_pass.hpp"
#include "window_kernels.hpp"

namespace cobs_amd {

struct WindowWork : ScanWork {              // thr: [files][nq] thresholds | [files][nq] windows
    WindowWork() : ScanWork("window: the hit pool") {}
};

void destroy_window_work(WindowWork* w) { delete w; }

namespace {

// the scan of the pass's n queries over every resident chunk, into the pool
cobs_gpu_status launch_scans(const ScanCall& c, WindowWork* w, uint32_t window, cobs_gpu_batch* b, size_t n, uint64_t pool_cap,
                             hipStream_t st) {
    cobs_gpu_index* ix = c.ix;
    const size_t nf = ix->parts.size();
    for (size_t f = 0; f < nf; ++f) {
        const Part& p = ix->parts[f];
        WindowScanArgs sa{};
        sa.t = table_ref_for(b, f, p, c.z);
        sa.thr = w->thr.p + f * n;
        sa.win = w->thr.p + (nf + f) * n;
        sa.pool = w->hits.pool.p;
        sa.fill = w->hits.fill.p;
        sa.cap = pool_cap;
        sa.nq = (uint32_t)n;
        sa.num_docs = (uint32_t)p.meta.doc_names.size();
        sa.file_no = (uint32_t)f;
        sa.window = window;
        sa.seg = ix->tune.window_seg;        // (COBS_GPU_WINDOW_SEG, read when the index was opened)
        cobs_gpu_status s = for_each_resident_chunk(p, [&](const Chunk& ch) -> cobs_gpu_status {
            sa.data = ch.d_data;
            sa.pages = ch.d_pages;
            sa.pitch = ch.pitch;
            sa.cpp = ch.cpp;
            sa.total_chunks = ch.total_chunks;
            sa.tile_w = coverage_tile_w(ch.total_chunks);
            HIP_TRY(launch_window_scan(sa, st));
            return COBS_GPU_OK;
        });
        if (s != COBS_GPU_OK) return s;
    }
    return COBS_GPU_OK;
}

cobs_gpu_status search_window_impl(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq, uint32_t window,
                                   double threshold, size_t num_results, cobs_gpu_hit* hits, size_t cap, size_t* hit_offsets,
                                   size_t* bad_query) {
    if (!ix || !hit_offsets) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if ((nq && (!queries || !lens)) || (cap && !hits)) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if (nq >= 0xFFFFFFF0ull) return fail(COBS_GPU_ERR_ARG, "too many queries");
    if (window == 0) return fail(COBS_GPU_ERR_ARG, "window: a window holds at least one position");
    if (window > kWindowMax)
        return fail(COBS_GPU_ERR_UNSUPPORTED, "window: the scan's counters hold windows of at most " + std::to_string(kWindowMax) +
                    " positions (asked for " + std::to_string(window) + ")");
    if (ix->hbm_budget != 0 || any_streamed(ix)) return fail(COBS_GPU_ERR_UNSUPPORTED, "window: not on a handle with an HBM budget (its rows are not all resident)");
    if (ix->shard_count > 1) return fail(COBS_GPU_ERR_UNSUPPORTED, "window: not on one shard of several (a shard answers its own documents only)");
    for (size_t q = 0; q <= nq; ++q) hit_offsets[q] = 0;
    const size_t nf = ix->parts.size();
    const uint32_t z = ix->findere;
    // everything the host can refuse is refused before anything is launched
    cobs_gpu_status refused = check_query_lengths(ix, queries, lens, nq, z, [&](size_t q) -> cobs_gpu_status {
        if (lens[q] >= kWindowMaxLen)
            return fail(COBS_GPU_ERR_QUERY_TOO_LONG, "query too long: the window scan walks 32-bit positions and takes queries below " +
                        std::to_string(kWindowMaxLen) + " characters (query " + std::to_string(q) + ")");
        return COBS_GPU_OK;
    }, bad_query);
    if (refused != COBS_GPU_OK) return refused;
    if (nq == 0 || nf == 0) return COBS_GPU_OK;

    if (!ix->window) ix->window = new WindowWork;
    WindowWork* w = ix->window;
    std::vector<HitDev> recs;
    const ScanCall call{ix, queries, lens, threshold, bad_query, z, real_documents(*ix), &recs};
    // passes: K1's tables, a threshold and a window per (file, query) and -- when every document comes back -- the
    // pool's records stay below the search call's workspace limit
    const uint64_t terms_per_char = table_bytes_per_char(ix);
    const uint64_t pool_bytes = threshold > 0.0 ? 0 : call.real_total * sizeof(HitDev);
    cobs_gpu_status s = cut_passes(nq, ix->tune.pass_bytes,
        [&](size_t q) { return (uint64_t)(lens[q] + 16) * terms_per_char + pool_bytes + 8 * nf; },
        [&](size_t q0, size_t q1) {
            const size_t n = q1 - q0;
            return run_scan_pass(call, w, q0, q1, 2 * nf * n,
                // per (file, query): the query's positions depend on the file's term size, and with them w and the set
                // positions a window of w has to hold (0: every real document)
                [&](uint32_t* thr) {
                    for (size_t f = 0; f < nf; ++f) {
                        const uint64_t k = ix->parts[f].meta.term_size;
                        for (size_t q = q0; q < q1; ++q) {
                            const uint64_t pos = lens[q] - k + 1 - z;               // >= 1: check_query_lengths
                            const uint32_t win = (uint32_t)std::min<uint64_t>(window, pos);
                            thr[f * n + (q - q0)] = min_key<uint32_t>(threshold, win);
                            thr[(nf + f) * n + (q - q0)] = win;
                        }
                    }
                },
                [&](cobs_gpu_batch* b, uint64_t pool_cap, hipStream_t st) { return launch_scans(call, w, window, b, n, pool_cap, st); });
        });
    if (s != COBS_GPU_OK) return s;
    return hand_out_hits(recs, nq, num_results, hits, cap, hit_offsets);
}

}  // namespace
}  // namespace cobs_amd

using namespace cobs_amd;

extern "C" {

uint32_t cobs_gpu_best_window(const uint64_t* words, size_t n, uint32_t window, size_t* start) {
    return best_window(words, n, window, start);
}

cobs_gpu_status cobs_gpu_search_window(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                       uint32_t window, double threshold, size_t num_results, cobs_gpu_hit* hits, size_t cap,
                                       size_t* hit_offsets, size_t* bad_query) {
    return guarded([&]() {
        return search_window_impl(ix, queries, lens, nq, window, threshold, num_results, hits, cap, hit_offsets, bad_query);
    });
}

cobs_gpu_status cobs_gpu_window_ms(cobs_gpu_index* ix, double out[3]) {
    WindowWork* w = ix ? ix->window : nullptr;
    return take_ms(ix, out, 2, w ? w->ms : nullptr, w ? &w->passes : nullptr);
}

}  // extern "C"
