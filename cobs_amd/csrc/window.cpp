// cobs_amd/csrc/window.cpp -- cobs_gpu_search_window: a search whose score is the largest number of set positions in any
// window of w = min(window, the query's positions) consecutive positions of the query, and cobs_gpu_best_window, the same
// number (with the window's start) from one cobs_gpu_hit_positions bitmap on the host.  Per device pass (cut by the
// workspace limit, on the handle's scratch batch): K1 hashes the queries (unchanged: findere and the invalid-bases policy
// live in its table) and the window scan appends the documents that reach the query's threshold to a pool
// (window_kernels.hip).  A pool that overflows is grown to the fill the scan reports and the scan of that pass alone runs
// again.  The host orders every query's records and cuts them to num_results, as coverage.cpp does.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "coverage_kernels.hpp"     // coverage_tile_w: the scans share their mapping
#include "engine.hpp"
#include "prevalence_kernels.hpp"   // launch_prevalence_zero
#include "window_kernels.hpp"

namespace cobs_amd {

struct WindowWork {
    DevBuf<uint32_t> thr;                   // [files][nq] thresholds | [files][nq] windows
    DevBuf<HitDev> pool;
    DevBuf<unsigned long long> fill;
    PinnedBuf<uint32_t> h_thr;
    PinnedBuf<uint32_t> h_flags;            // K1's flag words | the pool's 64-bit fill
    PhaseEvents<3> ev;                      // before K1 | scan | after it
    double ms[2] = {0, 0};                  // hash | scan
    uint64_t passes = 0;
};

void destroy_window_work(WindowWork* w) { delete w; }

namespace {

struct Call {
    cobs_gpu_index* ix;
    const char* const* queries;
    const size_t* lens;
    uint32_t window;
    double threshold;
    size_t* bad_query;
    uint32_t z;
    uint64_t real_total;                    // real documents of all files
    std::vector<HitDev>* recs;              // the records of all passes, `query` = the call's query number
};

// set positions a window of w positions has to hold (0: every real document)
uint32_t window_threshold(double threshold, uint32_t w) {
    if (!(threshold > 0.0)) return 0u;
    const double v = std::ceil(threshold * (double)w);
    return !(v >= 1.0) ? 1u : v >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)v;
}

// the scan of the pass's queries over every resident chunk, into the pool
cobs_gpu_status launch_scans(const Call& c, WindowWork* w, cobs_gpu_batch* b, size_t n, uint64_t pool_cap, hipStream_t st) {
    cobs_gpu_index* ix = c.ix;
    const size_t nf = ix->parts.size();
    for (size_t f = 0; f < nf; ++f) {
        const Part& p = ix->parts[f];
        WindowScanArgs sa{};
        sa.t = table_ref_for(b, f, p, c.z);
        sa.thr = w->thr.p + f * n;
        sa.win = w->thr.p + (nf + f) * n;
        sa.pool = w->pool.p;
        sa.fill = w->fill.p;
        sa.cap = pool_cap;
        sa.nq = (uint32_t)n;
        sa.num_docs = (uint32_t)p.meta.doc_names.size();
        sa.file_no = (uint32_t)f;
        sa.window = c.window;
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

// one device pass over the queries [q0, q1)
cobs_gpu_status run_pass(const Call& c, size_t q0, size_t q1) {
    cobs_gpu_index* ix = c.ix;
    HIP_TRY(hipSetDevice(ix->device));
    if (!ix->window) ix->window = new WindowWork;
    WindowWork* w = ix->window;
    HIP_TRY(w->ev.create());
    cobs_gpu_batch* b = nullptr;
    if (cobs_gpu_status s = scratch_batch(ix, 0, &b); s != COBS_GPU_OK) return s;
    hipStream_t st = b->own_stream;
    const size_t n = q1 - q0;
    const size_t nf = ix->parts.size();
    size_t bad_local = 0;
    if (cobs_gpu_status s = set_queries_on(b, c.queries + q0, c.lens + q0, n, st, false, &bad_local, q0); s != COBS_GPU_OK) {
        if (c.bad_query && bad_local < n) *c.bad_query = q0 + bad_local;
        return s;
    }
    // per (file, query): the query's positions depend on the file's term size, and with them w and the threshold
    HIP_TRY(w->thr.reserve(2 * nf * n));
    HIP_TRY(w->h_thr.reserve(2 * nf * n));
    for (size_t f = 0; f < nf; ++f) {
        const uint64_t k = ix->parts[f].meta.term_size;
        for (size_t q = q0; q < q1; ++q) {
            const uint64_t pos = c.lens[q] - k + 1 - c.z;               // >= 1: check_query_lengths
            const uint32_t win = (uint32_t)std::min<uint64_t>(c.window, pos);
            w->h_thr.p[f * n + (q - q0)] = window_threshold(c.threshold, win);
            w->h_thr.p[(nf + f) * n + (q - q0)] = win;
        }
    }
    HIP_TRY(w->fill.reserve(1));
    HIP_TRY(w->h_flags.reserve(6));
    // the first guess of the pool (tuning key hit_cap: a small one, so that tests reach the overflow path)
    const uint64_t all = c.real_total * n;
    uint64_t pool_cap = c.threshold > 0.0 ? std::min<uint64_t>(all, std::max<uint64_t>(1u << 20, n * 1024ull)) : all;
    if (ix->tune.hit_cap) pool_cap = std::min<uint64_t>(pool_cap, ix->tune.hit_cap);
    pool_cap = std::max<uint64_t>(pool_cap, 1);
    auto reserve_pool = [&]() -> cobs_gpu_status {
        if (w->pool.reserve((size_t)pool_cap) != hipSuccess) {
            (void)hipGetLastError();
            // (not ERR_CAPACITY: that status promises the needed size of the CALLER's buffer in hit_offsets)
            return fail(COBS_GPU_ERR_HIP, "out of device memory for " + std::to_string(pool_cap) + " hit records; raise the threshold or use fewer queries per call");
        }
        return COBS_GPU_OK;
    };
    if (cobs_gpu_status s = reserve_pool(); s != COBS_GPU_OK) return s;

    HIP_TRY(hipMemcpyAsync(w->thr.p, w->h_thr.p, 2 * nf * n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_clear_flags(b->flags.p, st));
    HIP_TRY(launch_prevalence_zero(reinterpret_cast<uint32_t*>(w->fill.p), 2, st));
    HIP_TRY(w->ev.mark(0, st));
    if (cobs_gpu_status s = launch_hash_files(ix, b, n, c.z, st, [&](size_t f) { return ix->parts[f].num_tpages() != 0; });
        s != COBS_GPU_OK)
        return s;
    HIP_TRY(w->ev.mark(1, st));
    if (cobs_gpu_status s = launch_scans(c, w, b, n, pool_cap, st); s != COBS_GPU_OK) return s;
    HIP_TRY(w->ev.mark(2, st));
    HIP_TRY(hipMemcpyAsync(w->h_flags.p, b->flags.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(w->h_flags.p + 4, w->fill.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (w->ev.add_elapsed(w->ms)) w->passes++;
    if (cobs_gpu_status s = invalid_base_from_flags(w->h_flags.p[0], n, c.bad_query, q0); s != COBS_GPU_OK) return s;
    uint64_t fill = (uint64_t)w->h_flags.p[5] << 32 | w->h_flags.p[4];
    if (fill > pool_cap) {
        // overflow: the pool grows to the reported fill and the scan of this pass alone runs again (K1's table stays)
        pool_cap = fill;
        if (cobs_gpu_status s = reserve_pool(); s != COBS_GPU_OK) return s;
        HIP_TRY(launch_prevalence_zero(reinterpret_cast<uint32_t*>(w->fill.p), 2, st));
        HIP_TRY(w->ev.mark(1, st));
        if (cobs_gpu_status s = launch_scans(c, w, b, n, pool_cap, st); s != COBS_GPU_OK) return s;
        HIP_TRY(w->ev.mark(2, st));
        HIP_TRY(hipMemcpyAsync(w->h_flags.p + 4, w->fill.p, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        (void)w->ev.add_elapsed(w->ms, 1, 2);
        fill = (uint64_t)w->h_flags.p[5] << 32 | w->h_flags.p[4];
        if (fill > pool_cap) return fail(COBS_GPU_ERR_HIP, "window: the hit pool overflowed twice");
    }
    const size_t at = c.recs->size();
    c.recs->resize(at + (size_t)fill);
    if (fill) {
        HIP_TRY(hipMemcpy(c.recs->data() + at, w->pool.p, (size_t)fill * sizeof(HitDev), hipMemcpyDeviceToHost));
        for (size_t i = at; i < c.recs->size(); ++i) (*c.recs)[i].query += (uint32_t)q0;
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

    uint64_t real_total = 0;
    for (const Part& p : ix->parts) {
        const uint64_t docs = p.meta.doc_names.size();
        real_total += docs > p.slot_begin ? std::min<uint64_t>(docs - p.slot_begin, p.slot_count) : 0;
    }
    std::vector<HitDev> recs;
    const Call call{ix, queries, lens, window, threshold, bad_query, z, real_total, &recs};
    // passes: K1's tables, a threshold and a window per (file, query) and -- when every document comes back -- the
    // pool's records stay below the search call's workspace limit
    const uint64_t kLimit = ix->tune.pass_bytes;
    const uint64_t terms_per_char = table_bytes_per_char(ix);
    const uint64_t pool_bytes = threshold > 0.0 ? 0 : real_total * sizeof(HitDev);
    size_t first = 0;
    uint64_t bytes = 0;
    for (size_t q = 0; q < nq; ++q) {
        const uint64_t qb = (uint64_t)(lens[q] + 16) * terms_per_char + pool_bytes + 8 * nf;
        if (q > first && bytes + qb > kLimit) {
            if (cobs_gpu_status s = run_pass(call, first, q); s != COBS_GPU_OK) return s;
            first = q;
            bytes = 0;
        }
        bytes += qb;
    }
    if (cobs_gpu_status s = run_pass(call, first, nq); s != COBS_GPU_OK) return s;

    // ---- ordering: per query by best descending, then (file, document) ascending; num_results cuts the list
    std::sort(recs.begin(), recs.end(), [](const HitDev& a, const HitDev& b) {
        if (a.query != b.query) return a.query < b.query;
        if (a.score != b.score) return a.score > b.score;
        if (a.part != b.part) return a.part < b.part;
        return a.doc < b.doc;
    });
    std::vector<size_t> begin(nq + 1, 0);
    for (const HitDev& r : recs) begin[r.query + 1]++;
    for (size_t q = 0; q < nq; ++q) begin[q + 1] += begin[q];
    size_t used = 0;
    for (size_t q = 0; q < nq; ++q) {
        const size_t have = begin[q + 1] - begin[q];
        used += num_results ? std::min(have, num_results) : have;
        hit_offsets[q + 1] = used;
    }
    if (used > cap) return fail(COBS_GPU_ERR_CAPACITY, "result buffer too small; hit_offsets[nq] holds the needed size");
    for (size_t q = 0; q < nq; ++q) {
        const HitDev* r = recs.data() + begin[q];
        cobs_gpu_hit* out = hits + hit_offsets[q];
        for (size_t i = 0, n = hit_offsets[q + 1] - hit_offsets[q]; i < n; ++i) out[i] = cobs_gpu_hit{r[i].part, r[i].doc, r[i].score};
    }
    return COBS_GPU_OK;
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
    if (!ix || !out) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    for (int i = 0; i < 3; ++i) out[i] = 0;
    if (WindowWork* w = ix->window) {
        for (int i = 0; i < 2; ++i) {
            out[i] = w->ms[i];
            w->ms[i] = 0;
        }
        out[2] = (double)w->passes;
        w->passes = 0;
    }
    return COBS_GPU_OK;
}

}  // extern "C"
