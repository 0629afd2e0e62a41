// cobs_amd/csrc/weighted.cpp -- cobs_gpu_search_weighted: a search whose score is the sum of IDF weights of the positions
// a document holds.  Per device pass (cut by the workspace limit, on the handle's scratch batch): K1 hashes the queries
// (unchanged: findere and the invalid-bases policy live in its table), the prevalence kernel counts the documents of
// every position into device cells, the weight kernel turns the cells into one byte per position plus W(q, f) and the
// threshold of every (query, file), and the weighted scan appends the documents that reach it to a pool
// (weighted_kernels.hip).  The pool with its retry, the pass cutter and the hand-over are the shared ones
// (pooled_pass.hpp, pooled_call.hpp).  The pass itself stands here and not in run_scan_pass: two kernels run in front of
// the scan, under five events, and the totals come home in the sync the flag words come home in.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "engine.hpp"
#include "pooled_pass.hpp"
#include "prevalence_kernels.hpp"
#include "weighted_kernels.hpp"

namespace cobs_amd {

struct WeightedWork {
    DevBuf<uint32_t> cells;
    DevBuf<uint8_t> weights;
    DevBuf<uint64_t> seg_off, total;
    DevBuf<uint32_t> thr;                   // [file][nq]
    HitPool<HitDev> hits{"weighted: the hit pool", launch_prevalence_zero};
    PinnedBuf<uint64_t> h_seg_off, h_total;
    PassLanding land;
    PhaseEvents<5> ev;                      // before K1 | prevalence | weights | scan | after it
    double ms[4] = {0, 0, 0, 0};            // hash | prevalence | weights | scan
    uint64_t passes = 0;
};

void destroy_weighted_work(WeightedWork* w) { delete w; }

namespace {

struct Call : ScanCall {
    uint64_t* total_weight;
};

// the scan of the pass's queries over every resident chunk, into the pool
cobs_gpu_status launch_scans(const Call& c, WeightedWork* w, cobs_gpu_batch* b, size_t n, size_t max_len, uint64_t pool_cap,
                             hipStream_t st) {
    cobs_gpu_index* ix = c.ix;
    const size_t nf = ix->parts.size();
    for (size_t f = 0; f < nf; ++f) {
        const Part& p = ix->parts[f];
        WeightedScanArgs sa{};
        sa.t = table_ref_for(b, f, p, c.z);
        sa.seg_off = w->seg_off.p + f;
        sa.weights = w->weights.p;
        sa.thr = w->thr.p + f * n;
        sa.pool = w->hits.pool.p;
        sa.fill = w->hits.fill.p;
        sa.cap = pool_cap;
        sa.seg_stride = (uint32_t)nf;
        sa.nq = (uint32_t)n;
        sa.num_docs = (uint32_t)p.meta.doc_names.size();
        sa.file_no = (uint32_t)f;
        const int planes = weighted_planes_for(max_len - p.meta.term_size + 1 - c.z);
        cobs_gpu_status s = for_each_resident_chunk(p, [&](const Chunk& ch) -> cobs_gpu_status {
            sa.data = ch.d_data;
            sa.pages = ch.d_pages;
            sa.pitch = ch.pitch;
            sa.cpp = ch.cpp;
            sa.total_chunks = ch.total_chunks;
            sa.tile_w = weighted_tile_w(ch.total_chunks);
            HIP_TRY(launch_weighted_scan(sa, planes, st));
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
    if (!ix->weighted) ix->weighted = new WeightedWork;
    WeightedWork* w = ix->weighted;
    HIP_TRY(w->ev.create());
    cobs_gpu_batch* b = nullptr;
    if (cobs_gpu_status s = pass_queries(ix, c.queries, c.lens, q0, q1, c.bad_query, &b); s != COBS_GPU_OK) return s;
    hipStream_t st = b->own_stream;
    const size_t n = q1 - q0, nf = ix->parts.size();
    // the cells of the pass: one segment per (query, file), each padded to a multiple of 8 -- the scan reads the eight
    // weights of a block with one aligned load, the padding weighs 0
    HIP_TRY(w->seg_off.reserve(n * nf + 1));
    HIP_TRY(w->h_seg_off.reserve(n * nf + 1));
    uint64_t ncells = 0;
    size_t max_len = 0;
    for (size_t q = q0; q < q1; ++q) {
        max_len = std::max(max_len, c.lens[q]);
        for (size_t f = 0; f < nf; ++f) {
            w->h_seg_off.p[(q - q0) * nf + f] = ncells;
            ncells += round_up(c.lens[q] - ix->parts[f].meta.term_size + 1 - c.z, 8);
        }
    }
    w->h_seg_off.p[n * nf] = ncells;
    HIP_TRY(w->cells.reserve(ncells));
    HIP_TRY(w->weights.reserve(ncells));
    HIP_TRY(w->total.reserve(n * nf));
    HIP_TRY(w->h_total.reserve(n * nf));
    HIP_TRY(w->thr.reserve(n * nf));
    HIP_TRY(w->land.reserve());

    HIP_TRY(hipMemcpyAsync(w->seg_off.p, w->h_seg_off.p, (n * nf + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_clear_flags(b->flags.p, st));
    uint64_t fill = 0;
    cobs_gpu_status s = w->hits.run(first_pool_cap(ix->tune.hit_cap, c.threshold, c.real_total, n), st, scan_pool_no_room,
        [&](uint64_t pool_cap, int attempt) -> cobs_gpu_status {
            if (attempt == 0) {         // (the retry scans alone: cells, weights and thresholds stay)
                // K1 and the prevalence of every position into the cells, exactly as cobs_gpu_prevalence fills its own
                if (cobs_gpu_status p = launch_prevalence_cells(ix, b, w->seg_off.p, w->cells.p, ncells, n, max_len, c.z, st, w->ev.ev[0], w->ev.ev[1]);
                    p != COBS_GPU_OK)
                    return p;
                HIP_TRY(w->ev.mark(2, st));
                for (size_t f = 0; f < nf; ++f) {
                    const Part& p = ix->parts[f];
                    WeightArgs wa{};
                    wa.cells = w->cells.p;
                    wa.weights = w->weights.p;
                    wa.seg_off = w->seg_off.p + f;
                    wa.q_len = b->d_qlen;
                    wa.total = w->total.p + f;
                    wa.thr = w->thr.p + f * n;
                    wa.threshold = c.threshold;
                    wa.seg_stride = (uint32_t)nf;
                    wa.term_size = p.meta.term_size;
                    wa.findere = c.z;
                    wa.num_docs = (uint32_t)p.meta.doc_names.size();
                    HIP_TRY(launch_weights(wa, (uint32_t)n, st));
                }
            }
            HIP_TRY(w->ev.mark(3, st));
            if (cobs_gpu_status k = launch_scans(c, w, b, n, max_len, pool_cap, st); k != COBS_GPU_OK) return k;
            HIP_TRY(w->ev.mark(4, st));
            return COBS_GPU_OK;
        },
        [&](int attempt, uint64_t* filled) -> cobs_gpu_status {
            if (attempt == 0) HIP_TRY(w->land.flags_home(b, st));
            HIP_TRY(w->land.fill_home(w->hits.fill.p, st));
            if (attempt == 0) HIP_TRY(hipMemcpyAsync(w->h_total.p, w->total.p, n * nf * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            *filled = w->land.fill();
            if (attempt != 0) {
                (void)w->ev.add_elapsed(w->ms, 3, 4);
                return COBS_GPU_OK;
            }
            if (w->ev.add_elapsed(w->ms)) w->passes++;
            return invalid_base_from_flags(w->land.invalid_word(), n, c.bad_query, q0);
        }, &fill);
    if (s != COBS_GPU_OK) return s;
    if (c.total_weight) std::memcpy(c.total_weight + q0 * nf, w->h_total.p, n * nf * sizeof(uint64_t));
    return append_pass_records(*c.recs, w->hits.pool.p, fill, q0);
}

cobs_gpu_status search_weighted_impl(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                     double threshold, size_t num_results, cobs_gpu_hit* hits, size_t cap, size_t* hit_offsets,
                                     uint64_t* total_weight, size_t* bad_query) {
    if (!ix || !hit_offsets) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if ((nq && (!queries || !lens)) || (cap && !hits)) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if (nq >= 0xFFFFFFF0ull) return fail(COBS_GPU_ERR_ARG, "too many queries");
    if (ix->hbm_budget != 0 || any_streamed(ix)) return fail(COBS_GPU_ERR_UNSUPPORTED, "weighted: not on a handle with an HBM budget (its rows are not all resident)");
    if (ix->shard_count > 1) return fail(COBS_GPU_ERR_UNSUPPORTED, "weighted: not on one shard of several (the weights need every shard's counts)");
    for (size_t q = 0; q <= nq; ++q) hit_offsets[q] = 0;
    const size_t nf = ix->parts.size();
    const uint32_t z = ix->findere;
    uint32_t min_term = 0xFFFFFFFFu;
    for (const Part& p : ix->parts) min_term = std::min(min_term, p.meta.term_size);
    // everything the host can refuse is refused before anything is launched
    cobs_gpu_status refused = check_query_lengths(ix, queries, lens, nq, z, [&](size_t q) -> cobs_gpu_status {
        // 15 * n stays below 2^20, the counter planes of the scan
        if (nf && lens[q] - min_term + 1 - z > kWeightedMaxPositions)
            return fail(COBS_GPU_ERR_QUERY_TOO_LONG, "query too long: weighted search scores at most " +
                        std::to_string(kWeightedMaxPositions) + " positions (query " + std::to_string(q) + ")");
        return COBS_GPU_OK;
    }, bad_query);
    if (refused != COBS_GPU_OK) return refused;
    if (total_weight) std::fill(total_weight, total_weight + nq * nf, 0ull);
    if (nq == 0 || nf == 0) return COBS_GPU_OK;

    std::vector<HitDev> recs;
    const Call call{{ix, queries, lens, threshold, bad_query, z, real_documents(*ix), &recs}, total_weight};
    // passes: K1's tables, 5 bytes per position and file, and -- when every document comes back -- the pool's records stay
    // below the search call's workspace limit
    const uint64_t terms_per_char = table_bytes_per_char(ix);
    const uint64_t pool_bytes = threshold > 0.0 ? 0 : call.real_total * sizeof(HitDev);
    cobs_gpu_status s = cut_passes(nq, ix->tune.pass_bytes,
        [&](size_t q) {
            uint64_t qb = (uint64_t)(lens[q] + 16) * terms_per_char + pool_bytes;
            for (const Part& p : ix->parts) qb += 5ull * round_up(lens[q] - p.meta.term_size + 1 - z, 8);
            return qb;
        },
        [&](size_t q0, size_t q1) { return run_pass(call, q0, q1); });
    if (s != COBS_GPU_OK) return s;
    return hand_out_hits(recs, nq, num_results, hits, cap, hit_offsets);
}

}  // namespace
}  // namespace cobs_amd

using namespace cobs_amd;

extern "C" {

uint32_t cobs_gpu_idf_weight(uint64_t num_docs, uint64_t count) { return idf_weight(num_docs, count); }

cobs_gpu_status cobs_gpu_search_weighted(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                         double threshold, size_t num_results, cobs_gpu_hit* hits, size_t cap,
                                         size_t* hit_offsets, uint64_t* total_weight, size_t* bad_query) {
    return guarded([&]() {
        return search_weighted_impl(ix, queries, lens, nq, threshold, num_results, hits, cap, hit_offsets, total_weight, bad_query);
    });
}

cobs_gpu_status cobs_gpu_weighted_ms(cobs_gpu_index* ix, double out[5]) {
    WeightedWork* w = ix ? ix->weighted : nullptr;
    return take_ms(ix, out, 4, w ? w->ms : nullptr, w ? &w->passes : nullptr);
}

}  // extern "C"
