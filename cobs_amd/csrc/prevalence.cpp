// cobs_amd/csrc/prevalence.cpp -- cobs_gpu_prevalence: for every position of a query, HOW MANY documents hold it.  The
// queries are hashed by K1 (unchanged: findere and the invalid-bases policy live in its table) and the prevalence kernel
// (prevalence_kernels.hip) gathers the looked-up rows of every resident chunk once, as K2 does, but reduces across the
// documents.  The counts are additive over column slices, so one shard of several answers for the documents it holds.
// Cut into passes by the workspace limit of the search call.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "engine.hpp"
#include "prevalence_kernels.hpp"

namespace cobs_amd {

struct PrevalenceWork {
    DevBuf<uint32_t> cells;
    DevBuf<uint64_t> seg_off;
    PinnedBuf<uint64_t> h_seg_off;
    PinnedBuf<uint32_t> h_flags;
    PhaseEvents<3> ev;          // before K1 | after K1 | after the prevalence kernels
    double ms[2] = {0, 0};      // hash | prevalence
    uint64_t passes = 0;
};

void destroy_prevalence_work(PrevalenceWork* w) { delete w; }

namespace {

struct Call {
    cobs_gpu_index* ix;
    const char* const* queries;
    const size_t* lens;
    uint32_t* counts;
    const size_t* offsets;
    size_t* bad_query;
    uint32_t z;
};

// one device pass over the queries [q0, q1)
cobs_gpu_status run_pass(const Call& c, size_t q0, size_t q1) {
    cobs_gpu_index* ix = c.ix;
    HIP_TRY(hipSetDevice(ix->device));
    if (!ix->prevalence) ix->prevalence = new PrevalenceWork;
    PrevalenceWork* w = ix->prevalence;
    HIP_TRY(w->ev.create());
    cobs_gpu_batch* b = nullptr;
    if (cobs_gpu_status s = scratch_batch(ix, 0, &b); s != COBS_GPU_OK) return s;
    hipStream_t st = b->own_stream;
    const size_t n = q1 - q0, nf = ix->parts.size();
    size_t bad_local = 0;
    if (cobs_gpu_status s = set_queries_on(b, c.queries + q0, c.lens + q0, n, st, false, &bad_local, q0); s != COBS_GPU_OK) {
        if (c.bad_query && bad_local < n) *c.bad_query = q0 + bad_local;
        return s;
    }
    // the cells of the pass: the caller's segments of its queries, back to back
    const size_t cell0 = c.offsets[q0 * nf], ncells = c.offsets[q1 * nf] - cell0;
    HIP_TRY(w->cells.reserve(ncells));
    HIP_TRY(w->seg_off.reserve(n * nf + 1));
    HIP_TRY(w->h_seg_off.reserve(n * nf + 1));
    HIP_TRY(w->h_flags.reserve(4));
    for (size_t i = 0; i <= n * nf; ++i) w->h_seg_off.p[i] = c.offsets[q0 * nf + i] - cell0;
    HIP_TRY(hipMemcpyAsync(w->seg_off.p, w->h_seg_off.p, (n * nf + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_clear_flags(b->flags.p, st));
    size_t max_len = 0;
    for (size_t q = q0; q < q1; ++q) max_len = std::max(max_len, c.lens[q]);
    if (cobs_gpu_status s = launch_prevalence_cells(ix, b, w->seg_off.p, w->cells.p, ncells, n, max_len, c.z, st, w->ev.ev[0], w->ev.ev[1]);
        s != COBS_GPU_OK)
        return s;
    HIP_TRY(w->ev.mark(2, st));
    HIP_TRY(hipMemcpyAsync(w->h_flags.p, b->flags.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(c.counts + cell0, w->cells.p, ncells * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (w->ev.add_elapsed(w->ms)) w->passes++;
    return invalid_base_from_flags(w->h_flags.p[0], n, c.bad_query, q0);
}

cobs_gpu_status prevalence_impl(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq, uint32_t* counts,
                                size_t cap, size_t* offsets, size_t* needed, size_t* bad_query) {
    if (!ix || !offsets) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if (nq && (!queries || !lens)) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if (cap && !counts) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    offsets[0] = 0;
    if (needed) *needed = 0;
    if (ix->hbm_budget != 0 || any_streamed(ix)) return fail(COBS_GPU_ERR_UNSUPPORTED, "prevalence: not on a handle with an HBM budget (its rows are not all resident)");
    const uint32_t z = ix->findere;
    const size_t nf = ix->parts.size();
    // everything the host can refuse is refused before anything is launched
    size_t cells = 0;
    cobs_gpu_status refused = check_query_lengths(ix, queries, lens, nq, z, [&](size_t q) -> cobs_gpu_status {
        // (the kernel's position arithmetic is 32-bit with room for one launch's stride)
        if (lens[q] >= 0xFFFFFFF0ull - (1u << 20)) return fail(COBS_GPU_ERR_QUERY_TOO_LONG, "query too long (query " + std::to_string(q) + ")");
        for (size_t f = 0; f < nf; ++f) {
            cells += lens[q] - ix->parts[f].meta.term_size + 1 - z;
            offsets[q * nf + f + 1] = cells;
        }
        return COBS_GPU_OK;
    }, bad_query);
    if (refused != COBS_GPU_OK) return refused;
    if (needed) *needed = cells;
    if (cells > cap) return fail(COBS_GPU_ERR_CAPACITY, "count buffer too small; *needed holds the needed size");
    if (cells == 0) return COBS_GPU_OK;

    const Call call{ix, queries, lens, counts, offsets, bad_query, z};
    // passes: K1's tables (all files of the handle share the pass's queries) plus 4 bytes per position and file stay
    // below the search call's workspace limit
    const uint64_t kLimit = ix->tune.pass_bytes;
    const uint64_t terms_per_char = table_bytes_per_char(ix);
    size_t first = 0;
    uint64_t bytes = 0;
    for (size_t q = 0; q < nq; ++q) {
        const uint64_t qb = (uint64_t)(lens[q] + 16) * terms_per_char + 4ull * (offsets[(q + 1) * nf] - offsets[q * nf]);
        if (q > first && (bytes + qb > kLimit || q - first >= 0x7FFFFFF0ull)) {
            if (cobs_gpu_status s = run_pass(call, first, q); s != COBS_GPU_OK) return s;
            first = q;
            bytes = 0;
        }
        bytes += qb;
    }
    return run_pass(call, first, nq);
}

}  // namespace
}  // namespace cobs_amd

using namespace cobs_amd;

extern "C" {

cobs_gpu_status cobs_gpu_prevalence(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                    uint32_t* counts, size_t cap, size_t* offsets, size_t* needed, size_t* bad_query) {
    return guarded([&]() { return prevalence_impl(ix, queries, lens, nq, counts, cap, offsets, needed, bad_query); });
}

cobs_gpu_status cobs_gpu_prevalence_ms(cobs_gpu_index* ix, double out[3]) {
    if (!ix || !out) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    out[0] = out[1] = out[2] = 0;
    if (PrevalenceWork* w = ix->prevalence) {
        out[0] = w->ms[1];
        out[1] = w->ms[0];
        out[2] = (double)w->passes;
        w->ms[0] = w->ms[1] = 0;
        w->passes = 0;
    }
    return COBS_GPU_OK;
}

}  // extern "C"
