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
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};      // before K1 | after K1 | after the prevalence kernels
    double kernel_ms = 0, hash_ms = 0;
    uint64_t passes = 0;
    ~PrevalenceWork() {
        for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    }
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
    for (auto& e : w->ev) if (!e) HIP_TRY(hipEventCreate(&e));
    if (!ix->scratch[0]) {          // the workspace of the host-buffer calls (host_api.cpp): query upload and K1's tables
        cobs_gpu_status st = cobs_gpu_batch_create(ix, 0, 0, &ix->scratch[0]);
        if (st != COBS_GPU_OK) return st;
        HIP_TRY(hipStreamCreateWithFlags(&ix->scratch[0]->own_stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&ix->scratch[0]->done, hipEventDisableTiming));
    }
    cobs_gpu_batch* b = ix->scratch[0];
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
    HIP_TRY(launch_prevalence_zero(w->cells.p, ncells, st));
    HIP_TRY(hipEventRecord(w->ev[0], st));
    size_t max_len = 0;
    for (size_t q = q0; q < q1; ++q) max_len = std::max(max_len, c.lens[q]);
    for (size_t f = 0; f < nf; ++f) {
        const Part& p = ix->parts[f];
        if (p.num_tpages() == 0) continue;
        HashArgs ha;
        ha.text = b->d_text;
        ha.span_off = b->d_span_off;
        ha.q_len = b->d_qlen;
        ha.blk_off = b->work[f].blk_off;
        ha.pages = p.d_tpages;
        ha.table = b->work[f].table.p;
        ha.err_query = b->flags.p;
        ha.nq = (uint32_t)n;
        ha.npages = p.num_tpages();
        ha.term_size = p.meta.term_size;
        ha.canonicalize = p.meta.canonicalize;
        ha.num_hashes = (uint32_t)p.meta.num_hashes;
        ha.idx64 = p.idx64 ? 1u : 0u;
        ha.invalid_bases = ix->invalid_bases;     // (miss / skip: a position whose window holds an invalid character reads 0)
        ha.findere = c.z;
        ha.valid = nullptr;
        HIP_TRY(launch_hash(ha, round_up(b->span_off[n], 1024), st));
    }
    HIP_TRY(hipEventRecord(w->ev[1], st));
    for (size_t f = 0; f < nf; ++f) {
        const Part& p = ix->parts[f];
        PrevalenceArgs pa{};
        pa.table = b->work[f].table.p;
        pa.blk_off = b->work[f].blk_off;
        pa.q_len = b->d_qlen;
        pa.seg_off = w->seg_off.p + f;
        pa.out = w->cells.p;
        pa.seg_stride = (uint32_t)nf;
        pa.table_npages = p.num_tpages();
        pa.num_hashes = (uint32_t)p.meta.num_hashes;
        pa.term_size = p.meta.term_size;
        pa.findere = c.z;
        pa.num_docs = (uint32_t)p.meta.doc_names.size();
        pa.idx64 = p.idx64 ? 1u : 0u;
        const uint32_t max_positions = (uint32_t)(max_len - p.meta.term_size + 1 - c.z);
        for (const Chunk& ch : p.chunks) {
            if (!ch.d_data || ch.pages.empty()) continue;
            pa.data = ch.d_data;
            pa.pages = ch.d_pages;
            pa.pitch = ch.pitch;
            HIP_TRY(launch_prevalence(pa, ch.pages, (uint32_t)n, max_positions, st));
        }
    }
    HIP_TRY(hipEventRecord(w->ev[2], st));
    HIP_TRY(hipMemcpyAsync(w->h_flags.p, b->flags.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(c.counts + cell0, w->cells.p, ncells * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float hm = 0, km = 0;
    if (hipEventElapsedTime(&hm, w->ev[0], w->ev[1]) == hipSuccess && hipEventElapsedTime(&km, w->ev[1], w->ev[2]) == hipSuccess) {
        w->hash_ms += hm;
        w->kernel_ms += km;
        w->passes++;
    } else {
        (void)hipGetLastError();
    }
    if (w->h_flags.p[0] != 0u) {          // K1 keeps 2^32-1 - (first query with a non-ACGT character)
        const size_t bad = q0 + std::min<size_t>(0xFFFFFFFFu - w->h_flags.p[0], n - 1);
        if (c.bad_query) *c.bad_query = bad;
        return fail(COBS_GPU_ERR_INVALID_BASE, "Invalid DNA base pair in query string. Only ACGT are allowed. (query " +
                                               std::to_string(bad) + ")");
    }
    return COBS_GPU_OK;
}

cobs_gpu_status prevalence_impl(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq, uint32_t* counts,
                                size_t cap, size_t* offsets, size_t* needed, size_t* bad_query) {
    if (!ix || !offsets) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if (nq && (!queries || !lens)) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if (cap && !counts) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    offsets[0] = 0;
    if (needed) *needed = 0;
    bool streamed = ix->hbm_budget != 0;
    for (const Part& p : ix->parts) streamed = streamed || p.streamed;
    if (streamed) return fail(COBS_GPU_ERR_UNSUPPORTED, "prevalence: not on a handle with an HBM budget (its rows are not all resident)");
    const uint32_t z = ix->findere;
    const size_t nf = ix->parts.size();
    uint32_t max_term = 0;
    for (const Part& p : ix->parts) max_term = std::max(max_term, p.meta.term_size);
    // everything the host can refuse is refused before anything is launched
    size_t cells = 0;
    for (size_t q = 0; q < nq; ++q) {
        if (bad_query) *bad_query = q;
        if (!queries[q]) return fail(COBS_GPU_ERR_ARG, "NULL query (query " + std::to_string(q) + ")");
        if (lens[q] < (size_t)max_term + z)
            return fail(COBS_GPU_ERR_QUERY_TOO_SHORT, "query too short, needs to be at least " + std::to_string(max_term + z) +
                        " characters long" + (z ? " with findere z = " + std::to_string(z) : std::string()) +
                        " (query " + std::to_string(q) + ")");
        // (the kernel's position arithmetic is 32-bit with room for one launch's stride)
        if (lens[q] >= 0xFFFFFFF0ull - (1u << 20)) return fail(COBS_GPU_ERR_QUERY_TOO_LONG, "query too long (query " + std::to_string(q) + ")");
        for (size_t f = 0; f < nf; ++f) {
            cells += lens[q] - ix->parts[f].meta.term_size + 1 - z;
            offsets[q * nf + f + 1] = cells;
        }
    }
    if (bad_query) *bad_query = 0;
    if (needed) *needed = cells;
    if (cells > cap) return fail(COBS_GPU_ERR_CAPACITY, "count buffer too small; *needed holds the needed size");
    if (cells == 0) return COBS_GPU_OK;

    const Call call{ix, queries, lens, counts, offsets, bad_query, z};
    // passes: K1's tables (all files of the handle share the pass's queries) plus 4 bytes per position and file stay
    // below the search call's workspace limit
    const uint64_t kLimit = ix->tune.pass_bytes;
    uint64_t terms_per_char = 0;
    for (const Part& p : ix->parts) terms_per_char += 4ull * p.meta.num_hashes * std::max<uint32_t>(p.num_tpages(), 1) * (p.idx64 ? 2 : 1);
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
        out[0] = w->kernel_ms;
        out[1] = w->hash_ms;
        out[2] = (double)w->passes;
        w->kernel_ms = w->hash_ms = 0;
        w->passes = 0;
    }
    return COBS_GPU_OK;
}

}  // extern "C"
