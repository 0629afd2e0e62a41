// cobs_amd/csrc/positions.cpp -- cobs_gpu_hit_positions: WHERE in each query its hits matched.  A second call over the
// hit list a search returned (or over any (query, file, document) pairs): the queries that have hits are hashed again
// (K1, unchanged, once per file that has pairs) and the presence kernel reads, per pair, the one bit of every looked-up
// row.  Deliberately not fused into the scan: the final hit list of a query exists only after thresholds, limits and the
// per-file merge, and K1 costs about a hundredth of a scan.  Cut into passes by the workspace limit of the search call.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "engine.hpp"
#include "presence_kernels.hpp"

namespace cobs_amd {

struct PositionsWork {
    DevBuf<PresencePair> pairs;
    DevBuf<uint64_t> bits;
    PinnedBuf<uint32_t> h_flags;
    PhaseEvents<3> ev;          // before K1 | after K1 | after the presence kernels
    double ms[2] = {0, 0};      // hash | presence
    uint64_t passes = 0;
};

void destroy_positions_work(PositionsWork* w) { delete w; }

namespace {

// the column of document d of part p: the resident chunk and slice that hold it
bool resolve_column(const Part& p, uint64_t d, PresencePair* out) {
    const bool compact = p.meta.kind == IndexKind::Compact;
    const uint64_t page_docs = compact ? 8 * p.meta.header_page_size : ~0ull;
    const uint32_t fp = compact ? (uint32_t)(d / page_docs) : 0u;
    const uint64_t byte = (compact ? d - (uint64_t)fp * page_docs : d) / 8;
    for (const Chunk& ch : p.chunks)
        for (size_t v = 0; v < ch.vp.size(); ++v)
            if (ch.vp[v].fp == fp && byte >= ch.vp[v].col0 && byte < ch.vp[v].col0 + ch.vp[v].ncols && ch.d_data) {
                out->col = ch.d_data + ch.pages[v].base + (byte - ch.vp[v].col0);
                out->tpage = ch.pages[v].tpage;
                out->pitch = ch.pitch;
                out->bit = (uint32_t)(d & 7u);
                return true;
            }
    return false;
}

struct Call {
    cobs_gpu_index* ix;
    const char* const* queries;
    const size_t* lens;
    const cobs_gpu_hit* hits;
    const size_t* hit_offsets;
    uint64_t* bits;
    const size_t* bit_offsets;
    size_t* bad_query;
    uint32_t z;
};

// one device pass over the queries `qsel` (ascending; each has at least one hit)
cobs_gpu_status run_pass(const Call& c, const std::vector<size_t>& qsel) {
    cobs_gpu_index* ix = c.ix;
    HIP_TRY(hipSetDevice(ix->device));
    if (!ix->positions) ix->positions = new PositionsWork;
    PositionsWork* w = ix->positions;
    HIP_TRY(w->ev.create());
    cobs_gpu_batch* b = nullptr;
    if (cobs_gpu_status s = scratch_batch(ix, 0, &b); s != COBS_GPU_OK) return s;
    hipStream_t st = b->own_stream;
    const size_t n = qsel.size();
    std::vector<const char*> qp(n);
    std::vector<size_t> ql(n);
    for (size_t i = 0; i < n; ++i) { qp[i] = c.queries[qsel[i]]; ql[i] = c.lens[qsel[i]]; }
    size_t bad_local = 0;
    if (cobs_gpu_status s = set_queries_on(b, qp.data(), ql.data(), n, st, false, &bad_local); s != COBS_GPU_OK) {
        if (c.bad_query && bad_local < n) *c.bad_query = qsel[bad_local];
        return s;
    }
    // the pairs of the pass, bucketed by file; a pair's words start at bit_offsets[hit] - the pass's first word
    const size_t nf = ix->parts.size();
    const size_t h0 = c.hit_offsets[qsel.front()], h1 = c.hit_offsets[qsel.back() + 1];
    const size_t word0 = c.bit_offsets[h0], nwords = c.bit_offsets[h1] - word0;
    std::vector<size_t> first(nf + 1, 0);
    for (size_t i = 0; i < n; ++i)
        for (size_t h = c.hit_offsets[qsel[i]]; h < c.hit_offsets[qsel[i] + 1]; ++h) first[c.hits[h].file_no + 1]++;
    for (size_t f = 0; f < nf; ++f) first[f + 1] += first[f];
    std::vector<PresencePair> pairs(first[nf]);
    std::vector<size_t> fill(first.begin(), first.end() - 1);
    std::vector<uint32_t> max_words(nf, 0);
    for (size_t i = 0; i < n; ++i)
        for (size_t h = c.hit_offsets[qsel[i]]; h < c.hit_offsets[qsel[i] + 1]; ++h) {
            const cobs_gpu_hit& hit = c.hits[h];
            PresencePair pr{};
            if (!resolve_column(ix->parts[hit.file_no], hit.doc, &pr))
                return fail(COBS_GPU_ERR_UNSUPPORTED, "positions: document " + std::to_string(hit.doc) + " of file " +
                            std::to_string(hit.file_no) + " is not resident on this handle");
            pr.out = c.bit_offsets[h] - word0;
            pr.query = (uint32_t)i;
            pairs[fill[hit.file_no]++] = pr;
            max_words[hit.file_no] = std::max<uint32_t>(max_words[hit.file_no], (uint32_t)(c.bit_offsets[h + 1] - c.bit_offsets[h]));
        }
    HIP_TRY(w->pairs.reserve(pairs.size()));
    HIP_TRY(w->bits.reserve(nwords));
    HIP_TRY(w->h_flags.reserve(4));
    HIP_TRY(hipMemcpyAsync(w->pairs.p, pairs.data(), pairs.size() * sizeof(PresencePair), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_clear_flags(b->flags.p, st));
    HIP_TRY(w->ev.mark(0, st));
    // (K1 once per file that has pairs)
    if (cobs_gpu_status s = launch_hash_files(ix, b, n, c.z, st, [&](size_t f) { return first[f + 1] != first[f]; }); s != COBS_GPU_OK)
        return s;
    HIP_TRY(w->ev.mark(1, st));
    for (size_t f = 0; f < nf; ++f) {
        if (first[f + 1] == first[f]) continue;
        PresenceArgs pa;
        pa.t = table_ref_for(b, f, ix->parts[f], c.z);
        pa.pairs = w->pairs.p + first[f];
        pa.bits = w->bits.p;
        pa.npairs = (uint32_t)(first[f + 1] - first[f]);
        HIP_TRY(launch_presence(pa, max_words[f], st));
    }
    HIP_TRY(w->ev.mark(2, st));
    HIP_TRY(hipMemcpyAsync(w->h_flags.p, b->flags.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(c.bits + word0, w->bits.p, nwords * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (w->ev.add_elapsed(w->ms)) w->passes++;
    return invalid_base_from_flags(w->h_flags.p[0], n, c.bad_query, 0, qsel.data());
}

cobs_gpu_status hit_positions_impl(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                   const cobs_gpu_hit* hits, const size_t* hit_offsets, uint64_t* bits, size_t cap_words,
                                   size_t* bit_offsets, size_t* words_needed, size_t* bad_query) {
    if (!ix || !hit_offsets || !bit_offsets) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if (nq && (!queries || !lens)) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    bit_offsets[0] = 0;
    if (words_needed) *words_needed = 0;
    if (hit_offsets[0] != 0) return fail(COBS_GPU_ERR_ARG, "hit_offsets[0] is not 0");
    for (size_t q = 0; q < nq; ++q)
        if (hit_offsets[q + 1] < hit_offsets[q]) return fail(COBS_GPU_ERR_ARG, "hit_offsets are not ascending");
    const size_t n_hits = hit_offsets[nq];
    if ((n_hits && !hits) || (cap_words && !bits)) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if (ix->hbm_budget != 0 || any_streamed(ix)) return fail(COBS_GPU_ERR_UNSUPPORTED, "positions: not on a handle with an HBM budget (its rows are not all resident)");
    if (ix->shard_count > 1) return fail(COBS_GPU_ERR_UNSUPPORTED, "positions: not on one shard of several (its rows are not all resident)");
    const uint32_t z = ix->findere;
    // everything the host can refuse is refused before anything is launched (queries without hits are not looked at)
    size_t words = 0;
    cobs_gpu_status refused = check_query_lengths(ix, queries, lens, nq, z, [&](size_t q) -> cobs_gpu_status {
        if (lens[q] >= 0xFFFFFFF0ull) return fail(COBS_GPU_ERR_QUERY_TOO_LONG, "query too long (query " + std::to_string(q) + ")");
        for (size_t h = hit_offsets[q]; h < hit_offsets[q + 1]; ++h) {
            if (hits[h].file_no >= ix->parts.size())
                return fail(COBS_GPU_ERR_ARG, "hit " + std::to_string(h) + ": file number " + std::to_string(hits[h].file_no) + " out of range");
            const Part& p = ix->parts[hits[h].file_no];
            if (hits[h].doc >= p.meta.doc_names.size())
                return fail(COBS_GPU_ERR_ARG, "hit " + std::to_string(h) + ": document " + std::to_string(hits[h].doc) + " does not exist");
            const uint64_t npos = (uint64_t)lens[q] - p.meta.term_size + 1 - z;
            words += (size_t)((npos + 63) / 64);
            bit_offsets[h + 1] = words;
        }
        return COBS_GPU_OK;
    }, bad_query, [&](size_t q) { return hit_offsets[q + 1] == hit_offsets[q]; });
    if (refused != COBS_GPU_OK) return refused;
    if (words_needed) *words_needed = words;
    if (words > cap_words) return fail(COBS_GPU_ERR_CAPACITY, "bit buffer too small; *words_needed holds the needed size");
    if (n_hits == 0) return COBS_GPU_OK;

    const Call call{ix, queries, lens, hits, hit_offsets, bits, bit_offsets, bad_query, z};
    // passes: K1's tables (all files of the handle share the pass's queries) and the pairs + words of the pass stay
    // below the search call's workspace limit each
    const uint64_t kLimit = ix->tune.pass_bytes;
    const uint64_t terms_per_char = table_bytes_per_char(ix);
    std::vector<size_t> qsel;
    uint64_t table_bytes = 0, out_bytes = 0;
    for (size_t q = 0; q < nq; ++q) {
        const size_t nh = hit_offsets[q + 1] - hit_offsets[q];
        if (nh == 0) continue;
        const uint64_t tb = (uint64_t)(lens[q] + 16) * terms_per_char;
        const uint64_t ob = (uint64_t)nh * sizeof(PresencePair) + 8ull * (bit_offsets[hit_offsets[q + 1]] - bit_offsets[hit_offsets[q]]);
        if (!qsel.empty() && (table_bytes + tb > kLimit || out_bytes + ob > kLimit || qsel.size() >= 0xFFFFFFF0ull)) {
            if (cobs_gpu_status s = run_pass(call, qsel); s != COBS_GPU_OK) return s;
            qsel.clear();
            table_bytes = out_bytes = 0;
        }
        qsel.push_back(q);
        table_bytes += tb;
        out_bytes += ob;
    }
    return run_pass(call, qsel);
}

}  // namespace
}  // namespace cobs_amd

using namespace cobs_amd;

extern "C" {

cobs_gpu_status cobs_gpu_hit_positions(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                       const cobs_gpu_hit* hits, const size_t* hit_offsets, uint64_t* bits, size_t cap_words,
                                       size_t* bit_offsets, size_t* words_needed, size_t* bad_query) {
    return guarded([&]() {
        return hit_positions_impl(ix, queries, lens, nq, hits, hit_offsets, bits, cap_words, bit_offsets, words_needed, bad_query);
    });
}

cobs_gpu_status cobs_gpu_positions_ms(cobs_gpu_index* ix, double out[3]) {
    if (!ix || !out) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    out[0] = out[1] = out[2] = 0;
    if (PositionsWork* w = ix->positions) {
        out[0] = w->ms[1];
        out[1] = w->ms[0];
        out[2] = (double)w->passes;
        w->ms[0] = w->ms[1] = 0;
        w->passes = 0;
    }
    return COBS_GPU_OK;
}

}  // extern "C"
