// cobs_amd/csrc/hash_pass.cpp -- what every call that runs K1 on its own shares (declared in engine.hpp): the scratch
// batch of the host-buffer calls, the HashArgs of a file and K1's launch per file, the TableRef a reader of K1's table
// gets (row_table.hpp), the decode of K1's "invalid base" flag word with the reference's message, the length refusals
// with the reference's wording, the table bytes the passes are cut by, the prevalence cells both cobs_gpu_prevalence
// and cobs_gpu_search_weighted fill, and the bodies of pooled_pass.hpp that are no templates.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <string>

#include "engine.hpp"
#include "pooled_pass.hpp"
#include "prevalence_kernels.hpp"

namespace cobs_amd {

cobs_gpu_status scratch_batch(cobs_gpu_index* ix, int slot, cobs_gpu_batch** b) {
    if (!ix->scratch[slot]) {          // the workspace of the host-buffer calls: query upload and K1's tables
        cobs_gpu_status st = cobs_gpu_batch_create(ix, 0, 0, &ix->scratch[slot]);
        if (st != COBS_GPU_OK) return st;
        HIP_TRY(hipStreamCreateWithFlags(&ix->scratch[slot]->own_stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&ix->scratch[slot]->done, hipEventDisableTiming));
    }
    if (b) *b = ix->scratch[slot];
    return COBS_GPU_OK;
}

HashArgs hash_args_for(const cobs_gpu_batch* b, size_t f, const Part& p, size_t nq, uint32_t z, uint32_t invalid_bases,
                       uint32_t* valid) {
    HashArgs ha;
    ha.text = b->d_text;
    ha.span_off = b->d_span_off;
    ha.q_len = b->d_qlen;
    ha.blk_off = b->work[f].blk_off;
    ha.pages = p.d_tpages;
    ha.table = b->work[f].table.p;
    ha.err_query = b->flags.p;
    ha.nq = (uint32_t)nq;
    ha.npages = p.num_tpages();
    ha.term_size = p.meta.term_size;
    ha.canonicalize = p.meta.canonicalize;
    ha.num_hashes = (uint32_t)p.meta.num_hashes;
    ha.idx64 = p.idx64 ? 1u : 0u;
    ha.invalid_bases = invalid_bases;     // (miss / skip: a position whose window holds an invalid character reads 0)
    ha.findere = z;
    ha.valid = valid;
    return ha;
}

cobs_gpu_status launch_hash_file(const cobs_gpu_batch* b, const HashArgs& ha, size_t nq, hipStream_t stream) {
    // (the kernel bounds itself by span_off[nq] on the device; the grid is rounded up so that a
    // captured launch serves every batch of its shape class)
    HIP_TRY(launch_hash(ha, round_up(b->span_off[nq], 1024), stream));
    return COBS_GPU_OK;
}

cobs_gpu_status launch_hash_files(cobs_gpu_index* ix, const cobs_gpu_batch* b, size_t nq, uint32_t z, hipStream_t stream,
                                  const std::function<bool(size_t)>& file_filter) {
    for (size_t f = 0; f < ix->parts.size(); ++f) {
        if (!file_filter(f)) continue;
        const HashArgs args = hash_args_for(b, f, ix->parts[f], nq, z, ix->invalid_bases, nullptr);
        if (cobs_gpu_status s = launch_hash_file(b, args, nq, stream); s != COBS_GPU_OK) return s;
    }
    return COBS_GPU_OK;
}

TableRef table_ref_for(const cobs_gpu_batch* b, size_t f, const Part& p, uint32_t z) {
    TableRef t;
    t.table = b->work[f].table.p;
    t.blk_off = b->work[f].blk_off;
    t.q_len = b->d_qlen;
    t.table_npages = p.num_tpages();
    t.num_hashes = (uint32_t)p.meta.num_hashes;
    t.term_size = p.meta.term_size;
    t.findere = z;
    t.idx64 = p.idx64 ? 1u : 0u;
    return t;
}

std::string invalid_base_message(size_t query) {
    return "Invalid DNA base pair in query string. Only ACGT are allowed. (query " + std::to_string(query) + ")";
}

cobs_gpu_status invalid_base_from_flags(uint32_t flag_word, size_t n, size_t* bad_query, size_t base, const size_t* map) {
    if (flag_word == 0u) return COBS_GPU_OK;
    // K1 keeps 2^32-1 - (first query of the pass with a non-ACGT character)
    const size_t local = std::min<size_t>(0xFFFFFFFFu - flag_word, n ? n - 1 : 0);
    const size_t bad = map ? map[local] : base + local;
    if (bad_query) *bad_query = bad;
    return fail(COBS_GPU_ERR_INVALID_BASE, invalid_base_message(bad));
}

cobs_gpu_status query_too_short(uint64_t need, uint32_t z, size_t query) {
    return fail(COBS_GPU_ERR_QUERY_TOO_SHORT, "query too short, needs to be at least " + std::to_string(need) + " characters long" +
                (z ? " with findere z = " + std::to_string(z) : std::string()) + " (query " + std::to_string(query) + ")");
}

cobs_gpu_status check_query_lengths(const cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq, uint32_t z,
                                    const std::function<cobs_gpu_status(size_t)>& rule, size_t* bad_query,
                                    const std::function<bool(size_t)>& skip) {
    uint32_t max_term = 0;
    for (const Part& p : ix->parts) max_term = std::max(max_term, p.meta.term_size);
    for (size_t q = 0; q < nq; ++q) {
        if (skip && skip(q)) continue;
        if (bad_query) *bad_query = q;
        if (!queries[q]) return fail(COBS_GPU_ERR_ARG, "NULL query (query " + std::to_string(q) + ")");
        if (lens[q] < (size_t)max_term + z) return query_too_short((uint64_t)max_term + z, z, q);
        if (cobs_gpu_status s = rule(q); s != COBS_GPU_OK) return s;
    }
    if (bad_query) *bad_query = 0;
    return COBS_GPU_OK;
}

uint64_t table_bytes_per_char(const cobs_gpu_index* ix) {
    uint64_t terms_per_char = 0;          // 4 bytes per (hash, held sub-index) of every file, 8 in a wide table
    for (const Part& p : ix->parts) terms_per_char += 4ull * p.meta.num_hashes * std::max<uint32_t>(p.num_tpages(), 1) * (p.idx64 ? 2 : 1);
    return terms_per_char;
}

bool any_streamed(const cobs_gpu_index* ix) {
    for (const Part& p : ix->parts)
        if (p.streamed) return true;
    return false;
}

cobs_gpu_status launch_prevalence_cells(cobs_gpu_index* ix, const cobs_gpu_batch* b, const uint64_t* seg_off, uint32_t* cells,
                                        uint64_t ncells, size_t n, size_t max_len, uint32_t z, hipStream_t stream,
                                        hipEvent_t started, hipEvent_t hashed) {
    const size_t nf = ix->parts.size();
    HIP_TRY(launch_prevalence_zero(cells, ncells, stream));
    HIP_TRY(hipEventRecord(started, stream));
    if (cobs_gpu_status s = launch_hash_held(ix, b, n, z, stream); s != COBS_GPU_OK) return s;
    HIP_TRY(hipEventRecord(hashed, stream));
    for (size_t f = 0; f < nf; ++f) {
        const Part& p = ix->parts[f];
        PrevalenceArgs pa{};
        pa.t = table_ref_for(b, f, p, z);
        pa.seg_off = seg_off + f;
        pa.out = cells;
        pa.seg_stride = (uint32_t)nf;
        pa.num_docs = (uint32_t)p.meta.doc_names.size();
        const uint32_t max_positions = (uint32_t)(max_len - p.meta.term_size + 1 - z);
        cobs_gpu_status s = for_each_resident_chunk(p, [&](const Chunk& ch) -> cobs_gpu_status {
            pa.data = ch.d_data;
            pa.pages = ch.d_pages;
            pa.pitch = ch.pitch;
            HIP_TRY(launch_prevalence(pa, ch.pages, (uint32_t)n, max_positions, stream));
            return COBS_GPU_OK;
        });
        if (s != COBS_GPU_OK) return s;
    }
    return COBS_GPU_OK;
}

// ---- pooled_pass.hpp

cobs_gpu_status launch_hash_held(cobs_gpu_index* ix, const cobs_gpu_batch* b, size_t n, uint32_t z, hipStream_t st) {
    return launch_hash_files(ix, b, n, z, st, [&](size_t f) { return ix->parts[f].num_tpages() != 0; });
}

cobs_gpu_status pass_queries(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t q0, size_t q1,
                             size_t* bad_query, cobs_gpu_batch** b) {
    if (cobs_gpu_status s = scratch_batch(ix, 0, b); s != COBS_GPU_OK) return s;
    const size_t n = q1 - q0;
    size_t bad_local = 0;
    cobs_gpu_status s = set_queries_on(*b, queries + q0, lens + q0, n, (*b)->own_stream, false, &bad_local, q0);
    if (s != COBS_GPU_OK && bad_query && bad_local < n) *bad_query = q0 + bad_local;
    return s;
}

cobs_gpu_status scan_pool_no_room(uint64_t cap) {
    return fail(COBS_GPU_ERR_HIP, "out of device memory for " + std::to_string(cap) + " hit records; raise the threshold or use fewer queries per call");
}

cobs_gpu_status hand_out_hits(std::vector<HitDev>& recs, size_t nq, size_t num_results, cobs_gpu_hit* hits, size_t cap, size_t* hit_offsets) {
    return hand_out_lists(recs, nq, [](const HitDev& r) { return r.query; },
        [](const HitDev& a, const HitDev& b) {
            if (a.score != b.score) return a.score > b.score;
            if (a.part != b.part) return a.part < b.part;
            return a.doc < b.doc;
        }, num_results, hits, cap, hit_offsets, "nq", [](const HitDev& r) { return cobs_gpu_hit{r.part, r.doc, r.score}; });
}

cobs_gpu_status take_ms(const cobs_gpu_index* ix, double* out, int n, double* ms, uint64_t* passes) {
    if (!ix || !out) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    for (int i = 0; i <= n; ++i) out[i] = 0;
    if (!ms) return COBS_GPU_OK;
    for (int i = 0; i < n; ++i) {
        out[i] = ms[i];
        ms[i] = 0;
    }
    out[n] = (double)*passes;
    *passes = 0;
    return COBS_GPU_OK;
}

ScanWork::ScanWork(const char* pool_name) : hits(pool_name, launch_prevalence_zero) {}

}  // namespace cobs_amd
