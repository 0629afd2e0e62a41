// cobs_amd/csrc/sets.cpp -- document sets: cobs_gpu_set_doc_sets labels the documents of a file with set numbers, and
// cobs_gpu_search_sets scores every query against every non-empty set: `any` = the positions at least one member holds,
// `all` = the positions every member holds.  The labels become segment records per 16-byte column chunk of every resident
// slice -- built on the host when the labels are set, uploaded once, kept on the handle per file.  Per device pass (cut by
// the workspace limit, on the handle's scratch batch): K1 hashes the queries (unchanged: findere and the invalid-bases
// policy live in its table), the presence kernel ORs the two bit matrices [query][set][ceil(n / 32)] together, the select
// kernel counts their bits and appends the sets that reach the threshold to a pool (set_kernels.hip).  The host orders
// every query's records and cuts them to num_results (pooled_call.hpp: cut_passes, hand_out_lists).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "engine.hpp"
#include "prevalence_kernels.hpp"      // launch_prevalence_zero
#include "set_kernels.hpp"
#include "sets.hpp"                    // ChunkSegs, FileSets, SetsWork

namespace cobs_amd {

void destroy_sets_work(SetsWork* w) { delete w; }

namespace {

bool sets_supported(const cobs_gpu_index* ix) { return ix->hbm_budget == 0 && !any_streamed(ix) && ix->shard_count <= 1; }

// the distinct sets among the 128 slots of every 16-byte column chunk of every page of the chunk, as (set, mask) records:
// only slots of labelled real documents enter a mask
cobs_gpu_status build_segments(const Part& p, const Chunk& ch, const FileSets& fs, const std::vector<uint32_t>& local_of,
                               ChunkSegs& out) {
    const uint64_t docs = p.meta.doc_names.size();
    std::vector<uint32_t> first(ch.pages.size() * (size_t)ch.cpp + 1, 0), set;
    std::vector<uint4> mask;
    std::vector<std::pair<uint32_t, uint32_t>> slots;      // (set, slot of the column chunk)
    for (size_t pg = 0; pg < ch.pages.size(); ++pg) {
        const PageDev& pd = ch.pages[pg];
        const uint64_t live = docs > pd.doc0 ? std::min<uint64_t>(docs - pd.doc0, (uint64_t)pd.valid_bytes * 8) : 0;
        for (uint32_t c = 0; c < ch.cpp; ++c) {
            slots.clear();
            for (uint64_t s = (uint64_t)c * 128; s < std::min<uint64_t>(live, (uint64_t)c * 128 + 128); ++s) {
                const uint32_t l = fs.labels[pd.doc0 + s];
                if (l != COBS_GPU_NO_SET) slots.emplace_back(local_of[l], (uint32_t)(s - (uint64_t)c * 128));
            }
            std::sort(slots.begin(), slots.end());
            for (size_t i = 0; i < slots.size(); ++i) {
                if (i == 0 || slots[i].first != slots[i - 1].first) {
                    set.push_back(slots[i].first);
                    mask.push_back(uint4{0u, 0u, 0u, 0u});
                }
                uint32_t* m = &mask.back().x;
                m[slots[i].second >> 5] |= 1u << (slots[i].second & 31u);
            }
            if (set.size() >= 0xFFFFFFF0ull) return fail(COBS_GPU_ERR_ARG, "too many segment records");
            first[pg * ch.cpp + c + 1] = (uint32_t)set.size();
        }
    }
    HIP_TRY(out.first.reserve(first.size()));
    HIP_TRY(out.mask.reserve(mask.size()));
    HIP_TRY(out.set.reserve(set.size()));
    HIP_TRY(hipMemcpy(out.first.p, first.data(), first.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!set.empty()) {
        HIP_TRY(hipMemcpy(out.mask.p, mask.data(), mask.size() * sizeof(uint4), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(out.set.p, set.data(), set.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    out.built = true;
    return COBS_GPU_OK;
}

cobs_gpu_status set_doc_sets_impl(cobs_gpu_index* ix, size_t file_no, const uint32_t* labels, size_t n_docs, uint32_t n_sets) {
    if (!ix) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if (file_no >= ix->parts.size()) return fail(COBS_GPU_ERR_ARG, "file_no out of range");
    if (!labels) {                          // the file's labels are cleared
        if (ix->sets && file_no < ix->sets->files.size()) {
            ix->sets->files[file_no] = FileSets{};
        }
        return COBS_GPU_OK;
    }
    const Part& p = ix->parts[file_no];
    if (n_docs != p.meta.doc_names.size())
        return fail(COBS_GPU_ERR_ARG, "n_docs is not the file's document count (" + std::to_string(p.meta.doc_names.size()) + ")");
    if (n_sets > (1u << 28)) return fail(COBS_GPU_ERR_ARG, "n_sets: at most 2^28 sets per file");
    for (size_t d = 0; d < n_docs; ++d)
        if (labels[d] != COBS_GPU_NO_SET && labels[d] >= n_sets)
            return fail(COBS_GPU_ERR_ARG, "label " + std::to_string(labels[d]) + " of document " + std::to_string(d) + " is not below n_sets");
    FileSets fs;
    fs.labels.assign(labels, labels + n_docs);
    fs.n_sets = n_sets;
    fs.members.assign(n_sets, 0);
    for (size_t d = 0; d < n_docs; ++d)
        if (labels[d] != COBS_GPU_NO_SET) fs.members[labels[d]]++;
    std::vector<uint32_t> local_of(n_sets, COBS_GPU_NO_SET);
    for (uint32_t c = 0; c < n_sets; ++c)
        if (fs.members[c]) {
            local_of[c] = (uint32_t)fs.sets.size();
            fs.sets.push_back(c);
        }
    fs.chunks = std::vector<ChunkSegs>(p.chunks.size());
    // (a handle cobs_gpu_search_sets refuses keeps the labels and builds nothing)
    if (sets_supported(ix)) {
        HIP_TRY(hipSetDevice(ix->device));
        for (size_t c = 0; c < p.chunks.size(); ++c) {
            const Chunk& ch = p.chunks[c];
            if (!ch.d_data || ch.pages.empty()) continue;
            if (cobs_gpu_status s = build_segments(p, ch, fs, local_of, fs.chunks[c]); s != COBS_GPU_OK) return s;
        }
    }
    if (!ix->sets) ix->sets = new SetsWork;
    if (ix->sets->files.size() < ix->parts.size()) ix->sets->files.resize(ix->parts.size());
    ix->sets->files[file_no] = std::move(fs);
    return COBS_GPU_OK;
}

struct Call {
    cobs_gpu_index* ix;
    SetsWork* w;
    const char* const* queries;
    const size_t* lens;
    double threshold;
    uint32_t rank_by;
    size_t* bad_query;
    uint32_t z;
    const std::vector<SetItem>* items;
    std::vector<SetRec>* recs;              // the records of all passes, `query` = the call's query number
};

// words of ONE of the two bit matrices of query q: per labelled file, non-empty sets x ceil(n / 32)
uint64_t bitmap_words(const Call& c, size_t q) {
    uint64_t words = 0;
    for (size_t f = 0; f < c.ix->parts.size(); ++f)
        words += (uint64_t)c.w->files[f].sets.size() * ((c.lens[q] - c.ix->parts[f].meta.term_size + 1 - c.z + 31) / 32);
    return words;
}

// one device pass over the queries [q0, q1)
cobs_gpu_status run_pass(const Call& c, size_t q0, size_t q1) {
    cobs_gpu_index* ix = c.ix;
    SetsWork* w = c.w;
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(w->ev.create());
    cobs_gpu_batch* b = nullptr;
    if (cobs_gpu_status s = pass_queries(ix, c.queries, c.lens, q0, q1, c.bad_query, &b); s != COBS_GPU_OK) return s;
    hipStream_t st = b->own_stream;
    const size_t n = q1 - q0, nf = ix->parts.size(), nitems = c.items->size();
    // the bitmaps of the pass: per (query, file) its sets' words back to back; `miss` lies `words` behind `any`
    HIP_TRY(w->bm_off.reserve(n * nf + 1));
    HIP_TRY(w->h_bm_off.reserve(n * nf + 1));
    uint64_t words = 0;
    size_t max_len = 0;
    for (size_t q = q0; q < q1; ++q) {
        max_len = std::max(max_len, c.lens[q]);
        for (size_t f = 0; f < nf; ++f) {
            w->h_bm_off.p[(q - q0) * nf + f] = words;
            words += (uint64_t)w->files[f].sets.size() * ((c.lens[q] - ix->parts[f].meta.term_size + 1 - c.z + 31) / 32);
        }
    }
    w->h_bm_off.p[n * nf] = words;
    const uint64_t pool_cap = std::max<uint64_t>((uint64_t)n * nitems, 1);
    if (w->bits.reserve((size_t)(2 * words)) != hipSuccess || w->pool.reserve((size_t)pool_cap) != hipSuccess) {
        (void)hipGetLastError();
        return fail(COBS_GPU_ERR_HIP, "sets: out of device memory for the bitmaps and records of " + std::to_string(n) +
                    " queries; lower pass_bytes or use fewer queries per call");
    }
    HIP_TRY(w->fill.reserve(1));
    HIP_TRY(w->land.reserve());
    const bool count_valid = ix->invalid_bases == COBS_GPU_INVALID_SKIP;

    HIP_TRY(hipMemcpyAsync(w->bm_off.p, w->h_bm_off.p, (n * nf + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_clear_flags(b->flags.p, st, count_valid ? b->valid.p : nullptr, count_valid ? (uint32_t)(n * nf) : 0u));
    // (by a kernel, not a memset node)
    HIP_TRY(launch_prevalence_zero(w->bits.p, 2 * words, st));
    HIP_TRY(launch_prevalence_zero(reinterpret_cast<uint32_t*>(w->fill.p), 2, st));
    HIP_TRY(w->ev.mark(0, st));
    for (size_t f = 0; f < nf; ++f) {
        const Part& p = ix->parts[f];
        if (p.num_tpages() == 0) continue;
        const HashArgs ha = hash_args_for(b, f, p, n, c.z, ix->invalid_bases, count_valid ? b->valid.p + f * n : nullptr);
        if (cobs_gpu_status s = launch_hash_file(b, ha, n, st); s != COBS_GPU_OK) return s;
    }
    HIP_TRY(w->ev.mark(1, st));
    for (size_t f = 0; f < nf; ++f) {
        const Part& p = ix->parts[f];
        FileSets& fs = w->files[f];
        if (fs.sets.empty()) continue;
        SetPresenceArgs pa{};
        pa.t = table_ref_for(b, f, p, c.z);
        pa.bm_off = w->bm_off.p + f;
        pa.any = w->bits.p;
        pa.miss = w->bits.p + words;
        pa.bm_stride = (uint32_t)nf;
        pa.num_docs = (uint32_t)p.meta.doc_names.size();
        const uint32_t max_positions = (uint32_t)(max_len - p.meta.term_size + 1 - c.z);
        for (size_t ci = 0; ci < p.chunks.size(); ++ci) {
            const Chunk& ch = p.chunks[ci];
            if (!ch.d_data || ch.pages.empty()) continue;
            if (!fs.chunks[ci].built) return fail(COBS_GPU_ERR_ARG, "sets: the segments of a resident chunk are missing");
            pa.data = ch.d_data;
            pa.pages = ch.d_pages;
            pa.pitch = ch.pitch;
            pa.cpp = ch.cpp;
            pa.seg_first = fs.chunks[ci].first.p;
            pa.seg_mask = fs.chunks[ci].mask.p;
            pa.seg_set = fs.chunks[ci].set.p;
            HIP_TRY(launch_set_presence(pa, ch.pages, (uint32_t)n, max_positions, st));
        }
    }
    HIP_TRY(w->ev.mark(2, st));
    SetSelectArgs sa{};
    sa.any = w->bits.p;
    sa.miss = w->bits.p + words;
    sa.bm_off = w->bm_off.p;
    sa.items = w->items.p;
    sa.q_len = b->d_qlen;
    sa.valid = b->valid.p;
    sa.pool = w->pool.p;
    sa.fill = w->fill.p;
    sa.cap = pool_cap;
    sa.threshold = c.threshold;
    sa.nq = (uint32_t)n;
    sa.nitems = (uint32_t)nitems;
    sa.nfiles = (uint32_t)nf;
    sa.findere = c.z;
    sa.rank_by = c.rank_by;
    HIP_TRY(launch_set_select(sa, st));
    HIP_TRY(w->ev.mark(3, st));
    HIP_TRY(w->land.flags_home(b, st));
    HIP_TRY(w->land.fill_home(w->fill.p, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (w->ev.add_elapsed(w->ms)) w->passes++;
    if (cobs_gpu_status s = invalid_base_from_flags(w->land.invalid_word(), n, c.bad_query, q0); s != COBS_GPU_OK) return s;
    const uint64_t fill = w->land.fill();
    if (fill > pool_cap) return fail(COBS_GPU_ERR_HIP, "sets: the record pool overflowed");      // (it holds every item)
    return append_pass_records(*c.recs, w->pool.p, fill, q0);
}

cobs_gpu_status search_sets_impl(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq, double threshold,
                                 uint32_t rank_by, size_t num_results, cobs_gpu_set_hit* hits, size_t cap, size_t* hit_offsets,
                                 size_t* bad_query) {
    if (!ix || !hit_offsets) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if ((nq && (!queries || !lens)) || (cap && !hits)) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if (rank_by > COBS_GPU_SETS_BY_ALL) return fail(COBS_GPU_ERR_ARG, "rank_by: COBS_GPU_SETS_BY_ANY or COBS_GPU_SETS_BY_ALL");
    if (nq >= 0xFFFFFFF0ull) return fail(COBS_GPU_ERR_ARG, "too many queries");
    if (ix->hbm_budget != 0 || any_streamed(ix)) return fail(COBS_GPU_ERR_UNSUPPORTED, "sets: not on a handle with an HBM budget (its rows are not all resident)");
    if (ix->shard_count > 1) return fail(COBS_GPU_ERR_UNSUPPORTED, "sets: not on one shard of several (any and all are not additive over shards)");
    for (size_t q = 0; q <= nq; ++q) hit_offsets[q] = 0;
    const size_t nf = ix->parts.size();
    const uint32_t z = ix->findere;
    // everything the host can refuse is refused before anything is launched
    cobs_gpu_status refused = check_query_lengths(ix, queries, lens, nq, z, [&](size_t q) -> cobs_gpu_status {
        // (the kernels' position arithmetic is 32-bit)
        if (lens[q] >= 0xFFFFFFF0ull - (1u << 20)) return fail(COBS_GPU_ERR_QUERY_TOO_LONG, "query too long (query " + std::to_string(q) + ")");
        return COBS_GPU_OK;
    }, bad_query);
    if (refused != COBS_GPU_OK) return refused;
    if (nq == 0 || nf == 0) return COBS_GPU_OK;
    if (!ix->sets) ix->sets = new SetsWork;
    SetsWork* w = ix->sets;
    if (w->files.size() < nf) w->files.resize(nf);

    // the work items of a query: every non-empty set of every labelled file, by (file, set)
    std::vector<SetItem> items;
    const bool count_valid = ix->invalid_bases == COBS_GPU_INVALID_SKIP;
    for (size_t f = 0; f < nf; ++f) {
        const Part& p = ix->parts[f];
        for (size_t i = 0; i < w->files[f].sets.size(); ++i)
            items.push_back(SetItem{(uint32_t)f, w->files[f].sets[i], (uint32_t)i, p.meta.term_size,
                                    count_valid && p.meta.canonicalize != 0 ? 1u : 0u});
    }
    if (items.size() >= 0xFFFFFFF0ull) return fail(COBS_GPU_ERR_ARG, "too many sets");

    std::vector<SetRec> recs;
    const Call call{ix, w, queries, lens, threshold, rank_by, bad_query, z, &items, &recs};
    // passes: K1's tables, the two bitmaps of every (query, set) and a record per (query, set) stay below the search
    // call's workspace limit; a single query that does not fit is refused here, before any device work
    const uint64_t kLimit = ix->tune.pass_bytes;
    const uint64_t terms_per_char = table_bytes_per_char(ix);
    std::vector<uint64_t> qbytes(nq);
    for (size_t q = 0; q < nq; ++q) {
        const uint64_t bm = 8ull * bitmap_words(call, q) + sizeof(SetRec) * (uint64_t)items.size();
        if (bm > kLimit)
            return fail(COBS_GPU_ERR_HIP, "sets: the bitmaps of query " + std::to_string(q) + " (" + std::to_string(bm) +
                        " bytes) do not fit the pass workspace (pass_bytes = " + std::to_string(kLimit) + ")");
        qbytes[q] = (uint64_t)(lens[q] + 16) * terms_per_char + bm;
    }
    if (!items.empty()) {
        HIP_TRY(hipSetDevice(ix->device));
        HIP_TRY(w->items.reserve(items.size()));
        HIP_TRY(hipMemcpy(w->items.p, items.data(), items.size() * sizeof(SetItem), hipMemcpyHostToDevice));
    }
    if (cobs_gpu_status s = cut_passes(nq, kLimit, [&](size_t q) { return qbytes[q]; }, [&](size_t q0, size_t q1) { return run_pass(call, q0, q1); });
        s != COBS_GPU_OK)
        return s;

    // ---- ordering: per query by the key descending, then the other count descending, then (file, set) ascending -- the
    // items are in (file, set) order --; num_results cuts the list
    const double t0 = now_s();
    const bool by_all = rank_by == COBS_GPU_SETS_BY_ALL;
    const cobs_gpu_status handed = hand_out_lists(recs, nq, [](const SetRec& r) { return r.query; },
        [by_all](const SetRec& a, const SetRec& b) {
            const uint32_t ka = by_all ? a.all : a.any, kb = by_all ? b.all : b.any;
            if (ka != kb) return ka > kb;
            const uint32_t oa = by_all ? a.any : a.all, ob = by_all ? b.any : b.all;
            if (oa != ob) return oa > ob;
            return a.item < b.item;
        }, num_results, hits, cap, hit_offsets, "nq",
        [&](const SetRec& r) { return cobs_gpu_set_hit{items[r.item].file_no, items[r.item].set, r.any, r.all}; });
    w->ms[3] += (now_s() - t0) * 1e3;
    return handed;
}

}  // namespace
}  // namespace cobs_amd

using namespace cobs_amd;

extern "C" {

cobs_gpu_status cobs_gpu_set_doc_sets(cobs_gpu_index* ix, size_t file_no, const uint32_t* labels, size_t n_docs, uint32_t n_sets) {
    return guarded([&]() { return set_doc_sets_impl(ix, file_no, labels, n_docs, n_sets); });
}

cobs_gpu_status cobs_gpu_get_doc_sets(const cobs_gpu_index* ix, size_t file_no, uint32_t* n_sets, uint32_t* members, size_t cap) {
    if (!ix || !n_sets) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if (file_no >= ix->parts.size()) return fail(COBS_GPU_ERR_ARG, "file_no out of range");
    *n_sets = 0;
    if (!ix->sets || file_no >= ix->sets->files.size() || ix->sets->files[file_no].labels.empty()) return COBS_GPU_OK;
    const FileSets& fs = ix->sets->files[file_no];
    *n_sets = fs.n_sets;
    if (members) {
        if (cap < fs.n_sets) return fail(COBS_GPU_ERR_CAPACITY, "members needs n_sets entries");
        std::copy(fs.members.begin(), fs.members.end(), members);
    }
    return COBS_GPU_OK;
}

cobs_gpu_status cobs_gpu_search_sets(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                     double threshold, uint32_t rank_by, size_t num_results, cobs_gpu_set_hit* hits, size_t cap,
                                     size_t* hit_offsets, size_t* bad_query) {
    return guarded([&]() {
        return search_sets_impl(ix, queries, lens, nq, threshold, rank_by, num_results, hits, cap, hit_offsets, bad_query);
    });
}

cobs_gpu_status cobs_gpu_sets_ms(cobs_gpu_index* ix, double out[5]) {
    SetsWork* w = ix ? ix->sets : nullptr;
    return take_ms(ix, out, 4, w ? w->ms : nullptr, w ? &w->passes : nullptr);
}

}  // extern "C"
