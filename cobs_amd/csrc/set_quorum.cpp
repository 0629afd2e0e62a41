// cobs_amd/csrc/set_quorum.cpp -- cobs_gpu_search_sets_quorum and cobs_gpu_set_prevalence: for the labelled sets of
// cobs_gpu_set_doc_sets (sets.cpp) HOW MANY members of a set hold each position of a query, and the sets whose soft core --
// the positions held by at least need = max(1, ceil(quorum * members)) members -- reaches the threshold.  The labels become
// inverse records (set_count_kernels.hpp: per page and set the column chunks with members) on the first call that needs
// them, kept per file beside the labels and dropped with them.  Per device pass (cut by the workspace limit, on the handle's
// scratch batch): K1 hashes the queries, a kernel zeroes the cells [query][file][set][n], the count kernel adds the members
// up, and -- for the search -- the select kernel forms core and any per (query, set) and appends the sets that reach the
// threshold to a pool; the host orders every query's records (pooled_call.hpp: cut_passes, hand_out_lists).
// cobs_gpu_set_prevalence copies the cells out instead: they lie in the caller's layout.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "engine.hpp"
#include "prevalence_kernels.hpp"      // launch_prevalence_zero
#include "set_count_kernels.hpp"
#include "sets.hpp"

namespace cobs_amd {
namespace {

// the runs of one resident chunk: per page the slots of labelled real documents, grouped by (set, column chunk)
cobs_gpu_status build_runs(const Part& p, const Chunk& ch, const FileSets& fs, const std::vector<uint32_t>& local_of, ChunkRuns& out) {
    const uint64_t docs = p.meta.doc_names.size();
    std::vector<SetRun> runs;
    std::vector<uint32_t> col;
    std::vector<uint4> mask;
    std::vector<std::tuple<uint32_t, uint32_t, uint32_t>> slots;      // (set, column chunk, slot of the column chunk)
    uint32_t max_recs = 0;
    for (size_t pg = 0; pg < ch.pages.size(); ++pg) {
        const PageDev& pd = ch.pages[pg];
        const uint64_t live = docs > pd.doc0 ? std::min<uint64_t>(docs - pd.doc0, (uint64_t)pd.valid_bytes * 8) : 0;
        slots.clear();
        for (uint64_t s = 0; s < live; ++s) {
            const uint32_t l = fs.labels[pd.doc0 + s];
            if (l != COBS_GPU_NO_SET) slots.emplace_back(local_of[l], (uint32_t)(s / 128), (uint32_t)(s % 128));
        }
        std::sort(slots.begin(), slots.end());
        for (size_t i = 0; i < slots.size(); ++i) {
            const auto [set, c, bit] = slots[i];
            const bool new_run = i == 0 || std::get<0>(slots[i - 1]) != set;
            if (new_run) {
                if (col.size() >= 0xFFFFFFF0ull) return fail(COBS_GPU_ERR_ARG, "too many inverse set records");
                runs.push_back(SetRun{(uint32_t)pg, set, (uint32_t)col.size(), 0u});
            }
            if (new_run || std::get<1>(slots[i - 1]) != c) {
                col.push_back(c);
                mask.push_back(uint4{0u, 0u, 0u, 0u});
                max_recs = std::max(max_recs, ++runs.back().nrec);
            }
            uint32_t* m = &mask.back().x;
            m[bit >> 5] |= 1u << (bit & 31u);
        }
    }
    out.n_runs = runs.size();
    out.max_recs = max_recs;
    HIP_TRY(out.runs.reserve(runs.size()));
    HIP_TRY(out.col.reserve(col.size()));
    HIP_TRY(out.mask.reserve(mask.size()));
    if (!runs.empty()) {
        HIP_TRY(hipMemcpy(out.runs.p, runs.data(), runs.size() * sizeof(SetRun), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(out.col.p, col.data(), col.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(out.mask.p, mask.data(), mask.size() * sizeof(uint4), hipMemcpyHostToDevice));
    }
    return COBS_GPU_OK;
}

// ... of every labelled file that does not have them yet
cobs_gpu_status ensure_runs(cobs_gpu_index* ix, SetsWork* w) {
    for (size_t f = 0; f < ix->parts.size(); ++f) {
        FileSets& fs = w->files[f];
        const Part& p = ix->parts[f];
        if (fs.sets.empty() || fs.runs.size() == p.chunks.size()) continue;
        HIP_TRY(hipSetDevice(ix->device));
        std::vector<uint32_t> local_of(fs.n_sets, COBS_GPU_NO_SET);
        for (size_t i = 0; i < fs.sets.size(); ++i) local_of[fs.sets[i]] = (uint32_t)i;
        std::vector<ChunkRuns> runs(p.chunks.size());
        for (size_t c = 0; c < p.chunks.size(); ++c) {
            const Chunk& ch = p.chunks[c];
            if (!ch.d_data || ch.pages.empty()) continue;
            if (cobs_gpu_status s = build_runs(p, ch, fs, local_of, runs[c]); s != COBS_GPU_OK) return s;
        }
        fs.runs = std::move(runs);
    }
    return COBS_GPU_OK;
}

struct Call {
    cobs_gpu_index* ix;
    SetsWork* w;
    const char* const* queries;
    const size_t* lens;
    double threshold;
    size_t* bad_query;
    uint32_t z;
    const std::vector<SetQuorumItem>* items;    // the search: its work items; NULL: cobs_gpu_set_prevalence
    std::vector<SetQuorumRec>* recs;            // the records of all passes, `query` = the call's query number
    uint32_t* counts;                           // cobs_gpu_set_prevalence: the caller's cells
};

// cells of (query q, file f): non-empty sets x n
uint64_t file_cells(const Call& c, size_t q, size_t f) {
    return (uint64_t)c.w->files[f].sets.size() * (c.lens[q] - c.ix->parts[f].meta.term_size + 1 - c.z);
}

// one device pass over the queries [q0, q1); cell0 = the cells of the call's queries before q0
cobs_gpu_status run_pass(const Call& c, size_t q0, size_t q1, uint64_t cell0) {
    cobs_gpu_index* ix = c.ix;
    SetQuorumWork* w = &c.w->quorum;
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(w->ev.create());
    cobs_gpu_batch* b = nullptr;
    if (cobs_gpu_status s = pass_queries(ix, c.queries, c.lens, q0, q1, c.bad_query, &b); s != COBS_GPU_OK) return s;
    hipStream_t st = b->own_stream;
    const size_t n = q1 - q0, nf = ix->parts.size(), nitems = c.items ? c.items->size() : 0;
    // the cells of the pass: per (query, file) its sets' counts back to back, set-major
    HIP_TRY(w->cell_off.reserve(n * nf + 1));
    HIP_TRY(w->h_cell_off.reserve(n * nf + 1));
    uint64_t cells = 0;
    size_t max_len = 0;
    for (size_t q = q0; q < q1; ++q) {
        max_len = std::max(max_len, c.lens[q]);
        for (size_t f = 0; f < nf; ++f) {
            w->h_cell_off.p[(q - q0) * nf + f] = cells;
            cells += file_cells(c, q, f);
        }
    }
    w->h_cell_off.p[n * nf] = cells;
    const uint64_t pool_cap = std::max<uint64_t>((uint64_t)n * nitems, 1);
    if (w->cells.reserve((size_t)cells) != hipSuccess || w->pool.reserve((size_t)pool_cap) != hipSuccess) {
        (void)hipGetLastError();
        return fail(COBS_GPU_ERR_HIP, "set quorum: out of device memory for the counts and records of " + std::to_string(n) +
                    " queries; lower pass_bytes or use fewer queries per call");
    }
    HIP_TRY(w->fill.reserve(1));
    HIP_TRY(w->land.reserve());
    const bool count_valid = ix->invalid_bases == COBS_GPU_INVALID_SKIP;

    HIP_TRY(hipMemcpyAsync(w->cell_off.p, w->h_cell_off.p, (n * nf + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_clear_flags(b->flags.p, st, count_valid ? b->valid.p : nullptr, count_valid ? (uint32_t)(n * nf) : 0u));
    // (by a kernel, not a memset node)
    HIP_TRY(launch_prevalence_zero(w->cells.p, cells, st));
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
        FileSets& fs = c.w->files[f];
        if (fs.sets.empty()) continue;
        if (fs.runs.size() != p.chunks.size()) return fail(COBS_GPU_ERR_ARG, "set quorum: the inverse records of a file are missing");
        SetCountArgs ca{};
        ca.t = table_ref_for(b, f, p, c.z);
        ca.cell_off = w->cell_off.p + f;
        ca.cells = w->cells.p;
        ca.cell_stride = (uint32_t)nf;
        const uint32_t max_positions = (uint32_t)(max_len - p.meta.term_size + 1 - c.z);
        for (size_t ci = 0; ci < p.chunks.size(); ++ci) {
            const Chunk& ch = p.chunks[ci];
            const ChunkRuns& cr = fs.runs[ci];
            if (!ch.d_data || ch.pages.empty() || cr.n_runs == 0) continue;
            ca.data = ch.d_data;
            ca.pages = ch.d_pages;
            ca.pitch = ch.pitch;
            ca.runs = cr.runs.p;
            ca.rec_col = cr.col.p;
            ca.rec_mask = cr.mask.p;
            HIP_TRY(launch_set_count(ca, cr.n_runs, cr.max_recs, (uint32_t)n, max_positions, st));
        }
    }
    HIP_TRY(w->ev.mark(2, st));
    if (c.items) {
        SetQuorumSelectArgs sa{};
        sa.cells = w->cells.p;
        sa.cell_off = w->cell_off.p;
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
        HIP_TRY(launch_set_quorum_select(sa, st));
    }
    HIP_TRY(w->ev.mark(3, st));
    HIP_TRY(w->land.flags_home(b, st));
    HIP_TRY(w->land.fill_home(w->fill.p, st));
    if (c.counts && cells) HIP_TRY(hipMemcpyAsync(c.counts + cell0, w->cells.p, (size_t)cells * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (w->ev.add_elapsed(w->ms)) w->passes++;
    if (cobs_gpu_status s = invalid_base_from_flags(w->land.invalid_word(), n, c.bad_query, q0); s != COBS_GPU_OK) return s;
    if (!c.items) return COBS_GPU_OK;
    const uint64_t fill = w->land.fill();
    if (fill > pool_cap) return fail(COBS_GPU_ERR_HIP, "set quorum: the record pool overflowed");      // (it holds every item)
    return append_pass_records(*c.recs, w->pool.p, fill, q0);
}

// what both calls refuse on the handle and the queries, before anything is launched
cobs_gpu_status refuse(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq, size_t* bad_query) {
    if (nq >= 0xFFFFFFF0ull) return fail(COBS_GPU_ERR_ARG, "too many queries");
    if (ix->hbm_budget != 0 || any_streamed(ix)) return fail(COBS_GPU_ERR_UNSUPPORTED, "set quorum: not on a handle with an HBM budget (its rows are not all resident)");
    if (ix->shard_count > 1) return fail(COBS_GPU_ERR_UNSUPPORTED, "set quorum: not on one shard of several (the counts are additive over shards, but nothing adds them up yet)");
    return check_query_lengths(ix, queries, lens, nq, ix->findere, [&](size_t q) -> cobs_gpu_status {
        // (the kernels' position arithmetic is 32-bit with room for one launch's stride)
        if (lens[q] >= 0xFFFFFFF0ull - (1u << 20)) return fail(COBS_GPU_ERR_QUERY_TOO_LONG, "query too long (query " + std::to_string(q) + ")");
        return COBS_GPU_OK;
    }, bad_query);
}

// the passes of a call: K1's tables, 4 bytes per (set, position) and a record per (query, set) stay below the search
// call's workspace limit; a single query whose counts do not fit is refused before any device work
cobs_gpu_status run_passes(const Call& call, size_t nq, size_t rec_bytes_per_query) {
    cobs_gpu_index* ix = call.ix;
    const size_t nf = ix->parts.size();
    const uint64_t kLimit = ix->tune.pass_bytes;
    const uint64_t terms_per_char = table_bytes_per_char(ix);
    std::vector<uint64_t> qbytes(nq), qcells(nq);
    for (size_t q = 0; q < nq; ++q) {
        uint64_t cells = 0;
        for (size_t f = 0; f < nf; ++f) cells += file_cells(call, q, f);
        const uint64_t cb = 4ull * cells + rec_bytes_per_query;
        if (cb > kLimit)
            return fail(COBS_GPU_ERR_HIP, "set quorum: the counts of query " + std::to_string(q) + " (" + std::to_string(cb) +
                        " bytes) do not fit the pass workspace (pass_bytes = " + std::to_string(kLimit) + ")");
        qcells[q] = cells;
        qbytes[q] = (uint64_t)(call.lens[q] + 16) * terms_per_char + cb;
    }
    if (cobs_gpu_status s = ensure_runs(ix, call.w); s != COBS_GPU_OK) return s;
    uint64_t cell0 = 0;
    return cut_passes(nq, kLimit, [&](size_t q) { return qbytes[q]; }, [&](size_t q0, size_t q1) {
        const uint64_t at = cell0;
        for (size_t q = q0; q < q1; ++q) cell0 += qcells[q];
        return run_pass(call, q0, q1, at);
    });
}

cobs_gpu_status search_sets_quorum_impl(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                        double threshold, double quorum, size_t num_results, cobs_gpu_set_quorum_hit* hits,
                                        size_t cap, size_t* hit_offsets, size_t* bad_query) {
    if (!(quorum > 0.0 && quorum <= 1.0)) return fail(COBS_GPU_ERR_ARG, "quorum: a number in (0, 1]");
    if (!ix || !hit_offsets) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if ((nq && (!queries || !lens)) || (cap && !hits)) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if (nq < 0xFFFFFFF0ull)
        for (size_t q = 0; q <= nq; ++q) hit_offsets[q] = 0;
    if (cobs_gpu_status s = refuse(ix, queries, lens, nq, bad_query); s != COBS_GPU_OK) return s;
    const size_t nf = ix->parts.size();
    if (nq == 0 || nf == 0) return COBS_GPU_OK;
    if (!ix->sets) ix->sets = new SetsWork;
    SetsWork* w = ix->sets;
    if (w->files.size() < nf) w->files.resize(nf);

    // the work items of a query: every non-empty set of every labelled file, by (file, set), with the members it needs
    std::vector<SetQuorumItem> items;
    const bool count_valid = ix->invalid_bases == COBS_GPU_INVALID_SKIP;
    for (size_t f = 0; f < nf; ++f) {
        const Part& p = ix->parts[f];
        const FileSets& fs = w->files[f];
        for (size_t i = 0; i < fs.sets.size(); ++i) {
            // (in double, once per set and call: the device never multiplies by quorum)
            const double need = std::ceil(quorum * (double)fs.members[fs.sets[i]]);
            items.push_back(SetQuorumItem{(uint32_t)f, fs.sets[i], (uint32_t)i, p.meta.term_size,
                                          count_valid && p.meta.canonicalize != 0 ? 1u : 0u, need > 1.0 ? (uint32_t)need : 1u});
        }
    }
    if (items.size() >= 0xFFFFFFF0ull) return fail(COBS_GPU_ERR_ARG, "too many sets");

    std::vector<SetQuorumRec> recs;
    const Call call{ix, w, queries, lens, threshold, bad_query, ix->findere, &items, &recs, nullptr};
    if (!items.empty()) {
        HIP_TRY(hipSetDevice(ix->device));
        HIP_TRY(w->quorum.items.reserve(items.size()));
        HIP_TRY(hipMemcpy(w->quorum.items.p, items.data(), items.size() * sizeof(SetQuorumItem), hipMemcpyHostToDevice));
    }
    if (cobs_gpu_status s = run_passes(call, nq, sizeof(SetQuorumRec) * items.size()); s != COBS_GPU_OK) return s;

    // ---- ordering: per query by core descending, then any descending, then (file, set) ascending -- the items are in
    // (file, set) order --; num_results cuts the list
    const double t0 = now_s();
    const cobs_gpu_status handed = hand_out_lists(recs, nq, [](const SetQuorumRec& r) { return r.query; },
        [](const SetQuorumRec& a, const SetQuorumRec& b) {
            if (a.core != b.core) return a.core > b.core;
            if (a.any != b.any) return a.any > b.any;
            return a.item < b.item;
        }, num_results, hits, cap, hit_offsets, "nq",
        [&](const SetQuorumRec& r) { return cobs_gpu_set_quorum_hit{items[r.item].file_no, items[r.item].set, r.core, r.any}; });
    w->quorum.ms[3] += (now_s() - t0) * 1e3;
    return handed;
}

cobs_gpu_status set_prevalence_impl(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                    uint32_t* counts, size_t cap, size_t* offsets, size_t* needed, size_t* bad_query) {
    if (!ix || !offsets) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if (nq && (!queries || !lens)) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if (cap && !counts) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    offsets[0] = 0;
    if (needed) *needed = 0;
    if (cobs_gpu_status s = refuse(ix, queries, lens, nq, bad_query); s != COBS_GPU_OK) return s;
    const size_t nf = ix->parts.size();
    if (!ix->sets) ix->sets = new SetsWork;
    SetsWork* w = ix->sets;
    if (w->files.size() < nf) w->files.resize(nf);
    const Call call{ix, w, queries, lens, 0.0, bad_query, ix->findere, nullptr, nullptr, counts};
    size_t cells = 0;
    for (size_t q = 0; q < nq; ++q)
        for (size_t f = 0; f < nf; ++f) {
            cells += file_cells(call, q, f);
            offsets[q * nf + f + 1] = cells;
        }
    if (needed) *needed = cells;
    if (cells > cap) return fail(COBS_GPU_ERR_CAPACITY, "count buffer too small; *needed holds the needed size");
    if (cells == 0) return COBS_GPU_OK;
    return run_passes(call, nq, 0);
}

}  // namespace
}  // namespace cobs_amd

using namespace cobs_amd;

extern "C" {

cobs_gpu_status cobs_gpu_search_sets_quorum(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                            double threshold, double quorum, size_t num_results, cobs_gpu_set_quorum_hit* hits,
                                            size_t cap, size_t* hit_offsets, size_t* bad_query) {
    return guarded([&]() {
        return search_sets_quorum_impl(ix, queries, lens, nq, threshold, quorum, num_results, hits, cap, hit_offsets, bad_query);
    });
}

cobs_gpu_status cobs_gpu_set_prevalence(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                        uint32_t* counts, size_t cap, size_t* offsets, size_t* needed, size_t* bad_query) {
    return guarded([&]() { return set_prevalence_impl(ix, queries, lens, nq, counts, cap, offsets, needed, bad_query); });
}

cobs_gpu_status cobs_gpu_set_quorum_ms(cobs_gpu_index* ix, double out[5]) {
    SetsWork* w = ix ? ix->sets : nullptr;
    return take_ms(ix, out, 4, w ? w->quorum.ms : nullptr, w ? &w->quorum.passes : nullptr);
}

}  // extern "C"
