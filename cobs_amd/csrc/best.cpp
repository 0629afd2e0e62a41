// cobs_amd/csrc/best.cpp -- cobs_gpu_search_best: for every document the best query of a GROUP of queries (the allele of
// a locus that fits best).  Driven like cobs_gpu_search_groups (groups.cpp): the call's queries are cut into device
// passes by the workspace limit (pass_bytes) and run with the batch building blocks -- upload, K1, K2 with score rows
// kept, over two alternating scratch batches on one stream --; behind every pass's scan group_best_kernel merges its
// score rows into the per-(group, slot) state of the best member where they lie (best_kernels.hip), so the host stages
// pass i + 1 while the device scans pass i.  After the last pass the select kernel appends the documents whose best
// member reaches its threshold to a pool (its retry: pooled_pass.hpp); the host orders each group's records
// (pooled_call.hpp: hand_out_lists).  No per-query result leaves the device.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "best_kernels.hpp"
#include "engine.hpp"
#include "pooled_pass.hpp"

namespace cobs_amd {

struct BestWork {
    cobs_gpu_batch* batch[2] = {nullptr, nullptr};
    hipStream_t stream = nullptr;
    hipEvent_t landed[2] = {nullptr, nullptr};                  // a pass's flag words are home
    hipEvent_t ev_best[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    hipEvent_t ev_sel[2] = {nullptr, nullptr};
    PinnedBuf<uint32_t> h_land[2];          // flag words
    PinnedBuf<uint8_t> h_args[2];           // files | spans | folds | nominal P [file][nq] of a pass, as the kernels read them
    DevBuf<uint8_t> d_args[2];
    DevBuf<uint32_t> state;                 // four arrays [n_groups][local_counts], for the lifetime of a call
    DevBuf<uint32_t> part;                  // four arrays [pieces][local_counts]: the partial states of a pass's split groups
    HitPool<BestRec> hits{"best: the selection pool", launch_group_zero};
    DevBuf<GroupRange> ranges;
    double ms[3] = {0, 0, 0};               // best and merge kernels | select | host ordering of the last call
    uint64_t counts[4] = {0, 0, 0, 0};      // passes | spans that own their cells | partial states | folds of the last call
    ~BestWork() {
        for (auto* b : batch) delete b;
        for (auto& e : landed) if (e) (void)hipEventDestroy(e);
        for (auto& r : ev_best) for (auto& e : r) if (e) (void)hipEventDestroy(e);
        for (auto& e : ev_sel) if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

void destroy_best_work(BestWork* w) { delete w; }

namespace {

struct Call {
    cobs_gpu_index* ix;
    BestWork* w;
    const char* const* queries;
    const size_t* lens;
    const size_t* group_offsets;
    size_t n_groups;
    size_t* bad_query;
    bool count_valid;                       // invalid_bases = skip: P is K1's valid positions, on the device
    BestState state;
};

struct Pass { size_t g0, g1; int slot; size_t group0; };

BestState state_of(uint32_t* p, uint64_t ncells) { return BestState{p, p + ncells, p + 2 * ncells, p + 3 * ncells}; }

cobs_gpu_status init_work(cobs_gpu_index* ix) {
    if (!ix->best) ix->best = new BestWork;
    BestWork* w = ix->best;
    if (!w->stream) HIP_TRY(hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking));
    for (auto& e : w->landed) if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& r : w->ev_best) for (auto& e : r) if (!e) HIP_TRY(hipEventCreate(&e));
    for (auto& e : w->ev_sel) if (!e) HIP_TRY(hipEventCreate(&e));
    for (auto& b : w->batch)
        if (!b)
            if (cobs_gpu_status st = cobs_gpu_batch_create(ix, 0, 0, &b); st != COBS_GPU_OK) return st;
    return COBS_GPU_OK;
}

// a piece of a split group reads at least this many rows: its partial state costs 16 bytes per slot written and 16 read
// again, which 64 one-byte scores pay for
constexpr size_t kMinPiece = 64;

// upload, K1, K2 and the best-member merge of the queries [g0, g1), queued on the call's stream
cobs_gpu_status pass_begin(const Call& c, const Pass& ps) {
    cobs_gpu_index* ix = c.ix;
    BestWork* w = c.w;
    cobs_gpu_batch* b = w->batch[ps.slot];
    hipStream_t st = w->stream;
    const size_t n = ps.g1 - ps.g0, nf = ix->parts.size();
    const uint32_t z = ix->findere;
    size_t bad = 0;
    if (cobs_gpu_status s = set_queries_on(b, c.queries + ps.g0, c.lens + ps.g0, n, st, ix->tune.hash_stream != 0, &bad, ps.g0);
        s != COBS_GPU_OK) {
        if (c.bad_query) *c.bad_query = ps.g0 + bad;
        return s;
    }
    // (no threshold per pass: the select applies it to the best member alone)
    if (cobs_gpu_status s = run_impl(b, 0.0, 0, st, true); s != COBS_GPU_OK) return s;
    ix->host_passes++;
    w->counts[0]++;
    // the spans of the pass: the part of every group that lies in it.  Enough (group, tile) pairs to fill the device: one
    // span per group, every cell of the state has one writer.  Few groups (one locus): a group's queries are split over
    // several work-groups that write partial states, which the merge kernel folds into the stored state.
    const uint64_t nslots = ix->local_counts;
    const uint32_t tiles = (uint32_t)((nslots + group_tile_slots(b->elem_bytes) - 1) / group_tile_slots(b->elem_bytes));
    std::vector<BestSpan> spans;
    std::vector<BestFold> folds;
    size_t groups_in = 0;
    for (size_t g = ps.group0; g < c.n_groups && c.group_offsets[g] < ps.g1; ++g)
        groups_in += std::min(c.group_offsets[g + 1], ps.g1) > std::max(c.group_offsets[g], ps.g0) ? 1 : 0;
    const uint64_t kFill = 256, kTarget = 2048;         // compute units | work-groups a split launch aims for
    const uint64_t split = groups_in * tiles >= kFill ? 1 : (kTarget + groups_in * tiles - 1) / std::max<uint64_t>(groups_in * tiles, 1);
    uint32_t pieces = 0;
    for (size_t g = ps.group0; g < c.n_groups && c.group_offsets[g] < ps.g1; ++g) {
        const size_t q0 = std::max(c.group_offsets[g], ps.g0), q1 = std::min(c.group_offsets[g + 1], ps.g1);
        if (q1 <= q0) continue;
        const size_t step = std::max<size_t>(kMinPiece, (q1 - q0 + split - 1) / split);
        if (q1 - q0 <= step) {
            spans.push_back(BestSpan{(uint32_t)g, (uint32_t)(q0 - ps.g0), (uint32_t)(q1 - ps.g0), kBestNone});
            w->counts[1]++;
            continue;
        }
        const uint32_t piece0 = pieces;
        for (size_t q = q0; q < q1; q += step)
            spans.push_back(BestSpan{(uint32_t)g, (uint32_t)(q - ps.g0), (uint32_t)(std::min(q + step, q1) - ps.g0), pieces++});
        folds.push_back(BestFold{(uint32_t)g, piece0, pieces});
        w->counts[2] += pieces - piece0;
        w->counts[3]++;
    }
    if ((uint64_t)pieces * nslots >= (1ull << 38) || w->part.reserve((size_t)(4ull * pieces * nslots)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(COBS_GPU_ERR_CAPACITY, "no room for the partial states of " + std::to_string(pieces) + " pieces; use fewer groups per call");
    }
    const size_t files_bytes = round_up(nf * sizeof(BestFile), 16), spans_bytes = round_up(spans.size() * sizeof(BestSpan), 16);
    const size_t folds_bytes = round_up(folds.size() * sizeof(BestFold), 16), pos_bytes = nf * n * sizeof(uint32_t);
    const size_t args_bytes = files_bytes + spans_bytes + folds_bytes + pos_bytes;
    HIP_TRY(w->h_args[ps.slot].reserve(args_bytes));
    HIP_TRY(w->d_args[ps.slot].reserve(args_bytes));
    uint8_t* h = w->h_args[ps.slot].p;
    uint8_t* d = w->d_args[ps.slot].p;
    // P of every query of the pass per file: T - z, or where K1 counted them (`skip`, a file of canonical k-mers) its
    // valid positions [file][nq], read where they lie
    uint32_t* hpos = reinterpret_cast<uint32_t*>(h + files_bytes + spans_bytes + folds_bytes);
    const uint32_t* dpos = reinterpret_cast<const uint32_t*>(d + files_bytes + spans_bytes + folds_bytes);
    BestFile* hf = reinterpret_cast<BestFile*>(h);
    for (size_t f = 0; f < nf; ++f) {
        const Part& p = ix->parts[f];
        for (size_t q = 0; q < n; ++q) hpos[f * n + q] = (uint32_t)(c.lens[ps.g0 + q] - p.meta.term_size + 1 - z);
        const bool counted = c.count_valid && p.meta.canonicalize != 0;
        hf[f] = BestFile{(uint32_t)p.local_offset, (uint32_t)(p.local_offset + p.slot_count), counted ? b->valid.p + f * n : dpos + f * n};
    }
    if (!spans.empty()) std::memcpy(h + files_bytes, spans.data(), spans.size() * sizeof(BestSpan));
    if (!folds.empty()) std::memcpy(h + files_bytes + spans_bytes, folds.data(), folds.size() * sizeof(BestFold));
    HIP_TRY(hipMemcpyAsync(d, h, args_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(w->ev_best[ps.slot][0], st));
    const BestState part = state_of(w->part.p, (uint64_t)pieces * nslots);
    const size_t per_launch = std::max<size_t>(1, 0x7FFFFFFFull / std::max<uint32_t>(tiles, 1));
    for (size_t s0 = 0; s0 < spans.size(); s0 += per_launch) {
        BestArgs a{};
        a.rows = b->counts.p;
        a.spans = reinterpret_cast<const BestSpan*>(d + files_bytes) + s0;
        a.files = reinterpret_cast<const BestFile*>(d);
        a.state = c.state;
        a.part = part;
        a.nslots = nslots;
        a.nspans = (uint32_t)std::min(per_launch, spans.size() - s0);
        a.nfiles = (uint32_t)nf;
        a.tiles = tiles;
        a.score_bytes = b->elem_bytes;
        a.query0 = (uint32_t)ps.g0;
        HIP_TRY(launch_group_best(a, st));
    }
    if (!folds.empty()) {
        BestMergeArgs m{};
        m.folds = reinterpret_cast<const BestFold*>(d + files_bytes + spans_bytes);
        m.state = c.state;
        m.part = part;
        m.nslots = nslots;
        m.nfolds = (uint32_t)folds.size();
        HIP_TRY(launch_group_best_merge(m, st));
    }
    HIP_TRY(hipEventRecord(w->ev_best[ps.slot][1], st));
    // the flag words come home behind the pass
    HIP_TRY(w->h_land[ps.slot].reserve(4));
    HIP_TRY(hipMemcpyAsync(w->h_land[ps.slot].p, b->flags.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(w->landed[ps.slot], st));
    return COBS_GPU_OK;
}

cobs_gpu_status pass_end(const Call& c, const Pass& ps) {
    BestWork* w = c.w;
    HIP_TRY(hipEventSynchronize(w->landed[ps.slot]));
    w->batch[ps.slot]->synced = true;
    float ms = 0;
    if (hipEventElapsedTime(&ms, w->ev_best[ps.slot][0], w->ev_best[ps.slot][1]) == hipSuccess) w->ms[0] += ms;
    else (void)hipGetLastError();
    return invalid_base_from_flags(w->h_land[ps.slot].p[0], ps.g1 - ps.g0, c.bad_query, ps.g0);
}

// a before b in a group's list: the larger fraction (exact; positions = 0 is the fraction 0), then the larger score, then
// (file, document)
bool record_before(const BestRec& a, const BestRec& b) {
    const uint64_t x = (uint64_t)a.score * std::max(b.positions, 1u), y = (uint64_t)b.score * std::max(a.positions, 1u);
    if (x != y) return x > y;
    if (a.score != b.score) return a.score > b.score;
    if (a.file != b.file) return a.file < b.file;
    return a.doc < b.doc;
}

cobs_gpu_status search_best_impl(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                 const size_t* group_offsets, size_t n_groups, double threshold, size_t num_results,
                                 cobs_gpu_best_hit* hits, size_t cap, size_t* hit_offsets, size_t* bad_query) {
    if (!ix || !group_offsets || !hit_offsets) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if ((nq && (!queries || !lens)) || (cap && !hits)) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if (group_offsets[0] != 0) return fail(COBS_GPU_ERR_ARG, "group_offsets[0] is not 0");
    for (size_t g = 0; g < n_groups; ++g)
        if (group_offsets[g + 1] < group_offsets[g])
            return fail(COBS_GPU_ERR_ARG, "group_offsets are not ascending (group " + std::to_string(g) + ")");
    if (group_offsets[n_groups] != nq) return fail(COBS_GPU_ERR_ARG, "group_offsets[n_groups] is not the number of queries");
    if (n_groups >= 0xFFFFFFF0ull || nq >= 0xFFFFFFF0ull) return fail(COBS_GPU_ERR_ARG, "too many groups or queries");
    if (ix->hbm_budget != 0 || any_streamed(ix)) return fail(COBS_GPU_ERR_UNSUPPORTED, "best: not on a handle with an HBM budget (its score rows come range by range)");
    if (ix->shard_count > 1) return fail(COBS_GPU_ERR_UNSUPPORTED, "best: not on one shard of several (a shard holds a part of every file's documents; ask every shard)");
    for (size_t g = 0; g <= n_groups; ++g) hit_offsets[g] = 0;
    const uint32_t z = ix->findere;
    // everything the host can refuse is refused before anything is launched
    cobs_gpu_status refused = check_query_lengths(ix, queries, lens, nq, z, [&](size_t q) -> cobs_gpu_status {
        if (lens[q] >= 0xFFFFFFF0ull) return fail(COBS_GPU_ERR_QUERY_TOO_LONG, "query too long (query " + std::to_string(q) + ")");
        return COBS_GPU_OK;
    }, bad_query);
    if (refused != COBS_GPU_OK) return refused;
    if (n_groups == 0 || nq == 0) return COBS_GPU_OK;

    HIP_TRY(hipSetDevice(ix->device));
    if (cobs_gpu_status st = init_work(ix); st != COBS_GPU_OK) return st;
    BestWork* w = ix->best;
    w->ms[0] = w->ms[1] = w->ms[2] = 0;
    w->counts[0] = w->counts[1] = w->counts[2] = w->counts[3] = 0;
    const uint64_t nslots = ix->local_counts;
    const uint64_t ncells = n_groups * nslots;
    if (ncells >= (1ull << 38) || w->state.reserve((size_t)(4 * ncells)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(COBS_GPU_ERR_CAPACITY, "no room for the best-member state of " + std::to_string(n_groups) + " groups; use fewer groups per call");
    }
    hipStream_t st = w->stream;
    const BestState state = state_of(w->state.p, ncells);
    HIP_TRY(launch_best_init(state, ncells, st));

    const Call call{ix, w, queries, lens, group_offsets, n_groups, bad_query, ix->invalid_bases == COBS_GPU_INVALID_SKIP, state};
    auto drain = [&]() { (void)hipStreamSynchronize(st); };
    // passes: the score rows and K1's tables of a pass stay below the workspace limit
    const uint64_t kLimit = ix->tune.pass_bytes;
    uint32_t min_term = 0xFFFFFFFFu;
    for (const Part& p : ix->parts) min_term = std::min(min_term, p.meta.term_size);
    const uint64_t terms_per_char = table_bytes_per_char(ix);
    auto score_bytes = [&](uint64_t max_len) -> uint64_t {
        const uint64_t terms = max_len - min_term + 1;
        return std::max<uint64_t>(terms <= 255 ? 1 : terms <= 65535 ? 2 : 4, ix->tune.min_score_bytes);
    };
    std::vector<Pass> inflight;
    size_t g0 = 0, group0 = 0, npass = 0;
    while (g0 < nq) {
        uint64_t table_bytes = 0, max_len = 0;
        size_t g1 = g0;
        while (g1 < nq && g1 - g0 < 0xFFFFFFF0ull) {
            const uint64_t ml = std::max<uint64_t>(max_len, lens[g1]);
            const uint64_t tb = table_bytes + (uint64_t)(lens[g1] + 16) * terms_per_char;
            if (g1 > g0 && (tb > kLimit || (uint64_t)(g1 - g0 + 1) * nslots * score_bytes(ml) > kLimit)) break;
            max_len = ml;
            table_bytes = tb;
            ++g1;
        }
        while (group_offsets[group0 + 1] <= g0) ++group0;        // the first group with a query in the pass
        const Pass ps{g0, g1, (int)(npass & 1), group0};
        if (cobs_gpu_status s = pass_begin(call, ps); s != COBS_GPU_OK) { drain(); return s; }
        if (!inflight.empty()) {
            const Pass prev = inflight.front();
            inflight.clear();
            if (cobs_gpu_status s = pass_end(call, prev); s != COBS_GPU_OK) { drain(); return s; }
        }
        inflight.push_back(ps);
        g0 = g1;
        ++npass;
    }
    if (!inflight.empty())
        if (cobs_gpu_status s = pass_end(call, inflight.front()); s != COBS_GPU_OK) { drain(); return s; }
    HIP_TRY(hipStreamSynchronize(st));

    // ---- selection: real documents whose best member's score reaches the bound the select kernel forms from `threshold`
    // and the member's positions (min_key's rule, on the device; threshold <= 0: every real document of a group with
    // members).  The state stays where it is while the pool takes its retry (pooled_pass.hpp)
    const std::vector<GroupRange> ranges = real_ranges<GroupRange>(*ix);
    std::vector<BestRec> recs;
    if (!ranges.empty()) {
        HIP_TRY(w->ranges.reserve(ranges.size()));
        HIP_TRY(hipMemcpy(w->ranges.p, ranges.data(), ranges.size() * sizeof(GroupRange), hipMemcpyHostToDevice));
        uint64_t fill = 0;
        cobs_gpu_status s = select_through(w->hits, first_pool_cap(ix->tune.hit_cap, threshold, real_documents(*ix), n_groups), st, w->ev_sel, &w->ms[1],
            [](uint64_t cap) {
                return fail(COBS_GPU_ERR_CAPACITY, "no room for " + std::to_string(cap) + " best records; raise the threshold or use fewer groups per call");
            },
            [&](uint64_t pool_cap) {
                BestSelArgs sa{};
                sa.state = state;
                sa.ranges = w->ranges.p;
                sa.pool = w->hits.pool.p;
                sa.fill = w->hits.fill.p;
                sa.nslots = nslots;
                sa.cap = pool_cap;
                sa.threshold = threshold;
                sa.n_groups = (uint32_t)n_groups;
                sa.nranges = (uint32_t)ranges.size();
                return launch_group_best_select(sa, st);
            }, &fill);
        if (s != COBS_GPU_OK) return s;
        if (cobs_gpu_status c = append_records(recs, w->hits.pool.p, fill); c != COBS_GPU_OK) return c;
    }
    // ---- ordering: per group by fraction descending, then score descending, then (file, document); num_results cuts
    const double t0 = now_s();
    const cobs_gpu_status handed = hand_out_lists(recs, n_groups, [](const BestRec& r) { return r.group; }, record_before,
        num_results, hits, cap, hit_offsets, "n_groups",
        [](const BestRec& r) { return cobs_gpu_best_hit{r.file, r.doc, r.query, r.score, r.positions, r.ties}; });
    w->ms[2] = (now_s() - t0) * 1e3;
    return handed;
}

}  // namespace
}  // namespace cobs_amd

using namespace cobs_amd;

extern "C" {

cobs_gpu_status cobs_gpu_search_best(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                     const size_t* group_offsets, size_t n_groups, double threshold, size_t num_results,
                                     cobs_gpu_best_hit* hits, size_t cap, size_t* hit_offsets, size_t* bad_query) {
    return guarded([&]() {
        return search_best_impl(ix, queries, lens, nq, group_offsets, n_groups, threshold, num_results, hits, cap, hit_offsets,
                                bad_query);
    });
}

cobs_gpu_status cobs_gpu_best_ms(cobs_gpu_index* ix, double out[3]) {
    if (!ix || !out) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    out[0] = out[1] = out[2] = 0;
    if (BestWork* w = ix->best) {
        out[0] = w->ms[0];
        out[1] = w->ms[1];
        out[2] = w->ms[2];
    }
    return COBS_GPU_OK;
}

cobs_gpu_status cobs_gpu_best_counts(cobs_gpu_index* ix, uint64_t out[4]) {
    if (!ix || !out) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (BestWork* w = ix->best)
        for (int i = 0; i < 4; ++i) out[i] = w->counts[i];
    return COBS_GPU_OK;
}

}  // extern "C"
