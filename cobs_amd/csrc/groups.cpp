// cobs_amd/csrc/groups.cpp -- cobs_gpu_search_groups: which documents a SET of queries comes from.  The call's queries are
// cut into device passes by the workspace limit (pass_bytes) and driven with the batch building blocks -- upload, K1,
// K2 with the read threshold, over two alternating scratch batches on one stream --; behind every pass's scan the
// accumulate kernel adds its score rows to the per-group sums and votes where they lie (group_kernels.hip), so the host
// stages pass i + 1 while the device scans and accumulates pass i.  After the last pass the select kernel appends the
// documents that reach their group's threshold to a pool (its retry: pooled_pass.hpp); the host orders each group's
// records (pooled_call.hpp: hand_out_lists).  Not threaded through
// the pipelined collect paths of cobs_gpu_search_batch (host_api.cpp): no per-query result ever leaves the device.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "engine.hpp"
#include "group_kernels.hpp"
#include "pooled_pass.hpp"

namespace cobs_amd {

struct GroupsWork {
    cobs_gpu_batch* batch[2] = {nullptr, nullptr};
    hipStream_t stream = nullptr;
    hipEvent_t landed[2] = {nullptr, nullptr};                  // a pass's flags (and valid positions) are home
    hipEvent_t ev_acc[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    hipEvent_t ev_sel[2] = {nullptr, nullptr};
    PinnedBuf<uint32_t> h_land[2];          // flag words | K1's valid positions [file][nq] (invalid_bases = skip)
    PinnedBuf<uint8_t> h_args[2];           // files | spans of a pass, as the accumulate kernel reads them
    DevBuf<uint8_t> d_args[2];
    DevBuf<uint32_t> acc_sum, acc_votes;    // [n_groups][local_counts], for the lifetime of a call
    HitPool<GroupRec> hits{"groups: the selection pool", launch_group_zero};
    DevBuf<GroupRange> ranges;
    DevBuf<uint64_t> gthr;
    double ms[3] = {0, 0, 0};               // accumulate | select | host ordering of the last call
    ~GroupsWork() {
        for (auto* b : batch) delete b;
        for (auto& e : landed) if (e) (void)hipEventDestroy(e);
        for (auto& r : ev_acc) for (auto& e : r) if (e) (void)hipEventDestroy(e);
        for (auto& e : ev_sel) if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

void destroy_groups_work(GroupsWork* w) { delete w; }

namespace {

struct Call {
    cobs_gpu_index* ix;
    GroupsWork* w;
    const char* const* queries;
    const size_t* lens;
    const size_t* group_offsets;
    size_t n_groups;
    double read_threshold;
    size_t* bad_query;
    std::vector<uint64_t>* positions;       // [group][file]
    bool count_valid;                       // invalid_bases = skip: P is the sum of K1's valid positions
};

struct Pass { size_t g0, g1; int slot; size_t group0; };

cobs_gpu_status init_work(cobs_gpu_index* ix) {
    if (!ix->groups) ix->groups = new GroupsWork;
    GroupsWork* w = ix->groups;
    if (!w->stream) HIP_TRY(hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking));
    for (auto& e : w->landed) if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& r : w->ev_acc) for (auto& e : r) if (!e) HIP_TRY(hipEventCreate(&e));
    for (auto& e : w->ev_sel) if (!e) HIP_TRY(hipEventCreate(&e));
    for (auto& b : w->batch)
        if (!b)
            if (cobs_gpu_status st = cobs_gpu_batch_create(ix, 0, 0, &b); st != COBS_GPU_OK) return st;
    return COBS_GPU_OK;
}

// upload, K1, K2 and the accumulation of the queries [g0, g1), queued on the call's stream
cobs_gpu_status pass_begin(const Call& c, const Pass& ps) {
    cobs_gpu_index* ix = c.ix;
    GroupsWork* w = c.w;
    cobs_gpu_batch* b = w->batch[ps.slot];
    hipStream_t st = w->stream;
    const size_t n = ps.g1 - ps.g0, nf = ix->parts.size();
    size_t bad = 0;
    // (tuning key hash_stream: K1 would run on the batch's own stream, which does not wait for an upload in flight)
    if (cobs_gpu_status s = set_queries_on(b, c.queries + ps.g0, c.lens + ps.g0, n, st, ix->tune.hash_stream != 0, &bad, ps.g0);
        s != COBS_GPU_OK) {
        if (c.bad_query) *c.bad_query = ps.g0 + bad;
        return s;
    }
    if (cobs_gpu_status s = run_impl(b, c.read_threshold, 0, st, true); s != COBS_GPU_OK) return s;
    ix->host_passes++;
    // the spans of the pass: the part of every group that lies in it.  Enough (group, tile) pairs to fill the device:
    // one span per group, every accumulator cell has one writer.  Few groups (one sample): a group's queries are split
    // over several work-groups that combine with one atomic per cell each.
    const uint64_t nslots = ix->local_counts;
    const uint32_t tiles = (uint32_t)((nslots + group_tile_slots(b->elem_bytes) - 1) / group_tile_slots(b->elem_bytes));
    std::vector<GroupSpan> spans;
    size_t pieces = 0;
    for (size_t g = ps.group0; g < c.n_groups && c.group_offsets[g] < ps.g1; ++g)
        pieces += std::min(c.group_offsets[g + 1], ps.g1) > std::max(c.group_offsets[g], ps.g0) ? 1 : 0;
    const uint64_t kFill = 256, kTarget = 2048;         // compute units | work-groups a split launch aims for
    const uint64_t split = pieces * tiles >= kFill ? 1 : (kTarget + pieces * tiles - 1) / std::max<uint64_t>(pieces * tiles, 1);
    for (size_t g = ps.group0; g < c.n_groups && c.group_offsets[g] < ps.g1; ++g) {
        const size_t q0 = std::max(c.group_offsets[g], ps.g0), q1 = std::min(c.group_offsets[g + 1], ps.g1);
        if (q1 <= q0) continue;
        const size_t step = std::max<size_t>(8, (q1 - q0 + split - 1) / split);
        const uint32_t atomic = q1 - q0 > step ? 1u : 0u;
        for (size_t q = q0; q < q1; q += step)
            spans.push_back(GroupSpan{(uint32_t)g, (uint32_t)(q - ps.g0), (uint32_t)(std::min(q + step, q1) - ps.g0), atomic});
    }
    const size_t files_bytes = round_up(nf * sizeof(GroupFile), 16);
    HIP_TRY(w->h_args[ps.slot].reserve(files_bytes + spans.size() * sizeof(GroupSpan)));
    HIP_TRY(w->d_args[ps.slot].reserve(files_bytes + spans.size() * sizeof(GroupSpan)));
    GroupFile* hf = reinterpret_cast<GroupFile*>(w->h_args[ps.slot].p);
    for (size_t f = 0; f < nf; ++f) {
        const Part& p = ix->parts[f];
        hf[f] = GroupFile{(uint32_t)p.local_offset, (uint32_t)(p.local_offset + p.slot_count),
                          c.read_threshold > 0.0 ? b->work[f].thr.p : nullptr};
    }
    if (!spans.empty()) std::memcpy(w->h_args[ps.slot].p + files_bytes, spans.data(), spans.size() * sizeof(GroupSpan));
    HIP_TRY(hipMemcpyAsync(w->d_args[ps.slot].p, w->h_args[ps.slot].p, files_bytes + spans.size() * sizeof(GroupSpan),
                           hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(w->ev_acc[ps.slot][0], st));
    const size_t per_launch = std::max<size_t>(1, 0x7FFFFFFFull / std::max<uint32_t>(tiles, 1));
    for (size_t s0 = 0; s0 < spans.size(); s0 += per_launch) {
        GroupAccArgs a{};
        a.rows = b->counts.p;
        a.spans = reinterpret_cast<const GroupSpan*>(w->d_args[ps.slot].p + files_bytes) + s0;
        a.files = reinterpret_cast<const GroupFile*>(w->d_args[ps.slot].p);
        a.acc_sum = w->acc_sum.p;
        a.acc_votes = w->acc_votes.p;
        a.nslots = nslots;
        a.nspans = (uint32_t)std::min(per_launch, spans.size() - s0);
        a.nfiles = (uint32_t)nf;
        a.tiles = tiles;
        a.score_bytes = b->elem_bytes;
        HIP_TRY(launch_group_accumulate(a, st));
    }
    HIP_TRY(hipEventRecord(w->ev_acc[ps.slot][1], st));
    // the flag words and, under `skip`, K1's valid positions come home behind the pass
    const size_t nvalid = c.count_valid ? n * nf : 0;
    HIP_TRY(w->h_land[ps.slot].reserve(4 + nvalid));
    HIP_TRY(hipMemcpyAsync(w->h_land[ps.slot].p, b->flags.p, 16, hipMemcpyDeviceToHost, st));
    if (nvalid) HIP_TRY(hipMemcpyAsync(w->h_land[ps.slot].p + 4, b->valid.p, nvalid * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(w->landed[ps.slot], st));
    return COBS_GPU_OK;
}

cobs_gpu_status pass_end(const Call& c, const Pass& ps) {
    cobs_gpu_index* ix = c.ix;
    GroupsWork* w = c.w;
    HIP_TRY(hipEventSynchronize(w->landed[ps.slot]));
    w->batch[ps.slot]->synced = true;
    float ms = 0;
    if (hipEventElapsedTime(&ms, w->ev_acc[ps.slot][0], w->ev_acc[ps.slot][1]) == hipSuccess) w->ms[0] += ms;
    else (void)hipGetLastError();
    const uint32_t* land = w->h_land[ps.slot].p;
    const size_t n = ps.g1 - ps.g0, nf = ix->parts.size();
    if (cobs_gpu_status s = invalid_base_from_flags(land[0], n, c.bad_query, ps.g0); s != COBS_GPU_OK) return s;
    if (c.count_valid) {
        size_t g = ps.group0;
        for (size_t q = ps.g0; q < ps.g1; ++q) {
            while (c.group_offsets[g + 1] <= q) ++g;
            for (size_t f = 0; f < nf; ++f)
                if (ix->parts[f].meta.canonicalize != 0) (*c.positions)[g * nf + f] += land[4 + f * n + (q - ps.g0)];
        }
    }
    return COBS_GPU_OK;
}

cobs_gpu_status search_groups_impl(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                   const size_t* group_offsets, size_t n_groups, double threshold, double read_threshold,
                                   size_t num_results, cobs_gpu_group_hit* hits, size_t cap, size_t* hit_offsets,
                                   uint64_t* positions, size_t* bad_query) {
    if (!ix || !group_offsets || !hit_offsets) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if ((nq && (!queries || !lens)) || (cap && !hits)) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if (group_offsets[0] != 0) return fail(COBS_GPU_ERR_ARG, "group_offsets[0] is not 0");
    for (size_t g = 0; g < n_groups; ++g)
        if (group_offsets[g + 1] < group_offsets[g])
            return fail(COBS_GPU_ERR_ARG, "group_offsets are not ascending (group " + std::to_string(g) + ")");
    if (group_offsets[n_groups] != nq) return fail(COBS_GPU_ERR_ARG, "group_offsets[n_groups] is not the number of queries");
    if (n_groups >= 0xFFFFFFF0ull || nq >= 0xFFFFFFF0ull) return fail(COBS_GPU_ERR_ARG, "too many groups or queries");
    if (ix->hbm_budget != 0 || any_streamed(ix)) return fail(COBS_GPU_ERR_UNSUPPORTED, "groups: not on a handle with an HBM budget (its score rows are added up range by range)");
    if (ix->shard_count > 1) return fail(COBS_GPU_ERR_UNSUPPORTED, "groups: not on one shard of several (a group's totals are per shard)");
    for (size_t g = 0; g <= n_groups; ++g) hit_offsets[g] = 0;
    const size_t nf = ix->parts.size();
    const uint32_t z = ix->findere;
    // everything the host can refuse is refused before anything is launched
    cobs_gpu_status refused = check_query_lengths(ix, queries, lens, nq, z, [&](size_t q) -> cobs_gpu_status {
        if (lens[q] >= 0xFFFFFFF0ull) return fail(COBS_GPU_ERR_QUERY_TOO_LONG, "query too long (query " + std::to_string(q) + ")");
        return COBS_GPU_OK;
    }, bad_query);
    if (refused != COBS_GPU_OK) return refused;
    // P: the positions every group is scored over per file -- T - z summed (the nominal count, which also bounds a sum:
    // they are 32-bit), or under `skip` the valid positions K1 counts
    std::vector<uint64_t> pos(n_groups * nf, 0);
    for (size_t g = 0; g < n_groups; ++g)
        for (size_t f = 0; f < nf; ++f) {
            uint64_t n = 0;
            for (size_t q = group_offsets[g]; q < group_offsets[g + 1]; ++q) n += (uint64_t)lens[q] - ix->parts[f].meta.term_size + 1 - z;
            if (n >= (1ull << 32))
                return fail(COBS_GPU_ERR_ARG, "group " + std::to_string(g) + " is too large: its scores in file " + std::to_string(f) +
                            " could reach 2^32 (sums are 32-bit; split the group and add the parts)");
            pos[g * nf + f] = n;
        }
    const bool count_valid = ix->invalid_bases == COBS_GPU_INVALID_SKIP;
    if (count_valid)
        for (size_t g = 0; g < n_groups; ++g)
            for (size_t f = 0; f < nf; ++f)
                if (ix->parts[f].meta.canonicalize != 0) pos[g * nf + f] = 0;
    if (n_groups == 0) return COBS_GPU_OK;

    HIP_TRY(hipSetDevice(ix->device));
    if (cobs_gpu_status st = init_work(ix); st != COBS_GPU_OK) return st;
    GroupsWork* w = ix->groups;
    w->ms[0] = w->ms[1] = w->ms[2] = 0;
    const uint64_t nslots = ix->local_counts;
    if (n_groups * nslots >= (1ull << 40) || w->acc_sum.reserve((size_t)(n_groups * nslots)) != hipSuccess ||
        w->acc_votes.reserve((size_t)(n_groups * nslots)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(COBS_GPU_ERR_CAPACITY, "no room for the accumulators of " + std::to_string(n_groups) + " groups; use fewer groups per call");
    }
    hipStream_t st = w->stream;
    HIP_TRY(launch_group_zero(w->acc_sum.p, n_groups * nslots, st));
    HIP_TRY(launch_group_zero(w->acc_votes.p, n_groups * nslots, st));

    const Call call{ix, w, queries, lens, group_offsets, n_groups, read_threshold, bad_query, &pos, count_valid};
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
    if (positions) std::memcpy(positions, pos.data(), pos.size() * sizeof(uint64_t));

    // ---- selection: real documents whose sum reaches gthr = min_key(threshold, P) (pooled_call.hpp; 0: all of them).  The
    // accumulators stay where they are while the pool takes its retry (pooled_pass.hpp)
    const std::vector<GroupRange> ranges = real_ranges<GroupRange>(*ix);
    std::vector<uint64_t> gthr(nf * n_groups, 0);
    for (size_t f = 0; f < nf; ++f)
        for (size_t g = 0; g < n_groups; ++g) gthr[f * n_groups + g] = min_key<uint64_t>(threshold, pos[g * nf + f]);
    std::vector<GroupRec> recs;
    if (!ranges.empty()) {
        HIP_TRY(w->ranges.reserve(ranges.size()));
        HIP_TRY(w->gthr.reserve(gthr.size()));
        HIP_TRY(hipMemcpy(w->ranges.p, ranges.data(), ranges.size() * sizeof(GroupRange), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(w->gthr.p, gthr.data(), gthr.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        uint64_t fill = 0;
        cobs_gpu_status s = select_through(w->hits, first_pool_cap(ix->tune.hit_cap, threshold, real_documents(*ix), n_groups), st, w->ev_sel, &w->ms[1],
            [](uint64_t cap) {
                return fail(COBS_GPU_ERR_CAPACITY, "no room for " + std::to_string(cap) + " group records; raise the threshold or use fewer groups per call");
            },
            [&](uint64_t pool_cap) {
                GroupSelArgs sa{};
                sa.acc_sum = w->acc_sum.p;
                sa.acc_votes = w->acc_votes.p;
                sa.ranges = w->ranges.p;
                sa.gthr = w->gthr.p;
                sa.pool = w->hits.pool.p;
                sa.fill = w->hits.fill.p;
                sa.nslots = nslots;
                sa.cap = pool_cap;
                sa.n_groups = (uint32_t)n_groups;
                sa.nranges = (uint32_t)ranges.size();
                return launch_group_select(sa, st);
            }, &fill);
        if (s != COBS_GPU_OK) return s;
        if (cobs_gpu_status c = append_records(recs, w->hits.pool.p, fill); c != COBS_GPU_OK) return c;
    }
    // ---- ordering: per group by sum descending, then (file, document) ascending; num_results cuts the list
    const double t0 = now_s();
    const cobs_gpu_status handed = hand_out_lists(recs, n_groups, [](const GroupRec& r) { return r.group; },
        [](const GroupRec& a, const GroupRec& b) {
            if (a.sum != b.sum) return a.sum > b.sum;
            if (a.file != b.file) return a.file < b.file;
            return a.doc < b.doc;
        }, num_results, hits, cap, hit_offsets, "n_groups",
        [](const GroupRec& r) { return cobs_gpu_group_hit{r.file, r.doc, r.sum, r.votes}; });
    w->ms[2] = (now_s() - t0) * 1e3;
    return handed;
}

}  // namespace
}  // namespace cobs_amd

using namespace cobs_amd;

extern "C" {

cobs_gpu_status cobs_gpu_search_groups(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                       const size_t* group_offsets, size_t n_groups, double threshold, double read_threshold,
                                       size_t num_results, cobs_gpu_group_hit* hits, size_t cap, size_t* hit_offsets,
                                       uint64_t* positions, size_t* bad_query) {
    return guarded([&]() {
        return search_groups_impl(ix, queries, lens, nq, group_offsets, n_groups, threshold, read_threshold, num_results, hits,
                                  cap, hit_offsets, positions, bad_query);
    });
}

cobs_gpu_status cobs_gpu_groups_ms(cobs_gpu_index* ix, double out[3]) {
    if (!ix || !out) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    out[0] = out[1] = out[2] = 0;
    if (GroupsWork* w = ix->groups) {
        out[0] = w->ms[0];
        out[1] = w->ms[1];
        out[2] = w->ms[2];
    }
    return COBS_GPU_OK;
}

}  // extern "C"
