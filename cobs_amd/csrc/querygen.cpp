// cobs_amd/csrc/querygen.cpp -- `cobs generate-queries` (reference src/cobs.cpp:734-959) with the
// document term scan on the GPU.  The host draws the positive term indices and the negative
// candidates, the device fills a table of the candidates' terms (querygen_kernels.hip), and the
// documents stream through the staging sets of construction (staging.hpp): host threads parse
// the next batch while the GPU numbers the terms of the previous one, copies out the drawn
// positives and, with -N, probes every ACGT term.  Afterwards the host drops the candidates that
// were hit, pads the positives, shuffles and writes the reference's format.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <deque>
#include <set>
#include <string>
#include <vector>

#include "documents.hpp"
#include "engine.hpp"
#include "querygen_kernels.hpp"
#include "staging.hpp"

using namespace cobs_amd;

struct cobs_gpu_query_set {
    struct Entry {
        std::string text;
        uint64_t doc_index, term_index;
    };
    std::vector<Entry> entries;
    cobs_gpu_querygen_stats stats{};
};

namespace {

// draw i of seed S: the splitmix64 finaliser of S + i * 0x9E3779B97F4A7C15 (build_kernels.hip's mix64)
struct Draws {
    uint64_t seed, i = 0;
    explicit Draws(uint64_t s) : seed(s) {}
    uint64_t next() {
        uint64_t z = seed + (i++) * 0x9E3779B97F4A7C15ULL;
        z += 0x9E3779B97F4A7C15ULL;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        return z ^ (z >> 31);
    }
    char base() { return "ACGT"[next() % 4]; }
};

struct Params {
    uint32_t k = 31;
    uint64_t num_positive = 0, num_negative = 0, size = 0, seed = 0;
    bool true_negatives = false, canonical = false;
    int device = -1;
    uint64_t text_batch = 0;
};

struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

cobs_gpu_status generate(const std::vector<DocEntry>& list, const Params& pr, cobs_gpu_query_set& out) {
    const uint32_t k = pr.k;
    const size_t ndocs = list.size();
    // ---- the draws that need no document: positive indices, negative candidates ----------------------
    std::vector<uint64_t> prefix(ndocs + 1, 0);          // terms before document d, as num_terms counts them
    for (size_t d = 0; d < ndocs; ++d) prefix[d + 1] = prefix[d] + num_terms(list[d], k);
    const uint64_t total_terms = prefix[ndocs];
    if (pr.num_positive > total_terms)
        return cobs_gpu_set_error(COBS_GPU_ERR_ARG, "more positives requested than the documents hold terms");
    const uint64_t size = std::max<uint64_t>(pr.size, k);
    const uint64_t num_cand = (3 * pr.num_negative + 1) / 2;            // ceil(1.5 n)
    const uint64_t cand_terms = size - k + 1;
    const bool probe = pr.true_negatives && num_cand > 0;
    if (probe && (k > 32 * kQgMaxWords || num_cand * cand_terms >= 0xFFFFFFFFull))
        return cobs_gpu_set_error(COBS_GPU_ERR_UNSUPPORTED, "-N supports term sizes up to 256 and fewer than 2^32 negative terms");
    cobs_gpu_status st = pick_device(pr.device);
    if (st != COBS_GPU_OK) return st;

    Draws rng(pr.seed);
    std::vector<uint64_t> positives;
    {
        std::set<uint64_t> chosen;
        while (chosen.size() < pr.num_positive) chosen.insert(rng.next() % total_terms);
        positives.assign(chosen.begin(), chosen.end());                  // ascending
    }
    std::string cand((size_t)(num_cand * size), '\0');
    for (char& c : cand) c = rng.base();

    // ---- which documents are read: all of them with -N, else those holding a positive ---------------
    std::vector<size_t> visit;
    std::vector<uint64_t> vis_pos_off{0}, pos_local(positives.size()), pos_doc(positives.size());
    {
        size_t p = 0;
        for (size_t d = 0; d < ndocs; ++d) {
            const size_t p0 = p;
            for (; p < positives.size() && positives[p] < prefix[d + 1]; ++p) {
                pos_local[p] = positives[p] - prefix[d];
                pos_doc[p] = d;
            }
            if (p > p0 || pr.true_negatives) {
                visit.push_back(d);
                vis_pos_off.push_back(p);
            }
        }
    }
    if (visit.size() >= kBuildRawStretch - 1) return cobs_gpu_set_error(COBS_GPU_ERR_UNSUPPORTED, "too many documents");

    // ---- device state -------------------------------------------------------------------------------
    const uint64_t np = positives.size();
    DevBuf<uint64_t> d_vis_off, d_pos_local, d_keys, d_blk;
    DevBuf<unsigned long long> d_doc_base, d_probed;
    DevBuf<uint8_t> d_pos_text, d_pos_hit, d_found, d_cand;
    DevBuf<uint32_t> d_vals;
    StagingContext ctx;                                 // declared last: its streams drain before the buffers go
    if ((st = ctx.init(true)) != COBS_GPU_OK) return st;
    hipStream_t stream = ctx.stream;
    BUILD_TRY(d_vis_off.reserve(vis_pos_off.size()));
    BUILD_TRY(d_pos_local.reserve(std::max<uint64_t>(np, 1)));
    BUILD_TRY(d_pos_text.reserve((size_t)std::max<uint64_t>(np * k, 1)));
    BUILD_TRY(d_pos_hit.reserve((size_t)std::max<uint64_t>(np, 1)));
    BUILD_TRY(d_found.reserve((size_t)std::max<uint64_t>(num_cand, 1)));
    BUILD_TRY(d_probed.reserve(1));
    BUILD_TRY(hipMemcpyAsync(d_vis_off.p, vis_pos_off.data(), vis_pos_off.size() * 8, hipMemcpyHostToDevice, stream));
    if (np) BUILD_TRY(hipMemcpyAsync(d_pos_local.p, pos_local.data(), (size_t)np * 8, hipMemcpyHostToDevice, stream));
    BUILD_TRY(hipMemsetAsync(d_pos_hit.p, 0, (size_t)std::max<uint64_t>(np, 1), stream));
    BUILD_TRY(hipMemsetAsync(d_found.p, 0, (size_t)std::max<uint64_t>(num_cand, 1), stream));
    BUILD_TRY(hipMemsetAsync(d_probed.p, 0, 8, stream));
    std::deque<EventPair> timing;                       // (a deque: the pairs never move)
    auto timed = [&]() -> hipError_t {
        timing.emplace_back();
        hipError_t e = hipEventCreate(&timing.back().a);
        if (e == hipSuccess) e = hipEventCreate(&timing.back().b);
        if (e == hipSuccess) e = hipEventRecord(timing.back().a, stream);
        return e;
    };
    QgTable table{};
    if (probe) {
        const uint64_t entries = num_cand * cand_terms;
        uint64_t cap = 1;
        while (cap < 2 * entries) cap <<= 1;
        table.words = (k + 31) / 32;
        table.cand_terms = (uint32_t)cand_terms;
        table.mask = cap - 1;
        BUILD_TRY(d_keys.reserve((size_t)(cap * table.words)));
        BUILD_TRY(d_vals.reserve((size_t)cap));
        BUILD_TRY(d_cand.reserve(cand.size()));
        table.keys = d_keys.p;
        table.vals = d_vals.p;
        BUILD_TRY(hipMemsetAsync(d_vals.p, 0, (size_t)cap * 4, stream));
        BUILD_TRY(hipMemcpyAsync(d_cand.p, cand.data(), cand.size(), hipMemcpyHostToDevice, stream));
        QgInsertArgs ia;
        ia.cand_text = d_cand.p;
        ia.num_cand = num_cand;
        ia.size = size;
        ia.term_size = k;
        ia.canonical = pr.canonical ? 1u : 0u;
        ia.table = table;
        BUILD_TRY(timed());
        BUILD_TRY(launch_qg_insert(ia, stream));
        BUILD_TRY(hipEventRecord(timing.back().b, stream));
    }
    // the pageable uploads above have been read before the loop's staging sets are reused
    BUILD_TRY(hipStreamSynchronize(stream));

    // ---- the documents, batch by batch --------------------------------------------------------------
    const uint64_t text_batch = pr.text_batch ? pr.text_batch : kTextBatchBytes;
    ListSource src(list);
    StagedBatch batch;
    StageTimes tm;
    int cur = 0;
    for (size_t b0 = 0; b0 < visit.size();) {
        if ((st = stage_batch(ctx, cur, src, visit.data(), b0, visit.size(), k, text_batch, batch, tm)) != COBS_GPU_OK)
            return st;
        for (const Slot& sl : batch.slots) out.stats.text_bytes += sl.used;
        out.stats.documents_read += batch.b1 - batch.b0;
        if (batch.nsegs && batch.total) {
            const uint64_t blocks = (batch.total + 255) / 256, nd = batch.b1 - batch.b0;
            if (blocks > d_blk.cap || nd > d_doc_base.cap) {       // the previous batches' kernels still read them
                BUILD_TRY(hipStreamSynchronize(stream));
                BUILD_TRY(d_blk.reserve((size_t)std::max<uint64_t>(blocks, d_blk.cap)));
                BUILD_TRY(d_doc_base.reserve((size_t)std::max<uint64_t>(nd, d_doc_base.cap)));
            }
            QgBatchArgs a;
            a.text = batch.stage->d_text.p;
            a.seg_off = batch.stage->d_off.p;
            a.seg_col = batch.stage->d_col.p;
            a.total = batch.total;
            a.nsegs = (uint32_t)batch.nsegs;
            a.term_size = k;
            a.col_base = (uint32_t)batch.b0;
            a.ndocs = (uint32_t)nd;
            a.blk_cnt = d_blk.p;
            a.doc_base = d_doc_base.p;
            a.vis_pos_off = d_vis_off.p;
            a.pos_local = d_pos_local.p;
            a.pos_text = d_pos_text.p;
            a.pos_hit = d_pos_hit.p;
            a.probe = probe ? 1u : 0u;
            a.canonical = pr.canonical ? 1u : 0u;
            a.table = table;
            a.found = d_found.p;
            a.probed = d_probed.p;
            BUILD_TRY(timed());
            BUILD_TRY(launch_qg_batch(a, stream));
            BUILD_TRY(hipEventRecord(timing.back().b, stream));
            if ((st = finish_batch(ctx, batch)) != COBS_GPU_OK) return st;
        }
        cur = (cur + 1) % kStages;
        b0 = batch.b1;
    }
    BUILD_TRY(hipStreamSynchronize(stream));
    for (const EventPair& e : timing) {
        float ms = 0.f;
        BUILD_TRY(hipEventElapsedTime(&ms, e.a, e.b));
        out.stats.kernel_ms += ms;
    }
    std::string pos_text((size_t)(np * k), '\0');
    std::vector<uint8_t> pos_hit((size_t)np), found((size_t)num_cand);
    unsigned long long probed = 0;
    if (np) {
        BUILD_TRY(hipMemcpy(&pos_text[0], d_pos_text.p, pos_text.size(), hipMemcpyDeviceToHost));
        BUILD_TRY(hipMemcpy(pos_hit.data(), d_pos_hit.p, pos_hit.size(), hipMemcpyDeviceToHost));
    }
    if (probe) BUILD_TRY(hipMemcpy(found.data(), d_found.p, found.size(), hipMemcpyDeviceToHost));
    BUILD_TRY(hipMemcpy(&probed, d_probed.p, 8, hipMemcpyDeviceToHost));
    out.stats.terms_probed = probed;
    for (uint64_t p = 0; p < np; ++p)
        if (!pos_hit[p]) {
            const DocEntry& e = list[pos_doc[p]];
            return cobs_gpu_set_error(COBS_GPU_ERR_FORMAT, (e.path + ": holds fewer terms than its num_terms (" +
                                                            std::to_string(num_terms(e, k)) + ")").c_str());
        }

    // ---- the reference's negatives[i].clear(), padding, assembly, shuffle -----------------------------
    std::vector<uint64_t> survivors;
    for (uint64_t c = 0; c < num_cand && survivors.size() < pr.num_negative; ++c) {
        if (found[c]) continue;
        survivors.push_back(c);
    }
    for (uint64_t c = 0; c < num_cand; ++c) out.stats.negatives_removed += found[c] ? 1 : 0;
    if (survivors.size() < pr.num_negative)
        return cobs_gpu_set_error(COBS_GPU_ERR_ARG, "not enough true negatives left (try another seed)");
    std::vector<cobs_gpu_query_set::Entry>& q = out.entries;
    q.reserve((size_t)(np + pr.num_negative));
    for (uint64_t p = 0; p < np; ++p) {
        std::string t = pos_text.substr((size_t)(p * k), k);
        if (size > k) {
            const uint64_t pad = size - k, front = rng.next() % pad;
            std::string f((size_t)front, '\0'), b((size_t)(pad - front), '\0');
            for (char& c : f) c = rng.base();
            for (char& c : b) c = rng.base();
            t = f + t + b;
        }
        q.push_back({std::move(t), pos_doc[p], pos_local[p]});
    }
    for (uint64_t c : survivors) q.push_back({cand.substr((size_t)(c * size), (size_t)size), UINT64_MAX, 0});
    for (size_t i = q.size(); i > 1; --i) {
        const size_t j = (size_t)(rng.next() % i);
        std::swap(q[i - 1], q[j]);
    }
    return COBS_GPU_OK;
}

}  // namespace

extern "C" {

cobs_gpu_status cobs_gpu_generate_queries(const cobs_gpu_doclist* dl, const cobs_gpu_querygen_params* params,
                                          cobs_gpu_query_set** out) {
    if (!out) return cobs_gpu_set_error(COBS_GPU_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!dl || !params || dl->list.empty()) return cobs_gpu_set_error(COBS_GPU_ERR_ARG, "NULL argument or no documents");
    if (params->struct_size < sizeof(cobs_gpu_querygen_params))
        return cobs_gpu_set_error(COBS_GPU_ERR_ARG, "cobs_gpu_querygen_params.struct_size is too small");
    Params pr;
    pr.k = params->term_size;
    pr.num_positive = params->num_positive;
    pr.num_negative = params->num_negative;
    pr.size = params->size;
    pr.seed = params->seed;
    pr.true_negatives = params->true_negatives != 0;
    pr.canonical = params->canonical != 0;
    pr.device = params->device;
    pr.text_batch = params->text_batch_bytes;
    if (pr.k == 0 || params->true_negatives > 1 || params->canonical > 1)
        return cobs_gpu_set_error(COBS_GPU_ERR_ARG, "bad term_size / true_negatives / canonical");
    return guarded([&]() -> cobs_gpu_status {
        std::unique_ptr<cobs_gpu_query_set> set(new cobs_gpu_query_set);
        cobs_gpu_status st = generate(dl->list, pr, *set);
        if (st != COBS_GPU_OK) return st;
        *out = set.release();
        return COBS_GPU_OK;
    });
}

size_t cobs_gpu_query_set_size(const cobs_gpu_query_set* set) { return set ? set->entries.size() : 0; }

cobs_gpu_status cobs_gpu_query_set_entry(const cobs_gpu_query_set* set, size_t i, const char** text, size_t* len,
                                         uint64_t* doc_index, uint64_t* term_index) {
    if (!set || i >= set->entries.size()) return cobs_gpu_set_error(COBS_GPU_ERR_ARG, "bad argument");
    const cobs_gpu_query_set::Entry& e = set->entries[i];
    if (text) *text = e.text.c_str();
    if (len) *len = e.text.size();
    if (doc_index) *doc_index = e.doc_index;
    if (term_index) *term_index = e.term_index;
    return COBS_GPU_OK;
}

cobs_gpu_status cobs_gpu_query_set_write(const cobs_gpu_query_set* set, const cobs_gpu_doclist* dl, const char* path) {
    if (!set || !dl) return cobs_gpu_set_error(COBS_GPU_ERR_ARG, "NULL argument");
    return guarded([&]() -> cobs_gpu_status {
        std::string s;
        uint64_t negative_count = 0;
        for (const cobs_gpu_query_set::Entry& e : set->entries) {
            if (e.doc_index != UINT64_MAX) {
                if (e.doc_index >= dl->list.size()) return cobs_gpu_set_error(COBS_GPU_ERR_ARG, "the set belongs to another list");
                s += ">doc:" + std::to_string(e.doc_index) + ":term:" + std::to_string(e.term_index) + ":" +
                     dl->list[e.doc_index].name + "\n";
            } else {
                s += ">negative" + std::to_string(negative_count++) + "\n";
            }
            s += e.text;
            s += '\n';
        }
        FILE* f = path ? std::fopen(path, "wb") : stdout;
        if (!f) return cobs_gpu_set_error(COBS_GPU_ERR_OPEN, (std::string("could not create ") + path).c_str());
        const bool ok = s.empty() || std::fwrite(s.data(), 1, s.size(), f) == s.size();
        const bool closed = path ? std::fclose(f) == 0 : std::fflush(f) == 0;
        if (!ok || !closed) return cobs_gpu_set_error(COBS_GPU_ERR_OPEN, "short write");
        return COBS_GPU_OK;
    });
}

cobs_gpu_status cobs_gpu_query_set_stats(const cobs_gpu_query_set* set, cobs_gpu_querygen_stats* out) {
    if (!set || !out) return cobs_gpu_set_error(COBS_GPU_ERR_ARG, "NULL argument");
    *out = set->stats;
    return COBS_GPU_OK;
}

void cobs_gpu_query_set_free(cobs_gpu_query_set* set) { delete set; }

}  // extern "C"
