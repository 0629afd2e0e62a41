// cobs_amd/csrc/similarity.cpp -- cobs_gpu_doc_shared_bits: in how many rows a reference document and every document of
// its sub-index both have their bit set, counted on the device where the rows are (similarity_kernels.hip), and
// cobs_gpu_jaccard_estimate, the Bloom-filter estimate of Jaccard index and containment from those counts (host
// arithmetic).  The references of one sub-index are cut into panels of kSimRefs; a panel is one extraction of the
// references' bits per row (ref_rows_kernel) and one sweep over the sub-index's resident rows (shared_count_kernel),
// found as fill.cpp finds them: Chunk::pages, pitch, the zero row never read.  Nothing is cached: the answer of a panel
// goes to the caller's rows and the device cells are reused by the next panel.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <numeric>
#include <string>
#include <vector>

#include "engine.hpp"
#include "similarity_kernels.hpp"

namespace cobs_amd {

struct SimilarityWork {
    DevBuf<uint8_t> d_refw;                     // [rows of the sub-index] the panel's reference bits per row
    DevBuf<unsigned long long> d_out;           // [kSimRefs][slots of the sub-index] cells of one panel
    std::vector<uint64_t> h_out;
    hipStream_t stream = nullptr;
    PhaseEvents<3> ev;                          // before ref_rows | before the zeroing and the sweep | after
    SimTune tune;                               // COBS_GPU_SIM_GROUPS / COBS_GPU_SIM_SIDE, read once per handle (tests)
    bool tune_read = false;
    double ms[2] = {0, 0};                      // extract | sweep
    uint64_t bytes_read = 0, sweeps = 0;
    ~SimilarityWork() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

void destroy_similarity_work(SimilarityWork* w) { delete w; }

namespace {

// the resident page that holds score slot `doc` of the part, with its chunk
struct PageRef { const Chunk* chunk = nullptr; const PageDev* page = nullptr; };

PageRef find_page(const Part& p, uint64_t doc) {
    for (const Chunk& c : p.chunks) {
        if (!c.d_data) continue;
        for (const PageDev& pd : c.pages)
            if (doc >= pd.doc0 && doc < (uint64_t)pd.doc0 + (uint64_t)pd.valid_bytes * 8u) return {&c, &pd};
    }
    return {};
}

cobs_gpu_status init_work(cobs_gpu_index* ix) {
    if (!ix->similarity) ix->similarity = new SimilarityWork;
    SimilarityWork* w = ix->similarity;
    if (!w->tune_read) {
        if (const char* e = getenv("COBS_GPU_SIM_GROUPS")) w->tune.groups = (uint32_t)std::strtoul(e, nullptr, 0);
        if (const char* e = getenv("COBS_GPU_SIM_SIDE")) w->tune.max_side = (uint32_t)std::strtoul(e, nullptr, 0);
        w->tune_read = true;
    }
    if (!w->stream) HIP_TRY(hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking));
    HIP_TRY(w->ev.create());
    return COBS_GPU_OK;
}

// one panel: refs[order[k0 .. k1)] lie in page pr; their rows of cells go to shared + offsets[that ref]
cobs_gpu_status run_panel(cobs_gpu_index* ix, const PageRef& pr, const uint32_t* refs, const std::vector<size_t>& order, size_t k0,
                          size_t k1, const std::vector<uint64_t>& offsets, uint64_t* shared) {
    SimilarityWork* w = ix->similarity;
    const PageDev& pd = *pr.page;
    const Chunk& c = *pr.chunk;
    const uint32_t n = (uint32_t)(k1 - k0);
    const uint64_t nslots = (uint64_t)pd.valid_bytes * 8u;
    hipStream_t st = w->stream;
    HIP_TRY(w->d_refw.reserve((size_t)pd.sig));
    HIP_TRY(w->d_out.reserve((size_t)(nslots * kSimRefs)));
    RefRowsArgs ra{};
    ra.data = c.d_data;
    ra.base = pd.base;
    ra.sig = pd.sig;
    ra.refw = w->d_refw.p;
    ra.nrefs = n;
    ra.pitch = c.pitch;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t s = refs[order[k0 + j]] - pd.doc0;
        ra.ref[j] = {s / 8u, s % 8u};
    }
    SimArgs sa{};
    sa.data = c.d_data;
    sa.refw = w->d_refw.p;
    sa.out = w->d_out.p;
    sa.base = pd.base;
    sa.sig = pd.sig;
    sa.nslots = (uint32_t)nslots;
    sa.valid_bytes = pd.valid_bytes;
    sa.nrefs = n;
    sa.pitch = c.pitch;
    HIP_TRY(w->ev.mark(0, st));
    HIP_TRY(launch_ref_rows(ra, st));
    HIP_TRY(w->ev.mark(1, st));
    HIP_TRY(launch_sim_zero(w->d_out.p, nslots * n, st));
    HIP_TRY(launch_shared_count(sa, st, w->tune));
    HIP_TRY(w->ev.mark(2, st));
    w->h_out.resize((size_t)(nslots * n));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit cells");
    HIP_TRY(hipMemcpyAsync(w->h_out.data(), w->d_out.p, (size_t)(nslots * n) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    (void)w->ev.add_elapsed(w->ms);
    w->bytes_read += pd.sig * (uint64_t)pd.valid_bytes;
    ++w->sweeps;
    for (uint32_t j = 0; j < n; ++j)
        std::copy_n(w->h_out.data() + (size_t)j * nslots, (size_t)nslots, shared + offsets[order[k0 + j]]);
    return COBS_GPU_OK;
}

}  // namespace

}  // namespace cobs_amd

using namespace cobs_amd;

extern "C" {

cobs_gpu_status cobs_gpu_doc_shared_bits(cobs_gpu_index* ix, size_t file_no, const uint32_t* refs, size_t n_refs, uint64_t* offsets,
                                         uint64_t* shared, size_t cap, size_t* needed) {
    if (needed) *needed = 0;
    if (!ix) return fail(COBS_GPU_ERR_ARG, "NULL handle");
    if (file_no >= ix->parts.size()) return fail(COBS_GPU_ERR_ARG, "file number out of range");
    if (n_refs && !refs) return fail(COBS_GPU_ERR_ARG, "refs is NULL");
    return guarded([&]() -> cobs_gpu_status {
        const Part& p = ix->parts[file_no];
        const uint64_t num_docs = p.meta.doc_names.size();
        for (size_t i = 0; i < n_refs; ++i)
            if (refs[i] >= num_docs)
                return fail(COBS_GPU_ERR_ARG, "doc_shared_bits: reference " + std::to_string(refs[i]) + " is not a document of the file (" +
                                                  std::to_string(num_docs) + " documents)");
        if (ix->hbm_budget != 0 || any_streamed(ix))
            return fail(COBS_GPU_ERR_UNSUPPORTED, "doc_shared_bits: not on a handle opened with an HBM budget (its rows are not all resident)");
        if (ix->shard_count > 1)
            return fail(COBS_GPU_ERR_UNSUPPORTED, "doc_shared_bits: not on one shard of several (its columns are not all resident)");
        if (offsets) offsets[0] = 0;
        if (n_refs == 0) return COBS_GPU_OK;
        // the sub-index of every reference and where its row of cells begins
        std::vector<PageRef> pages(n_refs);
        std::vector<uint64_t> offs(n_refs + 1, 0);
        for (size_t i = 0; i < n_refs; ++i) {
            pages[i] = find_page(p, refs[i]);
            if (!pages[i].page) return fail(COBS_GPU_ERR_UNSUPPORTED, "doc_shared_bits: the sub-index of a reference is not resident");
            offs[i + 1] = offs[i] + (uint64_t)pages[i].page->valid_bytes * 8u;
        }
        if (offsets) std::copy(offs.begin(), offs.end(), offsets);
        const uint64_t total = offs[n_refs];
        if (needed) *needed = (size_t)total;
        if (!shared && cap == 0) return COBS_GPU_OK;       // the sizing call
        if (!shared || cap < total) return fail(COBS_GPU_ERR_CAPACITY, "doc_shared_bits: " + std::to_string(total) + " entries needed");
        HIP_TRY(hipSetDevice(ix->device));
        if (cobs_gpu_status s = init_work(ix); s != COBS_GPU_OK) return s;
        // references of one sub-index side by side, neighbours in the row first (their bits share cache lines in ref_rows_kernel)
        std::vector<size_t> order(n_refs);
        std::iota(order.begin(), order.end(), (size_t)0);
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return refs[a] < refs[b]; });
        for (size_t k0 = 0; k0 < n_refs;) {
            const PageDev* page = pages[order[k0]].page;
            size_t k1 = k0 + 1;
            while (k1 < n_refs && k1 - k0 < (size_t)kSimRefs && pages[order[k1]].page == page) ++k1;
            if (cobs_gpu_status s = run_panel(ix, pages[order[k0]], refs, order, k0, k1, offs, shared); s != COBS_GPU_OK) return s;
            k0 = k1;
        }
        return COBS_GPU_OK;
    });
}

cobs_gpu_status cobs_gpu_jaccard_estimate(uint64_t sig, uint32_t num_hashes, uint64_t bits_a, uint64_t bits_b, uint64_t shared_ab,
                                          double out[5]) {
    if (!out) return fail(COBS_GPU_ERR_ARG, "out is NULL");
    if (sig == 0 || num_hashes == 0) return fail(COBS_GPU_ERR_ARG, "jaccard_estimate: signature size and hash count must not be 0");
    if (bits_a > sig || bits_b > sig) return fail(COBS_GPU_ERR_ARG, "jaccard_estimate: more bits than rows");
    if (shared_ab > std::min(bits_a, bits_b)) return fail(COBS_GPU_ERR_ARG, "jaccard_estimate: more shared bits than either document has");
    const double S = (double)sig, H = (double)num_hashes;
    const uint64_t t_or_i = bits_a + bits_b - shared_ab;        // <= sig: a + b - c <= S whenever the counts come from one sub-index ...
    if (t_or_i > sig) return fail(COBS_GPU_ERR_ARG, "jaccard_estimate: more bits in the union than rows");   // ... and is refused otherwise
    const double t_or = (double)t_or_i;
    out[0] = t_or_i ? (double)shared_ab / t_or : 0.0;
    if (t_or_i == sig) {                                        // a saturated filter estimates nothing
        out[1] = out[2] = out[3] = out[4] = std::numeric_limits<double>::quiet_NaN();
        return COBS_GPU_OK;
    }
    auto n = [&](double t) { return -(S / H) * std::log1p(-t / S); };
    const double na = n((double)bits_a), nb = n((double)bits_b), nu = n(t_or);
    const double inter = std::max(0.0, na + nb - nu);
    out[1] = nu > 0.0 ? inter / nu : 0.0;
    out[2] = na > 0.0 ? std::min(1.0, inter / na) : 0.0;
    out[3] = nb > 0.0 ? std::min(1.0, inter / nb) : 0.0;
    out[4] = inter;
    return COBS_GPU_OK;
}

cobs_gpu_status cobs_gpu_similarity_ms(cobs_gpu_index* ix, double out[4]) {
    if (!ix || !out) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (SimilarityWork* w = ix->similarity) {
        out[0] = w->ms[0];
        out[1] = w->ms[1];
        out[2] = (double)w->bytes_read;
        out[3] = (double)w->sweeps;
        w->ms[0] = w->ms[1] = 0;
        w->bytes_read = w->sweeps = 0;
    }
    return COBS_GPU_OK;
}

}  // extern "C"
