// cobs_amd/csrc/staging.hpp -- the document batch producer shared by index construction
// (build.cpp) and generate-queries (querygen.cpp): where documents come from, the pooled pinned
// staging sets, the parser threads, and stage_batch(), which parses the next window of documents
// into a staging set, writes its stretch table and uploads both.  The consumer launches its
// kernels on ctx.stream (already ordered after the upload) and then calls finish_batch().
#pragma once

#include <hip/hip_runtime_api.h>

#include <condition_variable>
#include <cstdint>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "documents.hpp"
#include "engine.hpp"

__attribute__((visibility("hidden"))) cobs_gpu_status cobs_gpu_set_error(cobs_gpu_status st, const char* msg);   // engine.cpp

// a failed HIP call -> the library's error (COBS_GPU_ERR_NO_DEVICE when there is no usable device)
#define BUILD_TRY(expr)                                                             \
    do {                                                                            \
        hipError_t _e = (expr);                                                     \
        if (_e != hipSuccess) {                                                     \
            const bool nodev = _e == hipErrorNoDevice || _e == hipErrorInvalidDevice; \
            std::string m = std::string(#expr) + ": " + hipGetErrorString(_e);      \
            (void)hipGetLastError();                                                \
            return cobs_gpu_set_error(nodev ? COBS_GPU_ERR_NO_DEVICE : COBS_GPU_ERR_HIP, m.c_str()); \
        }                                                                           \
    } while (0)

namespace cobs_amd {

// the device of a construction-side call (-1 = the current one); COBS_GPU_ERR_NO_DEVICE without a GPU
cobs_gpu_status pick_device(int device);

// ---- where the documents come from ---------------------------------------------------------------
struct DocSource {
    virtual ~DocSource() = default;
    virtual size_t size() const = 0;
    virtual const char* name(size_t d) const = 0;
    virtual uint64_t terms(size_t d, uint32_t k) const = 0;          // what sizes a signature
    virtual uint64_t text_bound(size_t d, uint32_t k) const = 0;     // upper bound of the document's term text
    virtual bool parses() const = 0;                                 // loading reads and parses files
    // the document's term text into `out` (a span of the staging buffer), its stretches into `segs`
    virtual cobs_gpu_status load(size_t d, uint32_t k, TermSink& out, std::vector<TermSeg>& segs,
                                 std::string& scratch) const = 0;
};

// a document list (cobs_gpu_build_*_list, cobs_gpu_generate_queries)
struct ListSource final : DocSource {
    const std::vector<DocEntry>& list;
    explicit ListSource(const std::vector<DocEntry>& l) : list(l) {}
    size_t size() const override { return list.size(); }
    const char* name(size_t d) const override { return list[d].name.c_str(); }
    uint64_t terms(size_t d, uint32_t k) const override { return num_terms(list[d], k); }
    uint64_t text_bound(size_t d, uint32_t k) const override { return term_text_bound(list[d], k); }
    bool parses() const override { return true; }
    cobs_gpu_status load(size_t d, uint32_t k, TermSink& out, std::vector<TermSeg>& segs, std::string& scratch) const override {
        return load_terms(list[d], k, out, segs, scratch);
    }
};

// Documents reach the device in batches of at most this many bytes of term text (the reference
// batches documents by a memory budget too: classic_index.cpp:565-659 builds one small index per
// batch and interleaves them afterwards; here every batch sets its bits straight at the documents'
// final columns of the one matrix in HBM, so there is nothing to combine).
constexpr uint64_t kTextBatchBytes = 256ull << 20;
constexpr size_t kTextPad = 64;                 // readable bytes behind the text (build_kernel loads dwords)
// staging sets of a build: one being parsed into, one on its way over PCIe, one being hashed (with two,
// parsing waits for the kernel of the batch before last: 8.2 ms per 256 MiB batch instead of 6)
constexpr int kStages = 3;

// One of the staging sets of a build: pinned term text + stretch tables, their device copies,
// the event that tells when the GPU is done with them.  Host threads parse documents straight into
// `text` (every document of a batch owns a span sized by its text bound; what it leaves unused is
// a gap stretch the kernel skips), so a character is written once between the file and the H2D copy.
struct Stage {
    PinnedBuf<uint8_t> text;
    PinnedBuf<uint64_t> seg_off;
    PinnedBuf<uint32_t> seg_col;
    DevBuf<uint8_t> d_text;
    DevBuf<uint64_t> d_off;
    DevBuf<uint32_t> d_col;
    hipEvent_t done = nullptr, copied = nullptr;
    bool busy = false;
    ~Stage() {
        if (done) (void)hipEventDestroy(done);
        if (copied) (void)hipEventDestroy(copied);
    }
};

// Staging memory outlives a build: pinning 2 x 256 MiB costs more than hashing them.  The sets are
// checked out per build and handed back; never freed (a static destructor would run after the HIP
// runtime's own).
struct StagePool {
    std::mutex mu;
    std::vector<Stage*> idle;
    std::vector<DevBuf<uint8_t>*> idle_planes;     // byte-map planes (one buffer per build in flight)
    std::vector<DevBuf<uint8_t>*> idle_tables;     // min_count counting tables (one per build that uses the cutoff)
    int device = -1;
    // the counting table the last batch with a cutoff was counted in, for cobs_gpu_last_count_table (diagnostics):
    // its buffer, slots and text bytes as BuildContext::clear_table set them; forgotten when the idle buffers are freed
    DevBuf<uint8_t>* last_table = nullptr;
    uint64_t last_cap = 0, last_total = 0;
    void note_table(DevBuf<uint8_t>* b, uint64_t cap, uint64_t total) {
        std::lock_guard<std::mutex> g(mu);
        last_table = b;
        last_cap = cap;
        last_total = total;
    }
    void drop_idle() {                             // mu held
        for (Stage* s : idle) delete s;
        idle.clear();
        for (auto* b : idle_planes) delete b;
        idle_planes.clear();
        for (auto* b : idle_tables) delete b;
        idle_tables.clear();
        last_table = nullptr;
        last_cap = last_total = 0;
    }
    DevBuf<uint8_t>* take_table(int dev) {
        std::lock_guard<std::mutex> g(mu);
        if (device != dev) { drop_idle(); device = dev; }
        if (idle_tables.empty()) return new DevBuf<uint8_t>;
        DevBuf<uint8_t>* b = idle_tables.back();
        idle_tables.pop_back();
        return b;
    }
    void give_table(DevBuf<uint8_t>* b) {
        std::lock_guard<std::mutex> g(mu);
        idle_tables.push_back(b);
    }
    DevBuf<uint8_t>* take_planes(int dev) {
        std::lock_guard<std::mutex> g(mu);
        if (device != dev) { drop_idle(); device = dev; }
        if (idle_planes.empty()) return new DevBuf<uint8_t>;
        DevBuf<uint8_t>* b = idle_planes.back();
        idle_planes.pop_back();
        return b;
    }
    void give_planes(DevBuf<uint8_t>* b) {
        std::lock_guard<std::mutex> g(mu);
        idle_planes.push_back(b);
    }
    void release_idle() {
        std::lock_guard<std::mutex> g(mu);
        drop_idle();
    }
    Stage* take(int dev) {
        std::lock_guard<std::mutex> g(mu);
        if (device != dev) { drop_idle(); device = dev; }     // buffers belong to the device they were made on
        if (idle.empty()) return new Stage;
        Stage* s = idle.back();
        idle.pop_back();
        return s;
    }
    void give(Stage* s) {
        std::lock_guard<std::mutex> g(mu);
        idle.push_back(s);
    }
};
StagePool& stage_pool();

// Host threads that stay up for a whole build: a batch hands them one job (parse the documents of
// the batch), run() returns when every worker has finished it.  Spawning 64-128 threads per batch
// cost 1-2 ms of the ~6 ms a batch has.
class WorkerPool {
public:
    explicit WorkerPool(size_t n) {
        for (size_t t = 0; t < n; ++t) threads_.emplace_back([this, t]() { loop(t); });
    }
    ~WorkerPool() {
        {
            std::lock_guard<std::mutex> g(mu_);
            quit_ = true;
            ++gen_;
        }
        cv_.notify_all();
        for (auto& t : threads_) t.join();
    }
    size_t size() const { return threads_.size(); }
    void run(const std::function<void(size_t)>& fn) {
        {
            std::lock_guard<std::mutex> g(mu_);
            job_ = &fn;
            done_ = 0;
            ++gen_;
        }
        cv_.notify_all();
        std::unique_lock<std::mutex> lk(mu_);
        cv_done_.wait(lk, [&] { return done_ == threads_.size(); });
        job_ = nullptr;
    }

private:
    void loop(size_t tid) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(size_t)>* job;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return gen_ != seen; });
                seen = gen_;
                if (quit_) return;
                job = job_;
            }
            (*job)(tid);
            {
                std::lock_guard<std::mutex> g(mu_);
                ++done_;
            }
            cv_done_.notify_one();
        }
    }
    std::vector<std::thread> threads_;
    std::mutex mu_;
    std::condition_variable cv_, cv_done_;
    const std::function<void(size_t)>* job_ = nullptr;
    uint64_t gen_ = 0;
    size_t done_ = 0;
    bool quit_ = false;
};

struct Slot {                                   // one document of a batch
    size_t doc_col;                             // its column
    size_t src;                                 // its index in the source
    uint64_t begin, cap;                        // its span of the staging text
    uint64_t used = 0;
    std::vector<TermSeg> segs;
    cobs_gpu_status status = COBS_GPU_OK;
    std::string error;
};

// What one batched pass over documents keeps across its batches (and a compact build across its
// matrices): the two streams, the staging sets checked out of the pool, the parser threads and
// their scratch buffers.
struct StagingContext {
    hipStream_t stream = nullptr, copy_stream = nullptr;   // kernels | uploads (batch i + 1 beside the kernel of batch i)
    Stage* st[kStages] = {};
    std::unique_ptr<WorkerPool> workers;                   // created by the first batch with more than one document
    std::vector<std::string> scratch;                      // the file being parsed, one per worker, reused
    size_t max_threads = 1;
    bool ready = false;

    cobs_gpu_status init(bool parses);
    StagingContext() = default;
    StagingContext(const StagingContext&) = delete;
    StagingContext& operator=(const StagingContext&) = delete;
    ~StagingContext();
};

// One staged batch: documents docs[b0, b1) in column b0.. b1 - 1 (a stretch's seg_col is the
// document's index into `docs`, | kBuildRawStretch), `total` bytes of text in `nsegs` stretches.
// When nsegs && total the text and tables are on the device and ctx.stream waits for them.
struct StagedBatch {
    Stage* stage = nullptr;
    size_t b0 = 0, b1 = 0;
    uint64_t total = 0;
    size_t nsegs = 0;
    std::vector<Slot> slots;
};

// host seconds of the batches so far (COBS_GPU_BUILD_TRACE)
struct StageTimes {
    double wait = 0, parse = 0, table = 0, upload = 0;
};

// Stage documents docs[b0, n): as many as fit text_batch bytes by their text bounds (at least one),
// into staging set ctx.st[cur] (waiting for the GPU to be done with it).
cobs_gpu_status stage_batch(StagingContext& ctx, int cur, const DocSource& src, const size_t* docs, size_t b0, size_t n,
                            uint32_t term_size, uint64_t text_batch, StagedBatch& out, StageTimes& times);
// after the consumer's kernels of the batch are on ctx.stream: the staging set is busy until they end
cobs_gpu_status finish_batch(StagingContext& ctx, StagedBatch& b);

}  // namespace cobs_amd
