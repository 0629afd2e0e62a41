// cobs_amd/csrc/fill.cpp -- cobs_gpu_doc_bits: how many bits every document's Bloom filter has set, counted on the device
// where the rows are (fill_kernels.hip).  One sweep over the chunks of a file as the engine holds them: resident chunks
// are counted where they lie; the streamed chunks of a handle with an HBM budget go whole through the handle's two
// stream buffers (stream_chunk_in), the counting kernel of one chunk beside the copy of the next, ordered by the same
// events a search pass uses (pass.cpp) -- so the buffers are left in a state the next pass is correct from.  Row ranges of
// one sub-index add into the same cells (bits is a sum over rows), column slices fill their own.  The counts of a file
// are cached on the handle (8 bytes per slot); cobs_gpu_plant drops the cache of the file it changes.
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "engine.hpp"
#include "fill_kernels.hpp"

namespace cobs_amd {

struct FillWork {
    std::vector<std::vector<uint64_t>> bits;    // [file]: the cached counts of the file's local slots
    std::vector<uint8_t> have;                  // [file]
    DevBuf<unsigned long long> d_out;
    hipStream_t stream = nullptr;
    hipEvent_t k0[2] = {nullptr, nullptr}, k1[2] = {nullptr, nullptr};   // around the counting kernels of stream buffer i / of the resident chunks
    hipEvent_t c0[2] = {nullptr, nullptr}, c1[2] = {nullptr, nullptr};   // around stream_chunk_in of stream buffer i: the copy, and the host packing in front of it when the file is not pinned
    bool timed[2] = {false, false};
    FillTune tune;                              // COBS_GPU_FILL_GROUPS / COBS_GPU_FILL_SIDE, read once per handle (tests)
    bool tune_read = false;
    double kernel_ms = 0, pcie_ms = 0;
    uint64_t bytes_read = 0, passes = 0;
    ~FillWork() {
        for (auto* arr : {k0, k1, c0, c1})
            for (int i = 0; i < 2; ++i) if (arr[i]) (void)hipEventDestroy(arr[i]);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

void destroy_fill_work(FillWork* w) { delete w; }

void drop_fill_cache(cobs_gpu_index* ix, size_t f) {
    if (ix->fill && f < ix->fill->have.size()) ix->fill->have[f] = 0;
}

namespace {

cobs_gpu_status init_work(cobs_gpu_index* ix) {
    if (!ix->fill) ix->fill = new FillWork;
    FillWork* w = ix->fill;
    if (!w->tune_read) {
        if (const char* e = getenv("COBS_GPU_FILL_GROUPS")) w->tune.groups = (uint32_t)std::strtoul(e, nullptr, 0);
        if (const char* e = getenv("COBS_GPU_FILL_SIDE")) w->tune.max_side = (uint32_t)std::strtoul(e, nullptr, 0);
        w->tune_read = true;
    }
    w->bits.resize(ix->parts.size());
    w->have.resize(ix->parts.size(), 0);
    if (!w->stream) HIP_TRY(hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking));
    for (auto* arr : {w->k0, w->k1, w->c0, w->c1})
        for (int i = 0; i < 2; ++i) if (!arr[i]) HIP_TRY(hipEventCreate(&arr[i]));
    return COBS_GPU_OK;
}

// the event pairs of stream buffer `buf` have completed (the host waited for k1[buf]): add their durations
cobs_gpu_status collect(FillWork* w, int buf, bool copies) {
    if (!w->timed[buf]) return COBS_GPU_OK;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, w->k0[buf], w->k1[buf]));
    w->kernel_ms += ms;
    if (copies) {
        HIP_TRY(hipEventElapsedTime(&ms, w->c0[buf], w->c1[buf]));
        w->pcie_ms += ms;
    }
    w->timed[buf] = false;
    return COBS_GPU_OK;
}

cobs_gpu_status count_file(cobs_gpu_index* ix, size_t f) {
    FillWork* w = ix->fill;
    Part& p = ix->parts[f];
    StreamBufs& sb = ix->stream;
    hipStream_t st = w->stream;
    std::vector<uint64_t>& bits = w->bits[f];
    bits.assign((size_t)p.slot_count, 0);
    if (p.slot_count == 0) return COBS_GPU_OK;
    HIP_TRY(w->d_out.reserve((size_t)p.slot_count));
    HIP_TRY(launch_fill_zero(w->d_out.p, p.slot_count, st));
    // resident chunks, where they lie
    bool any_resident = false;
    for (const Chunk& c : p.chunks) {
        if (!c.d_data) continue;
        if (!any_resident) HIP_TRY(hipEventRecord(w->k0[0], st));
        any_resident = true;
        HIP_TRY(launch_fill_count(c.d_data, c.d_pages, c.pages, c.pitch, w->d_out.p, st, &w->bytes_read, w->tune));
    }
    if (any_resident) {
        HIP_TRY(hipEventRecord(w->k1[0], st));
        HIP_TRY(hipEventSynchronize(w->k1[0]));
        w->timed[0] = true;
        if (cobs_gpu_status s = collect(w, 0, false); s != COBS_GPU_OK) return s;
    }
    // streamed chunks: whole, through the two stream buffers, every chunk once
    for (const Chunk& c : p.chunks) {
        if (c.d_data) continue;
        const int buf = (int)(sb.seq++ & 1);
        if (sb.used[buf]) HIP_TRY(hipEventSynchronize(sb.scanned[buf]));      // the last kernel that read the buffer (a search pass's, or ours)
        if (cobs_gpu_status s = collect(w, buf, true); s != COBS_GPU_OK) return s;
        HIP_TRY(hipEventRecord(w->c0[buf], sb.copy_stream));
        if (cobs_gpu_status s = stream_chunk_in(ix, p, c, buf); s != COBS_GPU_OK) return s;
        HIP_TRY(hipEventRecord(w->c1[buf], sb.copy_stream));
        HIP_TRY(hipEventRecord(sb.copied[buf], sb.copy_stream));
        HIP_TRY(hipStreamWaitEvent(st, sb.copied[buf], 0));
        HIP_TRY(hipEventRecord(w->k0[buf], st));
        HIP_TRY(launch_fill_count(sb.sbuf[buf].p, c.d_pages, c.pages, c.pitch, w->d_out.p, st, &w->bytes_read, w->tune));
        HIP_TRY(hipEventRecord(w->k1[buf], st));
        HIP_TRY(hipEventRecord(sb.scanned[buf], st));
        sb.used[buf] = true;
        w->timed[buf] = true;
    }
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < 2; ++i)
        if (cobs_gpu_status s = collect(w, i, true); s != COBS_GPU_OK) return s;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit cells");
    HIP_TRY(hipMemcpy(bits.data(), w->d_out.p, (size_t)p.slot_count * sizeof(uint64_t), hipMemcpyDeviceToHost));
    ++w->passes;
    return COBS_GPU_OK;
}

}  // namespace

}  // namespace cobs_amd

using namespace cobs_amd;

extern "C" {

cobs_gpu_status cobs_gpu_doc_bits(cobs_gpu_index* ix, size_t file_no, uint64_t* bits, size_t cap, size_t* needed) {
    if (needed) *needed = 0;
    if (!ix) return fail(COBS_GPU_ERR_ARG, "NULL handle");
    if (file_no >= ix->parts.size()) return fail(COBS_GPU_ERR_ARG, "file number out of range");
    return guarded([&]() -> cobs_gpu_status {
        const Part& p = ix->parts[file_no];
        const size_t n = (size_t)p.slot_count;
        if (needed) *needed = n;
        if (cap < n) return fail(COBS_GPU_ERR_CAPACITY, "doc_bits: " + std::to_string(n) + " entries needed");
        if (n && !bits) return fail(COBS_GPU_ERR_ARG, "bits is NULL");
        HIP_TRY(hipSetDevice(ix->device));
        if (cobs_gpu_status s = init_work(ix); s != COBS_GPU_OK) return s;
        FillWork* w = ix->fill;
        if (!w->have[file_no]) {
            if (cobs_gpu_status s = count_file(ix, file_no); s != COBS_GPU_OK) return s;
            w->have[file_no] = 1;
        }
        if (n) std::memcpy(bits, w->bits[file_no].data(), n * sizeof(uint64_t));
        return COBS_GPU_OK;
    });
}

cobs_gpu_status cobs_gpu_doc_bits_ms(cobs_gpu_index* ix, double out[4]) {
    if (!ix || !out) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (const FillWork* w = ix->fill) {
        out[0] = w->kernel_ms;
        out[1] = (double)w->bytes_read;
        out[2] = w->pcie_ms;
        out[3] = (double)w->passes;
    }
    return COBS_GPU_OK;
}

cobs_gpu_status cobs_gpu_doc_bits_probe_ms(cobs_gpu_index* ix, size_t file_no, double* ms) {
    if (!ix || !ms) return fail(COBS_GPU_ERR_ARG, "NULL argument");
    if (file_no >= ix->parts.size()) return fail(COBS_GPU_ERR_ARG, "file number out of range");
    return guarded([&]() -> cobs_gpu_status {
        *ms = 0;
        HIP_TRY(hipSetDevice(ix->device));
        if (cobs_gpu_status s = init_work(ix); s != COBS_GPU_OK) return s;
        FillWork* w = ix->fill;
        DevBuf<uint32_t> sink;
        for (const Chunk& c : ix->parts[file_no].chunks) {
            if (!c.d_data) continue;
            const uint64_t lanes = fill_probe_lanes(c.pages, w->tune);
            if (lanes > (1ull << 30)) return fail(COBS_GPU_ERR_UNSUPPORTED, "probe: launch too large");
            HIP_TRY(sink.reserve((size_t)lanes));
            HIP_TRY(hipEventRecord(w->k0[0], w->stream));
            HIP_TRY(launch_fill_probe(c.d_data, c.d_pages, c.pages, c.pitch, sink.p, w->stream, w->tune));
            HIP_TRY(hipEventRecord(w->k1[0], w->stream));
            HIP_TRY(hipEventSynchronize(w->k1[0]));
            float t = 0;
            HIP_TRY(hipEventElapsedTime(&t, w->k0[0], w->k1[0]));
            *ms += t;
        }
        return COBS_GPU_OK;
    });
}

}  // extern "C"
