// cobs_amd/csrc/pooled_pass.hpp -- the device half of a pooled search call (the host arithmetic is pooled_call.hpp): the
// hit pool with its one retry, the words a pass brings home, the records of a pass appended to the call's, and
// run_scan_pass, the device pass of the pooled scans whose front is K1 alone (coverage.cpp, window.cpp).  The bodies that
// are no templates stand in hash_pass.cpp.
#pragma once
#include <hip/hip_runtime_api.h>

#include <string>
#include <vector>

#include "engine.hpp"
#include "pooled_call.hpp"

namespace cobs_amd {

// A pool the kernels append records to, and the 64-bit count of what they wanted to append.  `what` names the pool in
// the one message of a second overflow; `zero` is the family's zeroing kernel (words, count, stream).
template <typename Rec>
struct HitPool {
    const char* what;
    hipError_t (*zero)(uint32_t*, uint64_t, hipStream_t);
    DevBuf<Rec> pool;
    DevBuf<unsigned long long> fill;
    HitPool(const char* what_, hipError_t (*zero_)(uint32_t*, uint64_t, hipStream_t)) : what(what_), zero(zero_) {}

    // The pool holds `cap` records (it does not: no_room(cap) is the status) | the fill is zeroed on `st` | queue(cap,
    // attempt) launches what appends | read(attempt, &fill) brings the fill home behind it, waits, and may refuse.  A fill
    // above cap: the pool grows to it and all of that runs once more, attempt = 1.  -> *filled records lie in the pool.
    template <typename NoRoom, typename Queue, typename Read>
    cobs_gpu_status run(uint64_t cap, hipStream_t st, NoRoom&& no_room, Queue&& queue, Read&& read, uint64_t* filled) {
        HIP_TRY(fill.reserve(1));
        for (int attempt = 0; attempt < 2; ++attempt) {
            if (pool.reserve((size_t)cap) != hipSuccess) {
                (void)hipGetLastError();
                return no_room(cap);
            }
            HIP_TRY(zero(reinterpret_cast<uint32_t*>(fill.p), 2, st));
            if (cobs_gpu_status s = queue(cap, attempt); s != COBS_GPU_OK) return s;
            if (cobs_gpu_status s = read(attempt, filled); s != COBS_GPU_OK) return s;
            if (*filled <= cap) return COBS_GPU_OK;
            cap = *filled;
        }
        return fail(COBS_GPU_ERR_HIP, std::string(what) + " overflowed twice");
    }
};

// no_room of the pooled scans (not ERR_CAPACITY: that status promises the needed size of the CALLER's buffer in hit_offsets)
cobs_gpu_status scan_pool_no_room(uint64_t cap);

// The selection of groups.cpp and best.cpp through their pool: select(cap) between the two events, its time added to *ms,
// the fill read into a word on the stack.
template <typename Rec, typename NoRoom, typename Select>
cobs_gpu_status select_through(HitPool<Rec>& hp, uint64_t cap, hipStream_t st, hipEvent_t (&ev)[2], double* ms, NoRoom&& no_room,
                               Select&& select, uint64_t* filled) {
    return hp.run(cap, st, no_room,
        [&](uint64_t pool_cap, int) -> cobs_gpu_status {
            HIP_TRY(hipEventRecord(ev[0], st));
            HIP_TRY(select(pool_cap));
            HIP_TRY(hipEventRecord(ev[1], st));
            return COBS_GPU_OK;
        },
        [&](int, uint64_t* fill) -> cobs_gpu_status {
            unsigned long long n = 0;
            HIP_TRY(hipMemcpyAsync(&n, hp.fill.p, sizeof n, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            *fill = n;
            float t = 0;
            if (hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess) *ms += t;
            else (void)hipGetLastError();
            return COBS_GPU_OK;
        }, filled);
}

// What a pass on a scratch batch brings home in one sync: K1's four flag words | the pool's 64-bit fill, pinned.
struct PassLanding {
    PinnedBuf<uint32_t> h;
    hipError_t reserve() { return h.reserve(6); }
    hipError_t flags_home(const cobs_gpu_batch* b, hipStream_t st) { return hipMemcpyAsync(h.p, b->flags.p, 16, hipMemcpyDeviceToHost, st); }
    hipError_t fill_home(const unsigned long long* fill, hipStream_t st) { return hipMemcpyAsync(h.p + 4, fill, 8, hipMemcpyDeviceToHost, st); }
    uint32_t invalid_word() const { return h.p[0]; }
    uint64_t fill() const { return (uint64_t)h.p[5] << 32 | h.p[4]; }
};

// The head of a pass on the handle's scratch batch 0 (the device is set): the batch, with the queries [q0, q1) of the call
// uploaded on its stream; a query it refuses comes back in *bad_query under its number in the call.
cobs_gpu_status pass_queries(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t q0, size_t q1,
                             size_t* bad_query, cobs_gpu_batch** b);

// `fill` records of the pool at d_pool behind the call's records
template <typename Rec>
cobs_gpu_status append_records(std::vector<Rec>& recs, const Rec* d_pool, uint64_t fill) {
    const size_t at = recs.size();
    recs.resize(at + (size_t)fill);
    if (fill) HIP_TRY(hipMemcpy(recs.data() + at, d_pool, (size_t)fill * sizeof(Rec), hipMemcpyDeviceToHost));
    return COBS_GPU_OK;
}

// ... of a pass over the queries from q0 on: `query` becomes the call's query number
template <typename Rec>
cobs_gpu_status append_pass_records(std::vector<Rec>& recs, const Rec* d_pool, uint64_t fill, size_t q0) {
    const size_t at = recs.size();
    if (cobs_gpu_status s = append_records(recs, d_pool, fill); s != COBS_GPU_OK) return s;
    for (size_t i = at; i < recs.size(); ++i) recs[i].query += (uint32_t)q0;
    return COBS_GPU_OK;
}

// The hand-over of the pooled scans (weighted, coverage, window): per query by score descending, then (file, document)
cobs_gpu_status hand_out_hits(std::vector<HitDev>& recs, size_t nq, size_t num_results, cobs_gpu_hit* hits, size_t cap, size_t* hit_offsets);

// The body of a cobs_gpu_*_ms getter: out[0 .. n] = 0, or -- the family has run on the handle, ms is its timers --
// out[0 .. n) = ms, out[n] = passes, and both start again
cobs_gpu_status take_ms(const cobs_gpu_index* ix, double* out, int n, double* ms, uint64_t* passes);

// What a pooled scan whose front is K1 alone keeps on the handle
struct ScanWork {
    DevBuf<uint32_t> thr;                   // what the family stages per query (its layout is the family's)
    PinnedBuf<uint32_t> h_thr;
    HitPool<HitDev> hits;
    PassLanding land;
    PhaseEvents<3> ev;                      // before K1 | scan | after it
    double ms[2] = {0, 0};                  // hash | scan
    uint64_t passes = 0;
    explicit ScanWork(const char* pool_name);
};

struct ScanCall {
    cobs_gpu_index* ix;
    const char* const* queries;
    const size_t* lens;
    double threshold;
    size_t* bad_query;
    uint32_t z;
    uint64_t real_total;                    // real documents of all files
    std::vector<HitDev>* recs;              // the records of all passes, `query` = the call's query number
};

// K1 on every file that holds sub-indexes, for the batch's n queries
cobs_gpu_status launch_hash_held(cobs_gpu_index* ix, const cobs_gpu_batch* b, size_t n, uint32_t z, hipStream_t st);

// One device pass of such a scan over the queries [q0, q1), on the handle's scratch batch: the queries up | stage(h_thr)
// fills the pass's thr_words words, they go up | flags cleared | through the pool: K1 on every file (the first attempt
// alone: its table stays), scans(b, pool_cap, st) | the flag words and the fill home in one sync | a query with an
// invalid base refuses the call | the records behind the call's.
template <typename Stage, typename Scans>
cobs_gpu_status run_scan_pass(const ScanCall& c, ScanWork* w, size_t q0, size_t q1, size_t thr_words, Stage&& stage, Scans&& scans) {
    cobs_gpu_index* ix = c.ix;
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(w->ev.create());
    cobs_gpu_batch* b = nullptr;
    if (cobs_gpu_status s = pass_queries(ix, c.queries, c.lens, q0, q1, c.bad_query, &b); s != COBS_GPU_OK) return s;
    hipStream_t st = b->own_stream;
    const size_t n = q1 - q0;
    HIP_TRY(w->thr.reserve(thr_words));
    HIP_TRY(w->h_thr.reserve(thr_words));
    stage(w->h_thr.p);
    HIP_TRY(w->land.reserve());
    HIP_TRY(hipMemcpyAsync(w->thr.p, w->h_thr.p, thr_words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_clear_flags(b->flags.p, st));
    uint64_t fill = 0;
    cobs_gpu_status s = w->hits.run(first_pool_cap(ix->tune.hit_cap, c.threshold, c.real_total, n), st, scan_pool_no_room,
        [&](uint64_t pool_cap, int attempt) -> cobs_gpu_status {
            if (attempt == 0) {
                HIP_TRY(w->ev.mark(0, st));
                if (cobs_gpu_status h = launch_hash_held(ix, b, n, c.z, st); h != COBS_GPU_OK) return h;
            }
            HIP_TRY(w->ev.mark(1, st));
            if (cobs_gpu_status k = scans(b, pool_cap, st); k != COBS_GPU_OK) return k;
            HIP_TRY(w->ev.mark(2, st));
            return COBS_GPU_OK;
        },
        [&](int attempt, uint64_t* filled) -> cobs_gpu_status {
            if (attempt == 0) HIP_TRY(w->land.flags_home(b, st));
            HIP_TRY(w->land.fill_home(w->hits.fill.p, st));
            HIP_TRY(hipStreamSynchronize(st));
            *filled = w->land.fill();
            if (attempt != 0) {
                (void)w->ev.add_elapsed(w->ms, 1, 2);
                return COBS_GPU_OK;
            }
            if (w->ev.add_elapsed(w->ms)) w->passes++;
            return invalid_base_from_flags(w->land.invalid_word(), n, c.bad_query, q0);
        }, &fill);
    if (s != COBS_GPU_OK) return s;
    return append_pass_records(*c.recs, w->hits.pool.p, fill, q0);
}

}  // namespace cobs_amd
