/*
 * include/cobs_gpu_diag.h -- diagnostics and test hooks of libcobs_gpu.so (nothing a caller of the search path
 * needs): the planners as host arithmetic (shards, exchanges -- what lets N ranks be checked without N GPUs), rows of
 * the resident matrix read back, per-launch bookkeeping for rooflines, counters of the engine's internal choices.
 */
#ifndef COBS_GPU_DIAG_H
#define COBS_GPU_DIAG_H

#include "cobs_gpu_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- planners (host only) ------------------------------------------------ */
/* Host only (no device needed): the score slots [slot_begin[r], slot_begin[r] + slot_count[r]) and
 * the index bytes shard r of shard_count would hold of the file at `path` (arrays of shard_count
 * entries; bytes may be NULL).  The slot ranges are disjoint, ascending and cover counts_size. */
cobs_gpu_status cobs_gpu_plan_shards(const char* path, uint32_t shard_count, uint32_t shard_mode,
                                     uint64_t* slot_begin, uint64_t* slot_count, uint64_t* bytes);

/* The exchange as a plan (host arithmetic only, no device, no communicator): what rank `rank` of
 * `nranks` sends to / receives from every peer and how the received slices are assembled, given all
 * ranks' slot layouts (slot_begin / slot_count: [nranks][nfiles], as cobs_gpu_info reports them).
 * cobs_gpu_batch_exchange_counts executes exactly this plan over RCCL; tests emulate N ranks with it. */
typedef struct cobs_gpu_xfer {
    uint64_t peer;
    uint64_t send_offset, send_bytes;   /* inside this rank's local count rows */
    uint64_t recv_offset, recv_bytes;   /* inside this rank's staging buffer */
} cobs_gpu_xfer;
typedef struct cobs_gpu_copy2d {        /* strided copy into the assembled rows (global document order) */
    uint64_t src_rank;
    uint64_t src_is_local;              /* 1: source is this rank's own count rows, 0: the staging buffer */
    uint64_t src_offset, src_pitch, dst_offset, dst_pitch, width, height;
} cobs_gpu_copy2d;
/* xfers: nranks entries; copies: *n_copies capacity in, count out (at most nranks * nfiles);
 * out = { q_begin, q_count, staging_bytes, assembled_bytes, uses_ncclAllGather, local_row_bytes } */
cobs_gpu_status cobs_gpu_exchange_plan(const uint64_t* slot_begin, const uint64_t* slot_count, const uint64_t* doc_offset,
                                       size_t nranks, size_t nfiles, uint64_t total_counts, size_t nq, uint32_t elem_bytes,
                                       uint32_t mode, size_t rank, cobs_gpu_xfer* xfers, cobs_gpu_copy2d* copies,
                                       size_t* n_copies, uint64_t out[6]);
/* ... as a plan (host arithmetic only): counts[r * nranks + j] = records rank r holds for the queries of rank j;
 * xfers[j] = what `rank` sends to / receives from rank j (bytes; send offsets inside its pool bucketed by owner,
 * receive offsets inside its staging buffer, rank after rank); out = { bytes received incl. its own bucket,
 * bytes of its pool }.  cobs_gpu_batch_exchange_hits_owned executes exactly this plan. */
cobs_gpu_status cobs_gpu_hit_exchange_plan(const uint64_t* counts, size_t nranks, size_t rank, cobs_gpu_xfer* xfers,
                                           uint64_t out[2]);
/* Diagnostics / tests: the device-side half of that exchange for any rank count, without a communicator: the hit
 * pool of the last synced thresholded run bucketed by owner as `nranks` ranks would bucket it -- counts[j] records
 * for rank j, the buckets back to back in `records` as (query, file, document, score) quadruples of uint32. */
cobs_gpu_status cobs_gpu_batch_bucketed_hits(cobs_gpu_batch* b, uint32_t nranks, uint64_t* counts, uint32_t* records,
                                             size_t cap_records, size_t* n_records);

/* ---- rows of the matrix as HBM holds them --------------------------------- */
/* copy `n` bytes of row `row` of sub-index `page` back from HBM (diagnostics/tests) */
cobs_gpu_status cobs_gpu_read_row(const cobs_gpu_index* ix, size_t file_no, uint32_t page,
                                  uint64_t row, uint8_t* out, size_t n);

/* row bytes [*col0, *col0 + *ncols) of sub-index `page` that this shard holds (0, 0 if none) */
cobs_gpu_status cobs_gpu_page_columns(const cobs_gpu_index* ix, size_t file_no, uint32_t page,
                                      uint64_t* col0, uint64_t* ncols);
/* the valid bytes of rows [row0, row0+nrows) of a held sub-index, out_pitch bytes apart */
cobs_gpu_status cobs_gpu_read_rows(const cobs_gpu_index* ix, size_t file_no, uint32_t page,
                                   uint64_t row0, uint64_t nrows, uint8_t* out, size_t out_pitch);

/* ---- the counting table of a build with min_count ------------------------- */
/* The open-addressing table the LAST batch of the last build with min_count >= 2 was counted in (abundance_kernels.hpp),
 * read back from the current device: out[0] = its slots (a power of two, 0 = there is no table: no such build yet, the
 * buffers released by cobs_gpu_build_release_buffers, or another device current), out[1] = the text bytes of that batch.
 * owner[slot] = 0 (free) or tag << 40 | (batch offset of the term's first occurrence + 1), count[slot] = its occurrences,
 * saturating at min_count.  Either array may be NULL; both NULL asks for out alone; cap_slots < out[0] is
 * COBS_GPU_ERR_CAPACITY with out filled in.  Host code only (a copy from the buffer the stage pool keeps); not to be called
 * while a build is running.  Tests read it to see which slots known keys took. */
cobs_gpu_status cobs_gpu_last_count_table(uint64_t out[2], uint64_t* owner, uint32_t* count, size_t cap_slots);

/* ---- bookkeeping ---------------------------------------------------------- */
/* Per-launch bookkeeping of the last cobs_gpu_batch_run (for rooflines):
 * out[0] = algorithmic bytes of the scan kernel(s): sum over queries of
 *          T * H * (row bytes gathered) + score bytes written
 * out[1] = number of scan-kernel launches, out[2] = k-mer lookups (sum T),
 * out[3] = bytes of row-index table written by K1 and read by K2 IN THIS RUN: 0 for a
 *          run whose scan work-groups hashed their query's terms themselves (tuning
 *          key "scan_self_hash"; no K1 launch).  The table's memory stays reserved
 *          by cobs_gpu_batch_set_queries either way -- the other call families and
 *          a run of the same batch on the table path use it --, so this is traffic,
 *          not footprint.                                                          */
cobs_gpu_status cobs_gpu_batch_stats(const cobs_gpu_batch* b, uint64_t out[4]);
/* The launch geometry of the last scan-kernel launch of the batch that ran outside a replayed graph: out[0] = tile width
 * in 16-byte chunks, out[1] = waves per work-group, out[2] = 1 for the multi-query form, out[3] = 1 for the LDS-staged
 * variant.  All 0 before the first launch.  Tests read it to see that a forced tuning key reached the launch. */
cobs_gpu_status cobs_gpu_batch_scan_geometry(const cobs_gpu_batch* b, uint32_t out[4]);
/* HIP-event duration (ms) of the scan kernel(s) / hash kernel, averaged over the
 * runs since the previous call (at most the last 64); events are recorded on the
 * stream the kernels were launched on.  Call after cobs_gpu_batch_sync. */
cobs_gpu_status cobs_gpu_batch_kernel_ms(cobs_gpu_batch* b, float* scan_ms, float* hash_ms);

/* HIP-event durations (ms) of the kernels of the cobs_gpu_hit_positions calls on this handle since the previous call of
 * this function, summed over their passes: out[0] = the presence kernel, out[1] = K1 (hashing), out[2] = passes. */
cobs_gpu_status cobs_gpu_positions_ms(cobs_gpu_index* ix, double out[3]);

/* HIP-event durations (ms) of the kernels of the cobs_gpu_prevalence calls on this handle since the previous call of this
 * function, summed over their passes: out[0] = the prevalence kernel, out[1] = K1 (hashing), out[2] = passes. */
cobs_gpu_status cobs_gpu_prevalence_ms(cobs_gpu_index* ix, double out[3]);

/* HIP-event durations (ms) of the stages of the cobs_gpu_search_weighted calls on this handle since the previous call of
 * this function, summed over their passes: out[0] = K1 (hashing), out[1] = the prevalence kernel, out[2] = the weight
 * kernel, out[3] = the weighted scan (a scan repeated after a pool overflow included), out[4] = passes. */
cobs_gpu_status cobs_gpu_weighted_ms(cobs_gpu_index* ix, double out[5]);   /* hash, prevalence, weights, scan, passes; reset on read */

/* Durations (ms) of the stages of the cobs_gpu_search_sets calls on this handle since the previous call of this function,
 * summed over their passes: out[0] = K1 (hashing), out[1] = the set presence kernel, out[2] = the select kernel (HIP
 * events), out[3] = the host's ordering of the records, out[4] = passes. */
cobs_gpu_status cobs_gpu_sets_ms(cobs_gpu_index* ix, double out[5]);   /* hash, presence, select, ordering, passes; reset on read */

/* Durations (ms) of the stages of the cobs_gpu_search_sets_quorum and cobs_gpu_set_prevalence calls on this handle since the
 * previous call of this function, summed over their passes: out[0] = K1 (hashing), out[1] = the set count kernel, out[2] =
 * the quorum select kernel (HIP events; 0 for cobs_gpu_set_prevalence), out[3] = the host's ordering of the records,
 * out[4] = passes. */
cobs_gpu_status cobs_gpu_set_quorum_ms(cobs_gpu_index* ix, double out[5]);   /* hash, count, select, ordering, passes; reset on read */

/* HIP-event durations (ms) of the stages of the cobs_gpu_search_coverage calls on this handle since the previous call of
 * this function, summed over their passes: out[0] = K1 (hashing), out[1] = the coverage scan (a scan repeated after a pool
 * overflow included), out[2] = passes. */
cobs_gpu_status cobs_gpu_coverage_ms(cobs_gpu_index* ix, double out[3]);   /* hash, scan, passes; reset on read */

/* The same for the cobs_gpu_search_window calls on this handle: out[0] = K1 (hashing), out[1] = the window scan (a scan
 * repeated after a pool overflow included), out[2] = passes. */
cobs_gpu_status cobs_gpu_window_ms(cobs_gpu_index* ix, double out[3]);     /* hash, scan, passes; reset on read */

/* Durations (ms) of the LAST cobs_gpu_search_groups call on this handle: out[0] = the accumulate kernel (HIP events, summed
 * over the call's passes), out[1] = the select kernel (HIP events), out[2] = the host's ordering of the records. */
cobs_gpu_status cobs_gpu_groups_ms(cobs_gpu_index* ix, double out[3]);

/* Durations (ms) of the LAST cobs_gpu_search_best call on this handle: out[0] = the best-member kernel and the merge of
 * partial states (HIP events, summed over the call's passes), out[1] = the select kernel (HIP events), out[2] = the host's
 * ordering of the records. */
cobs_gpu_status cobs_gpu_best_ms(cobs_gpu_index* ix, double out[3]);
/* How the last cobs_gpu_search_best call was launched: out[0] = device passes, out[1] = (group, pass) spans whose
 * work-groups owned their cells of the state, out[2] = partial states written by groups whose queries were split over
 * several work-groups, out[3] = such groups (folds of the merge kernel). */
cobs_gpu_status cobs_gpu_best_counts(cobs_gpu_index* ix, uint64_t out[4]);

/* The cobs_gpu_doc_bits sweeps of this handle so far (cache hits add nothing): out[0] = milliseconds of the counting
 * kernels (HIP events), out[1] = index bytes they read (rows x valid row bytes), out[2] = milliseconds between HIP events
 * recorded on the copy stream before and after every streamed chunk is brought in (0 on a resident handle) -- the copies
 * over PCIe and, for a file whose mapping is not registered with HIP, the host threads that pack the rows into pinned
 * staging before each copy is queued --, out[3] = sweeps (one per file counted). */
cobs_gpu_status cobs_gpu_doc_bits_ms(cobs_gpu_index* ix, double out[4]);
/* The arithmetic-free yardstick of the counting kernel: the same loads over the resident chunks of file_no, one XOR per
 * load and one store per lane; *ms = HIP-event milliseconds of one such sweep (scripts/probes/fill_probe.py). */
cobs_gpu_status cobs_gpu_doc_bits_probe_ms(cobs_gpu_index* ix, size_t file_no, double* ms);

/* The cobs_gpu_doc_shared_bits panels of this handle since the last read (the figures are reset by this call): out[0] =
 * milliseconds of the kernels that extract the references' bits of every row, out[1] = milliseconds of the sweeps (the
 * zeroing of the cells and the counting kernel), both between HIP events, out[2] = index bytes the sweeps read (rows x
 * valid row bytes), out[3] = sweeps (one per panel of up to 8 references of one sub-index). */
cobs_gpu_status cobs_gpu_similarity_ms(cobs_gpu_index* ix, double out[4]);

/* Diagnostics of tuning builds (libcobs_gpu_timing.so, `make -C cobs_amd/csrc timing`): s_memtime stamps
 * [work-group slot][wave 0..3][8 phases] of the work-groups sampled from the last scan launch after
 * cobs_gpu_set_tuning(ix, "phase_slots", n).  The production library records nothing (*n_words = 0). */
cobs_gpu_status cobs_gpu_batch_phase_stamps(cobs_gpu_batch* b, uint64_t* out, size_t cap_words, size_t* n_words);

/* Small calls of the host-buffer API (up to 16 queries) are captured into a hipGraph the second time
 * a pass of the same shape class (query count, score width, launch geometry -- not the exact query lengths --, same
 * parameters) comes along and replayed with one launch afterwards;
 * this counts the replays (diagnostics; tuning key "graph" = 0 turns the path off). */
uint64_t cobs_gpu_graph_replays(const cobs_gpu_index* ix);
/* Device passes the host-buffer calls (cobs_gpu_search, _search_batch, _search_batch_view, _counts) have launched on this
 * handle so far, replays included: a call is cut into passes (cobs_gpu.h), and a call that came back with
 * COBS_GPU_ERR_CAPACITY and was made again has paid for its passes twice -- the view call grows its arena instead. */
uint64_t cobs_gpu_host_passes(const cobs_gpu_index* ix);
/* Passes on this handle so far that ran in the self-hashing form of the scan (tuning key "scan_self_hash": no K1 launch,
 * the scan work-groups hash their query's terms themselves), whichever call drove them: the host-buffer calls, the view
 * call, cobs_gpu_search_groups, cobs_gpu_search_best and the runs of a caller's own batches on the handle.  A replay of a
 * graph that was captured from such a pass counts too, as in cobs_gpu_graph_replays.  Says which form a call took where no
 * batch of the caller's is at hand to ask (cobs_gpu_batch_stats: table_bytes). */
uint64_t cobs_gpu_self_hash_passes(const cobs_gpu_index* ix);

/* Out-of-core handles (hbm_budget_bytes): how the chunks of all passes so far were brought into HBM.
 * out[0] = chunks whose looked-up rows were fetched one by one from the registered file mapping (a batch that
 * touches a fraction of the chunk's rows: the access pattern of the reference's mmap / AIO back-ends,
 * compact_index/mmap_search_file.cpp:34-67, aio_search_file.cpp:58-97), out[1] = chunks copied whole.
 * Tuning keys "row_fetch" (0 = always whole) and "row_fetch_alpha" (fetch when alpha x looked-up bytes <= the
 * chunk's bytes; default 1, 0 = whenever the rows fit a stream buffer) steer the choice. */
cobs_gpu_status cobs_gpu_stream_counters(const cobs_gpu_index* ix, uint64_t out[2]);
/* The same two counters in out[0] / out[1] plus out[2] / out[3] = the bytes those two ways asked of PCIe (the DISTINCT
 * looked-up rows x row pitch -- a row that several terms of a batch look up crosses once since round 6; counted by the
 * gather on the device, so this call waits for the device --; the rows of the whole chunks).  (Its own symbol: round 4 had widened cobs_gpu_stream_counters to
 * four words under the old name, which writes past the two-word buffer of a caller built against the older header.) */
cobs_gpu_status cobs_gpu_stream_traffic(const cobs_gpu_index* ix, uint64_t out[4]);
/* The plan of an out-of-core handle: out[0] = bytes of ONE of its two stream buffers, out[1] = bytes of the streamed
 * files' slices that stay RESIDENT beside them (the budget is spent per slice, not per file: what the buffers leave
 * over keeps the subset of whole slices with the most bytes in HBM), out[2] = row bytes a pass moves over PCIe when it
 * copies every other chunk whole, out[3] = number of those chunks.  COBS_GPU_STREAM_BUF_KIB (read when the index is
 * opened) bounds a stream buffer (default 256 MiB, 0 = half the budget as in rounds 1-4). */
cobs_gpu_status cobs_gpu_stream_plan(const cobs_gpu_index* ix, uint64_t out[4]);
/* How file `file_no` of the handle is laid out (what the plan decided when the index was opened): out[0] = held slices
 * that stay in HBM (every one of a resident file), out[1] = streamed chunks of whole slices (one or several sub-indexes
 * each), out[2] = streamed column slices of a sub-index, out[3] = streamed row ranges of a sub-index. */
cobs_gpu_status cobs_gpu_stream_layout(const cobs_gpu_index* ix, size_t file_no, uint64_t out[4]);
/* The same plan as host arithmetic, without a device (what cobs_gpu_open would decide for `path` under the budget and
 * the shard options): out as above (for a file that fits: out[1] = its bytes, the rest 0); resident[i] (optional, `cap`
 * entries; *n_slices = how many there are) = 1 if the i-th held slice stays in HBM.  For tests of the planner. */
cobs_gpu_status cobs_gpu_plan_stream(const char* path, uint64_t hbm_budget_bytes, uint32_t shard_rank, uint32_t shard_count,
                                     uint32_t shard_mode, uint64_t out[4], uint8_t* resident, size_t cap, size_t* n_slices);

#ifdef __cplusplus
}
#endif
#endif /* COBS_GPU_DIAG_H */
