// cobs_amd/csrc/kernels.hpp -- host-callable launchers of the gfx950 kernels.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "device_types.hpp"

namespace cobs_amd {

// K1: one thread per query position (total_threads = span_off[nq]).
hipError_t launch_hash(const HashArgs& a, uint64_t total_threads, hipStream_t stream);
hipError_t launch_skip_thresholds(const SkipThresholdArgs& a, hipStream_t stream);

// Smallest instantiated plane count that can hold counts up to max_terms
// (4, 8 -> u8 scores as the reference's T < 255 path; 10, 12, 16 -> u16; 20, 24, 32 -> u32); -1 if none.
int scan_planes_for(uint64_t max_terms);
inline uint32_t scan_score_bytes(int planes) { return planes <= 8 ? 1u : planes <= 16 ? 2u : 4u; }

// K2: ntiles * nq work-groups of nw (1, 2 or 4) waves; multi_query: ntiles * ceil(nq / (64 / tile_w))
// work-groups whose lane groups serve different queries (short queries; see scan_has_multi_query).
// max_blocks: the longest query of the batch in 8-term blocks (read by the self-hashing form only, which is refused
// where a tile's row indices would not fit its LDS array: the kernel itself writes nothing for such a work-group).
hipError_t launch_scan(const ScanArgs& a, uint32_t ntiles, int planes, int nw, bool multi_query, uint64_t max_blocks,
                       hipStream_t stream);
// The sub-indexes one tile of tile_w chunks can lie in, of npages sub-indexes cpp chunks wide.  Tiles start at multiples of
// tile_w: where tile_w divides cpp no tile crosses a boundary; otherwise a tile that starts on a sub-index's last chunk
// reaches 1 + ceil((tile_w - 1) / cpp) of them (page_size 200 B, 13 chunks: two under W = 8, six under W = 64).
inline uint32_t scan_tile_pages(uint64_t npages, uint32_t cpp, uint32_t tile_w) {
    if (npages <= 1 || cpp == 0 || tile_w == 0 || cpp % tile_w == 0) return 1;
    const uint64_t reach = 1ull + (tile_w - 1ull + cpp - 1ull) / cpp;
    return (uint32_t)(reach < npages ? reach : npages);
}
// ... and whether the self-hashing form's LDS array holds their row indices for queries of up to max_blocks blocks
inline bool scan_self_hash_fits(uint64_t npages, uint32_t cpp, uint32_t tile_w, uint64_t max_blocks) {
    return (uint64_t)scan_tile_pages(npages, cpp, tile_w) * (max_blocks + 1) * 8 <= kSelfHashEntries;
}
// (which instantiations exist: defined here, so that launch_scan and the host code that picks a variant -- geometry.cpp,
// pass.cpp and the host-only program under tests/host -- read one definition)
inline bool scan_has_multi_query(int planes, uint32_t num_hashes, uint32_t tile_w) {
    return num_hashes == 1 && tile_w < 64 && (planes == 4 || planes == 8 || planes == 10 || planes == 12);
}
// run_topk without score rows (ScanArgs::cand): the tile_topk epilogue exists for files with 32-bit row indices
inline bool scan_has_tile_topk(uint32_t num_hashes, bool idx64) { (void)num_hashes; return !idx64; }
// the LDS-staged A/B variant exists for the headline shape only (H = 1, 10 planes, 2 or 4 waves)
inline bool scan_has_lds_staged(int planes, uint32_t num_hashes, int nw) {
    return num_hashes == 1 && planes == 10 && (nw == 2 || nw == 4);
}
// the self-hashing form (ScanArgs::self_hash: no table from K1, the work-groups hash their query's terms into LDS) exists
// for one hash function over 31-mers, 32-bit row indices and up to 12 planes (2048 terms need 12 at the most: the wider
// score types never meet the LDS array's limit); launch_scan takes it with multi_query off, no candidate pool, no
// findere, and only where the LDS array holds the indices of every tile (scan_self_hash_fits)
inline bool scan_has_self_hash(int planes, uint32_t num_hashes, uint32_t term_size, bool idx64) {
    return num_hashes == 1 && term_size == 31 && !idx64 && (planes == 4 || planes == 8 || planes == 10 || planes == 12);
}

// K3: per query the k best (score desc, doc asc) documents with score >= threshold.
hipError_t launch_topk(const TopkArgs& a, hipStream_t stream);

// Ranking of every document (rank_kernels.hip): one pass of the stable radix sort by score; a.nq work-groups.
hipError_t launch_rank(const RankArgs& a, bool first, bool last, hipStream_t stream);
hipError_t launch_pack_slots(const SlotPackArgs& a, hipStream_t stream);
// Distribution of the scores of a pass over its real documents (rank_kernels.hip): nq x nranges work-groups.
hipError_t launch_score_hist(const HistArgs& a, hipStream_t stream);

// Row-selective out-of-core access (fetch_kernels.hip): one thread per (looked-up row, 16-byte piece).
// count_rows: how many rows the batch looks up in every streamed piece of a part (one counter per piece);
// gather: slots for exactly the DISTINCT looked-up rows of a unit's pages, ascending (gather_mark / _rank / _assign / _list_kernel;
// a.bitmap zeroed), then the rows themselves (gather_copy_kernel).
hipError_t launch_count_rows(const CountArgs& a, uint64_t total_entries, bool idx64, hipStream_t stream);
hipError_t launch_gather_assign(const GatherArgs& a, bool idx64, uint32_t max_words, hipStream_t stream);
// grid_limit: work-groups of the copy (a grid-stride loop): few when other kernels of the pass run beside it, see pass.cpp
hipError_t launch_gather_copy(const GatherArgs& a, uint32_t grid_limit, hipStream_t stream);
// Row-range chunks of a streamed sub-index (fetch_kernels.hip): rewrite the `entries` row indices of one sub-index for
// the rows a chunk holds; add a chunk's partial scores to the score rows.
hipError_t launch_remap_rows(const RemapArgs& a, uint64_t entries, bool idx64, hipStream_t stream);
hipError_t launch_add_scores(const AddScoresArgs& a, hipStream_t stream);
// ... and the threshold filter over the scores a sub-index's row ranges added up (topk_kernels.hip: select_rows_kernel)
hipError_t launch_select_rows(const SelectRowsArgs& a, hipStream_t stream);
// a row-range unit's in-range terms per query: a compact second table + its block offsets (count, scan, write)
hipError_t launch_compact_terms(const CompactArgs& a, hipStream_t stream);
hipError_t launch_clear_flags(uint32_t* flags, hipStream_t stream, uint32_t* valid = nullptr, uint32_t nvalid = 0);

// Owner-routed hit exchange (xchg_kernels.hip): count == true -> records per owner into a.cursor, else scatter.
hipError_t launch_bucket_hits(const BucketArgs& a, bool count, hipStream_t stream);
// The hit pool in result order (xchg_kernels.hip): count per query, scan, scatter, one wave per query orders its bucket.
// a.cnt ([nq + 1]) and a.cur ([nq]) must be zero.
hipError_t launch_order_pool(const PoolArgs& a, hipStream_t stream);
constexpr uint32_t kPoolSegMax = 1024;      // buckets the device orders (larger ones: the host)
// The all-gathered best-of lists of the shards ([rank][lists][k] + counts) side by side per list for K3's pool mode
// ([lists][stride], stride >= nranks * k and a multiple of 8; unused entries marked).
hipError_t launch_merge_lists(const uint2* all, const uint32_t* cnt, uint2* out, uint32_t nranks, uint64_t lists, uint32_t k,
                              uint32_t stride, hipStream_t stream);
// One rank's record of a sharded pass (sharded.cpp): status | first invalid query word | hit-pool fill | extra, 4 x u64.
hipError_t launch_pass_meta(const uint32_t* flags, uint64_t* rec, uint64_t status, uint64_t extra, hipStream_t stream);

// Index construction: one thread per text position hashes its term and sets the bits.
hipError_t launch_build(const BuildArgs& a, uint64_t total_bytes, hipStream_t stream);
hipError_t launch_pack_bytemap(const PackArgs& a, hipStream_t stream);

hipError_t launch_random_build(const RandomBuildArgs& a, uint64_t ndocs, hipStream_t stream);
hipError_t launch_combine(const CombineArgs& a, hipStream_t stream);
hipError_t launch_synth(const SynthArgs& a, hipStream_t stream);
hipError_t launch_synth_rows(const SynthRowsArgs& a, hipStream_t stream);
hipError_t launch_plant(const PlantArgs& a, hipStream_t stream);
hipError_t launch_repitch(const RepitchArgs& a, hipStream_t stream);

}  // namespace cobs_amd
