// cobs_amd/csrc/abundance_kernels.hpp -- the k-mer abundance cutoff of index construction
// (cobs_gpu_build_params.min_count, no reference counterpart: the reference reads .ctx files that an
// external McCortex run has cleaned).  With min_count = c >= 2 the builder replaces build_kernel by
// the two kernels declared here; with c <= 1 nothing of this file runs and no table exists.
//
// Semantics.  A term sets its bits in document d's column only if it occurs at least c times WITHIN
// document d.  Occurrences are the term positions build_kernel hashes (process_terms order; sequence
// boundaries and gap stretches respected, raw stretches included); occurrences in other documents
// never count.  Two occurrences are the same term when the bytes handed to the hash function are
// equal: after canonicalisation (canonicalize = 1 counts a k-mer and its reverse complement together,
// canonicalize = 0 apart) and after the mapping of invalid characters to 0 that goes with it.
// Sizing does not change: signature_size = 0 and the compact grouping, sort and page heuristic still
// come from the unfiltered num_terms (sizing from kept terms needs a second pass over the corpus).
//
// A staged batch always holds whole documents (stage_batch), so one table per batch is enough:
//   owner[slot]  0 = free, else (tag << 40) | (batch offset of the term's first occurrence + 1);
//                tag = 24 hash bits of (document, term).  Claimed with ONE 64-bit atomicCAS, so the
//                tag is visible whenever the claim is -- there is no window in which a prober sees
//                an owner without its fingerprint
//   count[slot]  occurrences, saturating at c (a multi-GiB homopolymer document cannot wrap it)
// The key is exact: a probe that meets an equal tag compares the document and the hashed bytes at
// the stored offset with its own.  Offsets are 64-bit in the kernels; 40 bits of them are stored
// (1 TiB of text in one batch, beyond the memory of the part), launch_abundance refuses more.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "device_types.hpp"

namespace cobs_amd {

constexpr uint32_t kAbundanceOffsetBits = 40;
constexpr uint64_t kAbundanceSlotBytes = 12;    // owner word + count word

struct AbundanceArgs {
    BuildArgs b;                    // text, stretch tables, matrix / byte-map planes: as for build_kernel
    uint64_t total;                 // bytes of text in the batch
    unsigned long long* owner;      // mask + 1 slots, zeroed
    uint32_t* count;                // mask + 1 slots, zeroed
    uint64_t mask;                  // capacity - 1; capacity = the power of two >= 2 * total
    uint32_t min_count;             // >= 2
};

// slots of the table of a batch of `total` text bytes
inline uint64_t abundance_capacity(uint64_t total) {
    uint64_t cap = 1024;
    while (cap < 2 * total) cap <<= 1;
    return cap;
}

// count, then emit, on `stream`; the caller has zeroed owner[] and count[] on the same stream
hipError_t launch_abundance(const AbundanceArgs& a, hipStream_t stream);

}  // namespace cobs_amd
