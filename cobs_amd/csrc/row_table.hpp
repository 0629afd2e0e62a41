// cobs_amd/csrc/row_table.hpp -- THE definition of K1's row-index table, shared by its writer (hash_kernel, hash_kernels.hip)
// and every kernel that reads it (K2, the fetch kernels, presence, prevalence, weighted scan).
//
// Layout of one file's table:  [query q][held sub-index p][block b][hash j][8]
//   * a query has nblk(q) = blk_off[q + 1] - blk_off[q] blocks of 8 terms PLUS ONE all-padding block behind them
//     (every entry of it names the sub-index's zero row; lanes without work point at it), so query q starts
//     blk_off[q] + q blocks into a sub-index's share and owns nblk(q) + 1 of them per sub-index;
//   * a block holds, per hash function, the row indices of its 8 terms side by side: term t of the query and hash j sit
//     at block t / 8, entry j * 8 + t % 8;
//   * entries are u32, or u64 when some sub-index has 2^32 - 1 rows or more (Part::idx64, COBS_GPU_IDX64).
// Only address arithmetic lives here; all of it is 64-bit, with the (b0 + q) term first.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace cobs_amd {

constexpr uint32_t kRowTableLanes = 8;      // terms of a block; the stride between the hash functions of a term

// What a reader needs to find a file's table: filled by table_ref_for (hash_pass.cpp) for the pass's batch.
struct TableRef {
    const void* table;          // K1's row indices (u32, or u64 when idx64)
    const uint64_t* blk_off;    // nq + 1 prefix sums of 8-term blocks per query (this file's term size)
    const uint32_t* q_len;      // characters per query
    uint32_t table_npages;      // sub-indexes in the table (its page stride); PageDev::tpage selects one
    uint32_t num_hashes;
    uint32_t term_size;
    uint32_t findere;           // z (0..7) of the pass
    uint32_t idx64;
};

// entries per block
__host__ __device__ __forceinline__ uint64_t row_table_per(uint32_t H) { return 8ull * H; }

// ... of one block in ALL sub-indexes: the stride of a query's blocks in the whole table
__host__ __device__ __forceinline__ uint64_t row_table_per_all(uint32_t H, uint32_t npages) { return row_table_per(H) * npages; }

// first entry of (query q, sub-index tpage): b0 = blk_off[q], blocks = the query's blocks INCLUDING the padding block,
// per = row_table_per(H)
__host__ __device__ __forceinline__ uint64_t row_table_first(uint64_t b0, uint32_t q, uint32_t npages, uint64_t tpage,
                                                             uint64_t blocks, uint64_t per) {
    return ((b0 + q) * npages + tpage * blocks) * per;
}

// first entry of query q inside ONE sub-index's entries taken alone ([query][block + padding block][hash][8]): what the
// kernels with a thread per entry of a sub-index search for.  With per = row_table_per(H) * npages: ... inside the whole
// table (a thread per entry of every sub-index)
__host__ __device__ __forceinline__ uint64_t row_table_query_first(uint64_t b0, uint32_t q, uint64_t per) { return (b0 + q) * per; }

// The blocks of (query q, sub-index tpage), for a reader.
template <typename IdxT>
struct RowTable {
    const IdxT* base;       // block 0
    uint32_t H;
    uint32_t nblk;          // the query's blocks; block nblk is the padding block

    __device__ __forceinline__ RowTable(const void* table, const uint64_t* blk_off, uint32_t npages, uint32_t q, uint32_t tpage,
                                        uint32_t H_)
        : H(H_) {
        const uint64_t b0 = blk_off[q];
        nblk = (uint32_t)(blk_off[q + 1] - b0);
        base = reinterpret_cast<const IdxT*>(table) + row_table_first(b0, q, npages, tpage, nblk + 1u, row_table_per(H_));
    }
    __device__ __forceinline__ RowTable(const TableRef& r, uint32_t q, uint32_t tpage, uint32_t H_)
        : RowTable(r.table, r.blk_off, r.table_npages, q, tpage, H_) {}

    __device__ __forceinline__ uint32_t blocks() const { return nblk + 1u; }
    __device__ __forceinline__ uint32_t padding_block() const { return nblk; }
    // the 8 x H entries of block b
    __device__ __forceinline__ const IdxT* block(uint32_t b) const { return base + (uint64_t)b * (8u * H); }
    // term t, hash 0; hash j is kRowTableLanes * j entries on
    __device__ __forceinline__ const IdxT* term(uint32_t t) const { return block(t >> 3) + (t & 7u); }
    __device__ __forceinline__ IdxT entry(uint32_t t, uint32_t j) const { return term(t)[j * kRowTableLanes]; }
};

// All sub-indexes of query q, for K1: thread (block blk, lane sub) writes hash j of sub-index p.
template <typename IdxT>
struct RowTableWriter {
    IdxT* base;             // sub-index 0, block 0 of the query
    uint32_t H;
    uint32_t tblk;          // blocks per sub-index: the query's blocks + the padding block

    __device__ __forceinline__ RowTableWriter(void* table, uint64_t b0, uint32_t q, uint32_t npages, uint32_t H_, uint32_t tblk_)
        : base(reinterpret_cast<IdxT*>(table) + row_table_first(b0, q, npages, 0, tblk_, row_table_per(H_))), H(H_), tblk(tblk_) {}

    __device__ __forceinline__ IdxT& out(uint32_t p, uint32_t blk, uint32_t j, uint32_t sub) const {
        return base[((uint64_t)p * tblk + blk) * row_table_per(H) + j * kRowTableLanes + sub];
    }
};

}  // namespace cobs_amd
