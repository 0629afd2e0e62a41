// cobs_amd/csrc/build_kernels.hip -- index construction and staging kernels (gfx950, wave64):
//   build_kernel / pack_bytemap_kernel   classic construction (classic_index.cpp:40-73): hash terms, set document bits
//   random_build_kernel / combine_kernel classic_construct_random, classic_combine
//   synth_kernel / plant_kernel / synth_rows_kernel / repitch_kernel   the procedural index and index staging helpers.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_types.hpp"
#include "kernels.hpp"
#include "term_hash.hpp"     // xxh64_view, xxh64_31 / canon31, all_acgt / has_newline / set_term_bit

namespace cobs_amd {

// ---------------------------------------------------------------------------
// Construction: the reference sets bit (doc % 8) of byte doc / 8
// of row XXH64(canon(term), seed j) % signature_size for every term of every document
// (cobs/construction/classic_index.cpp:40-73).  One thread per position of the term text; the
// text is a sequence of stretches (documents.hpp): in a raw stretch every k-gram is a term, in a
// line stretch a position starts a term if the next k characters hold no '\n'.  With
// canonicalize = 1 the reference hashes the canonicalised buffer even when it holds invalid
// characters (mapped to 0), which the generic byte view reproduces; 31-mers of valid bases --
// nearly all of a DNA collection -- take the register path of the query hash kernel instead
// (unaligned dword loads, canon31, unrolled XXH64).  set_term_bit (term_hash.hpp) is where a bit goes.

// One thread per (four consecutive rows, one 32-document word of the matrix row): reads the rows'
// bytes from every plane whose column falls into the word (dword loads, coalesced across the
// rows of a wave), ORs the bits into the four words.  Launches of one build are ordered on one
// stream and every (row, word) belongs to one thread, so the read-modify-write needs no atomic.
__global__ __launch_bounds__(256) void pack_bytemap_kernel(PackArgs a) {
    const uint32_t w0 = a.col_base >> 5, w1 = (a.col_base + a.ndocs - 1u) >> 5;      // words the launch touches
    const uint64_t nquads = (a.rows + 3u) / 4u;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t quad = gid % nquads;                   // consecutive threads = consecutive rows
    const uint32_t w = w0 + (uint32_t)(gid / nquads);
    if (w > w1) return;
    const uint64_t r0 = quad * 4u;
    const uint32_t c0 = max(a.col_base, w << 5), c1 = min(a.col_base + a.ndocs, (w + 1u) << 5);
    uint32_t acc[4] = {0u, 0u, 0u, 0u};
    for (uint32_t c = c0; c < c1; ++c) {
        const uint32_t x = *reinterpret_cast<const uint32_t*>(a.bytemap + (uint64_t)(c - a.col_base) * a.bm_stride + r0);
        const uint32_t b = c & 31u;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] |= ((x >> (8 * i)) & 1u) << b;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (r0 + i < a.rows && acc[i] != 0u) {
            uint32_t* m = a.matrix + ((r0 + i) * a.row_bytes) / 4u + w;
            *m |= acc[i];
        }
    }
}

__global__ __launch_bounds__(256) void build_kernel(BuildArgs a, uint64_t total_bytes) {
    // the stretch of the block's first position (wave-uniform search), then a few steps per thread
    const uint64_t base = (uint64_t)blockIdx.x * 256u;
    uint32_t lo = 0, hi = a.nsegs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.seg_off[mid] <= base) lo = mid; else hi = mid;
    }
    const uint64_t gid = base + threadIdx.x;
    if (gid >= total_bytes) return;
    while (a.seg_off[lo + 1] <= gid) ++lo;            // seg_off[nsegs] = total_bytes > gid
    const uint32_t k = a.term_size;
    if (gid + k > a.seg_off[lo + 1]) return;          // the term would leave its stretch
    const uint32_t colw = a.seg_col[lo];
    if (colw == kBuildGapStretch) return;
    const bool raw = (colw & kBuildRawStretch) != 0u;
    const uint32_t doc = colw & ~kBuildRawStretch;
    const uint8_t* p = a.text + gid;
    if (k == 31u) {
        // the 31-mer and one following byte as 8 (unaligned) dwords; the text buffer is padded
        uint32_t f[8];
        {
            const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
            const uint32_t* w = reinterpret_cast<const uint32_t*>(p - mis);
            uint32_t r[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) r[j] = w[j];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                f[j] = mis == 0 ? r[j] : (uint32_t)(((uint64_t)r[j] | ((uint64_t)r[j + 1] << 32)) >> (8 * mis));
        }
        f[7] &= 0x00FFFFFFu;
        if (!raw) {
            bool nl = false;
#pragma unroll
            for (int j = 0; j < 8; ++j) nl |= has_newline(f[j]);
            if (nl) return;                           // the term would span a sequence boundary
        }
        bool fast = true;
        uint32_t c[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) c[j] = f[j];
        if (a.canonicalize != 0) {
#pragma unroll
            for (int j = 0; j < 7; ++j) fast &= all_acgt(f[j]);
            fast &= all_acgt(f[7] | 0x41000000u);
            if (fast) canon31(f, c);
        }
        if (fast) {
            for (uint32_t j = 0; j < a.num_hashes; ++j) {
                const uint64_t row = fast_mod(xxh64_31(c, (uint64_t)j), a.signature_size, a.magic);
                set_term_bit(a, doc, row);
            }
            return;
        }
    } else if (!raw) {
        for (uint32_t i = 0; i < k; ++i)
            if (p[i] == '\n') return;                 // the term would span a sequence boundary
    }
    KmerView kv{p, k, 0u};
    if (a.canonicalize != 0) {
        uint32_t mode = 1;
        for (uint32_t s = 0; s < k / 2; ++s) {
            const int f = (int)fwd_base(p[s]);
            const int r = (int)rev_base(p[k - 1 - s]);
            if (f < r) break;
            if (f > r) { mode = 2; break; }
        }
        kv.mode = mode;
    }
    for (uint32_t j = 0; j < a.num_hashes; ++j) {
        const uint64_t row = fast_mod(xxh64_view(kv, (uint64_t)j), a.signature_size, a.magic);
        set_term_bit(a, doc, row);
    }
}

// ---------------------------------------------------------------------------
// procedural index bits (same definition as the checker's generator)

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// classic_construct_random (construction/classic_index.cpp:661-725): every document is
// document_size random 31-mers; each is canonicalised, hashed and its bit set.  One thread per
// (document, k-mer); the 31 bases are the low 62 bits of mix64(mix64(seed ^ doc) + j), two bits
// per base (A C G T), first base in the lowest bits.
__global__ __launch_bounds__(256) void random_build_kernel(RandomBuildArgs a, uint64_t total) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const uint64_t doc = gid / a.document_size, j = gid - doc * a.document_size;
    uint64_t bits = mix64(mix64(a.seed ^ (a.doc0 + doc)) + j);
    uint32_t f[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t code = (uint32_t)(bits >> (2 * (4 * w + b))) & 3u;
            // A 0x41, C 0x43, G 0x47, T 0x54
            const uint32_t ch = code == 0 ? 0x41u : code == 1 ? 0x43u : code == 2 ? 0x47u : 0x54u;
            v |= ch << (8 * b);
        }
        f[w] = v;
    }
    f[7] &= 0x00FFFFFFu;
    uint32_t c[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) c[w] = f[w];
    canon31(f, c);
    const uint64_t col = a.doc0 + doc;
    const uint64_t byte_in_row = col >> 3;
    const uint32_t bit = 1u << ((uint32_t)(byte_in_row & 3u) * 8u + (uint32_t)(col & 7u));
    for (uint32_t h = 0; h < a.num_hashes; ++h) {
        const uint64_t row = fast_mod(xxh64_31(c, (uint64_t)h), a.signature_size, a.magic);
        atomicOr(a.matrix + (row * a.row_bytes + byte_in_row) / 4u, bit);
    }
}

// classic_combine (construction/classic_index.cpp:195-327): row r of the output is the rows r of
// the inputs concatenated at BIT granularity (input i contributes its row_bits[i] documents).
// One thread per output byte.
__global__ __launch_bounds__(256) void combine_kernel(CombineArgs a) {
    const uint64_t total = a.rows * a.dst_row_bytes;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t row = i / a.dst_row_bytes;
        const uint64_t ob = i - row * a.dst_row_bytes;
        uint64_t bit = ob * 8;                                  // first output document of this byte
        // source holding document `bit`: last s with bit_off[s] <= bit
        uint32_t lo = 0, hi = a.nsrc;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.bit_off[mid] <= bit) lo = mid; else hi = mid;
        }
        uint32_t sidx = lo, v = 0;
#pragma unroll 1
        for (uint32_t b = 0; b < 8 && bit < a.bit_off[a.nsrc]; ++b, ++bit) {
            while (bit >= a.bit_off[sidx + 1]) ++sidx;          // sources without documents are skipped
            const uint64_t sb = bit - a.bit_off[sidx];
            const uint8_t byte = a.src[sidx][row * a.src_row_bytes[sidx] + (sb >> 3)];
            v |= ((uint32_t)(byte >> (sb & 7u)) & 1u) << b;
        }
        a.dst[i] = (uint8_t)v;
    }
}

__device__ __forceinline__ uint64_t synth_word(uint64_t seed, uint32_t page, uint64_t row, uint64_t w) {
    const uint64_t key = mix64(seed ^ mix64(((uint64_t)page << 40) ^ row));
    const uint64_t c = key + w * 6;
    const uint64_t x = mix64(c) & mix64(c + 1);
    const uint64_t y = mix64(c + 2) & mix64(c + 3) & mix64(c + 4) & mix64(c + 5);
    return x | y;
}

// grid: blockIdx.y = local page, grid-stride over (row, 8-byte word) of that page
__global__ __launch_bounds__(256) void synth_kernel(SynthArgs a) {
    const uint32_t p = blockIdx.y;
    const PageDev pd = a.pages[p];
    const uint32_t wpr = a.pitch / 8u;                    // words per HBM row
    const uint64_t nwords = (pd.sig + 1) * (uint64_t)wpr; // incl. the zero row
    const uint32_t fpage = a.first_page + p;
    const uint64_t first_doc = (uint64_t)fpage * a.page_docs;
    const uint64_t live = a.num_docs > first_doc ? a.num_docs - first_doc : 0;   // real documents of the page
    uint64_t* dst = reinterpret_cast<uint64_t*>(a.blob + pd.base);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t row = i / wpr;
        const uint32_t w = (uint32_t)(i - row * wpr);
        uint64_t v = 0;
        if (row < pd.sig) {
            const uint64_t fb = a.col0 + (uint64_t)w * 8u;     // file-level byte of this word
            // local bytes beyond valid_bytes and file bytes beyond the row are zero
            const uint64_t gw = fb >> 3;
            uint64_t x = synth_word(a.seed, fpage, row, gw);
            if ((fb & 7u) != 0) {      // column shard not 8-byte aligned: stitch two words
                const uint64_t x2 = synth_word(a.seed, fpage, row, gw + 1);
                const uint32_t s = (uint32_t)(fb & 7u) * 8u;
                x = (x >> s) | (x2 << (64 - s));
            }
#pragma unroll
            for (uint32_t b = 0; b < 8; ++b) {
                const uint64_t lb = (uint64_t)w * 8u + b;      // local byte
                const uint64_t gb = fb + b;                    // file-level byte
                uint32_t byte = (uint32_t)(x >> (8 * b)) & 0xFFu;
                if (lb >= pd.valid_bytes || gb >= a.row_bytes || gb * 8 >= live) byte = 0;
                else if (gb * 8 + 8 > live) byte &= (1u << (uint32_t)(live - gb * 8)) - 1u;
                v |= (uint64_t)byte << (8 * b);
            }
        }
        dst[i] = v;
    }
}

// cobs_gpu_plant: one thread per term of the text.  Document i holds term t iff mix64(salt ^ doc << 32 ^ t) % 1000 <
// keep_permille (the test suite's checker restates this rule); a held term sets, for each of its H hashes, bit doc % 8
// of byte doc / 8 of row hash % S_p -- what classic_index.cpp:40-73 does for a document's own terms.
__global__ __launch_bounds__(256) void plant_kernel(PlantArgs a) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t k = a.term_size;
    if (a.len < k || t > a.len - k) return;
    const uint8_t* text = a.text + t;
    KmerView kv{text, k, 0u};
    if (a.canonicalize != 0) {
        for (uint32_t s = 0; s < k; ++s)
            if (fwd_base(text[s]) == 0) { *a.bad = 1u; return; }
        uint32_t mode = 1;
        for (uint32_t s = 0; s < k / 2; ++s) {
            const int f = (int)fwd_base(text[s]);
            const int r = (int)rev_base(text[k - 1 - s]);
            if (f < r) break;
            if (f > r) { mode = 2; break; }
        }
        kv.mode = mode;
    }
    for (uint32_t j = 0; j < a.num_hashes; ++j) {
        const uint64_t h = xxh64_view(kv, (uint64_t)j);
        for (uint32_t i = 0; i < a.ndocs; ++i) {
            const PlantDoc d = a.docs[i];
            if (!d.col) continue;
            if (mix64(a.salt ^ ((uint64_t)d.doc << 32) ^ (uint64_t)t) % 1000u >= d.keep_permille) continue;
            uint8_t* byte = d.col + (h % d.sig) * (uint64_t)d.pitch;
            const uintptr_t addr = reinterpret_cast<uintptr_t>(byte);
            atomicOr(reinterpret_cast<uint32_t*>(addr & ~(uintptr_t)3), 1u << (8u * (uint32_t)(addr & 3u) + d.bit));
        }
    }
}

// rows [row0, row0 + nrows) of one sub-index of the procedural index, packed `pitch` bytes apart
// (the file writer: cobs_gpu_write_synthetic)
__global__ __launch_bounds__(256) void synth_rows_kernel(SynthRowsArgs a) {
    const uint32_t wpr = a.pitch / 8u;
    const uint64_t nwords = a.nrows * (uint64_t)wpr;
    uint64_t* dst = reinterpret_cast<uint64_t*>(a.dst);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / wpr;
        const uint32_t w = (uint32_t)(i - r * wpr);
        const uint64_t x = synth_word(a.seed, a.page, a.row0 + r, w);
        uint64_t v = 0;
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) {
            const uint64_t gb = (uint64_t)w * 8u + b;          // row byte
            uint32_t byte = (uint32_t)(x >> (8 * b)) & 0xFFu;
            if (gb >= a.row_bytes || gb * 8 >= a.live_docs) byte = 0;
            else if (gb * 8 + 8 > a.live_docs) byte &= (1u << (uint32_t)(a.live_docs - gb * 8)) - 1u;
            v |= (uint64_t)byte << (8 * b);
        }
        dst[i] = v;
    }
}

// staged raw rows -> pitched rows (16 bytes per thread), zero padding to the pitch
__global__ __launch_bounds__(256) void repitch_kernel(RepitchArgs a) {
    const uint32_t cpr = a.dst_pitch / 16u;
    const uint64_t total = a.rows * cpr;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t row = i / cpr;
        const uint32_t c = (uint32_t)(i - row * cpr);
        const uint8_t* s = a.src + row * a.src_pitch + a.src_col0 + (uint64_t)c * 16u;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t b = 0; b < 16; ++b) {
            if (c * 16u + b < a.copy_bytes) w[b >> 2] |= (uint32_t)s[b] << (8 * (b & 3u));
        }
        *reinterpret_cast<uint4*>(a.dst + row * a.dst_pitch + (uint64_t)c * 16u) =
            make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ---------------------------------------------------------------------------
// launchers

hipError_t launch_build(const BuildArgs& a, uint64_t total_bytes, hipStream_t stream) {
    if (total_bytes == 0) return hipSuccess;
    const uint64_t blocks = (total_bytes + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(build_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, a, total_bytes);
    return hipGetLastError();
}

hipError_t launch_pack_bytemap(const PackArgs& a, hipStream_t stream) {
    if (a.ndocs == 0 || a.rows == 0) return hipSuccess;
    const uint32_t nwords = ((a.col_base + a.ndocs - 1u) >> 5) - (a.col_base >> 5) + 1u;
    const uint64_t threads = (a.rows + 3u) / 4u * nwords;
    const uint64_t blocks = (threads + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_bytemap_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_random_build(const RandomBuildArgs& a, uint64_t ndocs, hipStream_t stream) {
    const uint64_t total = ndocs * a.document_size;
    if (total == 0) return hipSuccess;
    const uint64_t blocks = (total + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(random_build_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, a, total);
    return hipGetLastError();
}

hipError_t launch_combine(const CombineArgs& a, hipStream_t stream) {
    if (a.rows == 0 || a.dst_row_bytes == 0) return hipSuccess;
    hipLaunchKernelGGL(combine_kernel, dim3(8192), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_synth(const SynthArgs& a, hipStream_t stream) {
    if (a.npages == 0) return hipSuccess;
    hipLaunchKernelGGL(synth_kernel, dim3(2048, a.npages), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_plant(const PlantArgs& a, hipStream_t stream) {
    if (a.len < a.term_size || a.ndocs == 0) return hipSuccess;
    const uint32_t terms = a.len - a.term_size + 1;
    hipLaunchKernelGGL(plant_kernel, dim3((terms + 255) / 256), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_synth_rows(const SynthRowsArgs& a, hipStream_t stream) {
    if (a.nrows == 0) return hipSuccess;
    hipLaunchKernelGGL(synth_rows_kernel, dim3(4096), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_repitch(const RepitchArgs& a, hipStream_t stream) {
    if (a.rows == 0) return hipSuccess;
    const uint64_t total = a.rows * (a.dst_pitch / 16u);
    uint64_t blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(repitch_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace cobs_amd
