/*
 * include/cobs_gpu_batch.h -- the part of libcobs_gpu.so's C ABI that sits BESIDE the drop-in boundary
 * (include/cobs_gpu.h): device-resident query batches (inputs and counts stay in HBM: the benchmark's step, the
 * building blocks of the search calls), grouped search (per-group document totals and read votes), the one exchange step of the sub-index-sharded multi-GPU layout over RCCL
 * (one rank per process), cobs_gpu_search_batch over such a sharded index, the procedural benchmark index, and findere
 * scoring and the invalid-bases policy (query-time options beyond the reference's search).
 * Same conventions as cobs_gpu.h: plain pointers and sizes, cobs_gpu_status, nothing aborts.
 */
#ifndef COBS_GPU_BATCH_H
#define COBS_GPU_BATCH_H

#include "cobs_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cobs_gpu_batch cobs_gpu_batch;   /* device workspace of one query batch */
typedef struct cobs_gpu_comm cobs_gpu_comm;     /* one rank of an RCCL communicator (multi-GPU exchange) */

/* Parameters of a procedural (synthetic) index filled directly in HBM; the
 * benchmark-sized stand-in for `cobs classic-construct-random`
 * (construction/classic_index.cpp:661-725).  Bits are a pure function of
 * (seed, page, row, byte) with density ~0.297 so that any row can be recomputed
 * by a checker; documents >= num_docs have no bits. */
typedef struct cobs_gpu_synth {
    uint32_t kind;            /* 0 classic, 1 compact */
    uint32_t term_size;
    uint32_t canonicalize;
    uint32_t num_pages;       /* classic: 1 */
    uint64_t num_hashes;
    uint64_t page_size;       /* compact only */
    uint64_t num_docs;
    uint64_t seed;
    const uint64_t* signature_sizes;   /* num_pages entries */
} cobs_gpu_synth;

/* ---- findere ------------------------------------------------------------ */
/* findere (Robidou & Peterlongo, SPIRE 2021; kmindex -z), beyond the reference: with z in 1..7 a position p of
 * the query scores in a document only when its z + 1 consecutive terms p .. p + z are all present there, which
 * false-positive bits of the Bloom filters rarely are.  A query of T = |q| - k + 1 terms then has T - z positions:
 * scores and max_counts count windows, thresholds are ceil(threshold * (T - z)), and a query needs k + z characters
 * (COBS_GPU_ERR_QUERY_TOO_SHORT).  0 (the default) is the reference's count.  Every call and batch of the handle
 * uses the z set when it runs.  ERR_ARG: NULL or z > 7; ERR_UNSUPPORTED: z > 0 on a handle with an HBM budget. */
cobs_gpu_status cobs_gpu_set_findere(cobs_gpu_index* ix, uint32_t z);
cobs_gpu_status cobs_gpu_get_findere(const cobs_gpu_index* ix, uint32_t* z);
/* findere on every shard of the device list (the same rules as cobs_gpu_set_findere; no shard changes on error) */
cobs_gpu_status cobs_gpu_multi_set_findere(cobs_gpu_multi* m, uint32_t z);
cobs_gpu_status cobs_gpu_multi_get_findere(const cobs_gpu_multi* m, uint32_t* z);

/* ---- invalid bases ------------------------------------------------------ */
/* What a character outside ACGT in a query does (files with canonicalize != 0; the others accept every byte), beyond the
 * reference, which dies on the first one (classic_search.cpp:93-96).  A scored position p of a query (p < T - z) is VALID
 * when its k + z characters [p, p + k + z) are all upper-case A C G T; V = a query's valid positions in a file.
 *   ERROR (0, default): the whole call fails with COBS_GPU_ERR_INVALID_BASE, *bad_query = the first such query.
 *   MISS  (1): a term that holds such a character is absent from every document and nothing fails: a score counts the
 *              valid positions whose z + 1 terms are present; thresholds stay ceil(threshold * (T - z)).
 *   SKIP  (2): the same scores, and invalid positions leave the denominator: the threshold is ceil(threshold * V), at least
 *              1 when threshold > 0 (a read without a valid position matches nothing), 0 when threshold <= 0.
 * Score widths and the "single hash in total: index order" rule keep the nominal (T - z) * num_hashes; a query shorter
 * than k + z still fails the call.  cobs_gpu_hit_positions follows: the bit of an invalid position is 0.  Every call and
 * batch of the handle uses the policy set when it runs; ranks of a one-rank-per-process sharded search must set the same
 * one (as with findere).  ERR_ARG: NULL or a mode > 2. */
enum { COBS_GPU_INVALID_ERROR = 0, COBS_GPU_INVALID_MISS = 1, COBS_GPU_INVALID_SKIP = 2 };
cobs_gpu_status cobs_gpu_set_invalid_bases(cobs_gpu_index* ix, uint32_t mode);
cobs_gpu_status cobs_gpu_get_invalid_bases(const cobs_gpu_index* ix, uint32_t* mode);
/* ... on every shard of the device list (no shard changes on error) */
cobs_gpu_status cobs_gpu_multi_set_invalid_bases(cobs_gpu_multi* m, uint32_t mode);
cobs_gpu_status cobs_gpu_multi_get_invalid_bases(const cobs_gpu_multi* m, uint32_t* mode);
/* The positions every query of a synced batch was scored over in file `file` (out: nq entries): V under MISS and SKIP,
 * T - z under ERROR (and for a file with canonicalize == 0) -- what a caller divides a score by. */
cobs_gpu_status cobs_gpu_batch_scored_positions(const cobs_gpu_batch* b, size_t file, uint32_t* out);

/* ---- procedural index ---------------------------------------------------- */
cobs_gpu_status cobs_gpu_open_synthetic(const cobs_gpu_synth* desc,
                                        const cobs_gpu_options* opts, cobs_gpu_index** out);
/* The procedural index of cobs_gpu_open_synthetic written as a .cobs_classic / .cobs_compact FILE
 * (the generator tool of SURVEY 8f rank 2, cf. `cobs classic-construct-random`, src/cobs.cpp:243-291):
 * rows are produced on the device chunk by chunk and streamed to the file. */
cobs_gpu_status cobs_gpu_write_synthetic(const cobs_gpu_synth* desc, const char* out_path, int device);

/* True positives for a RESIDENT index (the procedural one above, or any index that is not streamed): the documents
 * docs[0..ndocs) of file `file_no` additionally contain the terms of `text` -- document docs[i] holds term t (the
 * term_size characters from position t) iff mix64(salt ^ (uint64_t)docs[i] << 32 ^ t) % 1000 < keep_permille[i]
 * (mix64 = the splitmix64 finaliser the procedural bits use) -- and a held term sets, for each of the index's hash
 * functions, the bit of the document in row hash % S_p of its sub-index, exactly what index construction does for a
 * document's own terms (construction/classic_index.cpp:40-73).  Random bits alone give counts ~ Binomial(T, 0.3): no
 * query ever reaches the CLI's default threshold 0.8; with planted documents the thresholded paths --
 * selection, hit pool, D2H of hits, ranking, the hit exchange -- carry data at full size.  Documents a shard does not
 * hold are skipped (every rank plants what it holds).  The test suite's checker restates the rule. */
cobs_gpu_status cobs_gpu_plant(cobs_gpu_index* ix, size_t file_no, const char* text, size_t len, const uint32_t* docs,
                               const uint32_t* keep_permille, size_t ndocs, uint64_t salt);

/* cobs_gpu_search_batch with the results in memory the LIBRARY owns: *hits / *hit_offsets (nq + 1 entries) point into a
 * result arena kept on the handle -- grown on demand, its pages faulted in once and reused by every later call (huge pages
 * where the host offers them on request) -- and stay valid until the next search call on this handle.  The form for a
 * caller that would otherwise allocate a fresh result array per call: the reference's default call returns one record per
 * document and query (classic_search.cpp:450), 307 MB for 256 queries x 100 000 documents, and a fresh array costs
 * 75 000 first-touch page faults per call.  (The reference's own callers keep ONE result vector: src/cobs.cpp:618-626.)
 * It is also the form for a THRESHOLDED call whose number of hits the caller cannot guess: the arena grows while the
 * passes of the call come home, where cobs_gpu_search_batch can only report COBS_GPU_ERR_CAPACITY after the whole search
 * has run and be called a second time. */
cobs_gpu_status cobs_gpu_search_batch_view(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                           double threshold, size_t num_results, const cobs_gpu_hit** hits,
                                           const size_t** hit_offsets, size_t* bad_query);

/* WHERE in each query its hits matched: for the hit list a search call returned (hits[hit_offsets[j] .. hit_offsets[j+1])
 * belong to query j; `score` of the records is ignored, so any (file, document) pairs may be asked about) the per-position
 * presence vector of every hit.  With T = len - term_size(file) + 1 terms and the handle's findere z, a hit has
 * n = T - z positions; position p is set when terms p .. p + z are all present in the document (every term: all of the
 * file's hash bits set in the document's column, as the scan counts it).  Hit i owns the words
 * bits[bit_offsets[i] .. bit_offsets[i+1]) (bit_offsets: n_hits + 1 entries, in 64-bit words; ceil(n / 64) words per hit),
 * position p is bit p % 64 of word p / 64, bits >= n of the last word are 0 -- the popcount of a hit's words is the score
 * the search reported for it.  A second call over a hit list, not part of the scan: it hashes the queries that have hits
 * again and reads one bit per looked-up row.
 * Errors as cobs_gpu_search_batch reports them (*bad_query = the offending query); COBS_GPU_ERR_ARG for a file or
 * document number out of range or descending offsets; COBS_GPU_ERR_CAPACITY when cap_words is too small -- bit_offsets
 * and *words_needed (optional) are filled, so the call can be repeated (bits may be NULL when cap_words is 0);
 * COBS_GPU_ERR_UNSUPPORTED on a handle opened with an HBM budget or as one shard of several (the rows are not all
 * resident there). */
cobs_gpu_status cobs_gpu_hit_positions(cobs_gpu_index* ix, const char* const* queries, const size_t* lens,
                                       size_t nq, const cobs_gpu_hit* hits, const size_t* hit_offsets,
                                       uint64_t* bits, size_t cap_words, size_t* bit_offsets,
                                       size_t* words_needed, size_t* bad_query);

/* ---- grouped search ------------------------------------------------------ */
/* Which documents a SET of queries comes from (a read pair, the reads of an amplicon, a whole sample), beyond the
 * reference: the nq queries form n_groups CONTIGUOUS groups, group g = the queries [group_offsets[g], group_offsets[g+1])
 * (n_groups + 1 non-decreasing entries, the first 0, the last nq; empty groups are allowed).  With score(q, f, d) exactly
 * what cobs_gpu_search_batch scores for query q in document d of file f (the handle's findere z and invalid-bases policy):
 *   score = the SUM of score(q, f, d) over the group's queries,
 *   votes = the number of its queries with score(q, f, d) >= thr(q, f), the threshold cobs_gpu_search_batch applies for
 *           read_threshold (ceil(read_threshold * (T - z)), or the `skip` rule) -- "voted" is "was a hit of that search";
 *           read_threshold <= 0 gives every document the group's size,
 *   P[g][f] = the positions the group's queries are scored over in file f, summed: T - z under ERROR and MISS, V under SKIP
 *           (the denominators of the per-query thresholds); written to positions[g * n_files + f] when positions != NULL.
 * The result of group g is the real documents (padding slots never count) with score >= max(1, ceil(threshold * P[g][f])),
 * computed in double -- a group with P = 0 returns nothing --, every real document when threshold <= 0; ordered by score
 * descending, then (file_no, doc) ascending, cut to the first num_results when num_results > 0.  The reference's
 * "max_counts <= 1: index order" rule does NOT apply to groups.  hits[hit_offsets[g] .. hit_offsets[g+1]) belong to group g.
 * Sums are 32-bit: a group whose positions in some file could reach 2^32 fails the call with COBS_GPU_ERR_ARG (the message
 * names the group).  Sums and votes are additive: split such a sample over several calls and add the parts.
 * The scores never leave the device: every pass's score rows are added to the groups' totals where they lie.
 * Errors as cobs_gpu_search_batch reports them (too short, an invalid base under ERROR: *bad_query = the offending query);
 * COBS_GPU_ERR_CAPACITY when cap is too small -- hit_offsets then holds the needed sizes (hit_offsets[n_groups] the total),
 * known from the one scan that ran; COBS_GPU_ERR_ARG for malformed offsets; COBS_GPU_ERR_UNSUPPORTED on a handle opened
 * with an HBM budget or as one shard of several (and, in the mirrors, on the device list). */
typedef struct cobs_gpu_group_hit { uint32_t file_no, doc, score, votes; } cobs_gpu_group_hit;   /* 16 bytes */
cobs_gpu_status cobs_gpu_search_groups(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                       const size_t* group_offsets, size_t n_groups,
                                       double threshold, double read_threshold, size_t num_results,
                                       cobs_gpu_group_hit* hits, size_t cap, size_t* hit_offsets /* n_groups + 1 */,
                                       uint64_t* positions /* optional */, size_t* bad_query);

/* ---- best of a group ----------------------------------------------------- */
/* For every document the BEST query of a group, beyond the reference: typing -- the alleles of a locus, the members of a
 * gene family are one group, and the question is which of them fits a genome best, and how well.  The other half of the
 * grouped call (a best member cannot be recovered from a sum).  Group g is the queries [group_offsets[g],
 * group_offsets[g+1]) of the call, as in cobs_gpu_search_groups.  For query q and file f:
 *   s(q, d) = the score cobs_gpu_search_batch gives document d (the handle's findere z and invalid-bases policy),
 *   P(q, f) = the positions that score is out of: T - z under ERROR and MISS, under SKIP the valid positions K1 counts (it
 *             can be 0; a file with canonicalize == 0 keeps T - z) -- the per-query quantity cobs_gpu_search_groups sums.
 * Member a is BETTER than member b in document d when, in this order:
 *   1. s_a * P_b > s_b * P_a: the larger fraction s / P, compared exactly as 64-bit products.  A member with P = 0 has
 *      s = 0 and the fraction 0: it compares as 0 / 1 (its cross products would otherwise equal everybody's);
 *   2. s_a > s_b: at equal fraction the longer member, which carries more evidence;
 *   3. a < b by index in the call.
 * For every (group, file, real document) the call finds
 *   query     = the best member, as its index in the call,
 *   score     = its s,   positions = its P,
 *   ties      = the number of the group's members whose fraction EQUALS the best one's (s * P_best == s_best * P, P = 0
 *               taken as 0 / 1), the best one included: two alleles that fit equally well are an ambiguous call.
 * A document is reported for a group when score >= max(1, ceil(threshold * positions)), the product formed in double;
 * threshold <= 0 reports every real document of every file, score 0 included.  A group without members reports nothing.
 * A group's records are ordered by fraction descending (exact cross-multiplication), then score descending, then
 * (file_no, doc) ascending, cut to the first num_results when num_results > 0; the reference's "max_counts <= 1: index
 * order" rule does NOT apply; padding slots never appear.  hits[hit_offsets[g] .. hit_offsets[g+1]) belong to group g.
 * The scores never leave the device: every pass's score rows are merged into the per-(group, document) state of the best
 * member where they lie; the merge is associative, so a group that is cut by a device pass gives the same records.
 * Errors as cobs_gpu_search_groups reports them: too short, too long, an invalid base under ERROR (*bad_query = the
 * offending query) before anything is launched where the host can see it; COBS_GPU_ERR_CAPACITY when cap is too small --
 * hit_offsets then holds the needed sizes -- or when the state of n_groups x documents does not fit (use fewer groups per
 * call); COBS_GPU_ERR_ARG for malformed offsets; COBS_GPU_ERR_UNSUPPORTED on a handle opened with an HBM budget or as one
 * shard of several (and, in the mirrors, on the device list).  cobs_gpu_best_ms (cobs_gpu_diag.h) reads the timers. */
typedef struct cobs_gpu_best_hit { uint32_t file_no, doc, query, score, positions, ties; } cobs_gpu_best_hit;   /* 24 bytes */
cobs_gpu_status cobs_gpu_search_best(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                     const size_t* group_offsets, size_t n_groups, double threshold, size_t num_results,
                                     cobs_gpu_best_hit* hits, size_t cap, size_t* hit_offsets /* n_groups + 1 */,
                                     size_t* bad_query);

/* ---- filter fill --------------------------------------------------------- */
/* How many bits every document's Bloom filter has set, beyond the reference: bits[i] = the rows r in [0, S_p) of the
 * document's sub-index whose bit of score slot slot_begin + i is set (the zero row the engine appends is never counted;
 * a padding slot is counted like any other column and is 0 in a well-formed file).  `bits` receives slot_count entries
 * for the file-level slots [slot_begin, slot_begin + slot_count) of cobs_gpu_index_info -- the file's counts_size on an
 * unsharded handle; *needed (optional) is always set to that number.  With fill = bits / S_p a k-mer unrelated to the
 * document still hits it with probability fill^H: what a raw score is worth (the mirrors' doc_fill / fpr_adjust).
 * Counted on the device in one sweep over the index -- resident chunks where they lie, the streamed chunks of a handle
 * with an HBM budget whole through its stream buffers, once each -- on the first request for a file and cached on the
 * handle (8 bytes per slot); cobs_gpu_plant drops the cache of the file it changes.
 * COBS_GPU_ERR_ARG: NULL handle or file_no out of range (before any device work); COBS_GPU_ERR_CAPACITY: cap is too
 * small (host arithmetic, nothing runs; bits may be NULL when cap is 0).  The device list (cobs_gpu_multi_*) has no
 * counterpart: ask the shards (cobs_gpu_multi_index). */
cobs_gpu_status cobs_gpu_doc_bits(cobs_gpu_index* ix, size_t file_no, uint64_t* bits, size_t cap, size_t* needed);

/* ---- document similarity ------------------------------------------------- */
/* Shared filter bits of documents, beyond the reference.  For documents a and b of the SAME sub-index p of file f,
 *   shared(f, a, b) = the rows r in [0, S_p) in which both have their bit set;   shared(f, a, a) = cobs_gpu_doc_bits' value.
 * A classic index is one sub-index; the sub-index of document d of a compact index is d / (8 * page_size).  Documents of
 * different sub-indexes have different S_p and are not comparable: the call never pairs them.
 * For every reference refs[i] (a real document of file_no; references may repeat, come in any order and lie in different
 * sub-indexes) the cells shared[offsets[i] .. offsets[i+1]) receive shared(file_no, refs[i], d) for every score slot d of
 * refs[i]'s sub-index, in slot order: 8 * page_size cells for a compact index, counts_size for a classic one; a padding
 * slot is counted like any other column and is 0 in a well-formed file.  offsets (n_refs + 1 entries) is filled whenever
 * it is not NULL and *needed (optional) is set to offsets[n_refs], also by a call that fails with COBS_GPU_ERR_CAPACITY
 * (shared is NULL or cap is too small; shared is not written).  shared == NULL with cap == 0 is the sizing call and
 * succeeds.  n_refs == 0 succeeds with *needed = 0.
 * On the device the references of one sub-index are taken in panels of 8, in ascending document order: a panel is one
 * pass that extracts the references' bits of every row and one sweep over the sub-index's rows, so a call makes
 * sum over sub-indexes of ceil(its references / 8) sweeps (cobs_gpu_similarity_ms, cobs_gpu_diag.h).  Nothing is cached.
 * Everything the host can refuse is refused before any device work: COBS_GPU_ERR_ARG (NULL handle, NULL refs, file_no out
 * of range, a reference >= the file's num_docs), COBS_GPU_ERR_UNSUPPORTED on a handle opened with an HBM budget or as one
 * shard of several (its rows or columns are not all resident).  The device list (cobs_gpu_multi_*) has no counterpart. */
cobs_gpu_status cobs_gpu_doc_shared_bits(cobs_gpu_index* ix, size_t file_no, const uint32_t* refs, size_t n_refs,
                                         uint64_t* offsets /* n_refs + 1 */, uint64_t* shared, size_t cap, size_t* needed);
/* The Bloom-filter estimate of the Jaccard index and the containment of two documents' k-mer sets from their fills and
 * their shared bits (host arithmetic, no device): out = {bit_jaccard, jaccard, containment_a_in_b, containment_b_in_a,
 * n_inter}.  All in double, with t_or = bits_a + bits_b - shared_ab and n(t) = -(sig / num_hashes) * log1p(-t / sig):
 *   n_inter = max(0, n(bits_a) + n(bits_b) - n(t_or)),   jaccard = n_inter / n(t_or),
 *   containment_a_in_b = min(1, n_inter / n(bits_a)),   containment_b_in_a = min(1, n_inter / n(bits_b)),
 *   bit_jaccard = shared_ab / t_or;   a zero denominator gives 0.
 * t_or == sig (a saturated filter): the three estimates and n_inter are NaN, bit_jaccard still answers.
 * COBS_GPU_ERR_ARG: sig == 0, num_hashes == 0, shared_ab > min(bits_a, bits_b), bits_a or bits_b > sig, t_or > sig (no
 * two columns of one sub-index give that), out == NULL. */
cobs_gpu_status cobs_gpu_jaccard_estimate(uint64_t sig, uint32_t num_hashes, uint64_t bits_a, uint64_t bits_b, uint64_t shared_ab,
                                          double out[5]);

/* ---- query prevalence ---------------------------------------------------- */
/* For every position of a query, HOW MANY documents hold it, beyond the reference: the profile along the query (a
 * conservation track of a gene, the core and accessory stretches of a contig, the ubiquitous k-mers that inflate every
 * score of a read).  With T = len - term_size(file) + 1 terms and the handle's findere z a query has n = T - z positions in
 * a file; position p is set in document d when terms p .. p + z are all present in d (every term: all of the file's hash
 * bits set in d's column, as the scan counts it).  counts[offsets[q * n_files + f] + p] = the REAL documents of file f in
 * which position p of query q is set; padding slots never count, whatever bits a file holds there.  Segment (q, f) is
 * counts[offsets[q * n_files + f] .. offsets[q * n_files + f + 1]) -- offsets has nq * n_files + 1 entries.  Under
 * COBS_GPU_INVALID_MISS / _SKIP a position whose window holds a character outside ACGT is 0; under _ERROR the call fails
 * as a search does.  The sum of a segment equals the sum over the file's real documents of the scores a search reports
 * for q, and counts[..p] equals the hits whose cobs_gpu_hit_positions bit p is set.
 * On one shard of several the counts cover the documents of the shard's own slots: they are additive, the parts of all
 * shards add up to the unsharded answer.  One gather over the resident rows, as the scan's, reduced across documents.
 * Everything the host can refuse is refused before any device work: COBS_GPU_ERR_ARG (NULL arguments),
 * COBS_GPU_ERR_QUERY_TOO_SHORT / _TOO_LONG (*bad_query = the offending query), COBS_GPU_ERR_CAPACITY when cap is too small
 * -- offsets and *needed (optional) are filled, so the call can be repeated (counts may be NULL when cap is 0) --,
 * COBS_GPU_ERR_UNSUPPORTED on a handle opened with an HBM budget (its rows are not all resident).
 * COBS_GPU_ERR_INVALID_BASE comes from the device (*bad_query).  The device list (cobs_gpu_multi_*) has no counterpart:
 * ask the shards (cobs_gpu_multi_index) and add. */
/* offsets: nq * nfiles + 1 entries; segment (q, f) = counts[offsets[q*nfiles+f] .. offsets[q*nfiles+f+1]), length T_f - z */
cobs_gpu_status cobs_gpu_prevalence(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                    uint32_t* counts, size_t cap, size_t* offsets, size_t* needed, size_t* bad_query);

/* ---- IDF-weighted search ------------------------------------------------- */
/* A search in which rare k-mers count for more, beyond the reference.  A plain score counts every position as 1; a k-mer
 * that most of the collection holds then lifts every document over a threshold together.  Here, with c(q, f, p) exactly
 * what cobs_gpu_prevalence returns (the real documents of file f in which terms p .. p + z of query q are all present,
 * z the handle's findere) and D_f the real documents of file f, position p carries the weight
 *   w = cobs_gpu_idf_weight(D_f, c):  0 when c = 0, else 1 + max{ j in 0..14 : c * 2^j <= D_f }
 *                                     = 1 + min(14, floor(log2(D_f / c))), integer arithmetic only
 * -- 0..15: a k-mer in more than half of the documents weighs 1, a singleton among >= 16384 documents 15 --, and
 *   score(q, f, d) = the sum of w(q, f, p) over the positions p set in document d (real documents only),
 *   W(q, f)        = the sum of w(q, f, p) over all n = T_f - z positions; total_weight[q * n_files + f] when not NULL.
 * A position that no document holds carries no weight -- a sequencing error, or a window with a character outside ACGT
 * under COBS_GPU_INVALID_MISS / _SKIP: the two policies give the SAME result here (a skipped position and a missed one
 * both weigh 0 and W counts neither).  Under _ERROR an invalid base fails the call as it does for a search.
 * For threshold > 0 a real document is a hit when score >= max(1, ceil(threshold * W(q, f))), computed in double; a
 * (query, file) with W = 0 returns nothing.  For threshold <= 0 every real document is returned, score 0 included.
 * Per query the records are ordered by score descending, then (file_no, doc) ascending, and cut to the first num_results
 * when num_results > 0; the reference's "max_counts <= 1: index order" rule does NOT apply.  hits[hit_offsets[q] ..
 * hit_offsets[q+1]) belong to query q, `score` is the weighted score.
 * 15 * n must stay below 2^20 (the counter planes the scan is built for): a query with more than 69905 positions in some
 * file fails with COBS_GPU_ERR_QUERY_TOO_LONG.
 * Everything the host can refuse is refused before any device work: COBS_GPU_ERR_ARG (NULL arguments),
 * COBS_GPU_ERR_QUERY_TOO_SHORT / _TOO_LONG (*bad_query = the offending query), COBS_GPU_ERR_UNSUPPORTED on a handle opened
 * with an HBM budget (its rows are not all resident) or as one shard of several (the weights need every shard's counts).
 * COBS_GPU_ERR_INVALID_BASE comes from the device (*bad_query).  COBS_GPU_ERR_CAPACITY when cap is too small --
 * hit_offsets then holds the needed sizes (hit_offsets[nq] the total), known from the one scan that ran (hits may be NULL
 * when cap is 0).  COBS_GPU_ERR_HIP when the device has no room for the hit records of a pass (hit_offsets stay 0: raise the
 * threshold or pass fewer queries).  The device list (cobs_gpu_multi_*) has no counterpart.
 * On the device: K1, the prevalence kernel into device cells, a kernel that turns the cells into one byte per position,
 * W and the thresholds, and a scan shaped like K2 that adds a position's weight where K2 adds 1 and appends the documents
 * that pass to a pool; no score matrix exists.  cobs_gpu_weighted_ms (cobs_gpu_diag.h) reads the stage timers. */
uint32_t cobs_gpu_idf_weight(uint64_t num_docs, uint64_t count);      /* host arithmetic, no device */
cobs_gpu_status cobs_gpu_search_weighted(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                         double threshold, size_t num_results,
                                         cobs_gpu_hit* hits, size_t cap, size_t* hit_offsets /* nq + 1 */,
                                         uint64_t* total_weight /* optional, nq * n_files: W(q,f) */, size_t* bad_query);

/* ---- document sets ------------------------------------------------------- */
/* Score a query against labelled SETS of documents (the assemblies of a species, a lineage, an outbreak, the runs of a
 * sample), beyond the reference.  Labels are per file: label[d] of the real documents d < D_f of file f is a set number in
 * [0, n_sets) or COBS_GPU_NO_SET (the document is in no set).  A set without a member in a file does not exist for that
 * file.  With T = len - term_size(f) + 1 terms and the handle's findere z a query has n = T - z positions in file f;
 * position p is set in document d exactly as cobs_gpu_prevalence and cobs_gpu_hit_positions define it (terms p .. p + z all
 * present, every hash bit set, the invalid-bases policy through K1's table).  For a non-empty set c of file f:
 *   any(q, f, c) = the positions set in AT LEAST ONE member of c (the pan-genome score: robust against gaps in any one member),
 *   all(q, f, c) = the positions set in EVERY member of c (the core score).
 * Padding slots and unlabelled documents never take part, whatever bits the file holds there.  A one-member set has
 * any == all == the score cobs_gpu_search_batch reports for that document; with every document of a file in one set, any =
 * the positions with prevalence > 0 and all = the positions with prevalence == D_f; always all <= min and max <= any over
 * the members' scores, and any <= n.
 * cobs_gpu_set_doc_sets: n_docs must equal the file's real document count; labels == NULL clears the file's labels; labels
 * replace earlier ones.  At most 2^28 sets per file.  The labels become segment records per 16-byte column chunk, built on
 * the host and uploaded once.  cobs_gpu_get_doc_sets: *n_sets = the n_sets of the file's labels (0: none); members
 * (optional, cap >= n_sets entries, else COBS_GPU_ERR_CAPACITY) receives the member count of every set.
 * cobs_gpu_search_sets: a set is a hit when its key (any or all, by rank_by) is >= max(1, ceil(threshold * P)), computed in
 * double; P is the denominator the search uses for that query and file -- n under ERROR and MISS, the V of
 * cobs_gpu_batch_scored_positions under SKIP (the rule of a one-query group of cobs_gpu_search_groups); P = 0 returns
 * nothing.  threshold <= 0 returns every non-empty set of every labelled file, key 0 included.  Per query the records are
 * ordered by key descending, then the other count descending, then (file_no, set) ascending, and cut to num_results when it
 * is > 0; the reference's "max_counts <= 1: index order" rule does NOT apply.  hits[hit_offsets[q] .. hit_offsets[q+1])
 * belong to query q.  A file without labels contributes nothing.
 * Everything the host can refuse is refused before any device work: COBS_GPU_ERR_ARG (NULL arguments, an n_docs mismatch, a
 * label >= n_sets that is not COBS_GPU_NO_SET, rank_by > 1), COBS_GPU_ERR_QUERY_TOO_SHORT / _TOO_LONG (*bad_query = the
 * offending query), COBS_GPU_ERR_UNSUPPORTED on a handle opened with an HBM budget or as one shard of several (any and all
 * are not additive over shards: that takes an exchange of the bitmaps; the mirrors also refuse on the device list),
 * COBS_GPU_ERR_HIP, with a message, when the two bitmaps of a single query do not fit the pass workspace (tuning key
 * pass_bytes).  COBS_GPU_ERR_INVALID_BASE comes from the device (*bad_query).  COBS_GPU_ERR_CAPACITY when cap is too small --
 * hit_offsets then holds the needed sizes (hit_offsets[nq] the total; hits may be NULL when cap is 0).
 * On the device: K1, a presence kernel that ORs two bit matrices [query][set][ceil(n / 32)] together (the gather of the
 * prevalence kernel reduced over labelled subsets of the columns), and a select kernel; passes are cut by pass_bytes and the
 * results do not depend on the cut.  cobs_gpu_sets_ms (cobs_gpu_diag.h) reads the stage timers. */
#define COBS_GPU_NO_SET 0xFFFFFFFFu
#define COBS_GPU_SETS_BY_ANY 0u
#define COBS_GPU_SETS_BY_ALL 1u
typedef struct cobs_gpu_set_hit { uint32_t file_no, set, any, all; } cobs_gpu_set_hit;   /* 16 bytes */
cobs_gpu_status cobs_gpu_set_doc_sets(cobs_gpu_index* ix, size_t file_no, const uint32_t* labels, size_t n_docs,
                                      uint32_t n_sets);
cobs_gpu_status cobs_gpu_get_doc_sets(const cobs_gpu_index* ix, size_t file_no, uint32_t* n_sets,
                                      uint32_t* members /* optional, n_sets entries */, size_t cap);
cobs_gpu_status cobs_gpu_search_sets(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                     double threshold, uint32_t rank_by, size_t num_results,
                                     cobs_gpu_set_hit* hits, size_t cap, size_t* hit_offsets /* nq + 1 */,
                                     size_t* bad_query);

/* ---- document sets: quorum and per-set prevalence -------------------------- */
/* The soft core of a set and the frequency of a stretch per set, beyond the reference.  `all` of cobs_gpu_search_sets is
 * brittle -- one fragmented assembly among 5 000 zeroes a position --, so pan-genome tools score the positions that at least
 * 95 % or 99 % of a set's members hold, and report how many members of every set hold a position: cobs_gpu_prevalence split
 * by set.  Position, n = T - z, "set in document d", the denominator P and the invalid-bases policies are exactly those of
 * cobs_gpu_search_sets and cobs_gpu_prevalence; the labels are those of cobs_gpu_set_doc_sets.  For file f with labels let c
 * range over the file's non-empty sets in ascending set number, members(f, c) = the real documents of f labelled c:
 *   count(q, f, c, p) = the members of c in which position p of query q is set.  Padding slots, slots >= D_f and unlabelled
 *                       documents never count, whatever bits the file holds there; under COBS_GPU_INVALID_MISS / _SKIP a
 *                       position whose window holds a character outside ACGT is 0.
 *   need(f, c)        = max(1, ceil(quorum * members(f, c))) for 0 < quorum <= 1, computed on the host in double, once per
 *                       set and call (the device never multiplies by quorum); any other quorum, NaN included, is
 *                       COBS_GPU_ERR_ARG.
 *   core(q, f, c)     = the positions p < n with count >= need(f, c);  any(q, f, c) = the positions with count > 0.
 *                       quorum = 1 gives core = `all` of cobs_gpu_search_sets; a quorum small enough that need = 1 gives
 *                       core = its `any`.
 * cobs_gpu_search_sets_quorum: a set is a hit when core >= max(1, ceil(threshold * P)), computed in double; P = 0 returns
 * nothing; threshold <= 0 returns every non-empty set of every labelled file.  Per query the records are ordered by core
 * descending, then any descending, then (file_no, set) ascending, and cut to num_results when it is > 0.
 * hits[hit_offsets[q] .. hit_offsets[q+1]) belong to query q.  COBS_GPU_ERR_CAPACITY when cap is too small -- hit_offsets
 * then holds the needed sizes (hit_offsets[nq] the total; hits may be NULL when cap is 0).
 * cobs_gpu_set_prevalence: segment (q, f) = counts[offsets[q * n_files + f] .. offsets[q * n_files + f + 1]) holds
 * nonempty_sets(f) * n(q, f) counts, set-major: the c-th non-empty set in ascending set number (the order
 * cobs_gpu_get_doc_sets implies) has its position p at offsets[q * n_files + f] + c * n + p.  A file without labels has an
 * empty segment.  COBS_GPU_ERR_CAPACITY when cap is too small -- offsets and *needed (optional) are filled, so the call can
 * be repeated (counts may be NULL when cap is 0); the sizes are host arithmetic, nothing has run.
 * Both refuse before any device work: COBS_GPU_ERR_ARG (NULL arguments, a bad quorum), COBS_GPU_ERR_QUERY_TOO_SHORT /
 * _TOO_LONG (*bad_query = the offending query), COBS_GPU_ERR_UNSUPPORTED on a handle opened with an HBM budget or as one
 * shard of several (the counts are additive over shards, but nothing adds them up yet; the mirrors also refuse on the device
 * list), COBS_GPU_ERR_HIP, with the sizes in the message, when the counts of a single query -- 4 bytes per (set, position),
 * 16 times the two bitmaps of cobs_gpu_search_sets -- do not fit the pass workspace (tuning key pass_bytes).
 * COBS_GPU_ERR_INVALID_BASE comes from the device (*bad_query).
 * On the device: K1, a kernel that zeroes the cells, a count kernel that reduces the prevalence kernel's gather over the
 * columns of one set at a time (from inverse segment records, built from the labels on the first of these calls and
 * dropped when the labels are replaced or cleared), and for the search a select kernel over the counts; passes are cut by
 * pass_bytes and the results do not depend on the cut.  cobs_gpu_set_quorum_ms (cobs_gpu_diag.h) reads the stage timers. */
typedef struct cobs_gpu_set_quorum_hit { uint32_t file_no, set, core, any; } cobs_gpu_set_quorum_hit;   /* 16 bytes */
cobs_gpu_status cobs_gpu_search_sets_quorum(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                            double threshold, double quorum, size_t num_results,
                                            cobs_gpu_set_quorum_hit* hits, size_t cap, size_t* hit_offsets /* nq + 1 */,
                                            size_t* bad_query);
cobs_gpu_status cobs_gpu_set_prevalence(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                        uint32_t* counts, size_t cap, size_t* offsets /* nq * n_files + 1 */, size_t* needed,
                                        size_t* bad_query);

/* ---- coverage search ------------------------------------------------------ */
/* A search whose score is the number of query BASES covered by the k-mers a document holds, beyond the reference.  One
 * substitution in a read removes the k k-mers that overlap it, but all other bases still lie inside a present k-mer.
 *   File and query.  File f has term size k_f, the handle findere z, query q the length L = len(q).
 *   Positions.       In file f the query has n = L - k_f + 1 - z positions.
 *   Set position.    Position p is set in document d exactly as cobs_gpu_prevalence and cobs_gpu_hit_positions define it:
 *                    terms p .. p + z are all present (the invalid-bases policy included, through K1's table).
 *   Span.            span = k_f + z.
 *   Covered bases.   A set position p covers bases p .. p + span - 1 of the query.  coverage(q, f, d) is the number of
 *                    bases b in [0, L) covered by at least one set position of d: 0 .. L.
 *   Bounds.          With s > 0 set positions: s + span - 1 <= coverage <= min(L, s * span).
 *   Threshold.       For threshold > 0 a real document is a hit when coverage >= max(1, ceil(threshold * L)), computed
 *                    in double.  For threshold <= 0 every real document is returned, coverage 0 included.
 *   Invalid bases.   Under COBS_GPU_INVALID_MISS and _SKIP a position whose window holds a non-ACGT character is not set;
 *                    the denominator stays L under both, so the two policies give the SAME result here, as they do for
 *                    the weighted search.  Under _ERROR an invalid base fails the call as it does for a search.
 *   Order.           Per query the records are ordered by coverage descending, then (file_no, doc) ascending, and cut to
 *                    the first num_results when num_results > 0; the reference's index-order rule does NOT apply.
 *                    hits[hit_offsets[q] .. hit_offsets[q+1]) belong to query q, `score` carries the coverage.
 * Everything the host can refuse is refused before any device work: COBS_GPU_ERR_ARG (NULL arguments),
 * COBS_GPU_ERR_QUERY_TOO_SHORT, COBS_GPU_ERR_QUERY_TOO_LONG for L >= 2^20 (*bad_query = the offending query),
 * COBS_GPU_ERR_UNSUPPORTED when span > 255 in some file, on a handle opened with an HBM budget (its rows are not all
 * resident) or as one shard of several.  The device list (cobs_gpu_multi_*) has no counterpart.
 * COBS_GPU_ERR_INVALID_BASE comes from the device (*bad_query).  COBS_GPU_ERR_CAPACITY when cap is too small --
 * hit_offsets then holds the needed sizes (hit_offsets[nq] the total), known from the one scan that ran (hits may be NULL
 * when cap is 0).  COBS_GPU_ERR_HIP when the device has no room for the hit records of a pass.
 * On the device: K1 and one scan that walks every document's positions in order with a bit-sliced countdown and appends
 * the documents that pass to a pool; no score matrix exists.  cobs_gpu_coverage_ms (cobs_gpu_diag.h) reads the timers.
 * cobs_gpu_covered_bases is the same count on the host, from one cobs_gpu_hit_positions bitmap of n positions (bit p of
 * words[p / 64]; bits at or beyond n are ignored): for every hit of any search,
 *   cobs_gpu_covered_bases(its bitmap, n, k_f + z) == the coverage cobs_gpu_search_coverage gives the document. */
uint64_t cobs_gpu_covered_bases(const uint64_t* words, size_t n, uint32_t span);      /* host arithmetic, no device */
cobs_gpu_status cobs_gpu_search_coverage(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                         double threshold, size_t num_results,
                                         cobs_gpu_hit* hits, size_t cap, size_t* hit_offsets /* nq + 1 */,
                                         size_t* bad_query);

/* ---- window search -------------------------------------------------------- */
/* A search whose score is LOCAL to the query, beyond the reference: the largest number of set positions in any window of
 * `window` consecutive positions.  It is the call for a long query (a nanopore read, a contig, a plasmid) searched in
 * documents that may hold only a short stretch of it: 1 000 consecutive positions of a 20 000-position query score 0.05
 * in every global search, and 1 000 of 1 000 here with window = 1000.
 *   File and query.  File f has term size k_f, the handle findere z; query q has n = len(q) - k_f + 1 - z positions in f.
 *   Set position.    Position p is set in document d exactly as cobs_gpu_prevalence and cobs_gpu_hit_positions define it:
 *                    terms p .. p + z are all present (the invalid-bases policy included, through K1's table).
 *   Window.          w = min(window, n).  best(q, f, d) = the maximum over s in [0, n - w] of the number of set positions
 *                    in [s, s + w): 0 .. w.  best <= min(w, score of the plain search); window >= n gives that score,
 *                    window = 1 gives 1 where any position is set; best does not decrease when the window grows.
 *   Threshold.       For threshold > 0 a real document is a hit when best >= max(1, ceil(threshold * w)), computed in
 *                    double.  For threshold <= 0 every real document is returned, best 0 included.
 *   Invalid bases.   Under COBS_GPU_INVALID_MISS and _SKIP a position whose characters hold a non-ACGT character is not
 *                    set; the denominator is w under both, so the two policies give the SAME result here.  Under _ERROR
 *                    an invalid base fails the call as it does for a search.
 *   Order.           Per query the records are ordered by best descending, then (file_no, doc) ascending, and cut to the
 *                    first num_results when num_results > 0; the reference's index-order rule does NOT apply.
 *                    hits[hit_offsets[q] .. hit_offsets[q+1]) belong to query q, `score` carries best.
 * Everything the host can refuse is refused before any device work: COBS_GPU_ERR_ARG (NULL arguments, window = 0),
 * COBS_GPU_ERR_UNSUPPORTED for window > 4095 (the scan's counters have 12 planes), on a handle opened with an HBM budget
 * (its rows are not all resident) or as one shard of several, COBS_GPU_ERR_QUERY_TOO_SHORT, COBS_GPU_ERR_QUERY_TOO_LONG
 * for len(q) >= 2^30 (the scan walks 32-bit positions; *bad_query = the offending query).  The device list
 * (cobs_gpu_multi_*) has no counterpart.  COBS_GPU_ERR_INVALID_BASE comes from the device (*bad_query).
 * COBS_GPU_ERR_CAPACITY when cap is too small -- hit_offsets then holds the needed sizes (hit_offsets[nq] the total),
 * known from the one scan that ran (hits may be NULL when cap is 0).  COBS_GPU_ERR_HIP when the device has no room for
 * the hit records of a pass.
 * On the device: K1 and one scan that walks every document's positions in order with the window's count kept bit-sliced
 * (as its distance to the best so far) and appends the documents that pass to a pool; no score matrix exists, and the
 * counters do not bound the query's length.  cobs_gpu_window_ms (cobs_gpu_diag.h) reads the timers.
 * cobs_gpu_best_window is the same number on the host, from one cobs_gpu_hit_positions bitmap of n positions (bit p of
 * words[p / 64]; bits at or beyond n are ignored; n = 0, window = 0 or words = NULL give 0).  *start (may be NULL)
 * receives the smallest s whose window reaches it -- the device call does not report it.  For every hit of any search,
 *   cobs_gpu_best_window(its bitmap, n, window, NULL) == the best cobs_gpu_search_window gives the document. */
uint32_t cobs_gpu_best_window(const uint64_t* words, size_t n, uint32_t window, size_t* start);   /* host arithmetic, no device */
cobs_gpu_status cobs_gpu_search_window(cobs_gpu_index* ix, const char* const* queries, const size_t* lens, size_t nq,
                                       uint32_t window, double threshold, size_t num_results,
                                       cobs_gpu_hit* hits, size_t cap, size_t* hit_offsets /* nq + 1 */,
                                       size_t* bad_query);

/* score slots per query held by THIS shard (== cobs_gpu_total_counts when
 * unsharded); device count rows have this many elements */
uint64_t cobs_gpu_local_counts(const cobs_gpu_index* ix);

/* ---- device-resident batches (benchmark / multi-GPU plumbing) ---------- */
/* Workspace for up to max_queries queries of up to max_query_len characters. */
cobs_gpu_status cobs_gpu_batch_create(cobs_gpu_index* ix, size_t max_queries,
                                      size_t max_query_len, cobs_gpu_batch** out);
void cobs_gpu_batch_destroy(cobs_gpu_batch* b);
/* Copy query text to HBM (one H2D) and validate lengths.  After this call the
 * inputs of cobs_gpu_batch_run are resident in HBM.  A run of the batch that is
 * still in flight and was never synced is waited for first. */
cobs_gpu_status cobs_gpu_batch_set_queries(cobs_gpu_batch* b, const char* const* queries,
                                           const size_t* lens, size_t nq);
/* One pass of the hot path over the batch, asynchronously on `hip_stream`
 * (a hipStream_t, NULL = default stream): K1 canonicalise + XXH64 + row index
 * per sub-index (create_hashes, :66-107), K2 row gather + AND + bit-sliced
 * per-document count (read_from_disk / aggregate_rows / compute_counts,
 * :279-307, :643-1022), and, if threshold > 0, on-device selection of documents
 * with count >= ceil(threshold * T) (:127-132).  Counts stay in HBM.          */
cobs_gpu_status cobs_gpu_batch_run(cobs_gpu_batch* b, double threshold, void* hip_stream);
/* The same pass without score rows (threshold > 0 required): the comparison count >= ceil(threshold * T)
 * is done on the bit-sliced counters, only the selected (query, file, doc, score) records are
 * written.  cobs_gpu_batch_hits_host returns them; if the selection pool overflowed it fails
 * with COBS_GPU_ERR_ARG ("did not keep the score rows"): rerun with cobs_gpu_batch_run, as
 * cobs_gpu_search_batch does on its own. */
cobs_gpu_status cobs_gpu_batch_run_hits(cobs_gpu_batch* b, double threshold, void* hip_stream);
/* The same pass followed by K3: on-device selection of the num_results best
 * documents per query (score descending, ties by document ascending -- the set
 * std::partial_sort keeps, classic_search.cpp:134-145) among those with
 * count >= ceil(threshold * T), left in result order on the device (all score widths: 8, 16 and
 * 32 bit); cobs_gpu_batch_hits_host then moves only those.                      */
cobs_gpu_status cobs_gpu_batch_run_topk(cobs_gpu_batch* b, double threshold, size_t num_results,
                                        void* hip_stream);
/* The top-k pass WITHOUT score rows (the counterpart of cobs_gpu_batch_run_hits): counts_to_result keeps the
 * num_results best while it scans (classic_search.cpp:127-145) and needs no score matrix either.  K2 selects the
 * num_results best documents of every tile from its bit-sliced counters, K3 merges tiles x num_results
 * candidates per query; same result as cobs_gpu_batch_run_topk, cobs_gpu_batch_counts_* are not available
 * afterwards.  Where the tile-level selection does not apply (num_results > 128, a query with a single hash in
 * total, sub-indexes of 2^32 rows and more) the pass keeps score rows as cobs_gpu_batch_run_topk does. */
cobs_gpu_status cobs_gpu_batch_run_topk_only(cobs_gpu_batch* b, double threshold, size_t num_results,
                                             void* hip_stream);
/* wait for the stream and fetch device-side error flags (invalid bases, ...) */
cobs_gpu_status cobs_gpu_batch_sync(cobs_gpu_batch* b, void* hip_stream, size_t* bad_query);
/* Device pointer to the counts of the last run: row i (query i) starts at
 * ptr + i * row_stride_bytes and holds cobs_gpu_local_counts() elements of
 * elem_bytes each: 1 when no query of the batch has more than 255 terms, 2 up to
 * 65535, else 4 -- the Score widths of classic_search.cpp:453-504.  Valid until the
 * batch is destroyed. */
void* cobs_gpu_batch_counts_device(cobs_gpu_batch* b, uint32_t* elem_bytes, uint64_t* row_stride_bytes);
/* D2H of one query's counts widened to u32 */
cobs_gpu_status cobs_gpu_batch_counts_host(cobs_gpu_batch* b, size_t query_no, uint32_t* counts, size_t cap);
/* `cobs benchmark-fpr --dist` (src/cobs.cpp:627-632: counts[r.score]++ over every result of every query): after a run
 * that kept score rows, hist[s] += the (query, real document) pairs of the batch with score s (s >= nbins: the last
 * bin); tallied on the device.  On a shard: of the documents it holds. */
cobs_gpu_status cobs_gpu_batch_score_histogram(cobs_gpu_batch* b, uint64_t* hist, size_t nbins);
/* D2H + rank the hits of query `query_no` of the last run */
cobs_gpu_status cobs_gpu_batch_hits_host(cobs_gpu_batch* b, size_t query_no, size_t num_results,
                                         cobs_gpu_hit* hits, size_t cap, size_t* n_hits);

/* ---- multi-GPU: index sharded by sub-index block, one exchange per batch over RCCL / xGMI ----
 * (the shard boundary is the reference's own: sub-indexes cover disjoint document
 * ranges, compact_index/mmap_search_file.cpp:22-27, search_file.cpp:30-32.)  One rank = one GPU =
 * one cobs_gpu_index opened with shard_rank / shard_count = its rank / the communicator size.
 * The launcher (torch.distributed, MPI, threads of one process...) only has to hand the unique id
 * from rank 0 to the others.  All calls below are collective: every rank makes the same call.  */
#define COBS_GPU_UNIQUE_ID_BYTES 128
/* Side effect of the two calls below: RCCL prints a version banner to stdout when a process first initialises
 * it; while they run, file descriptor 1 of the PROCESS points at stderr (and is put back afterwards), so that the
 * caller's stdout stays clean -- output other threads write to stdout in that window lands on stderr. */
cobs_gpu_status cobs_gpu_comm_unique_id(uint8_t id[COBS_GPU_UNIQUE_ID_BYTES]);          /* ncclGetUniqueId */
cobs_gpu_status cobs_gpu_comm_create(const uint8_t id[COBS_GPU_UNIQUE_ID_BYTES], int rank, int nranks,
                                     int device /* -1 = current */, cobs_gpu_comm** out);  /* ncclCommInitRank */
void cobs_gpu_comm_destroy(cobs_gpu_comm* c);
int cobs_gpu_comm_rank(const cobs_gpu_comm* c);     /* ncclCommUserRank, -1 on error */
int cobs_gpu_comm_size(const cobs_gpu_comm* c);     /* ncclCommCount, 0 on error */
/* Failure behaviour of a communicator (the reference has no distributed code; this is the contract of the layer added
 * here): an RCCL call that fails marks the communicator BROKEN -- an open ncclGroupStart is closed first, a dead
 * communicator is aborted (ncclCommAbort) -- and every later call on it fails at once with COBS_GPU_ERR_RCCL on this
 * rank, before any collective.  A collective that a peer never enters does not fail, it waits: */
/* ... with a time limit, the stream waits the library itself performs around collectives (layout and size exchanges,
 * status agreements, the row exchanges of cobs_gpu_sharded_search_batch) give up after timeout_ms, abort the
 * communicator and return COBS_GPU_ERR_RCCL.  0 = wait for ever (the default, unless COBS_GPU_COMM_TIMEOUT_MS is set in the
 * environment when the communicator is created: the limit of communicators the library makes itself, cobs_gpu_multi_open). */
void cobs_gpu_comm_set_timeout(cobs_gpu_comm* c, uint32_t timeout_ms);
/* ... and what this rank entered last, as one line of text (RCCL calls entered / returned, the last call, whether its
 * stream is idle) -- callable from ANOTHER thread while the owner sits in a call: what a caller's watchdog prints
 * when a step does not come back.  -> characters written (NUL-terminated). */
size_t cobs_gpu_comm_state(const cobs_gpu_comm* c, char* buf, size_t cap);
/* Collective.  The first bytes a new communicator moves, each step under `timeout_ms` and every received byte checked:
 * one grouped ncclSend / ncclRecv all-to-all with a different size for every (sender, receiver) pair, one
 * ncclAllGather, ncclAllReduce(max, sum) -- the operations a batch exchange uses; big_bytes > 0 adds a timed all-to-all
 * of that many bytes per pair.  out = all-to-all bytes received | its microseconds | all-gather us | all-reduce us |
 * large all-to-all bytes received | its us (second round) | 0 | 0.  A failure leaves the communicator broken. */
cobs_gpu_status cobs_gpu_comm_preflight(cobs_gpu_comm* c, uint32_t timeout_ms, uint64_t big_bytes, uint64_t out[8]);

typedef enum cobs_gpu_exchange_mode {
    COBS_GPU_XCHG_ALLGATHER = 0,  /* every rank receives the count slices of all ranks for all queries
                                     (ncclAllGather when the slices have one size, else grouped send/recv) */
    COBS_GPU_XCHG_ALLTOALL = 1,   /* rank j receives the slices of the queries [nq*j/N, nq*(j+1)/N) only:
                                     every count crosses the fabric once (grouped ncclSend / ncclRecv)      */
    COBS_GPU_XCHG_REDUCE = 2      /* the counts "reduced over RCCL": every rank lays its slices into zeroed
                                     rows of global length, one ncclAllReduce(sum) over the bytes (disjoint
                                     slices: no byte has two non-zero addends, so the byte-wise sum is exact
                                     for every counter width).  The parity form; the gather forms move less */
} cobs_gpu_exchange_mode;
/* After cobs_gpu_batch_run on every rank: exchange the per-document counts of the shards on
 * `hip_stream` (asynchronous, ordered after the scan) and assemble rows in global document order. */
cobs_gpu_status cobs_gpu_batch_exchange_counts(cobs_gpu_batch* b, cobs_gpu_comm* c, uint32_t mode, void* hip_stream);
/* The assembled rows of queries [*q_begin, *q_begin + *q_count): cobs_gpu_total_counts() elements of
 * *elem_bytes each, *row_stride_bytes apart.  NULL before an exchange.  Valid until the next run. */
void* cobs_gpu_batch_global_counts_device(cobs_gpu_batch* b, uint64_t* q_begin, uint64_t* q_count,
                                          uint32_t* elem_bytes, uint64_t* row_stride_bytes);
/* bytes this rank received from other ranks in the last exchange */
uint64_t cobs_gpu_batch_exchange_bytes(const cobs_gpu_batch* b);
/* After a synced run with a threshold: gather the selected (query, file, doc, score) records of all
 * shards (sizes first, then the records); cobs_gpu_batch_hits_host then returns global results.
 * *overflow = 1 if a shard's pool overflowed (lists incomplete on every rank: rerun with score rows). */
cobs_gpu_status cobs_gpu_batch_exchange_hits(cobs_gpu_batch* b, cobs_gpu_comm* c, void* hip_stream, int* overflow);
/* The same exchange with every record sent ONCE, to the rank that owns its query: rank j owns the queries
 * [nq*j/N, nq*(j+1)/N) (as in COBS_GPU_XCHG_ALLTOALL) and ends with the hits of exactly those queries from every shard
 * (*q_begin / *q_count, optional); cobs_gpu_batch_hits_host then answers for them and refuses the others. */
cobs_gpu_status cobs_gpu_batch_exchange_hits_owned(cobs_gpu_batch* b, cobs_gpu_comm* c, void* hip_stream, int* overflow,
                                                   uint64_t* q_begin, uint64_t* q_count);
/* After a run with num_results > 0: all-gather the k best documents of every shard and merge them on the device into
 * the global k best of every (file, query) (K3 over the gathered lists; k > 8192: merged per query on the host);
 * cobs_gpu_batch_hits_host then answers from them.  Not for a query with a single hash in total: the reference does not order
 * such a result by score (max_counts <= 1, classic_search.cpp:134,177), it is the first documents in index order,
 * which per-shard best-of lists do not determine -- exchange the score rows for such a batch
 * (cobs_gpu_batch_exchange_counts; cobs_gpu_sharded_search_batch does). */
cobs_gpu_status cobs_gpu_batch_exchange_topk(cobs_gpu_batch* b, cobs_gpu_comm* c, void* hip_stream);
/* cobs_gpu_search_batch over the sharded index: same arguments and result on every rank. */
cobs_gpu_status cobs_gpu_sharded_search_batch(cobs_gpu_index* ix, cobs_gpu_comm* c, const char* const* queries,
                                              const size_t* lens, size_t nq, double threshold, size_t num_results,
                                              cobs_gpu_hit* hits, size_t cap, size_t* hit_offsets, size_t* bad_query);

/* The same call with the ranking SHARED by the ranks where that is possible: for the all-documents search (threshold <= 0
 * and no limit -- the reference's default call) every query yields one result per document, so every result's place in
 * `hits` is known up front; the count rows go all-to-all to query owners and rank j writes the results and offsets of the
 * queries [n*j/N, n*(j+1)/N) of every pass at their final places.  Ranks of ONE process pass the same arrays (together
 * they fill them, every entry written by exactly one rank: cobs_gpu_multi_search_batch does this); ranks in several
 * processes each get their part filled (hit_offsets[0] and, on ERR_CAPACITY, the needed sizes by rank 0 only).  All
 * ranks must pass the same cap.  Every other search behaves exactly like cobs_gpu_sharded_search_batch. */
cobs_gpu_status cobs_gpu_sharded_search_batch_split(cobs_gpu_index* ix, cobs_gpu_comm* c, const char* const* queries,
                                                    const size_t* lens, size_t nq, double threshold, size_t num_results,
                                                    cobs_gpu_hit* hits, size_t cap, size_t* hit_offsets, size_t* bad_query);

/* How both calls above run (round 6): the call is cut into passes that overlap inside the library, as the reference
 * parallelises inside search() (parallel_for over document batches, classic_search.cpp:355-400): upload + hashing of
 * pass i+1 | scan of pass i | the ranks' agreement, the exchange over RCCL and the ordering of the results of pass i-1,
 * on their own streams tied by events.  After a scan the ranks agree through ONE all-gathered record per pass (status,
 * first invalid query, hit-pool fill; written by the device, read once per pass while the next pass scans).  All ranks
 * must have set the tuning keys that cut passes (pass_bytes, pipe_chars) alike. */

/* ---- the device-resident form of the sharded search: what `bench.py --gpus N` times ----
 * ONE batch of queries, uploaded once; a step scans it on every rank against that rank's shard and leaves the count rows
 * on the device in global document order (cobs_gpu_batch_global_counts_device of every sub-batch).  The batch is cut
 * into `sub_batches` sub-batches over the queries -- the reference's own loop is per batch of documents,
 * classic_search.cpp:355-400 -- whose hashing (the sub-batch's own stream), scan (scan stream) and exchange (exchange
 * stream) overlap, also across steps: hash(i+1) | scan(i) | exchange(i-1).  Collective: every rank makes the same calls.
 * More than one sub-batch sets the handle's tuning key hash_stream. */
typedef struct cobs_gpu_sharded_batch cobs_gpu_sharded_batch;
cobs_gpu_status cobs_gpu_sharded_batch_create(cobs_gpu_index* ix, cobs_gpu_comm* c, uint32_t sub_batches,
                                              cobs_gpu_sharded_batch** out);
void cobs_gpu_sharded_batch_destroy(cobs_gpu_sharded_batch* sb);
/* sub-batch i holds the queries [nq*i/S, nq*(i+1)/S); synchronous (one upload per sub-batch) */
cobs_gpu_status cobs_gpu_sharded_batch_set_queries(cobs_gpu_sharded_batch* sb, const char* const* queries, const size_t* lens,
                                                   size_t nq);
/* one step, asynchronous: every sub-batch hashed, scanned, its count rows exchanged (mode: cobs_gpu_exchange_mode) */
cobs_gpu_status cobs_gpu_sharded_batch_step(cobs_gpu_sharded_batch* sb, double threshold, uint32_t mode);
/* waits for everything queued (the exchange stream under the communicator's time limit); invalid queries are reported
 * here, *bad_query = index in the batch */
cobs_gpu_status cobs_gpu_sharded_batch_sync(cobs_gpu_sharded_batch* sb, size_t* bad_query);
size_t cobs_gpu_sharded_batch_subs(const cobs_gpu_sharded_batch* sb);
/* sub-batch i (owned by sb) and its queries: for the batch-level accessors (global / local count rows, stats) */
cobs_gpu_batch* cobs_gpu_sharded_batch_sub(cobs_gpu_sharded_batch* sb, size_t i, size_t* q_begin, size_t* q_count);
/* After a sync; per step, summed over the sub-batches, averaged over the steps since the previous call (at most 64):
 * out = scan ms | hash ms | exchange ms | algorithmic bytes | bytes received from other ranks |
 * scan launches | steps averaged over | 0 -- HIP events on the streams the kernels and collectives ran on. */
cobs_gpu_status cobs_gpu_sharded_batch_times(cobs_gpu_sharded_batch* sb, double out[8]);

#ifdef __cplusplus
}
#endif
#endif /* COBS_GPU_BATCH_H */
