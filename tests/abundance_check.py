"""The k-mer abundance cutoff of index construction (cobs_gpu_build_params.min_count) restated in
plain Python -- TEST INFRASTRUCTURE ONLY; it shares no code with the library.

min_count = c: a term sets its bits in document d's column only if it occurs at least c times within
document d.  Occurrences are the k-windows of the document's sequences in process_terms order; two
occurrences are the same term when the bytes handed to the hash function are equal, i.e. after
canonicalisation (canonicalize_kmer, reference util/query.cpp:143-199: an invalid character maps to
0, the first strict difference between the mapped k-mer and its reverse complement among the first
k/2 positions picks the smaller, ties keep the forward one).  c = 0 and c = 1 keep everything.

The expected index of a build with min_count = c is the oracle's construction (oracle/construct.py)
over documents whose `hashes` are the KEPT rows of oracle.term_hashes while `size` and `num_terms`
stay the unfiltered ones (sizing does not change).
"""
import collections

import numpy as np

_COMP = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A")}
_VALID = frozenset(b"ACGT")


def canonical_bytes(term, canonicalize):
    """the bytes the builder hands to the hash function for this k-window"""
    if not canonicalize:
        return bytes(term)
    fwd = bytes(c if c in _VALID else 0 for c in term)
    rev = bytes(_COMP.get(c, 0) for c in reversed(term))
    for s in range(len(term) // 2):
        if fwd[s] < rev[s]:
            return fwd
        if fwd[s] > rev[s]:
            return rev
    return fwd


def kept_occurrences(sequences, k, canonicalize, c):
    """-> (indices of the term occurrences whose term reaches c, number of occurrences); an
    occurrence's index is its rank in process_terms order over the sequences"""
    keys = [canonical_bytes(s[i:i + k], canonicalize) for s in sequences for i in range(len(s) - k + 1)]
    counts = collections.Counter(keys)
    need = max(int(c), 1)
    return np.asarray([i for i, key in enumerate(keys) if counts[key] >= need], dtype=np.int64), len(keys)


def filtered_doc(oracle, construct, name, path, size, num_terms, sequences, k, canonicalize, num_hashes, c):
    """-> (construct.Doc with the kept hashes and the unfiltered size / num_terms, kept, total)"""
    sequences = [bytes(s) for s in sequences]
    hs = [oracle.term_hashes(s, k, canonicalize, num_hashes)[0] for s in sequences if len(s) >= k]
    hashes = np.concatenate(hs) if hs else np.zeros((0, num_hashes), dtype=np.uint64)
    kept, total = kept_occurrences(sequences, k, canonicalize, c)
    assert total == len(hashes)
    return construct.Doc(name, path, size, num_terms, hashes[kept]), len(kept), total


def memory_docs(oracle, construct, docs, k, canonicalize, num_hashes, c):
    """in-memory documents [(name, sequences)] (DocumentList.add_document) -> (Docs, kept, total)"""
    out, kept, total = [], 0, 0
    for name, seqs in docs:
        d, kp, tt = filtered_doc(oracle, construct, name, name, len(b"\n".join(seqs)) + 1,
                                 sum(max(len(s) - k + 1, 0) for s in seqs), seqs, k, canonicalize, num_hashes, c)
        out.append(d)
        kept += kp
        total += tt
    return out, kept, total


def entry_docs(oracle, construct, entries, k, canonicalize, num_hashes, c):
    """entries of oracle.documents.document_list (files of any type) -> (Docs, kept, total)"""
    out, kept, total = [], 0, 0
    for e in entries:
        d, kp, tt = filtered_doc(oracle, construct, e.name, e.path, e.size, e.num_terms(k), list(e.term_buffers(k)),
                                 k, canonicalize, num_hashes, c)
        d.subdoc = e.subdoc_index
        out.append(d)
        kept += kp
        total += tt
    return out, kept, total


# ---------------------------------------------------------------------------
# the corpus of the cutoff's tests

PARAMS = [(1, 1, 31), (1, 3, 31), (0, 2, 31), (1, 2, 20), (0, 1, 40)]      # (canonicalize, num_hashes, k)
CUTOFFS = [1, 2, 3, 5]
TEXT_BATCH = 12000      # bytes: the corpus takes several batches, most of them hold several documents


def revcomp(s):
    return bytes(_COMP[c] for c in reversed(s))


def make_corpus(seed, k, ndocs=40, return_shared=False):
    """Documents made for the cutoff: random segments repeated with chosen multiplicities (each copy
    a sequence of its own, or glued to its neighbour so that junction k-mers occur once), some copies
    as reverse complements (the same terms with canonicalize = 1, other terms without), invalid
    bases -- 'N' in one copy and 'X' at the same place in another, which canonicalize = 1 maps to
    the same bytes and canonicalize = 0 keeps apart --, and one shared segment that occurs ONCE in
    each of a run of neighbouring documents (staged in the same batch): it must never reach c = 2."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)

    def rand(n):
        return acgt[rng.integers(0, 4, n)].tobytes()

    shared = rand(k + 60)
    docs = []
    for d in range(ndocs):
        copies = []
        for m in (1, 1, 2, 3, 7, 1, 5, 2, 9)[:int(rng.integers(5, 10))]:
            seg = bytearray(rand(int(rng.integers(k + 5, k + 90))))
            bad = int(rng.integers(0, len(seg))) if rng.random() < 0.3 else -1
            for j in range(m):
                s = bytearray(seg)
                if bad >= 0:
                    s[bad] = ord("N") if j % 2 == 0 else ord("X")
                copies.append(revcomp(bytes(s)) if (bad < 0 and j % 3 == 1) else bytes(s))
        if 8 <= d < 20:
            copies.append(shared)
        order = rng.permutation(len(copies))
        seqs, cur = [], b""
        for i in order:
            cur += copies[i]
            if rng.random() < 0.7:
                seqs.append(cur)
                cur = b""
        if cur:
            seqs.append(cur)
        if d % 9 == 4:
            seqs.append(rand(k - 1))            # a sequence without a term
        docs.append(("doc_%04d" % d, seqs))
    return (docs, shared) if return_shared else docs
