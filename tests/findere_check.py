"""The findere checker (test infrastructure): an independent numpy restatement of the windowed score.

Term p of query q is present in document d when all H bits of its hashes are set in d's column; with findere z the
score of d counts the positions p in [0, T - z) whose z + 1 terms p .. p + z are all present.  The bits come from the
matrices the tests wrote (or read back); the row of a (term, hash) is oracle.term_hashes(q, k, canonicalize, H) % S_p.
At z = 0 this is the plain COBS count, which the tests anchor against oracle.Index.counts.
"""
import math

import numpy as np

from oracle import oracle as O


class FileBits:
    """One index file as the checker sees it: term size, canonicalize, hashes and the bit matrix of every sub-index
    (classic: one [S, ceil(D/8)] matrix; compact: one [S_p, page_size] matrix per sub-index), in score-slot order."""

    def __init__(self, term_size, canonicalize, num_hashes, mats, num_docs):
        self.term_size, self.canonicalize, self.num_hashes = term_size, canonicalize, num_hashes
        self.mats = [np.ascontiguousarray(m) for m in mats]
        self.num_docs = num_docs
        self.slots = sum(m.shape[1] * 8 for m in self.mats)

    def presence(self, q):
        """bool [T, slots]: term p present in the document of every score slot"""
        hashes, _good = O.term_hashes(q, self.term_size, self.canonicalize, self.num_hashes)
        T = len(hashes)
        out = []
        for m in self.mats:
            rows = (hashes % np.uint64(m.shape[0])).astype(np.int64)               # [T, H]
            bits = np.unpackbits(m[rows], axis=-1, bitorder="little")              # [T, H, 8 * width]
            out.append(bits.all(axis=1) if T else np.zeros((0, m.shape[1] * 8), dtype=bool))
        return np.concatenate(out, axis=1).astype(bool)

    def positions(self, q, z):
        return len(q) - self.term_size + 1 - z

    def scores(self, q, z):
        """uint32 [slots]: the findere score of every slot (z = 0: the COBS count)"""
        P = self.presence(q)
        n = P.shape[0] - z
        if n <= 0:
            return np.zeros(self.slots, dtype=np.uint32)
        win = np.ones((n, self.slots), dtype=bool)
        for j in range(z + 1):
            win &= P[j:j + n]
        return win.sum(axis=0).astype(np.uint32)

    def doc_of_slot(self):
        """slot -> document id (or -1 for padding slots)"""
        docs = np.full(self.slots, -1, dtype=np.int64)
        if len(self.mats) == 1:
            n = min(self.num_docs, self.slots)
            docs[:n] = np.arange(n)
        else:
            s = 0
            for m in self.mats:
                w = m.shape[1] * 8
                live = max(0, min(self.num_docs - s, w))
                docs[s:s + live] = np.arange(s, s + live)
                s += w
        return docs


def counts(files, q, z):
    """the raw score rows of all files side by side (Search.counts' layout)"""
    return np.concatenate([f.scores(q, z) for f in files])


BOUND_LIMIT = 2 ** 32 - 1


def ceil_product(threshold, positions, limit=BOUND_LIMIT):
    """ceil(threshold * positions) with the product in double, as an integer: 0 when the product is not > 0 (a NaN
    threshold, inf * 0), `limit` from there on (an infinite or huge threshold: no score reaches it)"""
    v = float(threshold) * float(positions)
    if not v > 0:
        return 0
    return limit if v >= float(limit) else int(math.ceil(v))


def threshold_for(threshold, positions):
    return ceil_product(threshold, positions)


def results(files, q, z, threshold=0.0, num_results=0):
    """ClassicSearch::search under findere: (file, doc, score) with score >= ceil(threshold * (T_f - z)); score
    descending, ties (file, doc) ascending; max_counts = sum_f (T_f - z) * H_f <= 1 keeps index order"""
    hits = []
    for fi, f in enumerate(files):
        sc = f.scores(q, z)
        docs = f.doc_of_slot()
        thr = threshold_for(threshold, f.positions(q, z))
        for slot in np.nonzero((docs >= 0) & (sc >= thr))[0]:
            hits.append((fi, int(docs[slot]), int(sc[slot])))
    max_counts = sum(f.positions(q, z) * f.num_hashes for f in files)
    if max_counts > 1:
        hits.sort(key=lambda h: (-h[2], h[0], h[1]))
    if num_results:
        hits = hits[:num_results]
    return hits


def classic_file(path):
    from oracle import construct as K
    k, canon, names, sig, nh, m = K.read_classic(path)
    return FileBits(k, canon, nh, [m], len(names))
