"""The weighted-search checker (test infrastructure), on top of tests/prevalence_check.py.  No engine code in it.

Definition (restated from include/cobs_gpu_batch.h).  For a file with D real documents, the handle's findere z and
invalid-bases policy, query q has n = T - z positions.  c[p] = prevalence_check.prevalence: the real documents in which
terms p .. p + z are all present.  The weight of a position is

    w = 0                                         when c = 0
    w = 1 + max{ j in 0..14 : c * 2^j <= D }      otherwise (integer arithmetic), i.e. 1 + min(14, floor(log2(D / c)))

score(d) = the sum of w[p] over the positions p set in document d (real documents only), W = the sum of all w[p].  For
threshold > 0 a real document is a hit when score >= max(1, ceil(threshold * W)) in double -- W = 0 returns nothing --,
for threshold <= 0 every real document is returned.  Per query the records are ordered by score descending, then (file,
document) ascending, and cut to num_results when it is > 0 (the reference's index-order rule does not apply).  A
position nobody holds weighs 0, so the policies `miss` and `skip` give the same result."""

import numpy as np

from tests import findere_check as F
from tests import prevalence_check as V


def idf_weight(D, c):
    D, c = int(D), int(c)
    if c == 0:
        return 0
    j = 0
    while j < 14 and c * 2 ** (j + 1) <= D:
        j += 1
    return 1 + j


def weights(fb, q, z, mode="error"):
    """uint8 [n]: the weight of every position of q in the file"""
    c = V.prevalence(fb, q, z, mode)
    by_count = {int(v): idf_weight(fb.num_docs, int(v)) for v in np.unique(c)}
    return np.array([by_count[int(v)] for v in c], dtype=np.uint8)


def scores(fb, q, z, mode="error", weights=None):
    """uint64 [slots]: the weighted score of the document of every score slot, w @ windows"""
    w = globals()["weights"](fb, q, z, mode) if weights is None else np.asarray(weights)
    win = V.windows(fb, q, z, mode)
    assert len(w) == win.shape[0]
    sc = np.zeros(win.shape[1], dtype=np.uint64)
    for v in np.unique(w):                       # (w @ windows, one weight value at a time: sums of bool rows)
        if v:
            sc += np.uint64(v) * win[w == v].sum(axis=0, dtype=np.uint64)
    return sc


def thresholds(threshold, total):
    """the score a document of a (query, file) with total weight `total` has to reach (0: every real document)"""
    if not threshold > 0:
        return 0
    return max(1, F.ceil_product(threshold, total))


def total_weights(files, q, z, mode="error"):
    return [int(weights(fb, q, z, mode).sum(dtype=np.uint64)) for fb in files]


def tables(files, q, z, mode="error", weights=None):
    """per file (W, scores of every slot, document of every slot, weights): what every threshold and cut of one query
    starts from"""
    out = []
    for fi, fb in enumerate(files):
        w = globals()["weights"](fb, q, z, mode) if weights is None else np.asarray(weights[fi])
        out.append((int(w.sum(dtype=np.uint64)), scores(fb, q, z, mode, weights=w), fb.doc_of_slot(), w))
    return out


def results_from(tabs, threshold=0.0, num_results=0):
    fs, ds, ss = [], [], []
    for fi, (total, sc, docs, _w) in enumerate(tabs):
        slots = np.nonzero((docs >= 0) & (sc >= np.uint64(thresholds(threshold, total))))[0]
        fs.append(np.full(len(slots), fi, dtype=np.int64))
        ds.append(docs[slots].astype(np.int64))
        ss.append(sc[slots].astype(np.int64))
    f, d, sc = np.concatenate(fs), np.concatenate(ds), np.concatenate(ss)
    order = np.lexsort((d, f, -sc))              # score descending, then (file, document) ascending
    if num_results:
        order = order[:num_results]
    return list(zip(f[order].tolist(), d[order].tolist(), sc[order].tolist()))


def results(files, q, z, threshold=0.0, num_results=0, mode="error", weights=None):
    """[(file, doc, score)] of one query in result order; weights: per file, or None = the definition's"""
    return results_from(tables(files, q, z, mode, weights), threshold, num_results)
