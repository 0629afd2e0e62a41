"""The coverage-search checker (test infrastructure), on top of tests/prevalence_check.py.  No engine code in it.

Definition (restated from include/cobs_gpu_batch.h).  File f has term size k_f, the handle findere z, query q the length
L = len(q).  In file f the query has n = L - k_f + 1 - z positions.  Position p is set in document d exactly as
prevalence_check.windows says: terms p .. p + z are all present (under `miss` and `skip` a window with a character
outside ACGT is not set).  span = k_f + z.  A set position p covers bases p .. p + span - 1 of the query;
coverage(q, f, d) is the number of bases b in [0, L) covered by at least one set position of d, 0 .. L.  With s > 0 set
positions, s + span - 1 <= coverage <= min(L, s * span).

For threshold > 0 a real document is a hit when coverage >= max(1, ceil(threshold * L)) in double; for threshold <= 0
every real document is returned.  The denominator is L under both invalid-bases policies, so `miss` and `skip` give the
same result.  Per query the records are ordered by coverage descending, then (file, document) ascending, and cut to
num_results when it is > 0 (the reference's index-order rule does not apply)."""

import numpy as np

from tests import findere_check as F
from tests import prevalence_check as V


def span_of(fb, z):
    return fb.term_size + z


def dilate(win, span):
    """bool [n, slots] set positions -> bool [n + span - 1, slots] covered bases: base b is covered when a position in
    [b - span + 1, b] is set"""
    n, slots = win.shape
    cov = np.zeros((n + span - 1, slots), dtype=bool)
    for j in range(span):
        cov[j:j + n] |= win
    return cov


def covered(fb, q, z, mode="error"):
    """bool [L, slots]: base b of q covered in the document of every score slot"""
    cov = dilate(V.windows(fb, q, z, mode), span_of(fb, z))
    assert cov.shape[0] == len(q)
    return cov


def coverage(fb, q, z, mode="error"):
    """uint64 [slots]: the covered bases of the document of every score slot"""
    return covered(fb, q, z, mode).sum(axis=0, dtype=np.uint64)


def coverage_by_bases(fb, q, z, mode="error"):
    """the same, base by base and slot by slot: the second restatement (slow; small inputs)"""
    win = V.windows(fb, q, z, mode)
    n, slots = win.shape
    span = span_of(fb, z)
    out = np.zeros(slots, dtype=np.uint64)
    for slot in range(slots):
        col = win[:, slot]
        if not col.any():
            continue
        total = 0
        for b in range(len(q)):
            lo, hi = max(0, b - span + 1), min(b, n - 1)
            if lo <= hi and col[lo:hi + 1].any():
                total += 1
        out[slot] = total
    return out


def covered_bases(bits, span):
    """covered bases of one bool vector of n positions (what cobs_gpu_covered_bases computes from the packed words)"""
    bits = np.asarray(bits, dtype=bool)
    if len(bits) == 0 or span == 0:
        return 0
    return int(dilate(bits[:, None], span).sum())


def thresholds(threshold, length):
    """the covered bases a document has to reach for a query of `length` characters (0: every real document)"""
    if not threshold > 0:
        return 0
    return max(1, F.ceil_product(threshold, length))


def tables(files, q, z, mode="error"):
    """per file (L, coverage of every slot, document of every slot, set positions of every slot): what every threshold
    and cut of one query starts from"""
    out = []
    for fb in files:
        win = V.windows(fb, q, z, mode)
        cov = dilate(win, span_of(fb, z)).sum(axis=0, dtype=np.uint64)
        out.append((len(q), cov, fb.doc_of_slot(), win.sum(axis=0, dtype=np.uint64)))
    return out


def results_from(tabs, threshold=0.0, num_results=0):
    fs, ds, ss = [], [], []
    for fi, (length, cov, docs, _s) in enumerate(tabs):
        slots = np.nonzero((docs >= 0) & (cov >= np.uint64(thresholds(threshold, length))))[0]
        fs.append(np.full(len(slots), fi, dtype=np.int64))
        ds.append(docs[slots].astype(np.int64))
        ss.append(cov[slots].astype(np.int64))
    f, d, sc = np.concatenate(fs), np.concatenate(ds), np.concatenate(ss)
    order = np.lexsort((d, f, -sc))              # coverage descending, then (file, document) ascending
    if num_results:
        order = order[:num_results]
    return list(zip(f[order].tolist(), d[order].tolist(), sc[order].tolist()))


def results(files, q, z, threshold=0.0, num_results=0, mode="error"):
    """[(file, doc, coverage)] of one query in result order"""
    return results_from(tables(files, q, z, mode), threshold, num_results)
