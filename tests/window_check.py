"""The window-search checker (test infrastructure), on top of tests/prevalence_check.py.  No engine code in it.

Definition (restated from include/cobs_gpu_batch.h).  File f has term size k_f, the handle findere z, query q has
n = len(q) - k_f + 1 - z positions in f.  Position p is set in document d exactly as prevalence_check.windows says: terms
p .. p + z are all present (under `miss` and `skip` a stretch with a character outside ACGT is not set).  With
w = min(W, n), best(q, f, d) is the maximum over s in [0, n - w] of the number of set positions in [s, s + w).

For threshold > 0 a real document is a hit when best >= max(1, ceil(threshold * w)) in double; for threshold <= 0 every
real document is returned.  The denominator is w under both invalid-bases policies, so `miss` and `skip` give the same
result.  Per query the records are ordered by best descending, then (file, document) ascending, and cut to num_results
when it is > 0 (the reference's index-order rule does not apply)."""

import numpy as np

from tests import findere_check as F
from tests import prevalence_check as V


def width(W, n):
    return min(int(W), int(n))


def best(win, W):
    """bool [n, slots] set positions -> int64 [slots]: the best window of every slot, by cumulative sums"""
    win = np.asarray(win, dtype=bool)
    n, slots = win.shape
    if n == 0:
        return np.zeros(slots, dtype=np.int64)
    w = width(W, n)
    cs = np.concatenate([np.zeros((1, slots), dtype=np.int64), np.cumsum(win, axis=0, dtype=np.int64)])
    return (cs[w:] - cs[:n - w + 1]).max(axis=0)


def best_by_slots(win, W):
    """the same, window by window and slot by slot: the second restatement (slow; small inputs)"""
    win = np.asarray(win, dtype=bool)
    n, slots = win.shape
    out = np.zeros(slots, dtype=np.int64)
    if n == 0:
        return out
    w = width(W, n)
    for slot in range(slots):
        col = win[:, slot]
        top = 0
        for s in range(n - w + 1):
            c = 0
            for p in range(s, s + w):
                c += 1 if col[p] else 0
            top = max(top, c)
        out[slot] = top
    return out


def best_window(bits, W):
    """(best, start) of one bool vector of n positions: what cobs_gpu_best_window computes from the packed words; start
    is the smallest one that reaches best"""
    bits = np.asarray(bits, dtype=bool)
    n = len(bits)
    if n == 0 or W == 0:
        return 0, 0
    w = width(W, n)
    cs = np.concatenate([[0], np.cumsum(bits, dtype=np.int64)])
    c = cs[w:] - cs[:n - w + 1]
    return int(c.max()), int(np.argmax(c))              # argmax: the first maximum


def thresholds(threshold, w):
    """the set positions a window of w positions has to hold (0: every real document)"""
    if not threshold > 0:
        return 0
    return max(1, F.ceil_product(threshold, w))


def tables(files, q, z, W, mode="error"):
    """per file (w, best of every slot, document of every slot, set positions of every slot): what every threshold and
    cut of one query starts from"""
    out = []
    for fb in files:
        win = V.windows(fb, q, z, mode)
        out.append((width(W, win.shape[0]), best(win, W), fb.doc_of_slot(), win.sum(axis=0, dtype=np.int64)))
    return out


def results_from(tabs, threshold=0.0, num_results=0):
    fs, ds, ss = [], [], []
    for fi, (w, b, docs, _s) in enumerate(tabs):
        slots = np.nonzero((docs >= 0) & (b >= thresholds(threshold, w)))[0]
        fs.append(np.full(len(slots), fi, dtype=np.int64))
        ds.append(docs[slots].astype(np.int64))
        ss.append(b[slots].astype(np.int64))
    f, d, sc = np.concatenate(fs), np.concatenate(ds), np.concatenate(ss)
    order = np.lexsort((d, f, -sc))              # best descending, then (file, document) ascending
    if num_results:
        order = order[:num_results]
    return list(zip(f[order].tolist(), d[order].tolist(), sc[order].tolist()))


def results(files, q, z, W, threshold=0.0, num_results=0, mode="error"):
    """[(file, doc, best)] of one query in result order"""
    return results_from(tables(files, q, z, W, mode), threshold, num_results)


# ---- the structure fixture of tests/test_gpu_window.py: its documents and what they have to reach ------------------------
STRUCT_K, STRUCT_LQ, STRUCT_W, STRUCT_DOCS = 31, 630, 100, 20


def structure_pieces(q, z):
    """{document: [pieces of the query]}: a document holds every k-mer of its pieces, so a piece of L characters sets the
    L - k + 1 - z positions from its offset on and nothing else: the matrix is otherwise empty, and the pieces of one
    document lie more than z positions apart (closer ones would share the terms of the positions between them).
    n = 600 - z positions, z <= 3; the default segments of this query (one chunk of documents: 256 lane groups) end at multiples of 100."""
    k = STRUCT_K

    def run(first, count):                      # the piece that sets `count` positions from `first` on
        return q[first:first + count + z + k - 1]

    n = len(q) - k + 1 - z
    scattered = []                              # (f): every fifth position, 110 of them: isolated set positions
    for p in range(20, 20 + 5 * 110, 5):
        scattered.append(run(p, 1))
    return {
        0: [run(250, 110)],                                     # (a) one run of >= W positions; as many as (f) holds
        1: [run(100, 40), run(155, 40)],                        # (b) two runs of 40 inside one window (95 positions apart)
        2: [run(100, 40), run(300, 40)],                        # (c) the same two runs more than W apart
        3: [q],                                                 # (d) a run across every segment boundary
        4: [run(30, 64), run(30 + 64 + 130, 65)],               # (e) 64 set, 130 unset, 65 set
        5: scattered,                                           # (f)
        6: [run(0, 1)],                                         # the first position alone
        7: [run(n - 1, 1)],                                     # the last
        8: [run(350, 100)],                                     # exactly one window, across the segment boundary at 400
        9: [run(0, 99)],                                        # one short of a window, from the first position
        10: [run(n - 99, 99)],                                  # ... to the last
        11: [run(60, 50), run(114, 50)],                        # four unset positions inside the best window
        12: [run(p, 10) for p in range(5, 580, 25)],            # runs of 10 every 25: 40 of every 100
        13: [run(390, 20)],                                     # a short run across the segment boundary at 400
        14: [run(200, 80), run(320, 80)],                       # two runs of 80, 40 apart: 80 beats any mix (60 + 40 unset)
        15: [run(10, 79)],                                      # just below 0.8
        16: [run(500, 80)],                                     # just at 0.8
        17: [run(150, 30), run(200, 30), run(250, 30)],         # three runs of 30 every 50: 60 of every 100
    }


def structure_conditions(win, docs):
    """what the fixture has to reach, asserted on the checker alone; win: bool [n, slots] at the fixture's W"""
    W = STRUCT_W
    n = win.shape[0]
    b = best(win, W)
    score = win.sum(axis=0, dtype=np.int64)
    w = width(W, n)
    real = docs >= 0
    assert (b[real] == w).any()                                                 # some document has best = w
    assert ((b > 0) & (b < np.minimum(w, score)) & real).any()                  # ... and some 0 < best < min(w, score)
    assert b[1] == 80 and b[2] == 40 and score[1] == score[2] == 80             # (b) beats (c)
    assert score[0] == score[5] and b[0] == w and b[5] == 20 and score[0] == 110                    # (a) and (f): equal plain scores
    assert (best(win, 50)[real] != b[real]).any()                               # W = 100 differs from W = 50
    hit = b[real] >= thresholds(0.8, w)
    assert hit.any() and not hit.all()                                          # threshold 0.8: some, not all
    assert score[3] == n                                                        # (d)
    assert b[4] == 65 and score[4] == 129                                       # (e): d climbs to 64 and the count back to 65
    assert b[11] == 96 and b[14] == 80 and b[17] == 60 and b[12] == 40
    return b, score
