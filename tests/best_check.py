"""The best-of-group checker (test infrastructure): a plain numpy / Python restatement of cobs_gpu_search_best on top of
tests/findere_check.py (FileBits: per-query scores under findere z) and tests/invalid_check.py (the `miss` / `skip`
policies), with no engine code in it.

Group g is the queries [offsets[g], offsets[g + 1]) of the call.  For query q and file f
    s(q, d) = the score the plain search gives document d (findere z, the invalid-bases policy),
    P(q, f) = the positions that score is out of: T - z under `error` and `miss`, V under `skip` (it can be 0).
Member a is BETTER than member b in document d when, in this order,
    1. s_a * P_b > s_b * P_a   (the larger fraction, exact; a member with P = 0 has s = 0 and the fraction 0: it is
                                compared as 0 / 1 -- literally its cross products would equal everybody's),
    2. s_a > s_b               (equal fraction: the longer member),
    3. a < b by index in the call.
Per (group, file, real document): query = the best member, score = its s, positions = its P, ties = the members whose
fraction equals the best one's (the best one included).  A document is reported when score >= max(1, ceil(threshold *
positions)) (in double; every real document when threshold <= 0); a group without members reports nothing.  A group's
records: by fraction descending (exact), then score descending, then (file, doc); num_results cuts the list.
"""
from fractions import Fraction

import numpy as np

from tests import findere_check as F
from tests import groups_check as G

NONE = 0xFFFFFFFF
EMPTY = (0, 0, NONE, 0)          # (score, positions, query, ties) of no member at all


def _den(P):
    return P if P > 0 else 1


def better(a, b):
    """members (s, P, q) as Python integers: a is better than b"""
    (sa, Pa, qa), (sb, Pb, qb) = a, b
    x, y = sa * _den(Pb), sb * _den(Pa)
    if x != y:
        return x > y
    if sa != sb:
        return sa > sb
    return qa < qb


def same_fraction(a, b):
    return a[0] * _den(b[1]) == b[0] * _den(a[1])


def best_of(members):
    """the definition, literally: members [(s, P, q)] of one cell -> (score, positions, query, ties)"""
    if not members:
        return EMPTY
    best = members[0]
    for m in members[1:]:
        if better(m, best):
            best = m
    return (best[0], best[1], best[2], sum(1 for m in members if same_fraction(m, best)))


def merge(x, y):
    """two states (score, positions, query, ties) of disjoint sets of members -> the state of their union"""
    a, b = x[:3], y[:3]
    if same_fraction(a, b):
        w = a if better(a, b) else b
        return (w[0], w[1], w[2], x[3] + y[3])
    return x if better(a, b) else y


def cells(files, queries, offsets, z=0, mode="error"):
    """-> per file (score, positions, query, ties), each int64 [n_groups, slots]: the best member of every cell, the
    members taken one after the other with the rule above (exact in int64: scores and P are below 2^31 here)"""
    ng = len(offsets) - 1
    assert offsets[0] == 0 and offsets[ng] == len(queries) and all(offsets[g] <= offsets[g + 1] for g in range(ng))
    out = []
    for fb in files:
        bs = np.zeros((ng, fb.slots), dtype=np.int64)
        bp = np.zeros((ng, fb.slots), dtype=np.int64)
        bq = np.full((ng, fb.slots), NONE, dtype=np.int64)
        members = [[] for _ in range(ng)]
        for g in range(ng):
            for q in range(int(offsets[g]), int(offsets[g + 1])):
                s = G.scores(fb, queries[q], z, mode).astype(np.int64)
                P = int(G.positions_of(fb, queries[q], z, mode))
                assert int(s.max(initial=0)) < 2 ** 31 and P < 2 ** 31 and (P > 0 or not s.any())
                members[g].append((s, P))
                x, y = s * np.maximum(bp[g], 1), bs[g] * _den(P)
                win = (x > y) | ((x == y) & ((s > bs[g]) | ((s == bs[g]) & (q < bq[g]))))
                bs[g] = np.where(win, s, bs[g])
                bp[g] = np.where(win, P, bp[g])
                bq[g] = np.where(win, q, bq[g])
        bt = np.zeros((ng, fb.slots), dtype=np.int64)
        for g in range(ng):
            for s, P in members[g]:
                bt[g] += s * np.maximum(bp[g], 1) == bs[g] * _den(P)
        out.append((bs, bp, bq, bt))
    return out


def threshold_of(threshold, positions):
    if not threshold > 0:
        return 0
    return max(1, F.ceil_product(threshold, positions))


def order_key(h):
    """h = (file, doc, query, score, positions, ties)"""
    return (-Fraction(h[3], _den(h[4])), -h[3], h[0], h[1])


_CELLS = {}      # shared between the thresholds and limits of a test, never written to


def results(files, queries, offsets, z=0, mode="error", threshold=0.0, num_results=0):
    """-> per group the list of (file, doc, query, score, positions, ties) in result order"""
    key = (tuple(id(f) for f in files), tuple(bytes(q) for q in queries), tuple(int(o) for o in offsets), z, mode)
    if key not in _CELLS:
        _CELLS[key] = (files, cells(files, queries, offsets, z, mode))
    per_file = _CELLS[key][1]
    out = []
    for g in range(len(offsets) - 1):
        hits = []
        if offsets[g + 1] > offsets[g]:
            for fi, fb in enumerate(files):
                bs, bp, bq, bt = (a[g] for a in per_file[fi])
                docs = fb.doc_of_slot()
                for slot in np.nonzero(docs >= 0)[0]:
                    if int(bs[slot]) >= threshold_of(threshold, int(bp[slot])):
                        hits.append((fi, int(docs[slot]), int(bq[slot]), int(bs[slot]), int(bp[slot]), int(bt[slot])))
        hits.sort(key=order_key)
        out.append(hits[:num_results] if num_results else hits)
    return out
