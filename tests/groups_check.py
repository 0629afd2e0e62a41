"""The grouped-search checker (test infrastructure): a plain numpy restatement of cobs_gpu_search_groups on top of
tests/findere_check.py (FileBits: per-query scores under findere z) and tests/invalid_check.py (the `miss` / `skip`
policies), with no engine code in it.

Group g is the queries [offsets[g], offsets[g + 1]).  Per (group, file, document):
    sum   = the sum of the per-query scores,
    votes = the queries whose score reaches the per-query threshold of read_threshold (ceil(rt * (T - z)); `skip`:
            max(1, ceil(rt * V)) when rt > 0, else 0),
    P     = the positions the queries are scored over, summed: T - z under `error` and `miss`, V under `skip`.
A group's result: the real documents with sum >= max(1, ceil(threshold * P)) (every real document when threshold <= 0),
by sum descending, then (file, document); num_results cuts the list.  No "single hash in total: index order" rule.
"""

import numpy as np

from tests import findere_check as F
from tests import invalid_check as I

MODES = ("error", "miss", "skip")

_SCORES = {}      # (file, query, z, mode) -> (file, scores): shared between tests, never written to


def scores(fb, q, z, mode):
    """uint32 [slots]: what cobs_gpu_search_batch scores for q in every slot of the file"""
    assert mode in MODES
    if mode != "error":
        return I.scores(fb, q, z)
    key = (id(fb), bytes(q), z)
    if key not in _SCORES:
        _SCORES[key] = (fb, fb.scores(q, z))
    return _SCORES[key][1]


def read_threshold_of(fb, q, z, mode, rt):
    if mode == "skip":
        return I.threshold("skip", rt, fb, q, z)
    return F.threshold_for(rt, fb.positions(q, z))


def positions_of(fb, q, z, mode):
    return I.valid_positions(fb, q, z) if mode == "skip" else fb.positions(q, z)


def totals(files, queries, offsets, z=0, mode="error", read_threshold=0.0):
    """-> (sums, votes: per file uint64 [n_groups, slots]; P uint64 [n_groups, n_files])"""
    ng = len(offsets) - 1
    assert offsets[0] == 0 and offsets[ng] == len(queries) and all(offsets[g] <= offsets[g + 1] for g in range(ng))
    sums = [np.zeros((ng, fb.slots), dtype=np.uint64) for fb in files]
    votes = [np.zeros((ng, fb.slots), dtype=np.uint64) for fb in files]
    P = np.zeros((ng, len(files)), dtype=np.uint64)
    for g in range(ng):
        for q in queries[int(offsets[g]):int(offsets[g + 1])]:
            for fi, fb in enumerate(files):
                sc = scores(fb, q, z, mode)
                sums[fi][g] += sc
                votes[fi][g] += sc >= read_threshold_of(fb, q, z, mode, read_threshold)
                P[g, fi] += positions_of(fb, q, z, mode)
    return sums, votes, P


def group_threshold(threshold, positions):
    if not threshold > 0:
        return 0
    return max(1, F.ceil_product(threshold, positions, 2 ** 64 - 1))      # (64-bit sums: clamped at 2^64 - 1)


def results(files, queries, offsets, z=0, mode="error", threshold=0.0, read_threshold=0.0, num_results=0):
    """-> (per group the list of (file, doc, sum, votes) in result order, P)"""
    sums, votes, P = totals(files, queries, offsets, z, mode, read_threshold)
    out = []
    for g in range(len(offsets) - 1):
        hits = []
        for fi, fb in enumerate(files):
            docs = fb.doc_of_slot()
            gthr = group_threshold(threshold, int(P[g, fi]))
            for slot in np.nonzero((docs >= 0) & (sums[fi][g] >= gthr))[0]:
                hits.append((fi, int(docs[slot]), int(sums[fi][g][slot]), int(votes[fi][g][slot])))
        hits.sort(key=lambda h: (-h[2], h[0], h[1]))
        out.append(hits[:num_results] if num_results else hits)
    return out, P
