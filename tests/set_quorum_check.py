"""The set-quorum checker (test infrastructure), on top of tests/prevalence_check.py and invalid_check.py: for a labelling of
a file's documents with sets, HOW MANY members of every set hold each position of a query, and the soft core of a set.
Position p of n = T_f - z is set in a document as prevalence_check.windows says (terms p .. p + z all present; under `miss` /
`skip` a window with a character outside ACGT is not set); the members of a set are the score slots of the real documents
that carry its label -- padding slots and unlabelled documents never count.  count[c][p] = the members of set c that hold
position p; need(c) = max(1, ceil(quorum * members(c))) in double; core = the positions with count >= need, any = the
positions with count > 0.  A set is a hit when core reaches max(1, ceil(threshold * P)), P = n, or under `skip` the valid
positions of invalid_check; threshold <= 0 returns every non-empty set.  Records are ordered by core descending, any
descending, (file, set) ascending.  No engine code in it, and none of tests/sets_check.py's."""
import math

import numpy as np

from tests import findere_check as F
from tests import invalid_check as I
from tests import prevalence_check as V

_PROFILES = {}    # (file, query, z, mode, labels) -> profile: a test asks for the same counts under many quorums and thresholds


def slot_of_doc(fb):
    """int64 [num_docs]: the score slot of every real document"""
    docs = fb.doc_of_slot()
    out = np.full(fb.num_docs, -1, dtype=np.int64)
    live = np.nonzero(docs >= 0)[0]
    out[docs[live]] = live
    assert (out >= 0).all()
    return out


def nonempty_sets(labels):
    """the set numbers with a member, ascending"""
    labels = np.asarray(labels, dtype=np.int64)
    return sorted(set(labels[labels >= 0].tolist()))


def members(labels):
    """{set: members}"""
    labels = np.asarray(labels, dtype=np.int64)
    sets, n = np.unique(labels[labels >= 0], return_counts=True)
    return dict(zip(sets.tolist(), n.tolist()))


def profile(fb, q, z, labels, mode="error"):
    """uint32 [non-empty sets, n]: row c = the c-th non-empty set in ascending set number (do not write to it)"""
    labels = np.asarray(labels, dtype=np.int64)
    assert len(labels) == fb.num_docs
    key = (id(fb), bytes(q), z, mode, labels.tobytes())
    if key not in _PROFILES:
        win = V.windows(fb, q, z, mode)                     # presence matrix [n, slots]
        slots = slot_of_doc(fb)
        # the labelled documents grouped by set (a stable sort), their columns summed group by group
        docs = np.nonzero(labels >= 0)[0]
        docs = docs[np.argsort(labels[docs], kind="stable")]
        out = np.zeros((0, win.shape[0]), dtype=np.uint32)
        if len(docs) and win.shape[0]:
            starts = np.nonzero(np.diff(labels[docs], prepend=-1))[0]
            out = np.add.reduceat(win[:, slots[docs]].astype(np.uint32), starts, axis=1).T
        elif len(docs):
            out = np.zeros((len(set(labels[docs].tolist())), 0), dtype=np.uint32)
        _PROFILES[key] = (fb, np.ascontiguousarray(out))    # (holds the file: its id stays its own)
    return _PROFILES[key][1]


def need(quorum, m):
    """max(1, ceil(quorum * members)): the double product, as the library's host code forms it"""
    if not (quorum > 0 and quorum <= 1):
        raise ValueError("quorum: a number in (0, 1] (the call refuses every other)")
    return max(1, int(math.ceil(float(quorum) * float(m))))


def counts(fb, q, z, labels, quorum, mode="error"):
    """{set: (core, any)} for the non-empty sets of `labels` (int [num_docs], -1: the document is in no set)"""
    prof = profile(fb, q, z, labels, mode)
    mem = members(labels)
    sets = nonempty_sets(labels)
    needs = np.array([need(quorum, mem[c]) for c in sets], dtype=np.int64).reshape(-1, 1)
    core = (prof.astype(np.int64) >= needs).sum(axis=1)
    held = (prof > 0).sum(axis=1)
    return {c: (int(core[i]), int(held[i])) for i, c in enumerate(sets)}


def denominator(fb, q, z, mode="error"):
    """P: the positions the search scores the query over in this file"""
    if mode == "skip" and fb.canonicalize:
        return I.valid_positions(fb, q, z)
    return fb.positions(q, z)


def threshold_for(t, P):
    """max(1, ceil(t * P)) in double for t > 0; 0 (every non-empty set) otherwise"""
    if not t > 0:
        return 0
    return max(1, F.ceil_product(t, P))


def results(files, labelings, q, z, quorum, threshold=0.0, num_results=0, mode="error"):
    """[(file_no, set, core, any)] of one query in result order; labelings: per file the labels or None (no labels)"""
    recs = []
    for fi, (fb, labels) in enumerate(zip(files, labelings)):
        if labels is None:
            continue
        P = denominator(fb, q, z, mode)
        for c, (core, held) in counts(fb, q, z, labels, quorum, mode).items():
            if threshold > 0 and (P == 0 or core < threshold_for(threshold, P)):
                continue
            recs.append((fi, c, core, held))
    recs.sort(key=lambda r: (-r[2], -r[3], r[0], r[1]))
    return recs[:num_results] if num_results else recs


def arrays(files, labelings, queries, z, quorum, threshold=0.0, num_results=0, mode="error"):
    """(offsets uint64 [nq + 1], records as an int64 [n, 4] array) in the layout Search.search_sets_quorum_arrays returns"""
    offs, rows = [0], []
    for q in queries:
        rows += results(files, labelings, q, z, quorum, threshold, num_results, mode)
        offs.append(len(rows))
    return np.array(offs, dtype=np.uint64), np.array(rows, dtype=np.int64).reshape(-1, 4)


def segments(files, labelings, queries, z, mode="error"):
    """(offsets uint64 [nq * nfiles + 1], counts uint32) in the layout cobs_gpu_set_prevalence returns"""
    parts, offs = [], [0]
    for q in queries:
        for fb, labels in zip(files, labelings):
            seg = profile(fb, q, z, labels, mode).reshape(-1) if labels is not None else np.zeros(0, dtype=np.uint32)
            parts.append(seg)
            offs.append(offs[-1] + len(seg))
    out = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)
    return np.array(offs, dtype=np.uint64), out.astype(np.uint32)
