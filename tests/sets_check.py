"""The document-set checker (test infrastructure), on top of tests/prevalence_check.py and invalid_check.py: for a labelling
of a file's documents with sets, the positions of a query that AT LEAST ONE member of a set holds (`any`) and that EVERY
member holds (`all`).  Position p of n = T_f - z is set in a document as prevalence_check.windows says (terms p .. p + z all
present; under `miss` / `skip` a window with a character outside ACGT is not set); the members of a set are the score slots
of the real documents that carry its label -- padding slots and unlabelled documents never take part.  A set is a hit when
its key reaches max(1, ceil(threshold * P)), P = n, or under `skip` the valid positions of invalid_check; threshold <= 0
returns every non-empty set.  Records are ordered by key descending, the other count descending, (file, set) ascending.
No engine code in it."""

import numpy as np

from tests import findere_check as F
from tests import invalid_check as I
from tests import prevalence_check as V

NO_SET = -1
_WINDOWS = {}     # (file, query, z, mode) -> windows: a test asks for the same reference under many labellings
_COUNTS = {}      # ... and (file, query, z, mode, labels) -> counts under many thresholds, keys and limits


def windows(fb, q, z, mode="error"):
    """prevalence_check.windows, shared between callers: do not write to it"""
    key = (id(fb), bytes(q), z, mode)
    if key not in _WINDOWS:
        _WINDOWS[key] = (fb, V.windows(fb, q, z, mode))          # (holds the file: its id stays its own)
    return _WINDOWS[key][1]


def slot_of_doc(fb):
    """int64 [num_docs]: the score slot of every real document"""
    docs = fb.doc_of_slot()
    out = np.full(fb.num_docs, -1, dtype=np.int64)
    live = np.nonzero(docs >= 0)[0]
    out[docs[live]] = live
    assert (out >= 0).all()
    return out


def counts(fb, q, z, labels, mode="error"):
    """{set: (any, all)} for the non-empty sets of `labels` (int [num_docs], -1: the document is in no set)"""
    labels = np.asarray(labels, dtype=np.int64)
    assert len(labels) == fb.num_docs
    key = (id(fb), bytes(q), z, mode, labels.tobytes())
    if key in _COUNTS:
        return dict(_COUNTS[key][1])
    win = windows(fb, q, z, mode)
    slots = slot_of_doc(fb)
    out = {}
    for c in sorted(set(labels[labels >= 0].tolist())):
        members = slots[labels == c]
        out[c] = (int(win[:, members].any(axis=1).sum()), int(win[:, members].all(axis=1).sum()))
    _COUNTS[key] = (fb, dict(out))
    return out


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


def results(files, labelings, q, z, threshold=0.0, rank_by="any", num_results=0, mode="error"):
    """[(file_no, set, any, all)] of one query in result order; labelings: per file the labels or None (no labels)"""
    assert rank_by in ("any", "all")
    recs = []
    for fi, (fb, labels) in enumerate(zip(files, labelings)):
        if labels is None:
            continue
        P = denominator(fb, q, z, mode)
        for c, (a, b) in counts(fb, q, z, labels, mode).items():
            key = a if rank_by == "any" else b
            if threshold > 0 and (P == 0 or key < threshold_for(threshold, P)):
                continue
            recs.append((fi, c, a, b))
    k, o = (2, 3) if rank_by == "any" else (3, 2)
    recs.sort(key=lambda r: (-r[k], -r[o], r[0], r[1]))
    return recs[:num_results] if num_results else recs


def arrays(files, labelings, queries, z, threshold=0.0, rank_by="any", num_results=0, mode="error"):
    """(offsets uint64 [nq + 1], records as an int64 [n, 4] array) in the layout Search.search_sets_arrays returns"""
    offs, rows = [0], []
    for q in queries:
        rows += results(files, labelings, q, z, threshold, rank_by, num_results, mode)
        offs.append(len(rows))
    return np.array(offs, dtype=np.uint64), np.array(rows, dtype=np.int64).reshape(-1, 4)
