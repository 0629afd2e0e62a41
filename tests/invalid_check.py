"""The invalid-bases checker (test infrastructure): a numpy restatement of the `miss` and `skip` policies on top of
findere_check.FileBits, with no engine code in it.

A character is valid when it is an upper-case A, C, G or T (files with canonicalize != 0; the others take every byte).
Term p of a query is forced ABSENT from every document when one of its k characters is invalid.  A scored position
p in [0, T - z) is valid when its k + z characters [p, p + k + z) all are; V counts them.  Scores count the valid
positions whose z + 1 terms are all present.  Thresholds: miss = ceil(t * (T - z)), skip = ceil(t * V), at least 1 when
t > 0 (a query without a valid position matches nothing), 0 when t <= 0.  The "single hash in total: index order" rule
keeps the nominal sum of (T - z) * H.
"""
import numpy as np

from tests import findere_check as F

MODES = ("miss", "skip")


def char_valid(fb, q):
    """bool [len(q)]"""
    a = np.frombuffer(bytes(q), dtype=np.uint8)
    if not fb.canonicalize:
        return np.ones(len(a), dtype=bool)
    return (a == ord("A")) | (a == ord("C")) | (a == ord("G")) | (a == ord("T"))


def run_valid(fb, q, width):
    """bool [len(q) - width + 1]: the `width` characters from every position are all valid"""
    ok = char_valid(fb, q)
    n = len(ok) - width + 1
    if n <= 0:
        return np.zeros(0, dtype=bool)
    bad_before = np.concatenate([[0], np.cumsum(~ok)])
    return (bad_before[width:width + n] - bad_before[:n]) == 0


def presence(fb, q):
    """FileBits.presence with the rows of terms that hold an invalid character forced false"""
    # (any valid letter in the place of an invalid one: the rows of those terms are overwritten)
    ok = char_valid(fb, q)
    clean = bytes(c if v else ord("A") for c, v in zip(bytes(q), ok))
    P = fb.presence(clean).copy()
    P[~run_valid(fb, q, fb.term_size)] = False
    return P


def position_valid(fb, q, z):
    """bool [T - z]"""
    return run_valid(fb, q, fb.term_size + z)


def valid_positions(fb, q, z):
    """V"""
    return int(position_valid(fb, q, z).sum())


_SCORES = {}      # (file, query, z) -> scores: a test asks for the same reference under many thresholds and limits


def scores(fb, q, z):
    """uint32 [slots] (shared between callers: do not write to it)"""
    key = (id(fb), bytes(q), z)
    if key not in _SCORES:
        _SCORES[key] = (fb, _scores(fb, q, z))          # (holds the file: its id stays its own)
    return _SCORES[key][1]


def _scores(fb, q, z):
    P = presence(fb, q)
    n = P.shape[0] - z
    if n <= 0:
        return np.zeros(fb.slots, dtype=np.uint32)
    win = np.ones((n, fb.slots), dtype=bool)
    for j in range(z + 1):
        win &= P[j:j + n]
    return win.sum(axis=0).astype(np.uint32)


def position_bits(fb, q, z, slot):
    """bool [T - z]: the presence vector of one score slot (what hit_positions reports)"""
    P = presence(fb, q)[:, slot]
    n = len(P) - z
    win = np.ones(n, dtype=bool)
    for j in range(z + 1):
        win &= P[j:j + n]
    return win


def counts(files, q, z):
    return np.concatenate([scores(f, q, z) for f in files])


def threshold(mode, t, fb, q, z):
    assert mode in MODES
    if mode == "miss":
        return F.threshold_for(t, fb.positions(q, z))
    if not t > 0:
        return 0
    return max(1, F.threshold_for(t, valid_positions(fb, q, z)))


def results(files, q, z, mode, t=0.0, num_results=0):
    """(file, doc, score) with score >= threshold(mode, ...); score descending, ties (file, doc) ascending; index order
    when the nominal max_counts = sum_f (T_f - z) * H_f is <= 1"""
    hits = []
    for fi, f in enumerate(files):
        sc = scores(f, q, z)
        docs = f.doc_of_slot()
        thr = threshold(mode, t, f, q, z)
        for slot in np.nonzero((docs >= 0) & (sc >= thr))[0]:
            hits.append((fi, int(docs[slot]), int(sc[slot])))
    if sum(f.positions(q, z) * f.num_hashes for f in files) > 1:
        hits.sort(key=lambda h: (-h[2], h[0], h[1]))
    if num_results:
        hits = hits[:num_results]
    return hits


def segments(fb, q, min_len):
    """the maximal runs of valid characters of at least min_len characters"""
    ok = char_valid(fb, q)
    out, start = [], None
    for i, v in enumerate(list(ok) + [False]):
        if v and start is None:
            start = i
        elif not v and start is not None:
            if i - start >= min_len:
                out.append(bytes(q)[start:i])
            start = None
    return out


# ---- the query sets of the GPU tests (their conditions are checked on the CPU: test_invalid_bases_cpu.py) ----

def with_n(q, offsets, ch=b"N"):
    b = bytearray(q)
    for o in offsets:
        b[o:o + 1] = ch
    return bytes(b)


def placement_queries(src, k, z=0):
    """one N at the edges of the first / last k-mer, two Ns k and k + 1 apart, a run across an 8-term block boundary, an
    all-N query, one valid window, lower case and other letters, and an untouched query"""
    ln = 3 * k + 40
    base = bytes(src[17:17 + ln])
    qs = [base]
    for o in (0, k - 1, k, ln - k, ln - 1):
        qs.append(with_n(base, [o]))
    qs.append(with_n(base, [20, 20 + k]))            # no valid term between them
    qs.append(with_n(base, [20, 20 + k + 1]))        # exactly one
    qs.append(with_n(base, range(5, 12)))            # terms 0 .. 11 die: across the boundary of blocks 0 and 1
    qs.append(with_n(base, range(k + 6, k + 19)))
    qs.append(b"N" * ln)                             # V = 0
    w = k + z
    one = bytearray(b"N" * ln)
    one[33:33 + w] = base[33:33 + w]                 # exactly one valid window
    qs.append(bytes(one))
    qs.append(with_n(base, [40], b"a"))              # lower case is invalid
    qs.append(with_n(base, [41, 90], b"R"))
    qs.append(with_n(base, [ln - k - 1 - z]))        # kills the last windows only
    return qs
