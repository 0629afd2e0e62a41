"""Thresholds exactly at the boundary (test infrastructure): the rule every search family turns a caller's threshold into
an integer bound with, stated once, and the doubles and fixtures that put a document exactly on that bound.

The rule (reference cobs/query/classic_search.cpp:444-449, pass.cpp: threshold_for): bound = ceil(threshold * P) with
the product formed in DOUBLE, a key is a hit when key >= bound, the bound is clamped at 2^32 - 1, and most families
say "at least 1" for a threshold > 0.  A threshold that is not > 0 (0, -0.0, negative, -inf, NaN) asks for every
document: bound 0.  A product that is NaN (inf * 0) counts as 0.

on_and_above / adversarial / CLASSES need nothing but the standard library.  The fixture half (Fixture, Family) builds
index files with oracle/construct.py and asks the *_check.py checkers; it never loads the GPU library.
"""
import math
from fractions import Fraction

LIMIT32 = 2 ** 32 - 1
LIMIT64 = 2 ** 64 - 1
_FROM64 = 18446744073709549568.0          # the largest double below 2^64: groups.cpp clamps from there on


def bound(t, P, at_least_one=False, limit=LIMIT32):
    """the rule above, as a Python integer (0: every document).  Written on its own on purpose: the checkers share
    findere_check.ceil_product, and this is what they are all held against -- it must never import that."""
    t = float(t)
    if not t > 0:
        return 0
    v = t * float(P)
    if v != v:
        v = 0.0
    if v >= (_FROM64 if limit == LIMIT64 else float(limit)):
        b = limit
    else:
        b = int(math.ceil(v))
    return max(b, 1) if at_least_one else b


def _ceil(t, P):
    return math.ceil(float(t) * float(P))


def on_and_above(c, P):
    """(t_on, t_above): the LARGEST double with ceil(t * P) == c and its successor, which has ceil(t * P) == c + 1"""
    assert 1 <= c and P >= 1
    t = c / P
    while _ceil(t, P) > c:
        t = math.nextafter(t, 0.0)
    assert _ceil(t, P) == c
    while _ceil(math.nextafter(t, math.inf), P) == c:
        t = math.nextafter(t, math.inf)
    above = math.nextafter(t, math.inf)
    assert _ceil(above, P) == c + 1, (c, P, t)
    return t, above


def adversarial(P_values):
    """-> [(direction, t, P, double bound, exact bound)]: thresholds whose double bound differs from exact arithmetic.
      "up"    t = the double nearest c / P, and t * P rounds UP past c: the double rule says c + 1, the rational c / P
              says c (0.07 * 100 -> 8);
      "down"  t a double strictly above c / P whose product with P rounds DOWN onto c: the double rule says c, the exact
              value of t says c + 1.
    Every c in [1, P) of every P is tried."""
    out = []
    for P in P_values:
        for c in range(1, int(P)):
            t = c / P
            if _ceil(t, P) == c + 1 and math.ceil(Fraction(c, P) * P) == c:
                out.append(("up", t, P, c + 1, c))
            u = t
            for _ in range(4):
                u = math.nextafter(u, math.inf)
                if Fraction(u) * P > c and u * float(P) == float(c):
                    out.append(("down", u, P, c, int(math.ceil(Fraction(u) * P))))
                    break
    return out


CLASSES = (5e-324, 1e-300, 1.0, math.nextafter(1.0, 2.0), 2.0, 1e300, math.inf, math.nan, -0.0, -1.0, -math.inf)


def case_list(keys, P, at_least_one, prefer_from=0, limit=LIMIT32, smallest=1):
    """the thresholds of one (family, target) and what each has to show -> [(name, t, bound)].

    keys: the checker's keys of the target's real documents at threshold 0.  One c with c - 1, c and c + 1 among the keys
    gives t_on and t_above; one adversarial pair per direction; every entry of CLASSES.  Condition (a): a bound inside
    [1, P] must have a key exactly on it and one exactly one below it -- an AssertionError otherwise, so no case is
    left out quietly.  A bound of 0 returns every document and a bound above P none: those classes have no boundary
    document by definition, and the caller compares the whole result.  prefer_from: bounds from that fraction of P on are
    taken first (a top-k pass of k documents shows a boundary only when fewer than k documents lie above it).  smallest:
    the smallest key above 0 the family can give (coverage: one set position covers term size + findere bases): a bound
    in [1, smallest] has its neighbours at 0 and at `smallest`."""
    have = set(int(k) for k in keys)
    P = int(P)

    def shown(b):
        return b in have and b - 1 in have

    cs = [c for c in range(P - 1, 1, -1) if shown(c) and c + 1 in have]
    pick = [c for c in cs if prefer_from * P <= c <= 0.95 * P] or cs
    assert pick, ("no c with c - 1, c, c + 1 among the keys", P, sorted(have)[:20])
    c = pick[0]
    t_on, t_above = on_and_above(c, P)
    out = [("t_on", t_on, c), ("t_above", t_above, c + 1)]
    adv = adversarial([P])
    for direction in ("up", "down"):
        cand = [a for a in adv if a[0] == direction and shown(a[3])]
        best = [a for a in cand if a[3] >= prefer_from * P] or cand
        assert best, ("no adversarial pair with documents on its bound", direction, P)
        out.append(("adversarial_" + direction, best[0][1], best[0][3]))
    for t in CLASSES:
        out.append(("class_%r" % t, t, bound(t, P, at_least_one, limit)))
    for name, t, b in out:
        assert b == bound(t, P, at_least_one, limit), (name, t, P, b)
        if 1 <= b <= smallest:
            assert 0 in have and smallest in have, ("condition (a): no document at 0 and at the smallest key", name, t, P, b)
        elif smallest < b <= P:
            assert shown(b), ("condition (a): no document on the bound and one below it", name, t, P, b)
    return out


# ---- the fixture: documents that hold PREFIXES of a query's terms, so that every key from 0 to P exists --------------------

K_MAIN, K_OTHER = 31, 20
SRC_LEN = 140                # the coverage query: 130 characters have no adversarial pair, 140 have them
Q_LEN = 130                  # 100 31-mers: a denominator with adversarial pairs in both directions
FINDERE_Z = 3
FINDERE_LEN = 133            # 103 terms, 100 positions
WINDOW = 50
SET0_MEMBERS = 100


def sources():
    """(SRC, R): the text the documents are planted from, and a member of a group no prefix document holds"""
    from oracle import oracle as O
    return O.random_sequence(SRC_LEN, 4711), O.random_sequence(Q_LEN, 4712)


def stair(num_docs, V):
    """the planted terms of every document: ("prefix", m) = the first m terms of SRC; document V holds all but the first.
    Documents 0 .. V - 1 hold 1 .. V terms (the set of SET0_MEMBERS members is cut from them), the others cycle through
    0 .. V again.  The documents V - 1 (every term) and V also hold every term of R: a group [Q, R] reaches its full sum and
    one below it there."""
    assert num_docs > V + 2
    out = []
    for j in range(num_docs):
        if j < V:
            out.append(("prefix", j + 1))
        elif j == V:
            out.append(("tail", 1))
        else:
            out.append(("prefix", (j - V - 1) % (V + 1)))
    return out


def labels_of(num_docs, V):
    """document sets: set 0 = the documents 0 .. 99 (1 .. 100 terms: position p is held by 100 - p members), and one set
    per number of terms among the other documents (members with equal columns: any = all = core)"""
    import numpy as np
    plan = stair(num_docs, V)
    lab = np.zeros(num_docs, dtype=np.int64)
    for j in range(SET0_MEMBERS, num_docs):
        kind, m = plan[j]
        lab[j] = 1 + (m if kind == "prefix" else V + 1)
    # (set numbers are dense for the library: renumber in ascending order)
    uniq = {v: i for i, v in enumerate(sorted(set(lab.tolist())))}
    return np.array([uniq[v] for v in lab.tolist()], dtype=np.int64)


def build_file(path, kind, k, num_hashes, sigs, num_docs, page_size=0):
    """write one index file over an otherwise empty matrix -> findere_check.FileBits"""
    import numpy as np
    from oracle import construct as K
    from oracle import oracle as O
    from tests import findere_check as F
    src, other = sources()
    hs, good = O.term_hashes(src, k, 1, num_hashes)
    ho, _ = O.term_hashes(other, k, 1, num_hashes)
    assert good.all()
    V = len(hs)
    docs = []
    for j, (what, m) in enumerate(stair(num_docs, V)):
        h = hs[:m] if what == "prefix" else hs[m:]
        if V - 1 <= j <= V:
            h = np.concatenate([h, ho])
        docs.append(K.Doc("doc_%05d" % j, "doc_%05d" % j, 0, len(h), h))
    names = [d.name for d in docs]
    if kind == "classic":
        m = K.build_matrix(docs, sigs[0], (num_docs + 7) // 8)
        K.write_classic(path, k, 1, names, sigs[0], num_hashes, m)
        return F.FileBits(k, 1, num_hashes, [m], num_docs)
    per = 8 * page_size
    assert (len(sigs) - 1) * per < num_docs < len(sigs) * per          # a partly filled last sub-index
    mats = [K.build_matrix(docs[p * per:(p + 1) * per], s, page_size) for p, s in enumerate(sigs)]
    K.write_compact(path, k, 1, page_size, [(s, num_hashes) for s in sigs], names, mats)
    return F.FileBits(k, 1, num_hashes, mats, num_docs)


FILES = {
    # name: (kind, k, H, signature sizes, documents, page_size)
    "classic": ("classic", K_MAIN, 1, [5003], 300, 0),
    "compact": ("compact", K_MAIN, 2, [3001, 4001, 5003], 300, 16),
    "other": ("compact", K_OTHER, 1, [3001, 4001, 2003], 290, 16),     # (290: a total weight with pairs in both directions)
    "rows": ("classic", K_MAIN, 1, [12000], 320, 0),                  # 40-byte rows: cut into row ranges under a budget
}
HANDLES = {"classic": ["classic"], "compact": ["compact"], "two_term_sizes": ["classic", "other"]}


def build_all(directory):
    """{name: (path, FileBits)}"""
    import os
    out = {}
    for name, (kind, k, H, sigs, docs, ps) in FILES.items():
        path = os.path.join(str(directory), "%s.cobs_%s" % (name, kind))
        out[name] = (path, build_file(path, kind, k, H, sigs, docs, ps))
    return out


def real_keys(fb, per_slot):
    import numpy as np
    return np.asarray(per_slot)[fb.doc_of_slot() >= 0]


class Family:
    """one search family on the checker's side: keys(files, f) of target file f at threshold 0, its denominator P(files, f),
    expected(files, t) in the device call's layout, and whether the family says "at least 1" """
    at_least_one = True
    limit = LIMIT32
    prefer_from = 0
    z = 0

    def smallest(self, files, f):
        return 1

    def __init__(self):
        self.src, self.other = sources()
        self.q = self.src[:Q_LEN]

    def labelings(self, files):
        return [labels_of(fb.num_docs, len(self.src) - fb.term_size + 1) for fb in files]

    def cases(self, files, f):
        return case_list(self.keys(files, f), self.P(files, f), self.at_least_one, self.prefer_from, self.limit,
                         self.smallest(files, f))


class Plain(Family):
    at_least_one = False
    prefer_from = 0.85          # fewer than 128 documents lie above: the top-k passes are cut by the threshold

    def keys(self, files, f):
        return real_keys(files[f], files[f].scores(self.q, self.z))

    def P(self, files, f):
        return files[f].positions(self.q, self.z)

    def expected(self, files, t):
        from tests import findere_check as F
        return F.results(files, self.q, self.z, t, 0)


class Findere(Plain):
    z = FINDERE_Z

    def __init__(self):
        Family.__init__(self)
        self.q = self.src[:FINDERE_LEN]


class PlainSkip(Plain):
    """an N in front of the query: T = 101 terms, V = 100 valid positions -- the bound is formed on the device"""
    at_least_one = True

    def __init__(self):
        Family.__init__(self)
        self.q = b"N" + self.src[:Q_LEN]

    def keys(self, files, f):
        from tests import invalid_check as I
        return real_keys(files[f], I.scores(files[f], self.q, 0))

    def P(self, files, f):
        from tests import invalid_check as I
        assert I.valid_positions(files[f], self.q, 0) == files[f].positions(self.q, 0) - 1
        return I.valid_positions(files[f], self.q, 0)

    def expected(self, files, t):
        from tests import invalid_check as I
        return I.results(files, self.q, 0, "skip", t, 0)


class Groups(Family):
    """group 0 = [Q, R], group 1 = [Q]; the group threshold moves, the read threshold stays"""
    limit = LIMIT64
    read_threshold = 0.5

    def __init__(self):
        Family.__init__(self)
        self.queries, self.offsets = [self.q, self.other, self.q], [0, 2, 3]

    def keys(self, files, f):
        from tests import groups_check as G
        sums, _votes, _P = G.totals(files, self.queries, self.offsets, 0, "error", self.read_threshold)
        return real_keys(files[f], sums[f][0])

    def P(self, files, f):
        return files[f].positions(self.q, 0) + files[f].positions(self.other, 0)

    def expected(self, files, t):
        from tests import groups_check as G
        return G.results(files, self.queries, self.offsets, 0, "error", t, self.read_threshold, 0)[0]


class GroupsRead(Groups):
    """the read threshold moves (votes), the group threshold is 0: every document comes back with its votes"""
    at_least_one = False
    limit = LIMIT32

    def keys(self, files, f):
        return real_keys(files[f], files[f].scores(self.q, 0))

    def P(self, files, f):
        return files[f].positions(self.q, 0)

    def expected(self, files, t):
        from tests import groups_check as G
        return G.results(files, self.queries, self.offsets, 0, "error", 0.0, t, 0)[0]


class Best(Family):
    def __init__(self):
        Family.__init__(self)
        self.queries, self.offsets = [self.q, self.other], [0, 2]

    def keys(self, files, f):
        from tests import best_check as B
        bs, bp, _bq, _bt = B.cells(files, self.queries, self.offsets, 0, "error")[f]
        assert (bp[0][files[f].doc_of_slot() >= 0] == self.P(files, f)).all()     # both members have P positions
        return real_keys(files[f], bs[0])

    def P(self, files, f):
        return files[f].positions(self.q, 0)

    def expected(self, files, t):
        from tests import best_check as B
        return B.results(files, self.queries, self.offsets, 0, "error", t, 0)


class Weighted(Family):
    def tabs(self, files):
        from tests import weighted_check as W
        key = tuple(id(fb) for fb in files)
        cache = self.__dict__.setdefault("_tabs", {})
        if key not in cache:
            cache[key] = (files, W.tables(files, self.q, 0))
        return cache[key][1]

    def keys(self, files, f):
        return real_keys(files[f], self.tabs(files)[f][1])

    def P(self, files, f):
        return self.tabs(files)[f][0]

    def expected(self, files, t):
        from tests import weighted_check as W
        return W.results_from(self.tabs(files), t, 0)


class Coverage(Family):
    def __init__(self):
        Family.__init__(self)
        self.q = self.src

    def smallest(self, files, f):
        return files[f].term_size

    def tabs(self, files):
        from tests import coverage_check as C
        return C.tables(files, self.q, 0)

    def keys(self, files, f):
        return real_keys(files[f], self.tabs(files)[f][1])

    def P(self, files, f):
        return len(self.q)

    def expected(self, files, t):
        from tests import coverage_check as C
        return C.results_from(self.tabs(files), t, 0)


class Window(Family):
    def tabs(self, files):
        from tests import window_check as B
        return B.tables(files, self.q, 0, WINDOW)

    def keys(self, files, f):
        return real_keys(files[f], self.tabs(files)[f][1])

    def P(self, files, f):
        assert self.tabs(files)[f][0] == WINDOW
        return WINDOW

    def expected(self, files, t):
        from tests import window_check as B
        return B.results_from(self.tabs(files), t, 0)


class Sets(Family):
    rank_by = "any"

    def keys(self, files, f):
        from tests import sets_check as S
        c = S.counts(files[f], self.q, 0, self.labelings(files)[f])
        return [v[0 if self.rank_by == "any" else 1] for v in c.values()]

    def P(self, files, f):
        return files[f].positions(self.q, 0)

    def expected(self, files, t):
        from tests import sets_check as S
        return S.results(files, self.labelings(files), self.q, 0, t, self.rank_by, 0)


class SetsAll(Sets):
    rank_by = "all"


class QuorumThreshold(Family):
    quorum = 1.0

    def keys(self, files, f):
        from tests import set_quorum_check as Q
        return [v[0] for v in Q.counts(files[f], self.q, 0, self.labelings(files)[f], self.quorum).values()]

    def P(self, files, f):
        return files[f].positions(self.q, 0)

    def expected(self, files, t):
        from tests import set_quorum_check as Q
        return Q.results(files, self.labelings(files), self.q, 0, self.quorum, t, 0)


class QuorumNeed(Family):
    """the quorum moves: need = max(1, ceil(quorum * members)) against the counts of set 0 (100 members); the threshold is
    0, so every set comes back with its core.  A quorum outside (0, 1] is refused by the call.  The query has 103 positions:
    its last ones are held by no member of set 0, so a count of 0 exists next to the count of 1."""

    def __init__(self):
        Family.__init__(self)
        self.q = self.src[:FINDERE_LEN]

    def keys(self, files, f):
        from tests import set_quorum_check as Q
        return Q.profile(files[f], self.q, 0, self.labelings(files)[f])[0].tolist()

    def P(self, files, f):
        from tests import set_quorum_check as Q
        assert Q.members(self.labelings(files)[f])[0] == SET0_MEMBERS
        return SET0_MEMBERS

    @staticmethod
    def refused(t):
        return not (t > 0.0 and t <= 1.0)

    def expected(self, files, t):
        from tests import set_quorum_check as Q
        return Q.results(files, self.labelings(files), self.q, 0, t, 0.0, 0)


FAMILIES = {
    "plain": Plain, "plain_skip": PlainSkip, "findere": Findere, "groups": Groups, "groups_read": GroupsRead, "best": Best,
    "weighted": Weighted, "sets_any": Sets, "sets_all": SetsAll, "quorum_threshold": QuorumThreshold,
    "quorum_need": QuorumNeed, "coverage": Coverage, "window": Window,
}
