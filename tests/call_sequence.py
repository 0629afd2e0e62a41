"""The call-sequence plan (test infrastructure, no GPU in it): ONE handle lives through a long deterministic sequence of
calls of every family that shares the scratch workspace (scratch_batch(ix, 0), set_queries_on, the captured graphs, the
flag words, the pools, the label caches), and after every step the result is compared exactly with the checkers.

The order of the families is an Eulerian circuit of the complete directed graph on them, self-loops included: every
ordered pair (A directly followed by B, A by A) occurs.  Into the circuit go the failure steps: for every failure kind and
every family F one failing call of ANOTHER family is put behind an occurrence of F and followed by a regular step of F
(the circuit's pairs stay as they are: ... F, failing X, F, next ...).  Between the steps findere z, the invalid-bases
policy, pass_bytes, graph, the query count and the query lengths change on a seeded schedule (COBS_FUZZ_SEED shifts it) in
which every family meets every value; the labels of the document sets go through five states in time order.

build_plan() gives the steps; Expect(files) turns a step into its expected value -- plain lists and tuples of ints, in the
same form tests/test_gpu_call_sequence.py brings the library's answers into -- from the suite's own checkers, computed
once per (queries, z, policy, labels, parameters)."""
import collections
import os

import numpy as np

from tests import coverage_check as G
from tests import fill_check as FC
from tests import findere_check as F
from tests import groups_check as GR
from tests import invalid_check as I
from tests import positions_check as P
from tests import prevalence_check as V
from tests import set_quorum_check as Q
from tests import sets_check as S
from tests import weighted_check as W
from tests import window_check as B

FAMILIES = ("search_small", "search_large", "counts", "view", "positions", "prevalence", "weighted", "coverage", "sets",
            "quorum", "set_prevalence", "groups", "doc_bits", "own_batch", "window", "window_positions", "adjusted")
SET_FAMILIES = ("sets", "quorum", "set_prevalence")
KINDS = ("invalid_base", "too_short", "overflow")              # the failure steps
CAN_FAIL = {
    "invalid_base": tuple(f for f in FAMILIES if f != "doc_bits"),
    "too_short": tuple(f for f in FAMILIES if f != "doc_bits"),
    "overflow": ("search_small", "search_large", "view", "groups", "sets", "coverage", "weighted", "window"),
}
K_MAX = 31                                                     # the largest term size of the handles the plan is walked on
ZS = (0, 3)
POLICIES = ("error", "miss", "skip")
PASS_SMALL = 30000                                             # with the MANY batch: at least 3 device passes (see many_batch)
PASS_BYTES = (0, PASS_SMALL)
GRAPHS = (-1, 0)                                               # automatic | off
SEARCHES = ((0.0, 0), (0.5, 0), (0.0, 3), (0.5, 3))
QUORUMS = (0.5, 0.95, 1.0)
WINDOWS = (7, 64, 300, 4095)                                   # one per plane count of the window scan (6, 8, 10, 12)
WINDOW_FAMILIES = ("window", "window_positions")
NQS = (1, 2, 16, 17, 24)
NQS_SMALL = (1, 2, 16)
LABEL_STATES = ("initial", "relabel1", "relabel2", "cleared", "again")
HIT_CAP_SMALL = 8
OVERFLOW_T = 0.3

Step = collections.namedtuple("Step", "index family prev kind after z policy labels pass_bytes graph queries params")
# kind: "regular" or one of KINDS; after: the kind of the failure step directly before this one, or None;
# labels: the label state in force; params: a dict of what the family's call takes besides the queries


def fuzz_seed():
    return int(os.environ.get("COBS_FUZZ_SEED", "0"))


# ---- the order ------------------------------------------------------------------------------------------------------------

def euler_circuit(n, rng):
    """vertex sequence (n * n + 1 entries) of an Eulerian circuit of the complete directed graph on n vertices with self-loops
    (Hierholzer; the order in which a vertex's edges are taken is drawn from rng)"""
    out_edges = [list(rng.permutation(n)) for _ in range(n)]
    start = int(rng.integers(n))
    stack, circuit = [start], []
    while stack:
        v = stack[-1]
        if out_edges[v]:
            stack.append(int(out_edges[v].pop()))
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    assert len(circuit) == n * n + 1 and circuit[0] == circuit[-1]
    return circuit


def _setting_rows():
    """14 rows (z, policy, pass_bytes, graph): the rows 0..5 hold every (z, policy) at pass_bytes 0, 6..11 at the small one;
    graph is off in four rows that cover both z and both pass_bytes"""
    rows = []
    for r in range(14):
        rows.append((ZS[r % 2], POLICIES[(r // 2) % 3], PASS_BYTES[1 if 6 <= r < 12 else 0], GRAPHS[1 if r in (3, 8, 12, 13) else 0]))
    return rows


# the window of a window step follows its setting row: every W meets both z, both pass_bytes and all three policies in the
# family's first 14 regular steps, whatever the seed (W 7: the rows 0, 3, 10, 13; 64: 1, 5, 8; 300: 4, 6, 9; 4095: 2, 7, 11, 12)
_WINDOW_OF_ROW = (0, 1, 3, 0, 2, 1, 2, 3, 1, 2, 0, 3, 3, 0)


def _window(row, j):
    """the W of the j-th step of a window family under setting row `row`; the second turn through the rows shifts it"""
    return WINDOWS[(_WINDOW_OF_ROW[row] + 2 * (j // len(_WINDOW_OF_ROW))) % len(WINDOWS)]


# ---- the labels -----------------------------------------------------------------------------------------------------------

def labelings(state, files):
    """per file the labels (int64 [num_docs], -1: in no set) or None, for one of LABEL_STATES.  Few sets per file: the
    cells of set_prevalence for the longest query stay below PASS_SMALL.  With two files only the second is labelled at
    first; the first relabelling labels the first too."""
    out = []
    for fi, fb in enumerate(files):
        d = np.arange(fb.num_docs, dtype=np.int64)
        if state == "initial":
            lab = None if (len(files) > 1 and fi == 0) else np.where(d % 7 == 0, -1, d % 3)
        elif state == "relabel1":
            lab = d * 4 // max(fb.num_docs, 1)                          # four runs of documents
        elif state == "relabel2":
            lab = np.where(d % 5 == 3, -1, (d // 2) % 4)
            lab[lab == 2] = -1                                          # set 2 has no member
            if fb.num_docs > 9:
                lab[9] = 2                                              # ... but one: a one-member set (any = all)
        elif state == "cleared":
            lab = None
        else:
            assert state == "again"
            lab = np.where(d % 11 == 1, -1, (d * 5 + fi) % 3)
        out.append(lab)
    return out


# ---- the queries ----------------------------------------------------------------------------------------------------------

def _source():
    from tests.test_gpu_weighted import SRC
    return SRC


def _cut(src, rng, ln):
    o = int(rng.integers(0, len(src) - ln))
    return src[o:o + ln]


def make_batch(rng, nq, z, has_long, with_n, many=False):
    """nq queries cut from the source: reads of K_MAX + z .. 150 characters (8-bit scores; the first is the shortest
    allowed), with has_long one query of 300 .. 700 positions (16-bit scores) in the last place; with_n: an N in the middle
    of query 1 (query 0 of a batch of one) and at the end of the last read.  many: the batch of the small pass_bytes: 24
    queries, reads of 120 .. 150 characters and two long queries -- more than 4500 characters, at 16 bytes of K1's table per
    character (four sub-indexes, one hash function, the narrow table: the least of the handles) more than 2 * PASS_SMALL"""
    src = _source()
    k = K_MAX
    qs = []
    for i in range(nq):
        if many:
            ln = int(rng.integers(120, 151))
        else:
            ln = k + z if i == 0 else int(rng.integers(k + z, 151))
        qs.append(_cut(src, rng, ln))
    longs = ([nq - 1, nq // 2] if many else [nq - 1]) if has_long else []
    for i in longs:
        qs[i] = _cut(src, rng, int(rng.integers(500 if many else 300, 601 if many else 701)) + k - 1 + z)
    if with_n:
        i = 1 if nq > 1 else 0
        qs[i] = I.with_n(qs[i], [len(qs[i]) // 2])
        j = nq - 2 if nq > 2 else None
        if j is not None and j != i:
            qs[j] = I.with_n(qs[j], [len(qs[j]) - 1])
    return tuple(bytes(q) for q in qs)


def _group_offsets(nq, shape):
    if shape == "all":
        return (0, nq)
    if shape == "ones":
        return tuple(range(nq + 1))
    offs = list(range(0, nq, 2)) + [nq]                                  # groups of two (the last may hold one)
    return tuple(offs)


# ---- the handles ----------------------------------------------------------------------------------------------------------

HANDLES = ("compact16", "two_files", "two_files_idx64")


def build_files(directory, handle):
    """write the index files of one handle -> (paths, [FileBits]): compact16 = page size 16, signature sizes 1, 2, 65 and
    4097, the last sub-index partly filled, one hash function, k = 31; two_files = a classic file of 129 documents, 2003
    rows, three hash functions and k = 20 in front of it (different term sizes in one handle)"""
    from tests.test_gpu_weighted import _classic, _compact
    sigs, page_size = [1, 2, 65, 4097], 16
    num_docs = len(sigs) * 8 * page_size - 5 * page_size - 3
    pc, fc = _compact(os.path.join(str(directory), "s.cobs_compact"), num_docs, page_size, sigs, 1, K_MAX, page_size)
    if handle == "compact16":
        return [pc], [fc]
    assert handle in HANDLES
    pa, fa = _classic(os.path.join(str(directory), "s.cobs_classic"), 129, 2003, 3, 20, 129)
    return [pa, pc], [fa, fc]


# ---- the plan -------------------------------------------------------------------------------------------------------------

def _with_failure_steps(circuit):
    """the circuit with the failure steps put in -> [[family, kind, after]]: for every kind and every family F, behind one
    occurrence of F: [a failing call (its family chosen later: None), a regular step of F]"""
    n = len(FAMILIES)
    occ = collections.defaultdict(list)
    for pos, v in enumerate(circuit[:-1]):                              # (the last entry closes the circuit)
        occ[v].append(pos)
    insert_after = {}
    for ki, kind in enumerate(KINDS):
        for v in range(n):
            insert_after[occ[v][(2 + 4 * ki + v) % len(occ[v])]] = kind      # three different occurrences of every family
    seq = []
    for pos, v in enumerate(circuit):
        seq.append([FAMILIES[v], "regular", None])
        if pos in insert_after:
            seq.append([None, insert_after[pos], None])
            seq.append([FAMILIES[v], "regular", insert_after[pos]])
    return seq


def _label_states(seq):
    """the label state of every step, in time order: a state lasts at least `span` steps and until every set family had a
    regular step in it (the last state takes what is left); the longest span with which all five states get theirs"""
    for span in range(len(seq) // len(LABEL_STATES), 0, -1):
        states, state, since, seen = [], 0, 0, set()
        for fam, kind, _after in seq:
            states.append(LABEL_STATES[state])
            since += 1
            if fam in SET_FAMILIES and kind == "regular":
                seen.add(fam)
            if state < len(LABEL_STATES) - 1 and since >= span and len(seen) == len(SET_FAMILIES):
                state, since, seen = state + 1, 0, set()
        if state == len(LABEL_STATES) - 1 and len(seen) == len(SET_FAMILIES):
            return states
    raise AssertionError("no place for the five label states")


def _choose_failing_families(seq, states):
    """the family of every failure step: the one that failed least so far among those that can fail this way, never the
    family that follows it, and no set family while no file is labelled (such a call has no work item)"""
    turn = collections.Counter()
    for i, (fam, kind, _after) in enumerate(seq):
        if fam is not None:
            continue
        able = [f for f in CAN_FAIL[kind] if f != seq[i + 1][0] and not (f in SET_FAMILIES and states[i] == "cleared")]
        seq[i][0] = min(able, key=lambda f: (turn[kind, f], CAN_FAIL[kind].index(f)))
        turn[kind, seq[i][0]] += 1


def _query_count(fam, kind, j, many):
    """search_large always sends 24 queries -- above the 16 of a captured graph: the pipelined passes --, its failure
    steps included; counts and adjusted take one query; the overflow step of every other family sends 16"""
    if fam == "search_large":
        return 24
    if fam in ("counts", "adjusted"):
        return 1
    if kind == "overflow":
        return 16
    if fam == "search_small":
        return 16 if many else NQS_SMALL[j % 3]
    return 24 if many else NQS[(j + FAMILIES.index(fam)) % len(NQS)]


def _step_queries(rng, fam, kind, j, z, policy, many, params):
    """the queries of one step; a failure step of the kinds invalid_base and too_short gets its bad query (params["bad"])"""
    nq = _query_count(fam, kind, j, many)
    has_long = bool(many or rng.integers(2))
    with_n = policy != "error" and bool(rng.integers(3))
    if fam == "adjusted" and policy == "skip":
        with_n = True                                                   # P is the count of the valid positions, not T - z
    if kind == "overflow":
        has_long, with_n = False, False
    queries = list(make_batch(rng, nq, z, has_long, with_n, many=many and nq == 24))
    if kind == "invalid_base":
        bad = nq - 1 if nq > 1 else 0                                   # query i > 0 holds the N (counts has one query)
        queries[bad] = I.with_n(queries[bad], [len(queries[bad]) // 3])
        params["bad"] = bad
    elif kind == "too_short":
        bad = nq // 2
        queries[bad] = queries[bad][:K_MAX + z - 1]
        params["bad"] = bad
    return tuple(queries)


def _family_params(fam, kind, i, j, nq, row, params):
    """what the family's call takes besides the queries (own_batch: see _own_batch_step); row: the step's setting row"""
    overflow = kind == "overflow"
    t, lim = (OVERFLOW_T, 0) if overflow else SEARCHES[(j + i) % 4]
    if fam in ("search_small", "search_large", "view", "weighted", "coverage", "adjusted"):
        params.update(t=t, lim=lim)
    elif fam == "window":
        params.update(W=_window(row, j), t=t, lim=lim)
    elif fam == "window_positions":
        params.update(W=_window(row, j))
    elif fam == "sets":
        params.update(t=0.0 if overflow else (0.0, 0.3)[j % 2], rank_by=("any", "all")[(j // 2) % 2],
                      lim=0 if overflow else (0, 2)[(j // 4) % 2])
    elif fam == "quorum":
        params.update(quorum=QUORUMS[j % 3], t=(0.0, 0.3)[(j // 3) % 2], lim=(0, 2)[(j // 6) % 2])
    elif fam == "groups":
        params.update(offsets=_group_offsets(nq, ("ones", "twos", "all")[j % 3]), t=t, rt=0.8, lim=lim)


def _own_batch_step(own, kind, j, queries, z, policy, params):
    """the long-lived Batch: run_topk, read it again, run(0.0), read it again, ...; `own` = the last run (what, params,
    queries, z, policy) or None -> (own, queries).  A failed run leaves nothing to read again."""
    if kind != "regular":
        params.update(what="topk", t=0.0, k=3)
        return None, queries
    what = "topk" if own is None else {"topk": "reread", "reread_topk": "counts", "counts": "reread", "reread_counts": "topk"}[own[0]]
    if what == "topk":
        params.update(what="topk", t=(0.0, 0.5)[j % 2], k=(3, 5)[(j // 2) % 2])
        return ("topk", dict(params), queries, z, policy), queries
    if what == "counts":
        params.update(what="counts")
        return ("counts", dict(params), queries, z, policy), queries
    # read the earlier run again: ITS queries and settings
    params.update(own[1], what="reread", of=own[1]["what"], run_z=own[3], run_policy=own[4])
    return ("reread_" + own[1]["what"],) + own[1:], own[2]


def build_plan(seed=None):
    """-> list of Step.  Deterministic: the same seed gives the same plan."""
    seed = fuzz_seed() if seed is None else seed
    rng = np.random.default_rng(20261019 + 100003 * seed)
    seq = _with_failure_steps(euler_circuit(len(FAMILIES), rng))
    states = _label_states(seq)
    _choose_failing_families(seq, states)
    # the settings: per family a seeded permutation of the 14 rows, taken by the family's regular occurrences in turn
    rows = _setting_rows()
    perm = {f: [int(j) for j in rng.permutation(len(rows))] for f in FAMILIES}
    count = collections.Counter()
    steps, own, prev = [], None, None
    for i, (fam, kind, after) in enumerate(seq):
        j = count[fam]
        row = perm[fam][j % len(rows)]
        z, policy, pass_bytes, graph = rows[row]
        if kind == "regular":
            count[fam] += 1
        else:
            pass_bytes = 0
            if kind == "invalid_base":
                policy = "error"
        params = {}
        queries = _step_queries(rng, fam, kind, j, z, policy, pass_bytes != 0, params)
        _family_params(fam, kind, i, j, len(queries), row, params)
        if fam == "own_batch":
            own, queries = _own_batch_step(own, kind, j, queries, z, policy, params)
        steps.append(Step(i, fam, prev, kind, after, z, policy, states[i], pass_bytes, graph, queries, params))
        prev = fam
    return steps


# ---- the device passes ----------------------------------------------------------------------------------------------------

PASS_READERS = {"positions": "positions_ms", "prevalence": "prevalence_ms", "weighted": "weighted_ms", "coverage": "coverage_ms",
                "sets": "sets_ms", "quorum": "set_quorum_ms", "set_prevalence": "set_quorum_ms", "window": "window_ms",
                "window_positions": "positions_ms"}


def needs_three_passes(st, expect):
    """must the step's call take at least 3 device passes (read off the family's *_ms reader)?  The small pass_bytes with
    the 24-query batch (make_batch: more than 2 * PASS_SMALL bytes of K1's table); hit_positions only looks up the queries
    that have a hit (window_positions: a window hit), and a set search without a labelled file has no work item; a
    window search at threshold 0 adds its pool's bytes to the estimate: more passes, never fewer"""
    if st.kind != "regular" or st.family not in PASS_READERS or not st.pass_bytes or len(st.queries) != 24:
        return False
    if st.family in ("positions", "window_positions"):
        return all(len(hits) > 0 for hits in expect.value(st)[0])
    if st.family in SET_FAMILIES:
        return any(lab is not None for lab in expect.labels(st.labels))
    return True


# ---- the expected values --------------------------------------------------------------------------------------------------

def _lists(offs, rows):
    rows = [tuple(int(x) for x in r) for r in rows]
    return [rows[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


class Expect:
    """the expected value of a step on a handle over `files` (findere_check.FileBits, in the handle's file order)"""

    def __init__(self, files):
        self.files = list(files)
        self._cache = {}
        self._packed = {}                                               # file -> the packed positions of the last query asked about
        self._labels = {s: labelings(s, self.files) for s in LABEL_STATES}

    def labels(self, state):
        return self._labels[state]

    def _memo(self, key, fn):
        if key not in self._cache:
            self._cache[key] = fn()
        return self._cache[key]

    def search(self, queries, z, policy, t, lim):
        def one(q):
            if policy == "error":
                return F.results(self.files, q, z, t, lim)
            return I.results(self.files, q, z, policy, t, lim)
        return self._memo(("search", queries, z, policy, t, lim), lambda: [one(q) for q in queries])

    def counts(self, q, z, policy):
        fn = F.counts if policy == "error" else I.counts
        return self._memo(("counts", q, z, policy), lambda: [int(x) for x in fn(self.files, q, z)])

    def slot_of(self, f):
        """{document: score slot} of file f (FileBits.doc_of_slot, inverted; padding slots have no document)"""
        return self._memo(("slot_of", f), lambda: {int(doc): s for s, doc in enumerate(self.files[f].doc_of_slot()) if doc >= 0})

    def position_words(self, q, z, policy, f, d):
        """positions_check.pack(positions_check.positions(files, q, z, f, d, policy)) as a list of ints.  The hits of a
        query come one after the other, so the columns of all slots of (query, file) are packed at once and kept until
        the next query (tests/test_call_sequence_cpu.py holds this against the checker's own two calls)"""
        key = (q, z, policy)
        if self._packed.get(f, (None,))[0] != key:
            fb = self.files[f]
            cols = V.windows(fb, q, z, policy)                          # bool [n, slots]: what positions() takes its column from
            win = np.zeros((fb.slots, (cols.shape[0] + 63) // 64 * 64), dtype=np.uint8)
            win[:, :cols.shape[0]] = cols.T
            words = np.packbits(win, axis=1, bitorder="little").view("<u8")         # [slots, words]; bits >= n zero
            self._packed[f] = (key, words)
        return self._packed[f][1][self.slot_of(f)[d]].tolist()

    def window_tables(self, q, z, W, policy):
        """window_check.tables of one query: per file (w, best of every slot, document of every slot, plain scores)"""
        return self._memo(("window", q, z, W, policy), lambda: B.tables(self.files, q, z, W, policy))

    def window(self, queries, z, policy, W, t, lim):
        return [B.results_from(self.window_tables(q, z, W, policy), t, lim) for q in queries]

    def valid_positions(self, q, z, policy, f):
        """the positions of q that a search of file f scores: T - z, under `skip` those whose k + z characters hold no N"""
        span = self.files[f].term_size + z
        n = len(q) - span + 1
        if policy != "skip":
            return n
        return sum(1 for p in range(n) if all(c in b"ACGT" for c in q[p:p + span]))

    def adjusted_floats(self, st):
        """[(expected_fp, adjusted)] of the results of an `adjusted` step, in result order: fill_check.adjust over the
        document's set bits and the signature size of its sub-index (compared with a tolerance, apart from value())"""
        q, z, pol = st.queries[0], st.z, st.policy
        out = []
        for (f, d, score) in self.search((q,), z, pol, st.params["t"], st.params["lim"])[0]:
            fb = self.files[f]
            bits = self._memo(("bits", f), lambda: FC.bits_of_mats(fb.mats))
            sigs = self._memo(("sigs", f), lambda: np.repeat([m.shape[0] for m in fb.mats], [m.shape[1] * 8 for m in fb.mats]))
            P = self._memo(("valid", q, z, pol, f), lambda: self.valid_positions(q, z, pol, f))
            slot = self.slot_of(f)[d]                                   # (bits and sigs are in slot order)
            a = FC.adjust(score, P, int(bits[slot]), int(sigs[slot]), fb.num_hashes, z)
            out.append((a["expected_fp"], a["adjusted"]))
        return out

    def value(self, st):
        """the expected value of a regular (or overflow) step"""
        fam, qs, p = st.family, st.queries, st.params
        z, pol = st.z, st.policy
        key = (fam, qs, z, pol, st.labels if fam in SET_FAMILIES else None, tuple(sorted((k, str(v)) for k, v in p.items())))
        return self._memo(key, lambda: self._value(st, fam, qs, p, z, pol))

    def _value(self, st, fam, qs, p, z, pol):
        files = self.files
        if fam in ("search_small", "search_large", "view"):
            return self.search(qs, z, pol, p["t"], p["lim"])
        if fam == "counts":
            return self.counts(qs[0], z, pol)
        if fam == "positions":
            hits = self.search(qs, z, pol, 0.5, 0)
            return (hits, [[self.position_words(q, z, pol, f, d) for (f, d, _sc) in hs] for q, hs in zip(qs, hits)])
        if fam == "prevalence":
            offs, counts = V.segments(files, list(qs), z, pol)
            return (offs.tolist(), counts.tolist())
        if fam == "weighted":
            tabs = [W.tables(files, q, z, pol) for q in qs]
            return ([W.results_from(tab, p["t"], p["lim"]) for tab in tabs], [[int(t[0]) for t in tab] for tab in tabs])
        if fam == "coverage":
            return [G.results(files, q, z, p["t"], p["lim"], pol) for q in qs]
        if fam == "window":
            return self.window(qs, z, pol, p["W"], p["t"], p["lim"])
        if fam == "window_positions":
            hits = self.window(qs, z, pol, p["W"], 0.5, 0)
            return (hits, [[self.position_words(q, z, pol, f, d) for (f, d, _sc) in hs] for q, hs in zip(qs, hits)])
        if fam == "adjusted":                                           # (document, score); the floats: adjusted_floats
            return [(d, sc) for (_f, d, sc) in self.search(qs, z, pol, p["t"], p["lim"])[0]]
        labs = self.labels(st.labels)
        if fam == "sets":
            offs, rows = S.arrays(files, labs, list(qs), z, p["t"], p["rank_by"], p["lim"], pol)
            return _lists(offs, rows.tolist())
        if fam == "quorum":
            offs, rows = Q.arrays(files, labs, list(qs), z, p["quorum"], p["t"], p["lim"], pol)
            return _lists(offs, rows.tolist())
        if fam == "set_prevalence":
            offs, counts = Q.segments(files, labs, list(qs), z, pol)
            return (offs.tolist(), counts.tolist())
        if fam == "groups":
            lists, P = GR.results(files, list(qs), list(p["offsets"]), z, pol, p["t"], p["rt"], p["lim"])
            return (lists, [[int(x) for x in row] for row in P])
        if fam == "doc_bits":
            return [[int(x) for x in FC.bits_of_mats(fb.mats)] for fb in files]
        assert fam == "own_batch"
        rz, rpol = (p["run_z"], p["run_policy"]) if p["what"] == "reread" else (z, pol)
        what = p["of"] if p["what"] == "reread" else p["what"]
        if what == "topk":
            return self.search(qs, rz, rpol, p["t"], p["k"])
        return [self.counts(q, rz, rpol) for q in qs]

    def nonempty(self, st):
        """does the step's expected value hold anything (a hit, a count above 0)?"""
        def any_in(v):
            if isinstance(v, (list, tuple)):
                return any(any_in(x) for x in v)
            return bool(v)
        v = self.value(st)
        if st.family in ("prevalence", "set_prevalence"):
            return any_in(v[1])
        if st.family in ("weighted", "groups", "positions", "window_positions"):
            return any_in(v[0])
        return any_in(v)


def describe(st):
    """one line for an assertion message: the pair and the settings in force"""
    return ("step %d: %s -> %s [%s%s] z=%d policy=%s labels=%s pass_bytes=%d graph=%d nq=%d lens=%s params=%s" % (
        st.index, st.prev, st.family, st.kind, (", after a failed " + st.after) if st.after else "", st.z, st.policy, st.labels,
        st.pass_bytes, st.graph, len(st.queries), [len(q) for q in st.queries][:6], {k: v for k, v in st.params.items() if k != "offsets"}))
