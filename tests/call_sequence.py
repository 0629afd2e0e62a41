"""The call-sequence plan (test infrastructure, no GPU in it): ONE handle lives through a long deterministic sequence of
calls of every family that shares the scratch workspace (scratch_batch(ix, 0), set_queries_on, the captured graphs, the
flag words, the pools, the label caches), and after every step the result is compared exactly with the checkers.

The order of the families is an Eulerian circuit of the complete directed graph on them, self-loops included: every
ordered pair (A directly followed by B, A by A) occurs.  Into the circuit go the failure steps: for every failure kind and
every family F one failing call of ANOTHER family is put behind an occurrence of F and followed by a regular step of F
(the circuit's pairs stay as they are: ... F, failing X, F, next ...).  Between the steps findere z, the invalid-bases
policy, pass_bytes, graph, the query count and the query lengths change on a seeded schedule (COBS_FUZZ_SEED shifts it) in
which every family meets every value; the labels of the document sets go through five states in time order.  The
self-hashing scan (tuning key scan_self_hash: 0 or 2) is one of those settings: must_self_hash / never_self_hash say for
which steps the handle's self_hash_passes counter has to grow and for which it must not.

build_plan() gives the steps; Expect(files) turns a step into its expected value -- plain lists and tuples of ints, in the
same form tests/test_gpu_call_sequence.py brings the library's answers into -- from the suite's own checkers, computed
once per (queries, z, policy, labels, parameters)."""
import collections
import os

import numpy as np

from tests import best_check as BC
from tests import coverage_check as G
from tests import fill_check as FC
from tests import findere_check as F
from tests import groups_check as GR
from tests import invalid_check as I
from tests import positions_check as P
from tests import prevalence_check as V
from tests import set_quorum_check as Q
from tests import sets_check as S
from tests import similarity_check as SC
from tests import weighted_check as W
from tests import window_check as B

FAMILIES = ("search_small", "search_large", "counts", "view", "positions", "prevalence", "weighted", "coverage", "sets",
            "quorum", "set_prevalence", "groups", "doc_bits", "own_batch", "window", "window_positions", "adjusted", "best",
            "similarity")
NO_QUERIES = ("doc_bits", "similarity")                        # families whose call takes no query: they cannot fail
SET_FAMILIES = ("sets", "quorum", "set_prevalence")
KINDS = ("invalid_base", "too_short", "overflow")              # the failure steps
CAN_FAIL = {
    "invalid_base": tuple(f for f in FAMILIES if f not in NO_QUERIES),
    "too_short": tuple(f for f in FAMILIES if f not in NO_QUERIES),
    # (best.cpp caps its selection pool by hit_cap and selects again into a grown pool, as groups.cpp does)
    "overflow": ("search_small", "search_large", "view", "groups", "sets", "coverage", "weighted", "window", "best"),
}
K_MAX = 31                                                     # the largest term size of the handles the plan is walked on
ZS = (0, 3)
POLICIES = ("error", "miss", "skip")
PASS_SMALL = 30000                                             # with the MANY batch: at least 3 device passes (see many_batch)
PASS_BYTES = (0, PASS_SMALL)
GRAPHS = (-1, 0)                                               # automatic | off
SELF_HASH = (0, 2)                                             # scan_self_hash: never | wherever the shape allows
SEARCHES = ((0.0, 0), (0.5, 0), (0.0, 3), (0.5, 3))
QUORUMS = (0.5, 0.95, 1.0)
WINDOWS = (7, 64, 300, 4095)                                   # one per plane count of the window scan (6, 8, 10, 12)
WINDOW_FAMILIES = ("window", "window_positions")
NQS = (1, 2, 16, 17, 24)
NQS_SMALL = (1, 2, 16)
LABEL_STATES = ("initial", "relabel1", "relabel2", "cleared", "again")
HIT_CAP_SMALL = 8
OVERFLOW_T = 0.3
SIMILARITY_REFS = (1, 8, 9, 17)                                # one reference, a full panel of 8, a panel and one, two and one
# the self-hashing scan (kernels.hpp: scan_self_hash_fits): its LDS array holds 2048 + 64 row indices, (sub-indexes a tile
# lies in) x (8-term blocks of the pass's longest query + 1) x 8 are needed
SELF_HASH_ENTRIES = 2048 + 64
# the families whose passes go through run_impl (no K1 of their own); own_batch: when it runs `counts`
RUN_IMPL_FAMILIES = ("search_small", "search_large", "counts", "view", "groups", "best", "adjusted", "own_batch")
SEARCH_FAMILIES = ("search_small", "search_large", "view", "adjusted")      # ... with the caller's threshold and limit
OWN_K1_FAMILIES = ("positions", "prevalence", "weighted", "coverage", "window", "window_positions", "sets", "quorum",
                   "set_prevalence")
LONG_MAX = 700                                                 # positions of the longest query there is
LONG_FITS = 520                                                # ... of the longest that still fits compact16's LDS array

Step = collections.namedtuple("Step", "index family prev kind after z policy labels pass_bytes graph self_hash queries params")
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
    """14 rows (z, policy, pass_bytes, graph, scan_self_hash): the rows 0..5 hold every (z, policy) at pass_bytes 0, 6..11
    at the small one; graph is off in four rows that cover both z and both pass_bytes.  The self-hashing scan is on in
    the rows 0, 2 and 4 -- z = 0 and pass_bytes = 0 under each policy: the rows of the `must` steps (MUST_ROWS) --, in 1 (z =
    3: it has to stay on the table), in 6 and 10 (cut calls at z = 0) and in 9; row 12 is row 0's shape with the switch at 0"""
    rows = []
    for r in range(14):
        rows.append((ZS[r % 2], POLICIES[(r // 2) % 3], PASS_BYTES[1 if 6 <= r < 12 else 0], GRAPHS[1 if r in (3, 8, 12, 13) else 0],
                     SELF_HASH[1 if r in (0, 1, 2, 4, 6, 9, 10) else 0]))
    return rows


MUST_ROWS = {"error": 0, "miss": 2, "skip": 4}                 # z = 0, pass_bytes = 0, the switch at 2
TABLE_ROW = 12                                                 # z = 0, pass_bytes = 0, `error`, the switch at 0


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


def make_batch(rng, nq, z, has_long, with_n, many=False, long_max=LONG_MAX):
    """nq queries cut from the source: reads of K_MAX + z .. 150 characters (8-bit scores; the first is the shortest
    allowed), with has_long one query of 300 .. long_max positions (16-bit scores) in the last place; with_n: an N in the middle
    of query 1 (query 0 of a batch of one) and at the end of the last read.  many: the batch of the small pass_bytes: 24
    queries, reads of 120 .. 150 characters and two long queries -- more than 4500 characters, at 16 bytes of K1's table per
    character (four sub-indexes, one hash function, the narrow table: the least of the handles) more than 2 * PASS_SMALL"""
    src = _source()
    k = K_MAX
    qs = []
    for i in range(nq):
        if many:
            ln = int(rng.integers(120, 151))
            if with_n and i == 1:
                # the read with the N in its middle is the longest there is: the N takes k + z positions out of it, and on
                # either side of them enough stay for a window of 64 to reach half its width (a window hit for every query
                # of the batch: hit_positions then looks all of them up, and the pass count of the step is known)
                ln = 150
        else:
            ln = k + z if i == 0 else int(rng.integers(k + z, 151))
        qs.append(_cut(src, rng, ln))
    longs = ([nq - 1, nq // 2] if many else [nq - 1]) if has_long else []
    for i in longs:
        qs[i] = _cut(src, rng, int(rng.integers(500 if many else 300, 601 if many else long_max + 1)) + k - 1 + z)
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
    if kind == "invalid_base" and fam in ("groups", "best"):
        return 24                                                       # the bad query, the last, lies above index 16
    if fam == "search_small":
        return 16 if many else NQS_SMALL[j % 3]
    return 24 if many else NQS[(j + FAMILIES.index(fam)) % len(NQS)]


def _step_queries(rng, fam, kind, j, z, policy, many, params, row=None):
    """the queries of one step; a failure step of the kinds invalid_base and too_short gets its bad query (params["bad"]).
    Under the rows of the `must` steps the lengths are set, not drawn: `error` holds a 16-bit query that still fits the
    self-hashing scan's LDS array on compact16, `miss` holds 8-bit queries only, `skip` holds an N and no query beyond
    the array"""
    nq = _query_count(fam, kind, j, many)
    has_long = bool(many or rng.integers(2))
    with_n = policy != "error" and bool(rng.integers(3))
    long_max = LONG_MAX
    if row in MUST_ROWS.values():
        long_max = LONG_FITS
        has_long = {MUST_ROWS["error"]: True, MUST_ROWS["miss"]: False}.get(row, has_long)
        with_n = with_n or (row == MUST_ROWS["skip"] and policy == "skip")      # (a failing step under `error` keeps its one N)
    if fam == "adjusted" and policy == "skip":
        with_n = True                                                   # P is the count of the valid positions, not T - z
    if kind == "overflow":
        has_long, with_n = False, False
    queries = list(make_batch(rng, nq, z, has_long, with_n, many=many and nq == 24, long_max=long_max))
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
    if not overflow and fam in SEARCH_FAMILIES and row in (MUST_ROWS["error"], MUST_ROWS["miss"]):
        t, lim = SEARCHES[(j + i) % 2]                                  # no limit: a top-k pass keeps K1's table
        if fam == "view" and j >= len(_WINDOW_OF_ROW):
            # ... but for the view call's second visit of its first row (build_plan: row 0, `error`, graph on): the top-k
            # search at z = 0 and pass_bytes 0 with the switch at 2, which has to stay on the table
            t, lim = SEARCHES[2 + (j + i) % 2]
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
        # (the read threshold is the threshold of the pass: under `skip` a positive one takes K1's valid positions)
        params.update(offsets=_group_offsets(nq, ("ones", "twos", "all")[j % 3]), t=t, rt=0.0 if row == MUST_ROWS["skip"] else 0.8, lim=lim)
    elif fam == "best":
        params.update(offsets=_group_offsets(nq, ("ones", "twos", "all")[j % 3]), t=t, lim=lim)
    elif fam == "similarity":
        # 1, 8, 9, 17 references: the first document of the first sub-index and the last of the last, partly filled one
        # (one reference: one of the two in turn), the others drawn from the sub-index of `side` -- panels of 7, 8 and 16
        # of one sub-index beside one of the other; of 8, 9 and 17 where the file has one sub-index; n = 9 repeats one
        n = SIMILARITY_REFS[j % 4]
        params.update(n=n, side=("first", "last")[(j // 4) % 2], picks=tuple(int(x) for x in np.random.default_rng(1000 * i + j).integers(0, 1 << 30, n)),
                      repeat=n == 9)


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


def _graph_form_steps(seq):
    """{position: scan_self_hash} of the search_small steps that hold ONE batch at z = 0, `error`, pass_bytes 0 and graph on
    with the switch at one value right after the other: a graph captured in one form must not be replayed in the other.
    The circuit has search_small directly behind search_small once (every ordered pair occurs once): there the switch goes
    0 -> 2.  The other order, 2 -> 0, is the pair around the too_short failure behind search_small: that call is refused on
    the host, nothing is launched between the two."""
    small = [i for i, (fam, kind, _a) in enumerate(seq) if fam == "search_small" and kind == "regular"]
    loop = next(i for i in small if i + 1 in small)
    fail = next(i for i, (_f, kind, _a) in enumerate(seq) if kind == "too_short" and seq[i + 1][0] == "search_small")
    forms = {loop: 0, loop + 1: 2}
    for pos, form in ((fail - 1, 2), (fail + 1, 0)):
        assert forms.setdefault(pos, form) == form                      # (where the two meet they agree)
    return forms


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
    perm["view"].remove(MUST_ROWS["error"])                             # the view call starts both its turns through the rows with
    perm["view"].insert(0, MUST_ROWS["error"])                          # row 0: a `must` step first, a top-k search the second time
    # own_batch runs `counts` every fourth step: those runs take the rows of the `must` steps and the table's first
    count_rows = [int(r) for r in rng.permutation(list(MUST_ROWS.values()) + [TABLE_ROW])]
    count_rows += [r for r in perm["own_batch"] if r not in count_rows]
    forms = _graph_form_steps(seq)
    form_batch = make_batch(rng, 2, 0, False, False)
    count = collections.Counter()
    steps, own, prev = [], None, None
    for i, (fam, kind, after) in enumerate(seq):
        j = count[fam]
        row = perm[fam][j % len(rows)]
        if i in forms:
            j = count[fam, "forms"]
            count[fam, "forms"] += 1
        elif fam == "own_batch" and kind == "regular" and own is not None and own[0] == "reread_topk":
            j = count[fam, "counts"]                                    # (_own_batch_step: this one runs `counts`)
            row = count_rows[j % len(rows)]
            count[fam, "counts"] += 1
        elif kind == "regular":
            count[fam] += 1
        z, policy, pass_bytes, graph, self_hash = rows[row]
        if kind != "regular":
            pass_bytes = 0
            if kind == "invalid_base":
                policy = "error"
                if fam in ("search_large", "groups", "best"):          # the scan's own report of a bad query above index 16
                    row = MUST_ROWS["error"]
                    z, self_hash = rows[row][0], rows[row][4]
        params = {}
        if i in forms:
            row = MUST_ROWS["error"]
            (z, policy, pass_bytes, graph, _), self_hash = rows[row], forms[i]
            queries = form_batch
            params.update(t=0.5, lim=0)                                 # one shape class but for the form of the scan
        else:
            queries = _step_queries(rng, fam, kind, j, z, policy, pass_bytes != 0, params, row)
            _family_params(fam, kind, i, j, len(queries), row, params)
        if fam == "own_batch":
            own, queries = _own_batch_step(own, kind, j, queries, z, policy, params)
        steps.append(Step(i, fam, prev, kind, after, z, policy, states[i], pass_bytes, graph, self_hash, queries, params))
        prev = fam
    return steps


# ---- the self-hashing scan ------------------------------------------------------------------------------------------------

def _tile_sub_indexes(handle):
    """the sub-indexes a tile of the scan lies in (kernels.hpp: scan_tile_pages).  compact16: four sub-indexes of one
    16-byte chunk each, the tile is the index's four chunks wide (geometry.cpp: an index narrower than the tile)"""
    assert handle == "compact16"
    npages, cpp, tile_w = 4, 1, 4
    return 1 if cpp % tile_w == 0 else min(npages, 1 + (tile_w - 1 + cpp - 1) // cpp)


def self_hash_fits(handle, queries):
    """does the LDS array of the self-hashing scan hold the row indices of a pass over `queries` (tests/test_gpu_self_hash.py:
    _expect_self_hash)?  Multi-query work-groups are off on an index of fewer than 8 chunks."""
    blocks = max((len(q) - K_MAX + 1 + 7) // 8 for q in queries)
    return _tile_sub_indexes(handle) * (blocks + 1) * 8 <= SELF_HASH_ENTRIES


def self_hash_handle(handle):
    """can a pass on the handle take the self-hashing form at all (kernels.hpp: scan_has_self_hash)?  two_files holds a file
    of 20-mers under three hash functions, two_files_idx64 has 64-bit row indices"""
    return handle == "compact16"


def _pass_threshold(st):
    """the threshold the family hands to the pass (under `skip` a positive one takes K1's valid positions) and whether the
    pass selects its top k (geometry.cpp: pass_self_hash)"""
    fam, p = st.family, st.params
    if fam in SEARCH_FAMILIES:
        return p["t"], p["lim"] > 0
    if fam == "groups":
        return p["rt"], False
    if fam == "own_batch":
        return 0.0, p["what"] != "counts"
    return 0.0, False                                                   # counts, best: threshold 0, filtered after the pass


def must_self_hash(st, handle, kind="regular"):
    """has self_hash_passes to grow over the step?  (kind: the invalid_base steps are asked with their own)"""
    if st.kind != kind or not self_hash_handle(handle) or st.self_hash != 2 or st.z != 0 or st.pass_bytes != 0:
        return False
    if st.family not in RUN_IMPL_FAMILIES or st.params.get("what") == "reread":
        return False
    t, topk = _pass_threshold(st)
    if topk or (st.policy == "skip" and t > 0):
        return False
    return self_hash_fits(handle, st.queries)


def never_self_hash(st, handle):
    """must self_hash_passes stay as it is over the step?  (positions: over its hit_positions call -- the search in front of
    it is a host-buffer search like any other)"""
    return (not self_hash_handle(handle) or st.self_hash == 0 or st.z != 0 or st.family in OWN_K1_FAMILIES
            or st.family in NO_QUERIES)


# ---- the device passes ----------------------------------------------------------------------------------------------------

PASS_READERS = {"positions": "positions_ms", "prevalence": "prevalence_ms", "weighted": "weighted_ms", "coverage": "coverage_ms",
                "sets": "sets_ms", "quorum": "set_quorum_ms", "set_prevalence": "set_quorum_ms", "window": "window_ms",
                "window_positions": "positions_ms", "best": "best_ms"}


def needs_three_passes(st, expect):
    """must the step's call take at least 3 device passes (read off the family's *_ms reader)?  The small pass_bytes with
    the 24-query batch (make_batch: more than 2 * PASS_SMALL bytes of K1's table); hit_positions only looks up the queries
    that have a hit (window_positions: a window hit), and a set search without a labelled file has no work item; a
    window search at threshold 0 adds its pool's bytes to the estimate: more passes, never fewer.  (best: `best_ms` reads
    the passes of the LAST call from cobs_gpu_best_counts, nothing is reset by reading)"""
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
        if fam == "best":
            return BC.results(files, list(qs), list(p["offsets"]), z, pol, p["t"], p["lim"])
        if fam == "similarity":
            return [[[int(x) for x in row] for row in SC.shared_of_index({"mats": fb.mats}, similarity_refs(st, fb))] for fb in files]
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


def similarity_refs(st, fb):
    """the references of a similarity step in one file (findere_check.FileBits): real documents"""
    p = st.params
    per = fb.mats[0].shape[1] * 8
    first = range(0, min(per, fb.num_docs))
    last = range((len(fb.mats) - 1) * per, fb.num_docs)
    if p["n"] == 1:
        return [first[0] if p["side"] == "first" else last[-1]]
    pool = first if p["side"] == "first" else last
    refs = [first[0]] + [pool[x % len(pool)] for x in p["picks"][2:]]
    refs.insert(len(refs) // 2, last[-1])
    if p["repeat"]:
        refs[-1] = refs[1]
    return refs


def describe(st):
    """one line for an assertion message: the pair and the settings in force"""
    return ("step %d: %s -> %s [%s%s] z=%d policy=%s labels=%s pass_bytes=%d graph=%d self_hash=%d nq=%d lens=%s params=%s" % (
        st.index, st.prev, st.family, st.kind, (", after a failed " + st.after) if st.after else "", st.z, st.policy, st.labels,
        st.pass_bytes, st.graph, st.self_hash, len(st.queries), [len(q) for q in st.queries][:6],
        {k: v for k, v in st.params.items() if k not in ("offsets", "picks")}))
