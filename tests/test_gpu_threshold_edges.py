"""GPU: every search family with its threshold exactly at the boundary, against its checker.

The rule ceil(threshold * P) in double, hit on key >= bound, stands at eleven sites; the other GPU files
run fixed thresholds against random documents whose keys lie far from the bound.  Here the documents hold PREFIXES of
the query's terms (tests/threshold_edges.py), so every key from 0 to P exists, and each family is asked at

  t_on / t_above         the largest double whose bound is c, and its successor (bound c + 1),
  adversarial up / down  a threshold whose double product rounds past, or down onto, an integer,
  CLASSES                5e-324, 1e-300, 1.0, its successor, 2.0, 1e300, inf, NaN, -0.0, -1.0, -inf,

on a classic file, a compact file (page_size 16, partly filled last sub-index) and a handle of two files of term sizes 31
and 20 (P differs per file; every file is the target once).  Every comparison is exact.  tests/threshold_edges.case_list
raises where the checker shows no document on a bound inside [1, P] or none one below it, so no case is left out
(tests/test_threshold_edges_cpu.py asserts the same for the same inputs without a GPU)."""
import pytest

from tests import findere_check as F
from tests import threshold_edges as E

pytestmark = pytest.mark.gpu

TOPK = 128               # the largest k of the tile-level selection


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    return E.build_all(tmp_path_factory.mktemp("threshold_edges"))


def _refused(gpu, call, word=None):
    from cobs_amd import _capi
    with pytest.raises(gpu.CobsGpuError) as e:
        call()
    assert e.value.status == _capi.ERR_ARG, e.value
    assert word is None or word in str(e.value)


NO_ROWS = "did not keep the score rows"          # what counts_host says after a pass of the tile-level selection


def _no_rows_kept(gpu, b):
    """the last run of the batch kept no score rows: counts_host refuses with exactly that (any other error is raised)"""
    from cobs_amd import _capi
    try:
        b.counts_host(0)
    except gpu.CobsGpuError as e:
        if e.status != _capi.ERR_ARG or NO_ROWS not in str(e):
            raise
        return True
    return False


_TILE_K = {}             # id(Search) -> (Search, k)


def _tile_k(gpu, s, q):
    """the largest k of 32, 16, ... 1 at which run_topk(keep_counts=False) keeps no score rows on this handle (0: none)"""
    if id(s) not in _TILE_K:
        found = 0
        for k in (32, 16, 8, 4, 2, 1):
            b = gpu.Batch(s)
            b.set_queries([q])
            b.run_topk(0.0, k, keep_counts=False)
            b.sync()
            if _no_rows_kept(gpu, b):
                found = k
            b.close()
            if found:
                break
        _TILE_K[id(s)] = (s, found)              # (holds the handle: its id stays its own)
    return _TILE_K[id(s)][1]


def _batch_paths(gpu, s, fam, t, want, rows_dropped):
    """the four result paths of a plain pass -> [(path, got, want)]; a hits-only pass without a threshold is refused before
    anything is launched (the statistics of the batch stay those of the run before)"""
    b = gpu.Batch(s)
    b.set_queries([fam.q])
    out = []
    b.run(t)
    b.sync()
    out.append(("score rows, host filter", b.hits_host(0), want))
    if t > 0:
        b.run_hits(t)
        b.sync()
        out.append(("hits-only pool", b.hits_host(0), want))
    else:
        before = b.stats()
        _refused(gpu, lambda: b.run_hits(t), "threshold > 0")
        assert b.stats() == before
    b.run_topk(t, TOPK, keep_counts=True)
    b.sync()
    out.append(("top-k, rows kept", b.hits_host(0, TOPK), want[:TOPK]))
    b.close()
    # the tile-level selection: the pass takes the score rows instead where tiles x k candidates would be larger than the
    # rows they replace (pass.cpp), so on these 300-document files k is the largest that keeps no rows
    k = _tile_k(gpu, s, fam.q)
    assert k or not rows_dropped, "no k at which a top-k pass keeps no score rows"
    b = gpu.Batch(s)
    b.set_queries([fam.q])
    b.run_topk(t, k or TOPK, keep_counts=False)
    b.sync()
    out.append(("tile top-k, no rows", b.hits_host(0, k or TOPK), want[:k or TOPK]))
    if k:
        assert _no_rows_kept(gpu, b)                        # (the tile-level path ran)
    b.close()
    out.append(("host call", s.search_hits([fam.q], t, 0)[0], want))
    return out


def _rows(offs, hits, i=0):
    return [tuple(r) for r in hits.tolist()[int(offs[i]):int(offs[i + 1])]]


def _per_group(offs, hits):
    return [_rows(offs, hits, g) for g in range(len(offs) - 1)]


def _device(gpu, s, family, fam, t, want):
    """-> [(path, got, want)] of one threshold"""
    if family in ("plain", "plain_skip", "findere"):
        return _batch_paths(gpu, s, fam, t, want, family == "plain")
    if family == "groups":
        offs, hits, _pos = s.search_groups_arrays(fam.queries, fam.offsets, t, fam.read_threshold, 0)
        return [("groups", _per_group(offs, hits), want)]
    if family == "groups_read":
        offs, hits, _pos = s.search_groups_arrays(fam.queries, fam.offsets, 0.0, t, 0)
        return [("read threshold", _per_group(offs, hits), want)]
    if family == "best":
        return [("best", _per_group(*s.search_best_arrays(fam.queries, fam.offsets, t, 0)), want)]
    if family == "weighted":
        offs, hits, _total = s.search_weighted_arrays([fam.q], t, 0)
        return [("weighted", _rows(offs, hits), want)]
    if family in ("sets_any", "sets_all"):
        return [(family, _rows(*s.search_sets_arrays([fam.q], t, fam.rank_by, 0)), want)]
    if family == "quorum_threshold":
        return [(family, _rows(*s.search_sets_quorum_arrays([fam.q], fam.quorum, t, 0)), want)]
    if family == "quorum_need":
        return [(family, _rows(*s.search_sets_quorum_arrays([fam.q], t, 0.0, 0)), want)]
    if family == "coverage":
        return [(family, _rows(*s.search_coverage_arrays([fam.q], t, 0)), want)]
    assert family == "window"
    return [(family, _rows(*s.search_window_arrays([fam.q], E.WINDOW, t, 0)), want)]


def _open(gpu, family, fam, paths, fbs):
    kw = {}
    if family == "plain_skip":
        kw["invalid_bases"] = "skip"
    if family == "findere":
        kw["findere"] = E.FINDERE_Z
    s = gpu.Search(paths if len(paths) > 1 else paths[0], **kw)
    if family.startswith(("sets", "quorum")):
        for f, labels in enumerate(fam.labelings(fbs)):
            s.set_doc_sets(labels, f)
    return s


_KEY_COLUMN = {"sets_all": 3, "best": 3}       # the column of the key in a record (default 2)


@pytest.mark.parametrize("handle", sorted(E.HANDLES))
@pytest.mark.parametrize("family", sorted(E.FAMILIES))
def test_family_at_the_boundary(gpu_lib, files, family, handle):
    fam = E.FAMILIES[family]()
    paths = [files[n][0] for n in E.HANDLES[handle]]
    fbs = [files[n][1] for n in E.HANDLES[handle]]
    s = _open(gpu_lib, family, fam, paths, fbs)
    boundaries = 0
    for f in range(len(fbs)):
        P = fam.P(fbs, f)
        for name, t, b in fam.cases(fbs, f):                     # (raises where condition (a) does not hold)
            if family == "quorum_need" and fam.refused(t):
                s.set_quorum_ms()
                _refused(gpu_lib, lambda: s.search_sets_quorum_arrays([fam.q], t, 0.0, 0), "quorum")
                assert s.set_quorum_ms()["passes"] == 0          # nothing was launched
                continue
            want = fam.expected(fbs, t)
            for path, got, w in _device(gpu_lib, s, family, fam, t, want):
                assert got == w, (family, handle, f, name, t, b, path, got[:3], w[:3])
            if family == "groups_read":
                # group 1 = [Q]: a document votes when its own score reaches the bound, and one on the bound does
                voted = sorted(r[2] for r in want[1] if r[0] == f and r[3] == 1)
                if 1 <= b <= P:
                    assert voted and voted[0] == b, (handle, f, name, t, b, voted[:3])
                    boundaries += 1
                else:
                    assert len(voted) == (0 if b > P else sum(1 for r in want[1] if r[0] == f)), (handle, f, name, t, b)
                continue
            if family == "quorum_need":
                # the core of the 100-member set 0 = its positions held by at least `need` members: cells on the bound count
                cells = [int(k) for k in fam.keys(fbs, f)]
                core = dict(((r[0], r[1]), r[2]) for r in want)[(f, 0)]
                assert core == sum(1 for k in cells if k >= b) and b in cells and b - 1 in cells, (handle, f, name, t, b, core)
                boundaries += 1
                continue
            recs = want[0] if family in ("groups", "best") else want
            mine = sorted(r[_KEY_COLUMN.get(family, 2)] for r in recs if r[0] == f)
            if fam.smallest(fbs, f) < b <= P:
                assert mine and mine[0] == b, (family, handle, f, name, t, b, mine[:3])       # the document on the bound is in
                assert b - 1 in set(int(k) for k in fam.keys(fbs, f))                          # ... the one below exists, and is out
                boundaries += 1
            elif b > P:
                assert mine == [], (family, handle, f, name, t)
    assert boundaries >= 5 * len(fbs)
    s.close()


@pytest.mark.parametrize("handle", sorted(E.HANDLES))
def test_tile_topk_is_cut_by_the_threshold_not_by_k(gpu_lib, files, handle):
    """the tile-level selection keeps no rows only for a small k on these files (see _batch_paths), and about 33 documents
    hold 95 of the 100 terms of the family test's query: its top-k is cut by k there.  The 140-character text itself
    has 110 (term size 20: 121) terms, which two documents of a file hold completely and three more all but one: with the
    bound on the last but one term and on the last, FEWER than k documents reach it, so the list ends where the threshold
    says -- a tile bound one too low or one too high shows"""
    fam = E.Plain()
    q = fam.src
    paths = [files[n][0] for n in E.HANDLES[handle]]
    fbs = [files[n][1] for n in E.HANDLES[handle]]
    s = gpu_lib.Search(paths if len(paths) > 1 else paths[0])
    k = _tile_k(gpu_lib, s, q)
    assert k, "no k at which a top-k pass keeps no score rows"
    cut_by_threshold = 0
    for f, fb in enumerate(fbs):
        P = fb.positions(q, 0)
        keys = set(int(x) for x in E.real_keys(fb, fb.scores(q, 0)))
        assert {P - 2, P - 1, P} <= keys
        for t, bound in zip(E.on_and_above(P - 1, P), (P - 1, P)):
            want = F.results(fbs, q, 0, t, 0)
            assert min(sc for (fi, _d, sc) in want if fi == f) == bound          # a document on the bound, none below it
            b = gpu_lib.Batch(s)
            b.set_queries([q])
            b.run_topk(t, k, keep_counts=False)
            b.sync()
            assert b.hits_host(0, k) == want[:k], (handle, f, t, bound, k)
            assert _no_rows_kept(gpu_lib, b)
            b.close()
            cut_by_threshold += len(want) < k
    assert cut_by_threshold >= 1, (handle, k)
    s.close()


def test_hits_only_pass_over_row_ranges(gpu_lib, files, monkeypatch):
    """a 480 KB classic file under a 32 KiB budget is scanned in row ranges.  With row_fetch 0 every range is copied whole:
    K2 sees partial counts, and the hits are selected from the complete scores behind the last range (select_rows_kernel)
    -- on the boundary.  The untouched handle fetches the looked-up rows of all ranges as one unit and selects in K2."""
    monkeypatch.setenv("COBS_GPU_ROW_RANGE_MIN", "48")
    path, fb = files["rows"]
    fam = E.Plain()
    for whole_ranges in (True, False):
        s = gpu_lib.Search(path, hbm_budget=32 * 1024)
        if whole_ranges:
            s.set_tuning("row_fetch", 0)
        assert s.stream_layout(0)[3] >= 3, s.stream_layout(0)
        b = gpu_lib.Batch(s)
        b.set_queries([fam.q])
        shown = 0
        for name, t, bound in fam.cases([fb], 0):
            want = fam.expected([fb], t)
            if not t > 0:
                _refused(gpu_lib, lambda: b.run_hits(t), "threshold > 0")
                continue
            b.run_hits(t)
            b.sync()
            assert b.hits_host(0) == want, (whole_ranges, name, t, bound)
            b.run(t)                                             # ... and the pass that keeps the rows (rows_select)
            b.sync()
            assert b.hits_host(0) == want, (whole_ranges, "rows kept", name, t, bound)
            assert s.search_hits([fam.q], t, 0)[0] == want, (whole_ranges, name, t, bound)
            if 1 <= bound <= fam.P([fb], 0):
                assert min(sc for (_f, _d, sc) in want) == bound
                shown += 1
        assert shown >= 5
        b.close()
        s.close()


def test_replayed_graph_takes_the_threshold_of_its_query(gpu_lib, files):
    """a small search is captured into a graph at its second call and replayed from the third.  The threshold is part of the
    graph's key, the query lengths are not: a graph captured for 103 terms is replayed for 100 and for 97 terms of the same
    shape class, and each replay has to stage ceil(t * T) of ITS query -- with t exactly on a bound of the 100-term
    query, above it, and at the adversarial pairs of 100"""
    path, fb = files["classic"]
    fam = E.Plain()
    src = fam.src
    queries = [src[:133], src[:E.Q_LEN], src[:127]]          # 103, 100 and 97 terms: 13 blocks of 8 terms each
    adv = E.adversarial([100])
    ts = list(E.on_and_above(90, 100)) + [[a for a in adv if a[0] == d and a[3] >= 50][0][1] for d in ("up", "down")]
    s = gpu_lib.Search(path)
    for t in ts:
        bounds = [E.bound(t, fb.positions(q, 0)) for q in queries]
        assert len(set(bounds)) == 3, (t, bounds)            # (a threshold left over from another query would show)
        replays = s.graph_replays
        for q in [queries[0]] * 3 + [queries[1], queries[2], queries[1], queries[2]]:
            got = s.search_hits([q], t, 0)[0]
            assert got == F.results([fb], q, 0, t, 0), (t, len(q))
            assert min(sc for (_f, _d, sc) in got) == E.bound(t, fb.positions(q, 0)), (t, len(q))
        # the third call of the long query replays; three replays mean that the other lengths were served by its graph too
        assert s.graph_replays - replays >= 3, (t, s.graph_replays - replays)
    s.close()
