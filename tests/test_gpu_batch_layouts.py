"""GPU: every pass of the Batch API on every layout the planner can give an index, against the oracle.

The layouts: resident (classic, compact with one and two hash functions); streamed in whole chunks; streamed as
column slices; streamed as ROW RANGES (copied whole, fetched row by row, or merged into one fetched unit); a mixed
plan that keeps some slices of a streamed file in HBM; two files in one handle, one resident and one in row ranges.
Every case first proves it is that layout (Search.stream_layout, stream_plan, stream_counters).

The passes: run(0.0), run(t), run_hits(t), run_topk(t, k) and run_topk(t, k, keep_counts=False), with the readers
after each (counts_host, hits_host, score_histogram, bucketed_hits and the one-rank hit, top-k and count exchanges),
over query sets of all three score widths, with thresholds that put a document exactly on ceil(t * T), and the
passes one after another on one Batch (a stale pool or stale candidates show up there)."""
import collections
import math

import numpy as np
import pytest

from tests import cases
from tests import findere_check as F

pytestmark = pytest.mark.gpu

K = 31
KIB = 1024


def _compact(path, num_docs, page_size, sigs, num_hashes, seed, planted, query):
    """a compact index (as cases.make_compact) and its bits for the findere checker"""
    rng = np.random.default_rng(seed)
    page_docs = 8 * page_size
    mats = [cases.mask_padding_docs(cases.random_bits(rng, (s, page_size), 0.3), p * page_docs, num_docs)
            for p, s in enumerate(sigs)]
    cases.plant(mats, sigs, page_docs, query, planted, K, 1, num_hashes)
    from oracle import construct as C
    C.write_compact(path, K, 1, page_size, [(s, num_hashes) for s in sigs], ["doc_%05d" % i for i in range(num_docs)], mats)
    return F.FileBits(K, 1, num_hashes, mats, num_docs)


@pytest.fixture(scope="module")
def data(gpu_lib, oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("layouts")
    src = oracle.random_sequence(700, 41)          # the planted query; the reads are cut from it
    out = {"src": src}
    # 500-byte rows at an odd file offset (pitch 512), 4.6 MB: four row ranges under 1.2 MB stream buffers
    p = str(d / "rr.cobs_classic")
    cases.make_classic(p, 4000, 9001, 1, K, 1, 0.3, 12, planted={5: 1.0, 1234: 0.8, 2711: 0.6, 3999: 0.9}, query=src)
    out["classic"] = (p, F.classic_file(p))
    # one hash function, the 20 011-row sub-index (2.5 MB at pitch 128) in five row ranges under 600 KB buffers
    ps = 96
    D = 3 * 8 * ps - 5
    p = str(d / "rr.cobs_compact")
    out["compact"] = (p, _compact(p, D, ps, [900, 20011, 1500], 1, 11,
                                  {0: 1.0, 8 * ps + 3: 0.95, 2 * 8 * ps - 1: 0.6, D - 1: 0.85}, src))
    # two hash functions: the 5000-row sub-index is cut into column slices under 200 KB buffers
    D = 5 * 8 * ps - 11
    p = str(d / "h2.cobs_compact")
    out["compact_h2"] = (p, _compact(p, D, ps, [700, 1500, 5000, 900, 2600], 2, 6,
                                     {0: 1.0, D - 1: 0.95, 1000: 0.6, 2500: 0.85}, src))
    # sub-indexes of about equal size: streamed, each fits a buffer (whole chunks, some shared)
    ps = 64
    D = 4 * 8 * ps - 9
    p = str(d / "whole.cobs_compact")
    out["compact_whole"] = (p, _compact(p, D, ps, [2000, 2600, 1800, 2200], 1, 21,
                                        {3: 1.0, 600: 0.7, D - 1: 0.9}, src))
    return out


def _reads(src, n, seed):
    """reads of 40-150 bp: most cut from the planted query, some random"""
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ln = int(rng.integers(40, 151))
        if i % 5 == 4:
            out.append(O.random_sequence(ln, 1000 + seed * 100 + i))
        else:
            a = int(rng.integers(0, len(src) - ln + 1))
            out.append(src[a:a + ln])
    return out


def _query_sets(oracle, src, which):
    sets = {
        "u8": (_reads(src, 10, 1), 1),
        "u16": (_reads(src, 6, 2) + [src], 2),
        "u32": ([oracle.random_sequence(66030, 4242), src[:200]], 4),
        # enough looked-up rows that a file's ranges do not fit one gather: fetched range by range (merged in pairs)
        "u8_many": (_reads(src, 60, 3), 1),
        "u16_many": (_reads(src, 40, 4) + [src], 2),
        # one or two queries: every range of a sub-index fetched as one unit
        "u8_tiny": ([src[100:190]], 1),
        "u16_tiny": ([src, src[300:420]], 2),
    }
    return [(name,) + sets[name] for name in which]


# ---- layouts ---------------------------------------------------------------------------------------------------------

def _resident_bytes(gpu, paths):
    s = gpu.Search(paths)
    n = sum(s.info(f).hbm_bytes for f in range(s.num_files))
    s.close()
    return n


def _open(gpu, data, monkeypatch, name):
    """-> (Search, file keys, query sets) of layout `name`, after asserting the layout's witness"""
    P = {k: data[k][0] for k in ("classic", "compact", "compact_h2", "compact_whole")}
    if name.startswith("resident_"):
        key = {"resident_classic": "classic", "resident_compact_h1": "compact", "resident_compact_h2": "compact_h2"}[name]
        s = gpu.Search(P[key])
        lay = s.stream_layout(0)
        assert lay == ({"classic": 1, "compact": 3, "compact_h2": 5}[key], 0, 0, 0) and s.stream_plan()[3] == 0, lay
        sets = ["u8", "u16", "u32"] if key == "classic" else ["u8", "u16"]
        return s, [key], sets
    if name == "streamed_whole":
        s = gpu.Search(P["compact_whole"], hbm_budget=int(0.75 * _resident_bytes(gpu, P["compact_whole"])))
        lay = s.stream_layout(0)
        assert lay[1] > 0 and lay[2] == 0 and lay[3] == 0, lay
        return s, ["compact_whole"], ["u8", "u16"]
    if name == "column_slices":
        s = gpu.Search(P["compact_h2"], hbm_budget=400 * KIB)
        lay = s.stream_layout(0)
        assert lay[2] > 0 and lay[3] == 0, lay
        return s, ["compact_h2"], ["u8", "u16"]
    if name in ("row_ranges_whole_classic", "row_ranges_whole_compact"):
        key = "classic" if name.endswith("classic") else "compact"
        s = gpu.Search(P[key], hbm_budget=2400 * KIB if key == "classic" else 1200 * KIB)
        s.set_tuning("row_fetch", 0)
        assert s.stream_layout(0)[3] >= 3, s.stream_layout(0)
        return s, [key], ["u8", "u16", "u32"] if key == "classic" else ["u8", "u16"]
    if name == "row_ranges_fetched":
        s = gpu.Search(P["classic"], hbm_budget=2400 * KIB)
        s.set_tuning("row_fetch_alpha", 0)
        assert s.stream_layout(0)[3] >= 3, s.stream_layout(0)
        return s, ["classic"], ["u8_many", "u16_many"]
    if name == "row_ranges_one_unit":
        s = gpu.Search(P["classic"], hbm_budget=2400 * KIB)
        s.set_tuning("row_fetch", 1)
        assert s.stream_layout(0)[3] >= 3, s.stream_layout(0)
        return s, ["classic"], ["u8_tiny", "u16_tiny"]
    if name == "mixed":
        # 600 KiB stream buffers out of 850: the two small sub-indexes stay in HBM beside them, the large one is streamed
        monkeypatch.setenv("COBS_GPU_STREAM_BUF_KIB", "600")
        s = gpu.Search(P["compact"], hbm_budget=1700 * KIB)
        plan, lay = s.stream_plan(), s.stream_layout(0)
        assert plan[1] > 0 and plan[3] > 0, plan
        assert lay[0] == 2 and lay[3] >= 3, lay
        return s, ["compact"], ["u8", "u16"]
    if name == "two_files":
        # the compact file stays resident (at most half the budget), the classic one is streamed in 1.2 MB ranges
        s = gpu.Search([P["compact_whole"], P["classic"]], hbm_budget=_resident_bytes(gpu, P["compact_whole"]) + 2400 * KIB)
        s.set_tuning("row_fetch", 0)
        l0, l1 = s.stream_layout(0), s.stream_layout(1)
        assert l0[0] > 0 and l0[1:] == (0, 0, 0), l0
        assert l1[3] >= 3, l1
        return s, ["compact_whole", "classic"], ["u8", "u16"]
    raise AssertionError(name)


LAYOUTS = ["resident_classic", "resident_compact_h1", "resident_compact_h2", "streamed_whole", "column_slices",
           "row_ranges_whole_classic", "row_ranges_whole_compact", "row_ranges_fetched", "row_ranges_one_unit",
           "mixed", "two_files"]


# ---- the oracle's side -----------------------------------------------------------------------------------------------

class Want:
    """the oracle's rows and result lists of one query set on a list of files (cached per threshold)"""

    def __init__(self, oracle, paths, queries):
        self.ixs = [oracle.Index.open(p) for p in paths]
        self.queries = queries
        self.rows = [np.concatenate([ix.counts(q) for ix in self.ixs]) for q in queries]
        self._res = {}

    def results(self, i, t, lim=0):
        if (i, t) not in self._res:
            self._res[(i, t)] = cases.oracle_results(self.ixs, self.queries[i], t, 0)
        r = self._res[(i, t)]
        return r[:lim] if lim else r

    def records(self, t):
        return sorted((i, f, d, sc) for i in range(len(self.queries)) for (f, d, sc) in self.results(i, t))

    def histogram(self):
        h = collections.Counter()
        for q in self.queries:
            for ix in self.ixs:
                h.update(int(v) for v in ix.counts(q)[:ix.num_docs])
        return h

    def thresholds(self):
        """t = c / T for the second-highest count c of the longest query and of a short one (a document lies exactly on
        ceil(t * T)), a little above the first, 0.35 (the tail of the random documents), 0.05 and 1.0"""
        def exact(i):
            T = len(self.queries[i]) - K + 1
            real = np.concatenate([ix.counts(self.queries[i])[:ix.num_docs] for ix in self.ixs])
            vals = np.unique(real)
            c = int(vals[-2] if len(vals) > 1 else vals[-1])
            assert c > 0
            t = c / T
            while math.ceil(t * T) > c:
                t = math.nextafter(t, 0.0)
            assert math.ceil(t * T) == c and (real == c).any()
            return t, (c + 0.5) / T
        longest = max(range(len(self.queries)), key=lambda j: len(self.queries[j]))
        t_long, t_above = exact(longest)
        return [t_long, t_above, exact(0)[0], 0.35, 0.05, 1.0]


def _global_rows(b, eb):
    q0, qn, t = b.global_counts_tensor()
    return q0, qn, t.cpu().numpy().astype(np.int64) & ((1 << (8 * eb)) - 1)


def _check_run(b, w, t, comm):
    """run(t): a thresholded pass that keeps the score rows"""
    n = len(w.queries)
    b.run(t)
    b.sync()
    for i in range(n):
        assert b.hits_host(i) == w.results(i, t), ("run", t, i)
        assert b.hits_host(i, 3) == w.results(i, t, 3), ("run", t, i)
        assert np.array_equal(b.counts_host(i), w.rows[i]), ("run", t, i)
    counts, rec = b.bucketed_hits(1)
    assert counts == [len(rec)] and sorted(map(tuple, rec.tolist())) == w.records(t), ("bucketed", t)
    assert b.exchange_hits(comm) is False
    for i in range(n):
        assert b.hits_host(i) == w.results(i, t), ("exchange_hits", t, i)
    b.run(t)
    b.sync()
    assert b.exchange_hits_owned(comm) == (False, 0, n)
    for i in range(n):
        assert b.hits_host(i) == w.results(i, t), ("exchange_hits_owned", t, i)


def _check_hits(b, w, t):
    from cobs_amd import _capi
    import cobs_amd
    b.run_hits(t)
    b.sync()
    for i in range(len(w.queries)):
        assert b.hits_host(i) == w.results(i, t), ("run_hits", t, i)
        assert b.hits_host(i, 2) == w.results(i, t, 2), ("run_hits", t, i)
    with pytest.raises(cobs_amd.CobsGpuError) as e:
        b.counts_host(0)
    assert e.value.status == _capi.ERR_ARG


def _check_topk(b, w, t, k, comm, eb):
    from cobs_amd import _capi
    n = len(w.queries)
    b.run_topk(t, k)
    b.sync()
    for i in range(n):
        assert b.hits_host(i, k) == w.results(i, t, k), ("run_topk", t, k, i)
        assert np.array_equal(b.counts_host(i), w.rows[i]), ("run_topk", t, k, i)
    b.exchange_topk(comm)
    b.sync()
    for i in range(n):
        assert b.hits_host(i, k) == w.results(i, t, k), ("exchange_topk", t, k, i)
    b.run_topk(t, k)
    b.exchange_counts(comm, _capi.XCHG_ALLGATHER)
    b.sync()
    q0, qn, rows = _global_rows(b, eb)
    assert (q0, qn) == (0, n)
    assert np.array_equal(rows, np.stack(w.rows)), ("exchange_counts", t, k)


def _check_topk_only(b, w, t, k):
    b.run_topk(t, k, keep_counts=False)
    b.sync()
    for i in range(len(w.queries)):
        assert b.hits_host(i, k) == w.results(i, t, k), ("run_topk_only", t, k, i)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_pass_and_reader(gpu_lib, oracle, data, comm_one_rank, monkeypatch, layout):
    s, keys, set_names = _open(gpu_lib, data, monkeypatch, layout)
    paths = [data[k][0] for k in keys]
    comm = comm_one_rank
    streamed = s.stream_plan()[3] > 0
    b = gpu_lib.Batch(s)
    for name, queries, eb in _query_sets(oracle, data["src"], set_names):
        w = Want(oracle, paths, queries)
        b.set_queries(queries)
        # run(0.0): the rows and their distribution over real documents
        b.run(0.0)
        b.sync()
        assert b.counts_device()[1] == eb, name
        for i in range(len(queries)):
            assert np.array_equal(b.counts_host(i), w.rows[i]), (name, i)
        nb = max(len(q) for q in queries) - K + 2
        h = b.score_histogram(nb)
        assert {i: int(c) for i, c in enumerate(h) if c} == dict(w.histogram()), name
        ts = w.thresholds()
        for t in ts:
            _check_run(b, w, t, comm)
            _check_hits(b, w, t)
            _check_topk(b, w, t, 5, comm, eb)
        for k in (1, 3, 17, 129):
            _check_topk_only(b, w, ts[0], k)
        _check_topk_only(b, w, 0.0, 17)
        # one Batch, the same queries, the pass kinds one after another: nothing of the previous pass may answer
        t0, t1 = ts[0], ts[2]
        _check_hits(b, w, t1)
        _check_run(b, w, t0, comm)
        _check_topk_only(b, w, t1, 3)
        _check_run(b, w, 0.05, comm)
        b.run(0.0)
        b.sync()
        for i in range(len(queries)):
            assert np.array_equal(b.counts_host(i), w.rows[i]), ("transition", name, i)
            assert b.hits_host(i, 4) == w.results(i, 0.0, 4), ("transition", name, i)
    if layout == "row_ranges_whole_classic" or layout == "row_ranges_whole_compact" or layout == "two_files":
        assert s.stream_counters()[0] == 0                   # row_fetch = 0: every range copied whole
    if layout in ("row_ranges_fetched", "row_ranges_one_unit"):
        assert s.stream_counters()[0] > 0                    # ... and here looked-up rows were fetched
    b.close()
    # findere: resident handles score windows (set_findere refuses a streamed one)
    from cobs_amd import _capi
    if streamed:
        with pytest.raises(gpu_lib.CobsGpuError) as e:
            s.set_findere(3)
        assert e.value.status == _capi.ERR_UNSUPPORTED
    else:
        files = [data[k][1] for k in keys]
        s.set_findere(3)
        bf = gpu_lib.Batch(s)
        queries = _reads(data["src"], 8, 5) + [data["src"]]
        bf.set_queries(queries)
        for t in (0.05, 0.5, 0.9):
            bf.run(t)
            bf.sync()
            for i, q in enumerate(queries):
                assert bf.hits_host(i) == F.results(files, q, 3, t, 0), ("findere", t, i)
                assert bf.hits_host(i, 3) == F.results(files, q, 3, t, 3), ("findere", t, i)
                assert np.array_equal(bf.counts_host(i), F.counts(files, q, 3)), ("findere", t, i)
        bf.close()
        s.set_findere(0)
    s.close()


# ---- pool overflow on small fixtures (tuning key hit_cap) ------------------------------------------------------------

@pytest.mark.parametrize("layout", ["resident_classic", "row_ranges_whole_classic", "row_ranges_fetched"])
def test_hit_pool_overflow(gpu_lib, oracle, data, comm_one_rank, monkeypatch, layout):
    import cobs_amd
    from cobs_amd import _capi
    s, keys, _ = _open(gpu_lib, data, monkeypatch, layout)
    paths = [data[k][0] for k in keys]
    comm = comm_one_rank
    src = data["src"]
    queries = _reads(src, 10, 1) if layout != "row_ranges_fetched" else _reads(src, 60, 3)
    w = Want(oracle, paths, queries)
    want = lambda t: [w.results(i, t) for i in range(len(queries))]  # noqa: E731
    with pytest.raises(cobs_amd.CobsGpuError) as e:
        s.set_tuning("hit_cap", -1)
    assert e.value.status == _capi.ERR_ARG
    # a low threshold: the pool holds half of the hits
    t = 0.05
    n = len(w.records(t))
    s.set_tuning("hit_cap", n // 2)
    b = gpu_lib.Batch(s)
    b.set_queries(queries)
    b.run_hits(t)
    b.sync()
    with pytest.raises(cobs_amd.CobsGpuError) as e:
        b.hits_host(0)
    assert e.value.status == _capi.ERR_ARG and "did not keep the score rows" in str(e.value)
    b.run_hits(t)
    b.sync()
    assert b.exchange_hits(comm) is True
    b.run(t)                      # the rows are kept: the readers answer from them
    b.sync()
    for i in range(len(queries)):
        assert b.hits_host(i) == w.results(i, t), i
    assert s.search_hits(queries, t, 0) == want(t)
    assert s.sharded_search_hits(comm, queries, t, 0) == want(t)
    # a high threshold and a cap just below the true hit count: the repeat with score rows must not fill its pool from
    # the partial counts of row ranges (fewer records, which would fit)
    t = w.thresholds()[0]
    n = len(w.records(t))
    assert n >= 2
    s.set_tuning("hit_cap", n - 1)
    assert s.search_hits(queries, t, 0) == want(t)
    assert s.sharded_search_hits(comm, queries, t, 0) == want(t)
    b.set_queries(queries)
    b.run(t)
    b.sync()
    for i in range(len(queries)):
        assert b.hits_host(i) == w.results(i, t), i
    # ... and at the true count it fits: the pool answers
    s.set_tuning("hit_cap", n)
    b.set_queries(queries)
    b.run_hits(t)
    b.sync()
    for i in range(len(queries)):
        assert b.hits_host(i) == w.results(i, t), i
    assert s.search_hits(queries, t, 0) == want(t)
    s.set_tuning("hit_cap", 0)
    b.close()
    s.close()
