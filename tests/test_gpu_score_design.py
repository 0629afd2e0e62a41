"""GPU: the three order-sensitive device stages -- K3 selection (topk_kernel, over score rows and over the candidate pool),
the full ranking (rank_kernel, rank_prefix_kernel) and the threshold filter over accumulated rows (select_rows_kernel) --
on DESIGNED score distributions (tests/score_design.py): scores on both sides of every digit edge of the radix plans, tie
runs split at the cut from chosen waves, exactly k - 1 / k / k + 1 documents passing, all scores equal, all zero, the
8192-survivor sort limit, and the three-level descent.  A long filler query in the batch sets the plan (8, 12, 16, 20, 24
or 32 planes) the short designed queries run under.  Every case compares the complete list (file, document, score, in
order) with the oracle's; the designed queries are also held against the numpy contract score_design.expected."""
import numpy as np
import pytest

from tests import cases
from tests import score_design as S

pytestmark = pytest.mark.gpu

TIE_K = 40
NO_ROWS = "did not keep the score rows"


class World:
    """the fixtures, built when first asked for, with the oracle's full list of every (query, threshold) kept"""

    def __init__(self, directory, oracle):
        self.dir, self.O, self.made, self.lists, self.scores = directory, oracle, {}, {}, {}

    def get(self, kind, b=0):
        key = (kind, b)
        if key not in self.made:
            d = {"small": lambda: S.build_small(self.dir, b), "paged": lambda: S.build_paged(self.dir, b),
                 "wide": lambda: S.build_wide(self.dir)}[kind]()
            self.made[key] = (d, self.O.Index.open(d.path))
        return self.made[key]

    def want(self, kind, b, q, t, k):
        key = (kind, b, q, float(t))
        if key not in self.lists and len(q) > 500000:
            # the 2^20- and 2^24 + 77-term fillers: scores from row multiplicities (held against the oracle's counts in
            # tests/test_score_design_cpu.py), the list from the numpy contract
            d = self.get(kind, b)[0]
            if (kind, b, q) not in self.scores:
                self.scores[(kind, b, q)] = S.design_scores(d, q)
            self.lists[key] = S.expected(self.scores[(kind, b, q)], S.bound_of(t, len(q) - S.K + 1), 0)
        if key not in self.lists:
            self.lists[key] = cases.oracle_results([self.get(kind, b)[1]], q, t, 0)
        full = self.lists[key]
        return full[:k] if k else full


@pytest.fixture(scope="module")
def world(tmp_path_factory, oracle):
    return World(tmp_path_factory.mktemp("score_design"), oracle)


def _no_rows_kept(gpu, b):
    from cobs_amd import _capi
    try:
        b.counts_host(0)
    except gpu.CobsGpuError as e:
        if e.status != _capi.ERR_ARG or NO_ROWS not in str(e):
            raise
        return True
    return False


def _batch_of(d, planes, extra=()):
    """(names, queries): every designed query, then the filler that sets the plan"""
    names = list(d.queries) + ["filler"] + ["extra%d" % i for i in range(len(extra))]
    qs = [d.queries[nm] for nm in d.queries] + [S.filler(planes)] + list(extra)
    assert S.planes_for(max(len(q) for q in qs) - S.K + 1) == planes
    return names, qs


def _check_topk(world, kind, b, d, bt, names, qs, t, k, what):
    for i, (nm, q) in enumerate(zip(names, qs)):
        got = bt.hits_host(i, k)
        want = world.want(kind, b, q, t, k)
        assert got == want, (what, nm, t, k, got[:3], want[:3])
        if nm in d.targets:
            assert want == S.expected(d.targets[nm], S.bound_of(t, d.terms[nm]), k), (nm, t, k)


def _tie_ks(n):
    _s, r0, run = S.tie_run_at_cut(n, TIE_K, "last")
    return S.tie_ks(TIE_K - 1, r0, run, n)


def _thresholds(d):
    """0 and the three thresholds that let exactly k - 1, k and k + 1 documents of `exactly` pass"""
    bounds = S.exactly(d.num_docs, TIE_K)[1]
    return [0.0] + [S.threshold_for(c, d.terms["exactly"]) for c in bounds]


PLANS = [(4, 8), (8, 12), (8, 16), (10, 20)]          # (designed digit width, planes of the batch)
# 32 planes (three K3 levels, three ranking passes) over the 10-bit design: every call moves the 16 MB filler, so it runs on
# `small` with the k at the cut, at the tie edges and at the ends, and on `paged` for one tile geometry of the pool
FILES_PLANS = [(kind, b, planes) for kind in ("small", "paged") for (b, planes) in PLANS] + [("small", 10, 32)]


@pytest.mark.parametrize("kind,b,planes", FILES_PLANS)
def test_k3_over_score_rows(gpu_lib, world, kind, b, planes):
    """run_topk with the rows kept: 8-bit rows (8 planes), 16-bit (12, 16) and 32-bit (20); every k of edge_ks and tie_ks
    at threshold 0, the k around the cut of `exactly` at its three bounds; and a pass that asked for no rows with the
    tile-level selection switched off"""
    d, _ix = world.get(kind, b)
    n = d.num_docs
    names, qs = _batch_of(d, planes)
    s = gpu_lib.Search(d.path)
    bt = gpu_lib.Batch(s)
    bt.set_queries(qs)
    ks = sorted(set(S.edge_ks(n, S.wave_per(n)) + _tie_ks(n) + [TIE_K - 1, TIE_K, TIE_K + 1]))
    if planes == 32:
        ks = sorted(set([1, 2, TIE_K - 1, TIE_K, TIE_K + 1, 512, 513, n - 1, n, n + 1] + _tie_ks(n)))
    for k in ks:
        bt.run_topk(0.0, k, keep_counts=True)
        bt.sync()
        _check_topk(world, kind, b, d, bt, names, qs, 0.0, k, "rows")
    row = bt.counts_host(names.index("staircase_up"))               # the rows are there, and they are the targets
    assert np.array_equal(row[:n], d.targets["staircase_up"])
    for t in _thresholds(d)[1:]:
        for k in ((TIE_K - 1, TIE_K, TIE_K + 1, n) if planes < 32 else (TIE_K,)):
            bt.run_topk(t, k, keep_counts=True)
            bt.sync()
            _check_topk(world, kind, b, d, bt, names, qs, t, k, "rows, threshold")
    s.set_tuning("tile_topk", 0)
    for k in ((1, TIE_K, 128, 513) if planes < 32 else (TIE_K,)):
        bt.run_topk(0.0, k, keep_counts=False)
        bt.sync()
        assert not _no_rows_kept(gpu_lib, bt)                       # (K3 read score rows)
        _check_topk(world, kind, b, d, bt, names, qs, 0.0, k, "tile_topk 0")
    bt.close()
    s.close()


@pytest.mark.parametrize("b,planes,tile_w,waves", [(b, planes, tile_w, waves) for (b, planes) in PLANS
                                                   for (tile_w, waves) in ((4, 1), (4, 4), (64, 1), (64, 4))] + [(10, 32, 4, 4)])
def test_k3_over_the_candidate_pool(gpu_lib, world, b, planes, tile_w, waves):
    """run_topk without rows on `paged`: K2 leaves the k best of every tile, K3 merges the pool.  The pass takes the rows
    instead where tiles x k candidates are larger than the rows they replace (pass.cpp), so which k ran on the pool is
    read from the batch (counts_host refuses), and the smallest ones must have; k = 129 is beyond the tile-level
    selection and must not"""
    kind = "paged"
    d, _ix = world.get(kind, b)
    n = d.num_docs
    names, qs = _batch_of(d, planes)
    s = gpu_lib.Search(d.path)
    s.set_tuning("tile_w", tile_w)
    s.set_tuning("waves", waves)
    bt = gpu_lib.Batch(s)
    bt.set_queries(qs)
    pooled = []
    ks = sorted(set([1, 2, 7, 8, 9, TIE_K - 1, TIE_K, TIE_K + 1, 128, 129] + [k for k in _tie_ks(n) if k <= 128]))
    if planes == 32:
        ks = [1, 2, TIE_K - 1, TIE_K, TIE_K + 1, 128, 129]
    for k in ks:
        for t in ([0.0] if k != TIE_K and (k != 128 or planes == 32) else _thresholds(d)):
            bt.run_topk(t, k, keep_counts=False)
            bt.sync()
            if _no_rows_kept(gpu_lib, bt):
                pooled.append(k)
            _check_topk(world, kind, b, d, bt, names, qs, t, k, "pool")
    assert sorted(set(pooled)) == [k for k in ks if S.pool_takes(k, tile_w, planes, s.local_counts)]
    assert {1, 2, TIE_K} <= set(pooled) and (128 in pooled) == (tile_w == 64 or planes >= 20)
    bt.close()
    s.close()


@pytest.mark.parametrize("b,planes", PLANS)
def test_accumulated_rows(gpu_lib, world, monkeypatch, b, planes):
    """`paged` under a budget that cuts every sub-index into row ranges, every range copied whole: the scan sees partial
    counts, K3 runs per sub-index over the accumulated rows as one tile (pad_out) before the pool merge, and a hits-only
    pass selects with select_rows_kernel -- at the bounds of `exactly`, and at 1 where all scores are equal"""
    monkeypatch.setenv("COBS_GPU_ROW_RANGE_MIN", "48")
    kind = "paged"
    d, _ix = world.get(kind, b)
    n = d.num_docs
    names, qs = _batch_of(d, planes)
    s = gpu_lib.Search(d.path, hbm_budget=256 * 1024)
    s.set_tuning("row_fetch", 0)
    assert s.stream_layout(0)[3] >= 3, s.stream_layout(0)
    bt = gpu_lib.Batch(s)
    bt.set_queries(qs)
    for k in (1, 2, 8, 9, TIE_K - 1, TIE_K, TIE_K + 1, 128):
        for t in ([0.0] if k != TIE_K else _thresholds(d)):
            bt.run_topk(t, k, keep_counts=False)
            bt.sync()
            fits = S.pool_takes(k, 0, planes, s.local_counts)       # (every sub-index is one tile of the pool)
            assert _no_rows_kept(gpu_lib, bt) == fits, k
            _check_topk(world, kind, b, d, bt, names, qs, t, k, "accumulated")
    assert bt.stats()["scan_launches"] >= 3 * len(S.PAGED_SIGS)
    one = S.threshold_for(1, d.terms["all_equal_1"])
    for t in _thresholds(d)[1:] + [one]:
        bt.run_hits(t)
        bt.sync()
        assert _no_rows_kept(gpu_lib, bt)
        _check_topk(world, kind, b, d, bt, names, qs, t, 0, "select_rows")
    assert len(world.want(kind, b, d.queries["all_equal_1"], one, 0)) == n
    assert len(world.want(kind, b, d.queries["all_equal_0"], one, 0)) == 0
    bt.close()
    s.close()


def test_sort_limit(gpu_lib, world):
    """`wide`, 8200 documents: k = 8192 is ordered on the device, k = 8193 by the host; exactly 8191, 8192 and 8193
    documents pass the three bounds of `exactly`; all scores equal and a rising staircase beside it"""
    d, _ix = world.get("wide")
    names, qs = _batch_of(d, 16)
    s = gpu_lib.Search(d.path)
    bt = gpu_lib.Batch(s)
    bt.set_queries(qs)
    bounds = S.wide_targets()[1]
    ts = [0.0] + [S.threshold_for(c, d.terms["exactly"]) for c in bounds]
    for k in (S.SORT_LIMIT - 1, S.SORT_LIMIT, S.SORT_LIMIT + 1, S.WIDE_DOCS):
        for t in ts:
            bt.run_topk(t, k, keep_counts=True)
            bt.sync()
            _check_topk(world, "wide", 0, d, bt, names, qs, t, k, "sort limit")
    for c, passing in zip(bounds, (S.SORT_LIMIT - 1, S.SORT_LIMIT, S.SORT_LIMIT + 1)):
        assert len(S.expected(d.targets["exactly"], c, 0)) == passing
    bt.close()
    s.close()


def _same(offs, hits, i, want):
    seg = hits[int(offs[i]):int(offs[i + 1])]
    got = list(zip(seg["file_no"].tolist(), seg["doc"].tolist(), seg["score"].tolist()))
    return got == want


@pytest.mark.parametrize("kind,b,planes", FILES_PLANS)
def test_full_ranking(gpu_lib, world, monkeypatch, capfd, kind, b, planes):
    """search_arrays(queries, 0, 0) and with a threshold bound, against the oracle; then one work-group per query, segments
    by row length and three segments, pairs instead of packed records, records instead of slot streams, and the host's
    ranking: identical arrays.  A batch that also holds a single-k-mer query (index order) takes the records."""
    monkeypatch.setenv("COBS_GPU_TRACE", "1")
    d, _ix = world.get(kind, b)
    names, qs = _batch_of(d, planes)
    s = gpu_lib.Search(d.path)
    ts = [0.0, _thresholds(d)[2]]
    base = {}
    for t in ts:
        capfd.readouterr()
        offs, hits = s.search_arrays(qs, t, 0)
        err = capfd.readouterr().err
        if t == 0.0 and S.rank_plan(planes)[0] == 1:
            assert "slot streams + score counts" in err
        for i, (nm, q) in enumerate(zip(names, qs)):
            want = world.want(kind, b, q, t, 0)
            assert _same(offs, hits, i, want), (nm, t)
            if nm in d.targets:
                assert want == S.expected(d.targets[nm], S.bound_of(t, d.terms[nm]), 0), (nm, t)
        base[t] = (offs, hits)
    one_pass = S.rank_plan(planes)[0] == 1
    variants = (("rank_segments", (1, 3, 0)), ("rank_pack", (0, 1)), ("rank_slim", (0, 1)), ("device_rank", (0, 1)))
    if not one_pass:             # (rank.cpp: only a single-pass sort is cut into segments, only its lists leave as slot streams)
        variants = (("rank_pack", (0, 1)), ("device_rank", (0, 1)))
    for key, values in variants:
        for v in values:
            s.set_tuning(key, v)
            for t in ts:
                capfd.readouterr()
                offs, hits = s.search_arrays(qs, t, 0)
                err = capfd.readouterr().err
                assert np.array_equal(offs, base[t][0]) and np.array_equal(hits, base[t][1]), (key, v, t)
                if key == "rank_slim" and v == 0 and t == 0.0:
                    assert "4-byte records" in err
                if key == "rank_pack" and v == 0 and t == 0.0:
                    assert "8-byte records" in err
                if key == "device_rank" and v == 0:
                    assert "device ranking" not in err
    one = d.queries["staircase_up"][:S.K]
    mixed, mnames = qs + [one], names + ["one"]
    offs, hits = s.search_arrays(mixed, 0.0, 0)
    for i, (nm, q) in enumerate(zip(mnames, mixed)):
        assert _same(offs, hits, i, world.want(kind, b, q, 0.0, 0)), nm
    seg = hits[int(offs[-2]):int(offs[-1])]
    assert np.array_equal(seg["doc"], np.arange(d.num_docs))            # a single hash: index order
    s.close()


def test_two_levels_of_twelve_bits(gpu_lib, world):
    """the 2^20-term filler: 24 planes, two K3 levels and two ranking passes of 12 bits, over `small` designed for 12-bit
    digits (4095 against 4096)"""
    kind, b = "small", S.WIDTH_24[0]
    d, _ix = world.get(kind, b)
    n = d.num_docs
    names, qs = _batch_of(d, 24)
    s = gpu_lib.Search(d.path)
    bt = gpu_lib.Batch(s)
    bt.set_queries(qs)
    for k in (1, TIE_K, 512, 513, n):
        bt.run_topk(0.0, k, keep_counts=True)
        bt.sync()
        _check_topk(world, kind, b, d, bt, names, qs, 0.0, k, "24 planes")
    bt.close()
    offs, hits = s.search_arrays(qs, 0.0, 0)
    for i, (nm, q) in enumerate(zip(names, qs)):
        assert _same(offs, hits, i, world.want(kind, b, q, 0.0, 0)), nm
    s.close()


def test_three_levels_and_three_passes(gpu_lib, tmp_path, oracle):
    """`coarse` under the 2^24 + 77-term query: 32 planes, three K3 levels (11, 11, 10 bits) and three ranking passes of 11
    bits; scores from 0 to 2^24 + 77 in every top-digit bin, 64 groups of exact ties.  run_topk at k = 1, inside a tie group
    and at k = n; the full ranking.  The expected scores are row multiplicities (tests/test_score_design_cpu.py holds
    them against the oracle)."""
    path, h = S.build_coarse(tmp_path)
    n = S.COARSE_DOCS
    long_q = S.filler(32)
    qs = [long_q, long_q[:5000], long_q[100:9000], long_q[:S.K + 1]]
    scores = [S.coarse_scores(q, h) for q in qs]
    top = S.expected(scores[0], 0, 0)
    group = sum(1 for (_f, _d, sc) in top if sc == top[0][2])
    assert group >= 20 and top[group][2] < top[0][2]
    s = gpu_lib.Search(path)
    bt = gpu_lib.Batch(s)
    bt.set_queries(qs)
    for k in (1, group // 2, group, group + 1, 512, 513, n - 1, n):
        bt.run_topk(0.0, k, keep_counts=True)
        bt.sync()
        for i in range(len(qs)):
            assert bt.hits_host(i, k) == S.expected(scores[i], 0, k), (i, k)
    bt.close()
    offs, hits = s.search_arrays(qs, 0.0, 0)
    for i in range(len(qs)):
        assert _same(offs, hits, i, S.expected(scores[i], 0, 0)), i
    s.set_tuning("device_rank", 0)
    offs2, hits2 = s.search_arrays(qs, 0.0, 0)
    assert np.array_equal(offs, offs2) and np.array_equal(hits, hits2)
    s.close()


def test_a_shard_cuts_a_tie_run(gpu_lib, world):
    """shard 1 of 3 of `small`: its slots begin and end inside the tie runs; the oracle's lists filtered to them, for K3
    and for the ranking"""
    kind, b, planes = "small", 8, 16
    d, _ix = world.get(kind, b)
    names, qs = _batch_of(d, planes)
    sh = gpu_lib.Search(d.path, shard_rank=1, shard_count=3)
    lo, cnt = int(sh.info(0).slot_begin), int(sh.info(0).slot_count)
    run = d.targets["tie_run_last"]
    assert run[lo - 1] == run[lo] == 5 and run[lo + cnt - 1] == run[lo + cnt] == 5        # both cuts inside the run

    def mine(q, t, k):
        full = [x for x in world.want(kind, b, q, t, 0) if lo <= x[1] < lo + cnt]
        return full[:k] if k else full

    bt = gpu_lib.Batch(sh)
    bt.set_queries(qs)
    for k in (1, TIE_K, 511, 512, 513, cnt):
        bt.run_topk(0.0, k, keep_counts=True)
        bt.sync()
        for i, q in enumerate(qs):
            assert bt.hits_host(i, k) == mine(q, 0.0, k), (names[i], k)
    bt.close()
    offs, hits = sh.search_arrays(qs, 0.0, 0)
    for i, q in enumerate(qs):
        assert _same(offs, hits, i, mine(q, 0.0, 0)), names[i]
    sh.close()
