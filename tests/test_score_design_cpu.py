"""No GPU: the conditions of tests/score_design.py's fixtures.  build() meets every target exactly (the oracle's counts equal
the targets on every fixture), every profile has the property its docstring claims under the restated plans, and the numpy
contract expected() equals the oracle's search for every profile, k and threshold the GPU tests use."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import score_design as S


def _lists(ix, q, t, k):
    oi, od, osc = O.search_arrays(ix, q, t, k)
    return list(zip(oi.tolist(), od.tolist(), osc.tolist()))


def test_plans_restate_the_sources():
    assert [S.k3_plan(p) for p in (8, 12, 16, 20, 24, 32)] == [(1, 8, 8), (1, 12, 12), (2, 8, 8), (2, 10, 10), (2, 12, 12), (3, 11, 10)]
    assert [S.rank_plan(p) for p in (8, 12, 16, 20, 24, 32)] == [(1, 8), (1, 12), (2, 8), (2, 10), (2, 12), (3, 11)]
    assert [S.planes_for(T) for T in S.FILLERS.values()] == list(S.FILLERS)
    assert S.wave_per(S.SMALL_DOCS) == 512 and S.wave_per(S.PAGED_DOCS) == 512 and S.wave_per(1920) == 512
    assert S.wave_per(S.WIDE_DOCS) == 2560 and S.wave_per(2049) == 1024 and S.wave_per(1800, 12) == 512
    assert S.digit_edges(12) == [] and S.digit_edges(16) == [8] and S.digit_edges(20) == [10] and S.digit_edges(32) == [10, 11, 21, 22]
    # every designed width is the digit width of the plans it runs under (one-level plans have no digit edge)
    for b, (cap, planes) in S.WIDTHS.items():
        for p in planes:
            assert (S.digit_edges(p) in ([], [b]) or (p == 32 and {b, b + 1} <= set(S.digit_edges(p)))) and cap < 2 ** p
    assert S.digit_edges(24) == [S.WIDTH_24[0]]
    # the candidate pool against the rows it replaces, on `paged` (1920 slots): 5 tiles of width 4, one of width 64
    assert [k for k in (40, 48, 49, 96, 97, 128, 129) if S.pool_takes(k, 4, 8, 1920)] == [40, 48]
    assert [k for k in (40, 48, 49, 96, 97, 128, 129) if S.pool_takes(k, 4, 16, 1920)] == [40, 48, 49, 96]
    assert [k for k in (96, 128, 129) if S.pool_takes(k, 64, 8, 1920)] == [96, 128] and S.pool_takes(128, 4, 20, 1920)
    assert [k for k in (40, 41, 80, 81, 128) if S.pool_takes(k, 0, 8, 1920)] == [40] and S.pool_takes(128, 0, 32, 1920)


@pytest.mark.parametrize("b", [4, 8, 10, 12])
def test_profiles_have_the_properties_they_claim(b):
    n = S.SMALL_DOCS
    cap = S.WIDTH_24[1] if b == 12 else S.WIDTHS[b][0]
    per = S.wave_per(n)
    prof = S.profiles(n, b, cap)
    assert all(len(v) == n and v.min() >= 0 and v.max() <= cap for v in prof.values())
    for nm in ("all_equal_0", "all_equal_1", "all_equal_mid", "all_equal_top"):
        assert len(set(prof[nm].tolist())) == 1
    assert [int(prof[nm][0]) for nm in ("all_equal_0", "all_equal_1", "all_equal_top")] == [0, 1, cap]
    lw = prof["low_wrap"]
    vals = sorted(set(lw.tolist()))
    for lo, hi in zip(vals[0::2], vals[1::2]):
        assert hi == lo + 1 and hi % 2 ** b == 0 and lo % 2 ** b == 2 ** b - 1 and hi >> b == (lo >> b) + 1
    assert (np.diff(lw) != 0).all()                                    # no value is contiguous
    sl = prof["same_low_digit"]
    digits = [0, 1] if b == 12 else [0, 1, 2]                           # (the 12-bit design holds two values: 40, 40 + 4096)
    assert len(set((sl % 2 ** b).tolist())) == 1 and sorted(set((sl >> b).tolist())) == digits and sl.min() % 2 ** b != 0
    for w in range(4):                                                  # every value in every wave range
        assert len(set(sl[w * per:(w + 1) * per].tolist())) == len(digits)
    up, down = prof["staircase_up"], prof["staircase_down"]
    assert (np.diff(up) >= 0).all() and (np.diff(down) <= 0).all() and up[0] == 0 and up[-1] == min(cap, n - 1)
    assert (len(set(up.tolist())) == n) == (cap >= n - 1)
    assert [d for (_f, d, _s) in S.expected(down)] == list(range(n))
    assert sorted(set(prof["sawtooth_3"].tolist())) == [0, 1, 2] and prof["sawtooth_wide"].max() == min(2 ** b, cap, n - 1)
    k = 40
    for where in ("last", "first", "wave3", "spread", "padding"):
        c = min(cap, 2 ** b + 1) if where == "spread" else 5
        s, r0, run = S.tie_run_at_cut(n, k, where, c=c)
        assert np.array_equal(s, prof["tie_run_" + where])
        assert (s > c).sum() == k - 1 and (s < c).sum() + (s == c).sum() == n - (k - 1)
        ties = np.nonzero(s == c)[0]
        if where == "padding":
            assert ties.tolist() == [n - 1]
            assert S.expected(s, 0, k)[-1][1] == n - 1 and S.expected(s, 0, k + 1)[-1][1] == 0
            continue
        if where == "wave3":
            assert set((ties // per).tolist()) == {3} and len(ties) == run == 100 and (np.diff(ties) == 1).all()
            assert S.expected(s, 0, k)[-1] == (0, int(ties[0]), c) and S.expected(s, 0, k + 99)[-1][1] == int(ties[-1])
            continue
        assert len(ties) > 2 * per and ties[0] == r0 and r0 + run - 2 <= ties[-1] <= r0 + run - 1
        waves = set((ties // per).tolist())
        above_waves = set((np.nonzero(s > c)[0] // per).tolist())
        assert {"last": above_waves == {3} and waves == {0, 1, 2, 3} and ties[0] // per == 0,
                "first": above_waves == {0} and 0 not in waves,
                "spread": above_waves == {0, 1, 2, 3} and ties[0] // per == 0}[where]
        # the k-th result is the first tie in document order
        assert S.expected(s, 0, k)[-1] == (0, int(ties[0]), c)
        if where == "last":
            ks = S.tie_ks(k - 1, r0, run, n)
            lasts = [S.expected(s, 0, kk)[-1][1] for kk in ks]
            assert any(d % 8 == 7 for d in lasts) and any(d % 64 == 0 for d in lasts) and any(d % 512 == 0 for d in lasts)
            assert any(d == per - 1 for d in lasts) and any(d == 2 * per for d in lasts)
    ex, bounds = S.exactly(n, k)
    assert np.array_equal(ex, prof["exactly"])
    assert [int((ex >= c).sum()) for c in bounds] == [k - 1, k, k + 1]
    assert set(S.edge_ks(n, per)) >= {1, 2, 511, 512, 513, 1023, 1025, 1535, 1537, n - 1, n, n + 1}
    wt, wb = S.wide_targets()
    assert [int((wt["exactly"] >= c).sum()) for c in wb] == [S.SORT_LIMIT - 1, S.SORT_LIMIT, S.SORT_LIMIT + 1]


def _check_design(d, ks, bounds_of):
    ix = O.Index.open(d.path)
    n = d.num_docs
    for nm, q in d.queries.items():
        got = ix.counts(q)
        assert np.array_equal(got[:n], d.targets[nm]), nm              # every target is met exactly
        P = d.terms[nm]
        for c in [0] + bounds_of(nm):
            t = S.threshold_for(c, P) if c else 0.0
            assert S.bound_of(t, P) == c
            for k in ks:
                assert S.expected(d.targets[nm], c, k) == _lists(ix, q, t, k), (nm, c, k)
    return ix


@pytest.mark.parametrize("b", [4, 8, 10])
@pytest.mark.parametrize("kind", ["small", "paged"])
def test_targets_are_met_and_the_contract_is_the_oracles(tmp_path, oracle, kind, b):
    d = (S.build_small if kind == "small" else S.build_paged)(tmp_path, b)
    n = d.num_docs
    _s, r0, run = S.tie_run_at_cut(n, 40, "last")
    ks = sorted(set(S.edge_ks(n, S.wave_per(n)) + S.tie_ks(39, r0, run, n) + [0, 39, 40, 41, 128, 129]))
    ix = _check_design(d, ks, lambda nm: list(S.exactly(n, 40)[1]) if nm == "exactly" else [1])
    if kind == "paged":                                                 # the padding slots are all ones
        raw = ix.counts(d.queries["all_equal_1"])
        assert len(raw) == 1920 and (raw[n:] == d.terms["all_equal_1"]).all()
    # the scores of any other query follow from row multiplicities: the fillers of this design's plans
    for planes in S.WIDTHS[b][1]:
        if planes <= 20 or kind == "small":                             # (2^24 + 77 terms: one oracle pass, on `small`)
            f = S.filler(planes)
            assert np.array_equal(ix.counts(f)[:n], S.design_scores(d, f)), planes
    # a single-k-mer query stays in index order
    q1 = d.queries["staircase_up"][:S.K]
    assert _lists(ix, q1, 0.0, 0) == S.expected(ix.counts(q1)[:n], 0, 0, by_score=False)


def test_wide_and_the_24_plane_design(tmp_path, oracle):
    d = S.build_wide(tmp_path)
    _check_design(d, [0, 1, S.SORT_LIMIT - 1, S.SORT_LIMIT, S.SORT_LIMIT + 1, S.WIDE_DOCS],
                  lambda nm: list(S.wide_targets()[1]) if nm == "exactly" else [])
    d = S.build_small(tmp_path, 12)
    ix = _check_design(d, [0, 1, 40, 513, S.SMALL_DOCS], lambda nm: [])
    assert np.array_equal(ix.counts(S.filler(24))[:S.SMALL_DOCS], S.design_scores(d, S.filler(24)))
    assert max(d.terms.values()) < S.FILLERS[24]


def test_coarse_scores_are_row_multiplicities(tmp_path, oracle):
    path, h = S.build_coarse(tmp_path)
    assert len(set(h.tolist())) == 64 and h.min() == 0 and h.max() == S.COARSE_SIG
    assert min(np.bincount(h)[np.unique(h)]) >= 20                      # equal row sets: exact ties
    ix = O.Index.open(path)
    q = S.filler(32)
    sc = S.coarse_scores(q, h)
    assert np.array_equal(ix.counts(q)[:S.COARSE_DOCS], sc)             # held once against the oracle
    assert sc.max() == S.FILLERS[32] and sc.min() == 0
    assert set((sc >> 21).tolist()) == set(range(9))                    # every top-digit bin of the 32-plane plan
    for short in (q[:5000], q[100:9000]):
        ssc = S.coarse_scores(short, h)
        assert np.array_equal(ix.counts(short)[:S.COARSE_DOCS], ssc)
        for k in (0, 1, 30, S.COARSE_DOCS):
            assert S.expected(ssc, 0, k) == _lists(ix, short, 0.0, k), k
