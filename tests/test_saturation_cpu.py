"""No GPU: the conditions of tests/saturation.py's fixtures, on the checkers' side.  For every case the numpy checkers can
restate (T <= 4096, n <= 274 for the weighted search) the checker agrees exactly with the analytic values the GPU tests
use, the top value is reached by a full document and the value just below it by a near-full one, and every position of
the weighted fixture weighs 15."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import coverage_check as CC
from tests import findere_check as F
from tests import saturation as S
from tests import weighted_check as W
from tests import window_check as B

SMALL_T = [T for T in S.PLAIN_T if T <= S.SMALL_T]


@pytest.fixture(scope="module")
def world(tmp_path_factory, oracle):
    return S.build(tmp_path_factory.mktemp("saturation_cpu"), S.SMALL_INDEXES + ("narrow_h3", "narrow_k248"))


def test_boundary_tables_restate_the_plane_tables():
    assert [S.planes_for(T) for T in S.PLAIN_T + S.PLAIN_T_HUGE] == [S.PLAIN_PLANES[T] for T in S.PLAIN_T + S.PLAIN_T_HUGE]
    for lo, hi in zip((S.PLAIN_T + S.PLAIN_T_HUGE)[0::2], (S.PLAIN_T + S.PLAIN_T_HUGE)[1::2]):
        assert hi == lo + 1 and S.planes_for(lo) < S.planes_for(hi)            # every pair straddles a plane count
    assert [S.score_bytes(T) for T in (255, 256, 65535, 65536)] == [1, 2, 2, 4]

    def weighted_planes(n):
        return [p for p in (8, 12, 14, 16, 20) if 15 * n < 2 ** p][0]
    assert [weighted_planes(n) for n in S.WEIGHTED_N] == [8, 12, 12, 14, 14, 16, 16, 20, 20] and 15 * 69906 >= 2 ** 20
    assert all(2 ** p - 1 in S.COVERAGE_L for p in (8, 12, 16, 20)) and all(2 ** p in S.COVERAGE_L for p in (8, 12, 16))
    assert all(2 ** p - 1 in S.WINDOW_W for p in (6, 8, 10, 12)) and all(2 ** p in S.WINDOW_W for p in (6, 8, 10))
    assert [m * S.GROUP_TERMS for m in S.GROUP_MEMBERS] == [510, 2 ** 16 - 1, 65790]


@pytest.mark.parametrize("name", S.SMALL_INDEXES + ("narrow_h3",))
def test_plain_and_findere_scores(world, name):
    ix = world[name]
    docs = ix.fb.doc_of_slot()
    real = docs >= 0
    oix = O.Index.open(ix.path)
    assert ix.padding_has_bits() == (name == "narrow")
    assert len(ix.full) == (4 if ix.num_docs == 12 else 6)
    for T in SMALL_T:
        q = ix.query(T)
        for z in (0, S.FINDERE_Z):
            P = T - z
            row = ix.fb.scores(q, z)
            want = S.plain_special(ix, T, z)
            assert {s: int(row[s]) for s in want} == want, (name, T, z)
            assert want[ix.near0] == P - 1 and int(row[real].max()) == P       # the top, and the value just below it
            assert sorted(np.nonzero(real & (row == P))[0].tolist()) == [s for s in sorted(want) if want[s] == P]
            if z == 0:
                assert np.array_equal(oix.counts(q), row), (name, T)
            for t, bound in zip(S.thresholds(P), (P, P - 1)):
                assert F.results([ix.fb], q, z, t, 0) == S.hits_of(want, bound) == S.hits_of_row(row, docs, bound), (name, T, z, t)
        for i, qq in enumerate(S.mixed_batch(ix, T)):
            assert ix.fb.positions(qq, 0) == (15, T, 100, 16)[i]


@pytest.mark.parametrize("name", S.SMALL_INDEXES + ("narrow_k248",))
def test_coverage(world, name):
    ix = world[name]
    zs = (7,) if name == "narrow_k248" else (0, S.FINDERE_Z)
    for L in [L for L in S.COVERAGE_L if L <= S.SMALL_T and (name != "narrow_k248" or L >= 4095)]:
        for z in zs:
            q = ix.src[:L]
            (length, cov, docs, _set), = CC.tables([ix.fb], q, z)
            want = S.coverage_special(ix, L, z)
            assert length == L and {s: int(cov[s]) for s in want} == want, (name, L, z)
            assert int(cov[docs >= 0].max()) == L and want[ix.near0] == L - 1


@pytest.mark.parametrize("name", S.SMALL_INDEXES)
def test_windows(world, name):
    ix = world[name]
    below = 0
    for Wd in S.WINDOW_W:
        for n in S.window_positions(Wd):
            if n > S.SMALL_T:
                continue
            (w, best, docs, _set), = B.tables([ix.fb], ix.query(n), 0, Wd)
            want = S.window_special(ix, Wd, n)
            assert w == min(Wd, n) and {s: int(best[s]) for s in want} == want, (name, Wd, n)
            assert int(best[docs >= 0].max()) == w
            below += (w - 1) in (want[ix.near0], want[ix.near_mid])
    assert below >= 3 * len(S.WINDOW_W) - 3              # n = W - 1, W and W + 1 show the value below the top


def test_every_weighted_position_weighs_15(tmp_path, oracle):
    path, fb = S.weighted_file(tmp_path)
    assert W.idf_weight(S.WEIGHTED_DOCS, 1) == 15
    for n in [n for n in S.WEIGHTED_N if n <= S.WEIGHTED_CHECKED]:
        for z in (0, S.FINDERE_Z):
            q = S.weighted_query(n, z)
            (total, sc, docs, w), = W.tables([fb], q, z)
            assert len(w) == n and (w == 15).all() and total == 15 * n
            assert int(sc[S.WEIGHTED_FULL]) == 15 * n and int(sc.sum()) == 15 * n
            for t in (0.0, 1.0, S.thresholds(15 * n)[1]):
                assert W.results_from([(total, sc, docs, w)], t, 0) == S.weighted_expected(n, t)[1], (n, z, t)
