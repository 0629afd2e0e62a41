"""GPU: the 64-bit row-index table (row_table.hpp: IdxT = u64) on indexes of a few kilobytes.  plan_part selects the wide
table only for a sub-index of 2^32 - 1 rows or more; COBS_GPU_IDX64=1, read when a handle is opened, forces it, so that
the u64 instantiations of K1, K2, the presence, prevalence and weighted kernels and the out-of-core kernels run here.

Every index is opened twice, normally and under COBS_GPU_IDX64=1.  The two handles must agree bit for bit, and the forced
handle's results also go through the numpy checkers (two equal wrong answers cannot pass).  That the forced handle really
keeps a wide table is read off the pass count of a prevalence call: the rule that cuts a call into device passes charges a
wide entry twice."""
import numpy as np
import pytest

from tests import cases
from tests import findere_check as F
from tests import positions_check as P
from tests import prevalence_check as V
from tests import test_gpu_weighted as TW        # its index builders: graded row densities, planted documents
from tests import weighted_check as W

pytestmark = pytest.mark.gpu

K = 31
ZS = (0, 3)
# position counts: k + z characters exactly | one 8-term block less one, exactly, plus one | a 64-position word less one,
# plus one (which also crosses the block edge 64 | 65) | several words
EDGES = (1, 7, 8, 9, 63, 65, 130, 300)
SEARCHES = ((0.0, 0), (0.5, 0), (0.0, 3), (0.5, 3))


def _build(tmp_path, kind):
    if kind.startswith("compact"):
        page_size = int(kind[len("compact"):])
        sigs = [1, 2, 65, 4097]
        num_docs = len(sigs) * 8 * page_size - 5 * page_size - 3        # the last sub-index partly filled
        return TW._compact(str(tmp_path / "w.cobs_compact"), num_docs, page_size, sigs, 1, K, page_size)
    return TW._classic(str(tmp_path / "w.cobs_classic"), 129, 2003, int(kind[len("classic_h"):]), K, 129)


def _open_pair(gpu_lib, monkeypatch, path, **kw):
    narrow = gpu_lib.Search(path, **kw)
    monkeypatch.setenv("COBS_GPU_IDX64", "1")
    wide = gpu_lib.Search(path, **kw)
    monkeypatch.delenv("COBS_GPU_IDX64")
    return narrow, wide


@pytest.mark.parametrize("kind", ["compact2", "compact16", "classic_h1", "classic_h3"])
def test_wide_equals_narrow_and_the_checkers(gpu_lib, monkeypatch, tmp_path, kind):
    path, fb = _build(tmp_path, kind)
    narrow, wide = _open_pair(gpu_lib, monkeypatch, path)
    for z in ZS:
        narrow.set_findere(z)
        wide.set_findere(z)
        qs = TW._edge_queries(TW.SRC, K, z, EDGES)
        assert [fb.positions(q, z) for q in qs] == list(EDGES) and len(qs[0]) == K + z
        # search
        for t, lim in SEARCHES:
            o0, h0 = narrow.search_arrays(qs, t, lim)
            o1, h1 = wide.search_arrays(qs, t, lim)
            assert np.array_equal(o0, o1) and np.array_equal(h0, h1), (kind, z, t, lim)
            rows = h1.tolist()
            got = [rows[int(o1[i]):int(o1[i + 1])] for i in range(len(qs))]
            assert got == [F.results([fb], q, z, t, lim) for q in qs], (kind, z, t, lim)
        # hit positions over the thresholded hits
        offs, hits = wide.search_arrays(qs, 0.5, 0)
        assert len(hits) > 0
        bo0, bits0 = narrow.hit_positions(qs, offs, hits)
        bo1, bits1 = wide.hit_positions(qs, offs, hits)
        assert np.array_equal(bo0, bo1) and np.array_equal(bits0, bits1), (kind, z)
        rows = hits.tolist()
        for qi, q in enumerate(qs):
            for i in range(int(offs[qi]), int(offs[qi + 1])):
                f, d, sc = rows[i]
                words = bits1[int(bo1[i]):int(bo1[i + 1])]
                assert np.array_equal(words, P.pack(P.positions([fb], q, z, f, d))) and P.popcount(words) == sc, (kind, z, qi, d)
        # prevalence
        po0, pc0 = narrow.prevalence_arrays(qs)
        po1, pc1 = wide.prevalence_arrays(qs)
        assert np.array_equal(po0, po1) and np.array_equal(pc0, pc1), (kind, z)
        want_offs, want = V.segments([fb], qs, z)
        assert np.array_equal(po1, want_offs) and np.array_equal(pc1, want), (kind, z)
        # weighted search: hits, W and offsets
        tabs = [W.tables([fb], q, z, "error") for q in qs]
        want_total = np.array([[t[0] for t in tab] for tab in tabs], dtype=np.uint64).reshape(len(qs), 1)
        for t, lim in SEARCHES:
            wo0, wh0, wt0 = narrow.search_weighted_arrays(qs, t, lim)
            wo1, wh1, wt1 = wide.search_weighted_arrays(qs, t, lim)
            assert np.array_equal(wo0, wo1) and np.array_equal(wh0, wh1) and np.array_equal(wt0, wt1), (kind, z, t, lim)
            assert np.array_equal(wt1, want_total), (kind, z, t, lim)
            rows = wh1.tolist()
            for i in range(len(qs)):
                assert rows[int(wo1[i]):int(wo1[i + 1])] == W.results_from(tabs[i], t, lim), (kind, z, t, lim, i)
    narrow.close()
    wide.close()


def test_the_forced_handle_keeps_a_wide_table(gpu_lib, monkeypatch, tmp_path):
    """the passes of a call are cut by the bytes of K1's tables, 4 per entry, 8 in a wide table: under a small workspace
    limit the forced handle needs more passes for the same queries"""
    path, fb = _build(tmp_path, "compact16")
    rng = np.random.default_rng(41)
    queries = []
    for _ in range(60):
        ln = int(rng.integers(80, 151))
        o = int(rng.integers(0, len(TW.SRC) - ln))
        queries.append(TW.SRC[o:o + ln])
    narrow, wide = _open_pair(gpu_lib, monkeypatch, path)
    want_offs, want = V.segments([fb], queries, 0)
    passes = []
    for s in (narrow, wide):
        s.set_tuning("pass_bytes", 30000)
        s.prevalence_ms()
        offs, counts = s.prevalence_arrays(queries)
        passes.append(s.prevalence_ms()["passes"])
        s.set_tuning("pass_bytes", 0)
        assert np.array_equal(offs, want_offs) and np.array_equal(counts, want)
        s.close()
    print("prevalence passes: narrow %d, wide %d" % tuple(passes))
    assert passes[0] >= 3 and passes[1] > passes[0], passes


def test_streamed_handle_takes_the_wide_table(gpu_lib, monkeypatch, oracle, tmp_path):
    """an index larger than its HBM budget: the fetch kernels that rewrite K1's table take either width (the compact
    second table of a row-range unit is 32-bit only and is not built for a wide table: such a unit walks every term)"""
    D, S = 4000, 3001                                # 500-byte rows, 1.5 MB
    q_long = oracle.random_sequence(1030, 8)
    path = cases.make_classic(cases.tmp(tmp_path, "st.cobs_classic"), D, S, 1, K, 1, 0.3, 7, planted={5: 1.0, 3999: 0.9},
                              query=q_long)
    ix = oracle.Index.open(path)
    queries = [q_long, q_long[:100], q_long[200:231]]
    narrow, wide = _open_pair(gpu_lib, monkeypatch, path, hbm_budget=600 * 1024)
    for t, lim in ((0.0, 0), (0.4, 0), (0.4, 3)):
        got0, got1 = narrow.search_hits(queries, t, lim), wide.search_hits(queries, t, lim)
        assert got0 == got1, (t, lim)
        for q, g in zip(queries, got1):
            assert g == cases.oracle_results([ix], q, t, lim), (t, lim)
    narrow.close()
    wide.close()
