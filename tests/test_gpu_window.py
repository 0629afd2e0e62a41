"""GPU: window search (cobs_gpu_search_window / Search.search_window) hit for hit against tests/window_check.py: hits,
hit_offsets and order at thresholds 0, 0.5, 0.8, 1.0 and num_results 0, 1, 5.  Every comparison is exact.

The layouts are those of tests/test_gpu_weighted.py (its builders are used as they are); the windows cross every plane
count of the scan (6, 8, 10, 12) against queries of w - 1, w, w + 1 and 2 w + 3 positions; the structure fixture plants
pieces of the query over an empty matrix -- what it has to reach is asserted on the checker's side
(window_check.structure_conditions, also in tests/test_window_cpu.py) before the GPU is asked."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import cases
from tests import coverage_check as G
from tests import findere_check as F
from tests import invalid_check as I
from tests import positions_check as P
from tests import prevalence_check as V
from tests import window_check as B
from tests.test_gpu_weighted import SRC, _classic, _compact, _edge_queries

pytestmark = pytest.mark.gpu

ZS = (0, 3)
THRESHOLDS = (0.0, 0.5, 0.8, 1.0)
LIMITS = (0, 1, 5)
SEGS = ("1", "13")                                   # COBS_GPU_WINDOW_SEG: the minimum, and no multiple of 8
PLANE_WINDOWS = (1, 2, 7, 8, 9, 63, 64, 255, 256, 1023, 1024, 4095)
LONG_SRC = SRC + O.random_sequence(3000, 78)         # the longest query: 2 * 4095 + 3 positions


def _check(s, files, queries, z, W, mode="error", thresholds=THRESHOLDS, limits=LIMITS, tabs=None):
    """every threshold and limit of one batch against the checker; -> the checker's tables"""
    tabs = tabs or [B.tables(files, q, z, W, mode) for q in queries]
    for t in thresholds:
        for nr in limits:
            offs, hits = s.search_window_arrays(queries, W, t, nr)
            assert offs.dtype == np.uint64 and len(offs) == len(queries) + 1
            rows = hits.tolist()
            for i in range(len(queries)):
                got = rows[int(offs[i]):int(offs[i + 1])]
                want = B.results_from(tabs[i], t, nr)
                assert got == want, (z, W, mode, t, nr, i, len(queries[i]), got[:4], want[:4])
            assert int(offs[-1]) == len(rows)
    return tabs


def _partial(tabs):
    """(query, slot) pairs whose best lies strictly between 0 and min(w, score)"""
    return sum(int(((b > 0) & (b < np.minimum(w, sc)) & (docs >= 0)).sum()) for tab in tabs for (w, b, docs, sc) in tab)


def _sweep(gpu_lib, path, fb, zs=ZS, windows=(1, 31, 64, 200), edges=(1, 2, 63, 64, 65, 129, 1500)):
    s = gpu_lib.Search(path)
    partial = 0
    for z in zs:
        s.set_findere(z)
        qs = _edge_queries(SRC, fb.term_size, z, edges)
        assert [fb.positions(q, z) for q in qs] == list(edges)
        for W in windows:
            partial += _partial(_check(s, [fb], qs, z, W))                  # a batch that mixes the lengths
    s.close()
    return partial


@pytest.mark.parametrize("num_hashes", [1, 3])
@pytest.mark.parametrize("num_docs", [1, 7, 8, 9, 127, 129, 300, 1027])
def test_classic_layouts(gpu_lib, tmp_path, num_docs, num_hashes):
    """the tail bits of the last byte, the tail bytes of the last 16-byte chunk, rows narrower and wider than a wave"""
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), num_docs, 2003, num_hashes, 31, num_docs)
    partial = _sweep(gpu_lib, path, fb)
    assert partial > 0 or num_docs < 16


@pytest.mark.parametrize("sigs", [[1, 2, 65, 4097], [1201, 997, 1500, 1103, 1301, 800]])
@pytest.mark.parametrize("page_size", [2, 8, 16, 200])
def test_compact_layouts(gpu_lib, tmp_path, page_size, sigs):
    """a last sub-index that is partly filled; narrow tiles whose lane groups walk different segments"""
    num_docs = len(sigs) * 8 * page_size - 5 * page_size - 3
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), num_docs, page_size, sigs, 1 if page_size != 8 else 2, 31, page_size)
    assert _sweep(gpu_lib, path, fb, windows=(31, 200)) > 0


def test_padding_slots_with_set_bits_do_not_come_back(gpu_lib, tmp_path):
    """files written WITHOUT masking the padding documents: their slots hold bits (the all-ones rows at least)"""
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), 100, 8, [211, 307, 401], 2, 31, 4, mask=False)
    q = SRC[:200]
    assert V.windows(fb, q, 0)[:, 100:128].any() and V.windows(fb, q, 0)[:, 128:].any()
    _sweep(gpu_lib, path, fb, windows=(31,), edges=(1, 64, 170))
    s = gpu_lib.Search(path)
    offs, hits = s.search_window_arrays([q], 31, 0.0, 0)
    assert len(hits) == 100 and int(hits["doc"].max()) == 99
    s.close()
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 5, 301, 1, 31, 3, mask=False)
    assert V.windows(fb, q, 0)[:, 5:].any()
    _sweep(gpu_lib, path, fb, windows=(31,), edges=(1, 64, 170))


def test_handle_over_two_files_of_different_term_size(gpu_lib, tmp_path):
    """n differs per file, and with it w and the threshold: 500 positions in one file are 511 in the other"""
    pa, fa = _classic(str(tmp_path / "a.cobs_classic"), 300, 2003, 1, 31, 1)
    pb, fb = _compact(str(tmp_path / "b.cobs_compact"), 150, 4, [499, 601, 701, 557, 811], 2, 20, 2)
    s = gpu_lib.Search([pa, pb])
    for z in ZS:
        s.set_findere(z)
        qs = _edge_queries(SRC, 31, z, (1, 2, 64, 65, 500))
        for W in (5, 64, 70, 505):
            tabs = _check(s, [fa, fb], qs, z, W)
        assert tabs[-1][0][0] == 500 and tabs[-1][1][0] == 505              # W = 505: w = n in the first file only
    s.set_findere(0)
    q = _edge_queries(SRC, 31, 0, (500,))[0]
    want = B.results([fa, fb], q, 0, 64, 0.5, 5)
    res = s.search_window(q.decode(), 64, 0.5, 5)                   # the list form of one query ...
    assert [(r.doc_name, r.score) for r in res] == [("doc_%05d" % d, sc) for (_f, d, sc) in want] and res
    both = s.search_window([q, q[:100]], 64, 0.5, 5)                # ... and of several
    assert [(r.doc_name, r.score) for r in both[0]] == [(r.doc_name, r.score) for r in res] and len(both) == 2
    s.close()


def test_wide_row_indices_give_the_same(gpu_lib, tmp_path, monkeypatch):
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), 700, 16, [1201, 997, 1500, 1103, 1301, 800], 1, 31, 3)
    pc, fc = _classic(str(tmp_path / "c.cobs_classic"), 129, 2003, 3, 31, 2)
    got = {}
    for wide in ("0", "1"):
        monkeypatch.setenv("COBS_GPU_IDX64", wide)
        for name, p, f in (("compact", path, fb), ("classic", pc, fc)):
            s = gpu_lib.Search(p)
            for z in ZS:
                s.set_findere(z)
                qs = _edge_queries(SRC, 31, z, (1, 33, 64, 129, 1500))
                for W in (40, 300):
                    _check(s, [f], qs, z, W)
                    got[wide, name, z, W] = s.search_window_arrays(qs, W, 0.5, 0)
            s.close()
    for (wide, name, z, W), (offs, hits) in got.items():
        assert np.array_equal(offs, got["0", name, z, W][0]) and np.array_equal(hits, got["0", name, z, W][1])


@pytest.mark.parametrize("W", PLANE_WINDOWS)
def test_windows_across_the_plane_boundaries(gpu_lib, tmp_path, W):
    """w below and at 2^6, 2^8, 2^10 and the last one the twelve planes hold, against queries of w - 1, w, w + 1 and
    2 w + 3 positions: w = n, the first full window alone, one step, and a walk longer than two windows"""
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 12, 2003, 1, 31, 12, planted={0: 0.9, 5: 0.6, 11: 0.35})
    s = gpu_lib.Search(path)
    ns = tuple(sorted({W - 1, W, W + 1, 2 * W + 3} - {0}))
    assert max(ns) <= 8200
    for z in ZS:
        s.set_findere(z)
        qs = _edge_queries(LONG_SRC, 31, z, ns)
        tabs = _check(s, [fb], qs, z, W)
        assert W < 63 or _partial(tabs) > 0                              # (short windows fill up in the planted documents)
    s.close()


def test_refused_windows(gpu_lib, tmp_path):
    from cobs_amd import _capi
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 12, 2003, 1, 31, 12)
    s = gpu_lib.Search(path)
    for W, status, word in ((0, _capi.ERR_ARG, "at least one"), (4096, _capi.ERR_UNSUPPORTED, "4095"),
                            (1 << 31, _capi.ERR_UNSUPPORTED, "4095")):
        with pytest.raises(gpu_lib.CobsGpuError) as e:
            s.search_window(SRC[:600], W, 0.5)
        assert e.value.status == status and word in str(e.value), (W, str(e.value))
    assert s.window_ms()["passes"] == 0
    _check(s, [fb], [SRC[:600]], 0, 4095, thresholds=(0.5,), limits=(0,))
    s.close()


# ---- the structure fixture: documents that hold pieces of the query over an EMPTY matrix ---------------------------------
def structure(tmp_path, z):
    """-> (path or None, FileBits, query); without a directory nothing is written (tests/test_window_cpu.py)"""
    K, LQ, D = B.STRUCT_K, B.STRUCT_LQ, B.STRUCT_DOCS
    q = SRC[1000:1000 + LQ]
    sig = 1000003
    m = np.zeros((sig, (D + 7) // 8), dtype=np.uint8)
    for d, pieces in B.structure_pieces(q, z).items():
        for text in pieces:
            cases.plant([m], [sig], 0, text, {d: 1.0}, K, 1, 1)
    path = None
    if tmp_path is not None:
        from oracle import construct as Kc
        path = str(tmp_path / ("s%d.cobs_classic" % z))
        Kc.write_classic(path, K, 1, ["doc_%05d" % i for i in range(D)], sig, 1, m)
    return path, F.FileBits(K, 1, 1, [m], D), q


@pytest.mark.parametrize("seg", ("",) + SEGS)
@pytest.mark.parametrize("z", ZS)
def test_structure_fixture(gpu_lib, tmp_path, monkeypatch, z, seg):
    if seg:
        monkeypatch.setenv("COBS_GPU_WINDOW_SEG", seg)
    else:
        monkeypatch.delenv("COBS_GPU_WINDOW_SEG", raising=False)
    path, fb, q = structure(tmp_path, z)
    B.structure_conditions(V.windows(fb, q, z), fb.doc_of_slot())
    s = gpu_lib.Search(path, findere=z)
    queries = [q, q[:200], q[100:], q[380:380 + 150]]
    for W in (B.STRUCT_W, 50, 64, 600):
        _check(s, [fb], queries, z, W)
    # what the call is for: at 0.8 the plain search finds the whole copy alone, the window search every document that
    # holds 80 of some 100 positions
    offs, hits = s.search_window_arrays([q], B.STRUCT_W, 0.8, 0)
    plain = {d for (_f, d, _sc) in s.search_hits([q], 0.8, 0)[0]}
    assert plain == {3} and set(hits["doc"].tolist()) == {0, 1, 3, 8, 9, 10, 11, 14, 16}
    s.close()


@pytest.mark.parametrize("seg", SEGS)
def test_forced_segments_on_a_wide_tile(gpu_lib, tmp_path, monkeypatch, seg):
    """a tile as wide as a wave has four lane groups, a narrow one 256: both merge paths"""
    monkeypatch.setenv("COBS_GPU_WINDOW_SEG", seg)
    path, fb = _classic(str(tmp_path / "w.cobs_classic"), 9000, 499, 1, 31, 4)
    assert _sweep(gpu_lib, path, fb, zs=(1,), windows=(31, 100), edges=(1, 31, 32, 33, 129, 1500)) > 0


def test_miss_and_skip_agree_and_error_names_the_query(gpu_lib, tmp_path):
    from cobs_amd import _capi
    path, fb = _compact(str(tmp_path / "n.cobs_compact"), 300, 8, [901, 1003, 777, 1300, 950], 2, 31, 9)
    base = SRC[40:40 + 260]
    qs = [I.with_n(base, [o]) for o in (0, 130, len(base) - 1)] + [base, I.with_n(base, [7, 200]), b"N" * 100]
    got = {}
    for mode in I.MODES:
        s = gpu_lib.Search(path, invalid_bases=mode)
        for z in ZS:
            s.set_findere(z)
            for W in (40, 250):
                tabs = _check(s, [fb], qs, z, W, mode)
                got[mode, z, W] = [s.search_window_arrays(qs, W, t, 0) for t in (0.0, 0.5)]
                # an N in the middle (query 1) unsets the positions whose characters hold it: no best grows; with w = n
                # (W = 250) every document that held one of them shrinks, a short window may lie elsewhere
                clean = B.tables([fb], base, z, W, mode)[0][1]
                assert (tabs[1][0][1] <= clean).all() and (W < 250 or (tabs[1][0][1] < clean).any())
                o = got[mode, z, W][1][0]
                assert int(o[6]) == int(o[5])                           # all N: nothing returned above a threshold
                assert not got[mode, z, W][0][1]["score"][int(got[mode, z, W][0][0][5]):].any()
        s.close()
    for z in ZS:
        for W in (40, 250):
            for a, b in zip(got["miss", z, W], got["skip", z, W]):
                assert all(np.array_equal(x, y) for x, y in zip(a, b))
    s = gpu_lib.Search(path, findere=1)
    good = [SRC[:100], SRC[200:340], SRC[400:480]]
    bad_base = [good[0], good[1], good[2][:40] + b"N" + good[2][41:]]
    st, bad, offs, hits, msg = _raw_call(s, bad_base, 30, 0.5, 0, 1000)
    assert st == _capi.ERR_INVALID_BASE and bad == 2 and "(query 2)" in msg
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.search_window(bad_base[2], 30, 0.5)
    assert e.value.status == _capi.ERR_INVALID_BASE
    _check(s, [fb], good, 1, 30, thresholds=(0.5,), limits=(0,))     # the handle still answers
    s.close()


@pytest.mark.parametrize("z", ZS)
def test_identities_with_hit_positions(gpu_lib, tmp_path, z):
    """for every hit of a window search, best_window over its hit_positions words is its score; with W >= n the score is
    the popcount of the words; W = 1 scores 1 where a position is set; the score does not fall when W grows"""
    pa, fa = _classic(str(tmp_path / "a.cobs_classic"), 300, 2003, 1, 31, 1)
    pb, fb = _compact(str(tmp_path / "b.cobs_compact"), 150, 4, [499, 601, 701, 557, 811], 2, 20, 2)
    s = gpu_lib.Search([pa, pb], findere=z)
    queries = _edge_queries(SRC, 31, z, (1, 64, 65, 700))
    ks = (31, 20)
    prev = None
    for W in (1, 20, 64, 300, 4095):
        offs, hits = s.search_window_arrays(queries, W, 0.0, 0)         # every real document, whatever it reaches
        assert len(hits) == 4 * 450
        bo, bits = s.hit_positions(queries, offs, hits)
        key = np.lexsort((hits["doc"], hits["file_no"], np.repeat(np.arange(4), 450)))
        by_doc = hits["score"][key].astype(np.int64)
        for i, q in enumerate(queries):
            for h in range(int(offs[i]), int(offs[i + 1])):                 # every returned hit
                k = ks[int(hits["file_no"][h])]
                n = len(q) - k + 1 - z
                words = bits[int(bo[h]):int(bo[h + 1])]
                best, start = gpu_lib.best_window(words, n, W)
                assert best == int(hits["score"][h]), (W, i, h)
                assert (best, start) == B.best_window(P.unpack(words, n), W)
                pop = P.popcount(words)
                assert best <= min(W, n, pop)
                if W >= n:
                    assert best == pop
                if W == 1:
                    assert best == int(pop > 0)
        assert prev is None or (by_doc >= prev).all()
        prev = by_doc
    assert len(set(hits["score"].tolist())) > 8
    s.close()


def test_several_device_passes_and_pool_overflow(gpu_lib, tmp_path):
    """the workspace limit cuts the call into passes, a small pool overflows and its pass is scanned again: same results"""
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), 700, 16, [1201, 997, 1500, 1103, 1301, 800], 1, 31, 3)
    rng = np.random.default_rng(41)
    queries = []
    for _ in range(39):
        ln = int(rng.integers(50, 151))
        o = int(rng.integers(0, len(SRC) - ln))
        queries.append(SRC[o:o + ln])
    queries.append(SRC[:1030])
    W = 40
    s = gpu_lib.Search(path, findere=3)
    zero = {"hash_ms": 0.0, "scan_ms": 0.0, "passes": 0}
    assert s.window_ms() == zero
    one = [s.search_window_arrays(queries, W, t, 0) for t in (0.0, 0.5)]
    t1 = s.window_ms()
    assert t1["passes"] == 2 and t1["hash_ms"] > 0 and t1["scan_ms"] > 0 and s.window_ms() == zero
    s.set_tuning("pass_bytes", 30000)
    many = [s.search_window_arrays(queries, W, t, 0) for t in (0.0, 0.5)]
    assert s.window_ms()["passes"] >= 6
    s.set_tuning("pass_bytes", 0)
    s.set_tuning("hit_cap", 7)                                      # the first pool holds 7 records
    small = [s.search_window_arrays(queries, W, t, 0) for t in (0.0, 0.5)]
    s.set_tuning("pass_bytes", 30000)
    both = [s.search_window_arrays(queries, W, t, 0) for t in (0.0, 0.5)]
    s.set_tuning("pass_bytes", 0)
    s.set_tuning("hit_cap", 0)
    for other in (many, small, both):
        for a, b in zip(one, other):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert len(one[0][1]) == 40 * 700 and 0 < len(one[1][1]) < 40 * 700
    _check(s, [fb], queries, 3, W)
    # searches before and after on the same handle are not disturbed (the call shares their workspace)
    assert s.search_hits(queries[:5], 0.0, 3) == [F.results([fb], q, 3, 0.0, 3) for q in queries[:5]]
    s.close()


def _raw_call(s, queries, W, threshold, num_results, cap, null_offsets=False):
    from cobs_amd import _capi
    lib = _capi.load()
    nq = len(queries)
    arr = (C.c_char_p * max(nq, 1))(*queries)
    lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in queries])
    hits = np.zeros(max(cap, 1), dtype=s.HIT_DTYPE)
    offs = np.full(nq + 1, 0xFFFF, dtype=np.uint64)
    bad = C.c_size_t(12345)
    st = lib.cobs_gpu_search_window(s._h, arr, lens, nq, W, threshold, num_results,
                                    C.cast(hits.ctypes.data, C.POINTER(_capi.Hit)) if cap else None, cap,
                                    None if null_offsets else C.cast(offs.ctypes.data, C.POINTER(C.c_size_t)), C.byref(bad))
    return st, bad.value, offs, hits, lib.cobs_gpu_last_error().decode()


def test_refusals_come_back_before_any_device_work(gpu_lib, tmp_path):
    from cobs_amd import _capi
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 300, 2003, 1, 31, 1)
    s = gpu_lib.Search(path, findere=3)
    good = [SRC[:100], SRC[200:340], SRC[400:480]]
    s.window_ms()
    lib = _capi.load()
    # NULL arguments
    assert lib.cobs_gpu_search_window(s._h, None, None, 3, 30, 0.5, 0, None, 0, None, None) == _capi.ERR_ARG
    assert _raw_call(s, good, 30, 0.5, 0, 100, null_offsets=True)[0] == _capi.ERR_ARG
    offs = (C.c_size_t * 4)()
    assert lib.cobs_gpu_search_window(s._h, None, None, 3, 30, 0.5, 0, None, 0, offs, None) == _capi.ERR_ARG
    arr = (C.c_char_p * 3)(*good)
    lens = (C.c_size_t * 3)(*[len(q) for q in good])
    assert lib.cobs_gpu_search_window(s._h, arr, lens, 3, 30, 0.5, 0, None, 5, offs, None) == _capi.ERR_ARG      # cap without hits
    # the window
    assert _raw_call(s, good, 0, 0.5, 0, 100)[0] == _capi.ERR_ARG
    st, bad, offs, hits, msg = _raw_call(s, good, 4096, 0.5, 0, 100)
    assert st == _capi.ERR_UNSUPPORTED and "4095" in msg
    # a query that is too short names the query
    st, bad, offs, hits, msg = _raw_call(s, [good[0], good[1], SRC[:31 + 2]], 30, 0.5, 0, 100)
    assert st == _capi.ERR_QUERY_TOO_SHORT and bad == 2 and str(31 + 3) in msg and "(query 2)" in msg
    # 2^30 characters are one too many for the walk's 32-bit positions: refused on the length alone, before the text
    # is looked at (the buffer behind the pointer is a short one)
    arr2 = (C.c_char_p * 2)(good[0], good[1])
    lens2 = (C.c_size_t * 2)(len(good[0]), 1 << 30)
    offs3 = (C.c_size_t * 3)()
    bad2 = C.c_size_t(12345)
    st = lib.cobs_gpu_search_window(s._h, arr2, lens2, 2, 30, 0.5, 0, None, 0, offs3, C.byref(bad2))
    msg = lib.cobs_gpu_last_error().decode()
    assert st == _capi.ERR_QUERY_TOO_LONG and bad2.value == 1 and "(query 1)" in msg and str(1 << 30) in msg and "32-bit" in msg
    assert s.window_ms()["passes"] == 0                             # none of these reached the device
    # a result buffer that is too small: the needed size from the one scan that ran, then success
    want = [B.results([fb], q, 3, 30, 0.5, 0) for q in good]
    need = sum(len(x) for x in want)
    assert need > 3
    st, bad, offs, hits, msg = _raw_call(s, good, 30, 0.5, 0, 0)
    assert st == _capi.ERR_CAPACITY and int(offs[3]) == need and [int(offs[i + 1]) - int(offs[i]) for i in range(3)] == [len(x) for x in want]
    st, bad, offs, hits, msg = _raw_call(s, good, 30, 0.5, 0, need - 1)
    assert st == _capi.ERR_CAPACITY and int(offs[3]) == need
    st, bad, offs, hits, msg = _raw_call(s, good, 30, 0.5, 0, need)
    assert st == _capi.OK and hits[:need].tolist() == [h for x in want for h in x], msg
    s.close()
    # a handle with an HBM budget, one shard of several, the device list
    s = gpu_lib.Search(path, hbm_budget=256 << 20)
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.search_window(good[0], 30, 0.5)
    assert e.value.status == _capi.ERR_UNSUPPORTED and "HBM budget" in str(e.value) and s.window_ms()["passes"] == 0
    s.close()
    s = gpu_lib.Search(path, shard_rank=0, shard_count=2)
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.search_window(good[0], 30, 0.5)
    assert e.value.status == _capi.ERR_UNSUPPORTED and "shard" in str(e.value) and s.window_ms()["passes"] == 0
    s.close()
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        gpu_lib.MultiSearch.search_window_arrays(gpu_lib.MultiSearch.__new__(gpu_lib.MultiSearch), good, 30)
    assert e.value.status == _capi.ERR_UNSUPPORTED


def test_call_sequence_on_one_handle(gpu_lib, tmp_path):
    """window -> coverage -> search -> window on ONE handle, z and the invalid-bases policy changed in between: every
    result is that of a fresh handle (the calls share the scratch batch and K1's tables)"""
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), 300, 8, [901, 1003, 777, 1300, 950], 2, 31, 9)
    clean = [SRC[:100], SRC[200:460], SRC[400:480]]
    dirty = [clean[0], I.with_n(clean[1], [130]), clean[2]]

    def window(s, qs, W):
        offs, hits = s.search_window_arrays(qs, W, 0.5, 0)
        return offs.tolist(), hits.tolist()

    def coverage(s, qs):
        offs, hits = s.search_coverage_arrays(qs, 0.5, 0)
        return offs.tolist(), hits.tolist()

    steps = [("window", 0, "error", clean, 40), ("coverage", 3, "error", clean, 0), ("search", 3, "miss", dirty, 0),
             ("window", 3, "miss", dirty, 200), ("window", 0, "skip", dirty, 40), ("coverage", 0, "skip", dirty, 0),
             ("window", 1, "error", clean, 40)]

    def run(s, step):
        kind, z, mode, qs, W = step
        if kind == "window":
            return window(s, qs, W)
        if kind == "coverage":
            return coverage(s, qs)
        return s.search_hits(qs, 0.5, 0)

    one = gpu_lib.Search(path)
    for step in steps:
        kind, z, mode, qs, W = step
        one.set_findere(z)
        one.invalid_bases = mode
        got = run(one, step)
        fresh = gpu_lib.Search(path, findere=z, invalid_bases=mode)
        assert got == run(fresh, step), step[:3]
        fresh.close()
        if kind == "window":
            want = [B.results([fb], q, z, W, 0.5, 0, mode) for q in qs]
            assert [got[1][got[0][i]:got[0][i + 1]] for i in range(len(qs))] == want and any(want)
        elif kind == "coverage":
            assert [got[1][got[0][i]:got[0][i + 1]] for i in range(len(qs))] == [G.results([fb], q, z, 0.5, 0, mode) for q in qs]
    one.close()
