"""GPU: coverage search (cobs_gpu_search_coverage / Search.search_coverage) hit for hit against tests/coverage_check.py:
hits, hit_offsets and order at thresholds 0, 0.3, 0.8, 1.0 and num_results 0, 1, 5.  Every comparison is exact.

The layouts are those of tests/test_gpu_weighted.py (its builders are used as they are); the structure fixture plants
mutated copies of the source so that the queries reach isolated set positions, overlapping ones, gaps of span - 1, span
and span + 1 positions, a run that ends at the last position and runs that cross every forced segment boundary --
asserted on the checker's side before the GPU is asked."""
import ctypes as C

import numpy as np
import pytest

from tests import cases
from tests import coverage_check as G
from tests import findere_check as F
from tests import invalid_check as I
from tests import prevalence_check as V
from tests.test_gpu_weighted import SRC, _classic, _compact, _edge_queries

pytestmark = pytest.mark.gpu

ZS = (0, 1, 3, 7)
THRESHOLDS = (0.0, 0.3, 0.8, 1.0)
LIMITS = (0, 1, 5)
SEGS = ("1", "13")                                   # COBS_GPU_COVERAGE_SEG: the minimum, and no multiple of 8


def _edges(span):
    return tuple(sorted({1, 2, span - 1, span, span + 1, 63, 64, 65, 128, 129, 1500, 5000} - {0}))


def _check(s, files, queries, z, mode="error", thresholds=THRESHOLDS, limits=LIMITS, tabs=None):
    """every threshold and limit of one batch against the checker; -> the checker's tables"""
    tabs = tabs or [G.tables(files, q, z, mode) for q in queries]
    for t in thresholds:
        for nr in limits:
            offs, hits = s.search_coverage_arrays(queries, t, nr)
            assert offs.dtype == np.uint64 and len(offs) == len(queries) + 1
            rows = hits.tolist()
            for i in range(len(queries)):
                got = rows[int(offs[i]):int(offs[i + 1])]
                want = G.results_from(tabs[i], t, nr)
                assert got == want, (z, mode, t, nr, i, len(queries[i]), got[:4], want[:4])
            assert int(offs[-1]) == len(rows)
    return tabs


def _sweep(gpu_lib, path, fb, zs=ZS, edges=None, alone=True):
    s = gpu_lib.Search(path)
    partial = 0
    for z in zs:
        s.set_findere(z)
        ns = edges or _edges(fb.term_size + z)
        qs = _edge_queries(SRC, fb.term_size, z, ns)
        assert [fb.positions(q, z) for q in qs] == list(ns)
        tabs = _check(s, [fb], qs, z)                                           # a batch that mixes the lengths
        if alone:
            for q, tab in zip(qs, tabs):                                        # ... and every position count alone
                _check(s, [fb], [q], z, thresholds=(0.0, 0.8), limits=(0,), tabs=[tab])
        for q, tab in zip(qs, tabs):
            length, cov, docs, _s = tab[0]
            partial += int(((cov > 0) & (cov < length) & (docs >= 0)).sum())
    s.close()
    return partial


@pytest.mark.parametrize("num_hashes", [1, 3])
@pytest.mark.parametrize("num_docs", [1, 7, 8, 9, 127, 129, 300, 1027])
def test_classic_layouts(gpu_lib, tmp_path, num_docs, num_hashes):
    """the tail bits of the last byte, the tail bytes of the last 16-byte chunk, rows narrower and wider than a wave"""
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), num_docs, 2003, num_hashes, 31, num_docs)
    partial = _sweep(gpu_lib, path, fb, alone=num_hashes == 1)
    # condition of the test: with the three planted documents some coverage lies strictly between 0 and L
    assert partial > 0 or num_docs < 16


@pytest.mark.parametrize("sigs", [[1, 2, 65, 4097], [1201, 997, 1500, 1103, 1301, 800]])
@pytest.mark.parametrize("page_size", [2, 8, 16, 200])
def test_compact_layouts(gpu_lib, tmp_path, page_size, sigs):
    """a last sub-index that is partly filled; narrow tiles whose lane groups walk different segments"""
    num_docs = len(sigs) * 8 * page_size - 5 * page_size - 3
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), num_docs, page_size, sigs, 1 if page_size != 8 else 2, 31, page_size)
    assert _sweep(gpu_lib, path, fb, zs=(0, 3), alone=False) > 0


def test_padding_slots_with_set_bits_do_not_come_back(gpu_lib, tmp_path):
    """files written WITHOUT masking the padding documents: their slots hold bits (the all-ones rows at least)"""
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), 100, 8, [211, 307, 401], 2, 31, 4, mask=False)
    q = SRC[:200]
    assert V.windows(fb, q, 0)[:, 100:128].any() and V.windows(fb, q, 0)[:, 128:].any()
    _sweep(gpu_lib, path, fb, zs=(0, 1), edges=(1, 64, 170), alone=False)
    s = gpu_lib.Search(path)
    offs, hits = s.search_coverage_arrays([q], 0.0, 0)
    assert len(hits) == 100 and int(hits["doc"].max()) == 99
    s.close()
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 5, 301, 1, 31, 3, mask=False)
    assert V.windows(fb, q, 0)[:, 5:].any()
    _sweep(gpu_lib, path, fb, zs=(0, 3), edges=(1, 64, 170), alone=False)


def test_handle_over_two_files_of_different_term_size(gpu_lib, tmp_path):
    pa, fa = _classic(str(tmp_path / "a.cobs_classic"), 300, 2003, 1, 31, 1)
    pb, fb = _compact(str(tmp_path / "b.cobs_compact"), 150, 4, [499, 601, 701, 557, 811], 2, 20, 2)
    s = gpu_lib.Search([pa, pb])
    for z in ZS:
        s.set_findere(z)
        _check(s, [fa, fb], _edge_queries(SRC, 31, z, (1, 2, 64, 65, 500)), z)
    s.set_findere(0)
    q = _edge_queries(SRC, 31, 0, (500,))[0]
    want = G.results([fa, fb], q, 0, 0.3, 5)
    res = s.search_coverage(q.decode(), 0.3, 5)                     # the list form of one query ...
    assert [(r.doc_name, r.score) for r in res] == [("doc_%05d" % d, sc) for (_f, d, sc) in want] and res
    both = s.search_coverage([q, q[:100]], 0.3, 5)                  # ... and of several
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
            for z in (0, 3):
                s.set_findere(z)
                qs = _edge_queries(SRC, 31, z, (1, 33, 64, 129, 1500))
                _check(s, [f], qs, z, thresholds=(0.0, 0.8), limits=(0, 5))
                got[wide, name, z] = s.search_coverage_arrays(qs, 0.3, 0)
            s.close()
    for (wide, name, z), (offs, hits) in got.items():
        assert np.array_equal(offs, got["0", name, z][0]) and np.array_equal(hits, got["0", name, z][1])


@pytest.mark.parametrize("seg", SEGS)
def test_forced_segments(gpu_lib, tmp_path, monkeypatch, seg):
    """every lane group starts its segments from an empty countdown and pre-rolls: the same results"""
    monkeypatch.setenv("COBS_GPU_COVERAGE_SEG", seg)
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 300, 2003, 1, 31, 1)
    assert _sweep(gpu_lib, path, fb, alone=False) > 0
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), 8 * 8 * 6 - 43, 8, [1201, 997, 1500, 1103, 1301, 800], 2, 31, 8)
    assert _sweep(gpu_lib, path, fb, zs=(0, 3), alone=False) > 0
    path, fb = _classic(str(tmp_path / "w.cobs_classic"), 9000, 499, 1, 31, 4)          # a tile as wide as a wave
    assert _sweep(gpu_lib, path, fb, zs=(1,), edges=(1, 31, 32, 33, 129, 1500), alone=False) > 0


@pytest.mark.parametrize("k", [3, 15, 16, 31, 32, 63, 64])
def test_term_sizes_cross_the_countdown_planes(gpu_lib, tmp_path, k):
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 129, 2003, 1, k, k)
    for z in (0, 1):
        s = gpu_lib.Search(path, findere=z)
        span = k + z
        qs = _edge_queries(SRC, k, z, tuple(sorted({1, 2, span - 1, span, span + 1, 129, 1500} - {0})))
        _check(s, [fb], qs, z, thresholds=(0.0, 0.8), limits=(0, 5))
        s.close()


def test_the_longest_span(gpu_lib, tmp_path):
    """k = 248 with z = 7: span 255, the most the eight countdown planes hold; one more base is refused"""
    from cobs_amd import _capi
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 129, 2003, 1, 248, 5)
    s = gpu_lib.Search(path, findere=7)
    qs = _edge_queries(SRC, 248, 7, (1, 2, 254, 255, 256, 1500))
    _check(s, [fb], qs, 7, thresholds=(0.0, 0.8), limits=(0, 5))
    s.close()
    path, fb = _classic(str(tmp_path / "d.cobs_classic"), 129, 2003, 1, 249, 5)
    s = gpu_lib.Search(path, findere=7)
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.search_coverage(SRC[:600], 0.5)
    assert e.value.status == _capi.ERR_UNSUPPORTED and "256" in str(e.value) and s.coverage_ms()["passes"] == 0
    s.set_findere(6)
    _check(s, [fb], [SRC[:600]], 6, thresholds=(0.8,), limits=(0,))
    s.close()


# ---- the structure fixture: documents that hold mutated copies of the source --------------------------------------------
K, LQ = 31, 400


def _mutate(q, subs=(), deletion=None, insertion=None):
    b = bytearray(q)
    for o in subs:
        b[o] = ord("ACGT"[("ACGT".index(chr(b[o])) + 1) % 4])
    if deletion is not None:
        del b[deletion]
    if insertion is not None:
        b.insert(insertion, ord("ACGT"[("ACGT".index(chr(b[insertion])) + 2) % 4]))
    return bytes(b)


NDOCS = 13


def _structure(tmp_path, z):
    """D = 40 documents over an EMPTY matrix (no random bits: every set position is planted).  Document d holds every
    k-mer of a mutated copy of the query."""
    span = K + z
    q = SRC[1000:1000 + LQ]
    copies = {
        0: q,                                                   # no substitution: one run over all positions
        1: _mutate(q, [200]),                                   # one: a gap of span positions
        2: _mutate(q, [150, 150 + span - 1]),                   # two, span - 1 bases apart
        3: _mutate(q, [150, 150 + span]),                       # ... span
        4: _mutate(q, [150, 150 + span + 1]),                   # ... span + 1: an isolated set position between them
        5: _mutate(q, [0]),
        6: _mutate(q, [LQ - 1]),
        7: _mutate(q, deletion=180),
        8: _mutate(q, insertion=180),                           # a gap of span - 1 positions
        9: _mutate(q, list(range(100, LQ, 10))),                # fails both thresholds
        10: _mutate(q, [60, 130, 215, 290, 350]),               # covered well, few k-mers: the case the feature is for
        11: _mutate(q, [150, 151]),                             # a gap of span + 1 positions
        12: q[250:250 + span],                                  # one set position and nothing else: coverage = span
    }
    assert len(copies) == NDOCS
    sig, num_docs = 1000003, 40
    m = np.zeros((sig, (num_docs + 7) // 8), dtype=np.uint8)
    for d, text in copies.items():
        cases.plant([m], [sig], 0, text, {d: 1.0}, K, 1, 1)
    from oracle import construct as Kc
    path = str(tmp_path / ("s%d.cobs_classic" % z))
    Kc.write_classic(path, K, 1, ["doc_%05d" % i for i in range(num_docs)], sig, 1, m)
    return path, F.FileBits(K, 1, 1, [m], num_docs), q


def _runs(col):
    """[(first, length)] of the runs of set positions, and of the gaps between them"""
    x = np.concatenate(([0], col.astype(np.int8), [0]))
    d = np.diff(x)
    starts, ends = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]
    runs = list(zip(starts.tolist(), (ends - starts).tolist()))
    gaps = [(runs[i][0] + runs[i][1], runs[i + 1][0] - runs[i][0] - runs[i][1]) for i in range(len(runs) - 1)]
    return runs, gaps


def _structure_conditions(fb, q, z):
    """what the fixture has to reach, asserted on the checker's side; -> the documents only the coverage search finds"""
    span = K + z
    win = V.windows(fb, q, z)
    n = win.shape[0]
    (length, cov, docs, s), = G.tables([fb], q, z)
    assert length == LQ and (s[NDOCS:] == 0).all()
    runs = {d: _runs(win[:, d]) for d in range(NDOCS)}
    all_runs = [r for d in runs for r in runs[d][0]]
    gap_lengths = {g for d in runs for (_a, g) in runs[d][1]}
    assert int(cov[0]) == LQ and int(s[0]) == n
    assert runs[12][0] == [(250, 1)] and int(cov[12]) == span                   # an isolated set position
    assert any(ln == 1 for (_a, ln) in runs[4][0]) and len(runs[4][0]) == 3     # ... and one between two gaps
    # two set positions closer than span whose stretches overlap: a run of 2 .. span - 1 positions between two gaps
    short = [(d, a, ln) for d in range(1, NDOCS) for (a, ln) in runs[d][0] if 2 <= ln < span and 0 < a and a + ln < n]
    assert short and all(int(cov[d]) < LQ for (d, _a, _ln) in short), short
    assert {span - 1, span, span + 1} <= gap_lengths, sorted(gap_lengths)
    assert any(a + ln == n for (a, ln) in all_runs) and runs[6][0][-1][0] + runs[6][0][-1][1] < n   # the tail term, and none
    assert runs[0][0] == [(0, n)]                                               # a run across every segment boundary
    thr_cov, thr_kmer = G.thresholds(0.8, LQ), F.threshold_for(0.8, n)
    rescued = [d for d in range(NDOCS) if int(cov[d]) >= thr_cov and int(s[d]) < thr_kmer]
    assert 10 in rescued, (cov[:NDOCS], s[:NDOCS])                              # the case the feature exists for
    assert 0 < int(s[9]) < thr_kmer and int(cov[9]) < thr_cov                   # fails both
    return rescued


@pytest.mark.parametrize("seg", ("",) + SEGS)
@pytest.mark.parametrize("z", [0, 3])
def test_structure_fixture(gpu_lib, tmp_path, monkeypatch, z, seg):
    if seg:
        monkeypatch.setenv("COBS_GPU_COVERAGE_SEG", seg)
    else:
        monkeypatch.delenv("COBS_GPU_COVERAGE_SEG", raising=False)
    path, fb, q = _structure(tmp_path, z)
    span = K + z
    rescued = _structure_conditions(fb, q, z)
    s = gpu_lib.Search(path, findere=z)
    queries = [q, q[:200], q[100:], q[150:150 + 2 * span + 40]]
    _check(s, [fb], queries, z)
    offs, hits = s.search_coverage_arrays([q], 0.8, 0)
    plain = {d for (_f, d, _sc) in s.search_hits([q], 0.8, 0)[0]}
    assert set(rescued) <= set(hits["doc"].tolist()) and not (set(rescued) & plain)
    s.close()


def test_miss_and_skip_agree_and_error_names_the_query(gpu_lib, tmp_path):
    from cobs_amd import _capi
    path, fb = _compact(str(tmp_path / "n.cobs_compact"), 300, 8, [901, 1003, 777, 1300, 950], 2, 31, 9)
    base = SRC[40:40 + 260]
    qs = [I.with_n(base, [o]) for o in (0, 130, len(base) - 1)] + [base, I.with_n(base, [7, 200]), b"N" * 100]
    got = {}
    for mode in I.MODES:
        s = gpu_lib.Search(path, invalid_bases=mode)
        for z in (0, 3):
            s.set_findere(z)
            tabs = _check(s, [fb], qs, z, mode)
            got[mode, z] = [s.search_coverage_arrays(qs, t, 0) for t in (0.0, 0.3)]
            # an N in the middle (query 1: base 130) leaves its base uncovered everywhere and unsets the span positions
            # whose window holds it; only the 2 span - 1 bases those positions reach can lose their cover
            span = fb.term_size + z
            clean, with_n = G.tables([fb], base, z, mode)[0][1].astype(np.int64), tabs[1][0][1].astype(np.int64)
            assert not G.covered(fb, qs[1], z, mode)[130].any()
            assert (with_n <= clean).all() and (clean - with_n <= 2 * span - 1).all() and (with_n < clean).any()
            assert int((clean - with_n).max()) >= (span if z == 0 else 1)
            o = got[mode, z][1][0]
            assert int(o[6]) == int(o[5])                           # all N: nothing returned above a threshold
            assert not got[mode, z][0][1]["score"][int(got[mode, z][0][0][5]):].any()
        s.close()
    for z in (0, 3):
        for a, b in zip(got["miss", z], got["skip", z]):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    s = gpu_lib.Search(path, findere=1)
    good = [SRC[:100], SRC[200:340], SRC[400:480]]
    bad_base = [good[0], good[1], good[2][:40] + b"N" + good[2][41:]]
    st, bad, offs, hits, msg = _raw_call(s, bad_base, 0.5, 0, 1000)
    assert st == _capi.ERR_INVALID_BASE and bad == 2 and "(query 2)" in msg
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.search_coverage(bad_base[2], 0.5)
    assert e.value.status == _capi.ERR_INVALID_BASE
    _check(s, [fb], good, 1, thresholds=(0.3,), limits=(0,))        # the handle still answers
    s.close()


@pytest.mark.parametrize("z", [0, 3])
def test_identity_with_hit_positions(gpu_lib, tmp_path, z):
    """for every hit of a coverage search, covered_bases(its hit_positions words, n, span) is its score"""
    pa, fa = _classic(str(tmp_path / "a.cobs_classic"), 300, 2003, 1, 31, 1)
    pb, fb = _compact(str(tmp_path / "b.cobs_compact"), 150, 4, [499, 601, 701, 557, 811], 2, 20, 2)
    s = gpu_lib.Search([pa, pb], findere=z)
    queries = _edge_queries(SRC, 31, z, (1, 64, 65, 700))
    offs, hits = s.search_coverage_arrays(queries, 0.0, 40)         # the 40 best of every query, whatever they reach
    assert len(hits) == 160 and {0, 1} <= set(hits["file_no"].tolist()) and len(set(hits["score"].tolist())) > 8
    bo, bits = s.hit_positions(queries, offs, hits)
    ks = (31, 20)
    for i, q in enumerate(queries):
        for h in range(int(offs[i]), int(offs[i + 1])):
            k = ks[int(hits["file_no"][h])]
            n = len(q) - k + 1 - z
            assert gpu_lib.covered_bases(bits[int(bo[h]):int(bo[h + 1])], n, k + z) == int(hits["score"][h]), (i, h)
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
    s = gpu_lib.Search(path, findere=3)
    zero = {"hash_ms": 0.0, "scan_ms": 0.0, "passes": 0}
    assert s.coverage_ms() == zero
    one = [s.search_coverage_arrays(queries, t, 0) for t in (0.0, 0.3)]
    t1 = s.coverage_ms()
    assert t1["passes"] == 2 and t1["hash_ms"] > 0 and t1["scan_ms"] > 0 and s.coverage_ms() == zero
    s.set_tuning("pass_bytes", 30000)
    many = [s.search_coverage_arrays(queries, t, 0) for t in (0.0, 0.3)]
    assert s.coverage_ms()["passes"] >= 6
    s.set_tuning("pass_bytes", 0)
    s.set_tuning("hit_cap", 7)                                      # the first pool holds 7 records
    small = [s.search_coverage_arrays(queries, t, 0) for t in (0.0, 0.3)]
    s.set_tuning("pass_bytes", 30000)
    both = [s.search_coverage_arrays(queries, t, 0) for t in (0.0, 0.3)]
    s.set_tuning("pass_bytes", 0)
    s.set_tuning("hit_cap", 0)
    for other in (many, small, both):
        for a, b in zip(one, other):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert len(one[0][1]) == 40 * 700 and 0 < len(one[1][1]) < 40 * 700
    _check(s, [fb], queries, 3, thresholds=(0.0, 0.3), limits=(0, 5))
    # searches before and after on the same handle are not disturbed (the call shares their workspace)
    assert s.search_hits(queries[:5], 0.0, 3) == [F.results([fb], q, 3, 0.0, 3) for q in queries[:5]]
    s.close()


def _raw_call(s, queries, threshold, num_results, cap, null_offsets=False):
    from cobs_amd import _capi
    lib = _capi.load()
    nq = len(queries)
    arr = (C.c_char_p * max(nq, 1))(*queries)
    lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in queries])
    hits = np.zeros(max(cap, 1), dtype=s.HIT_DTYPE)
    offs = np.full(nq + 1, 0xFFFF, dtype=np.uint64)
    bad = C.c_size_t(12345)
    st = lib.cobs_gpu_search_coverage(s._h, arr, lens, nq, threshold, num_results,
                                      C.cast(hits.ctypes.data, C.POINTER(_capi.Hit)) if cap else None, cap,
                                      None if null_offsets else C.cast(offs.ctypes.data, C.POINTER(C.c_size_t)), C.byref(bad))
    return st, bad.value, offs, hits, lib.cobs_gpu_last_error().decode()


def test_refusals_come_back_before_any_device_work(gpu_lib, oracle, tmp_path):
    from cobs_amd import _capi
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 300, 2003, 1, 31, 1)
    s = gpu_lib.Search(path, findere=3)
    good = [SRC[:100], SRC[200:340], SRC[400:480]]
    s.coverage_ms()
    lib = _capi.load()
    # NULL arguments
    assert lib.cobs_gpu_search_coverage(s._h, None, None, 3, 0.5, 0, None, 0, None, None) == _capi.ERR_ARG
    assert _raw_call(s, good, 0.5, 0, 100, null_offsets=True)[0] == _capi.ERR_ARG
    offs = (C.c_size_t * 4)()
    assert lib.cobs_gpu_search_coverage(s._h, None, None, 3, 0.5, 0, None, 0, offs, None) == _capi.ERR_ARG
    arr = (C.c_char_p * 3)(*good)
    lens = (C.c_size_t * 3)(*[len(q) for q in good])
    assert lib.cobs_gpu_search_coverage(s._h, arr, lens, 3, 0.5, 0, None, 5, offs, None) == _capi.ERR_ARG      # cap without hits
    # a query that is too short names the query
    st, bad, offs, hits, msg = _raw_call(s, [good[0], good[1], SRC[:31 + 2]], 0.5, 0, 100)
    assert st == _capi.ERR_QUERY_TOO_SHORT and bad == 2 and str(31 + 3) in msg and "(query 2)" in msg
    # 2^20 characters are one too many
    long_q = oracle.random_sequence(1 << 20, 5)
    st, bad, offs, hits, msg = _raw_call(s, [good[0], long_q], 0.5, 0, 100)
    assert st == _capi.ERR_QUERY_TOO_LONG and bad == 1 and "(query 1)" in msg
    assert s.coverage_ms()["passes"] == 0                           # none of these reached the device
    # ... and 2^20 - 1 are served: twenty count planes
    offs, hits = s.search_coverage_arrays([long_q[:-1]], 0.0, 3)
    assert len(hits) == 3 and s.coverage_ms()["passes"] == 1
    # a result buffer that is too small: the needed size from the one scan that ran, then success
    want = [G.results([fb], q, 3, 0.3, 0) for q in good]
    need = sum(len(x) for x in want)
    assert need > 3
    st, bad, offs, hits, msg = _raw_call(s, good, 0.3, 0, 0)
    assert st == _capi.ERR_CAPACITY and int(offs[3]) == need and [int(offs[i + 1]) - int(offs[i]) for i in range(3)] == [len(x) for x in want]
    st, bad, offs, hits, msg = _raw_call(s, good, 0.3, 0, need - 1)
    assert st == _capi.ERR_CAPACITY and int(offs[3]) == need
    st, bad, offs, hits, msg = _raw_call(s, good, 0.3, 0, need)
    assert st == _capi.OK and hits[:need].tolist() == [h for x in want for h in x], msg
    s.close()
    # a handle with an HBM budget, one shard of several, the device list
    s = gpu_lib.Search(path, hbm_budget=256 << 20)
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.search_coverage(good[0], 0.5)
    assert e.value.status == _capi.ERR_UNSUPPORTED and "HBM budget" in str(e.value) and s.coverage_ms()["passes"] == 0
    s.close()
    s = gpu_lib.Search(path, shard_rank=0, shard_count=2)
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.search_coverage(good[0], 0.5)
    assert e.value.status == _capi.ERR_UNSUPPORTED and "shard" in str(e.value) and s.coverage_ms()["passes"] == 0
    s.close()
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        gpu_lib.MultiSearch.search_coverage_arrays(gpu_lib.MultiSearch.__new__(gpu_lib.MultiSearch), good)
    assert e.value.status == _capi.ERR_UNSUPPORTED
