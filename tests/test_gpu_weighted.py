"""GPU: IDF-weighted search (cobs_gpu_search_weighted / Search.search_weighted / ClassicSearch::search_weighted /
--weighted) hit for hit against tests/weighted_check.py: hits, total_weight and hit_offsets at thresholds 0, 0.3, 0.8, 1.0
and num_results 0, 1, 5.  Every comparison is exact.

The fixtures have GRADED row densities -- row r holds bits of density 2^-(r mod 17), none for r mod 17 = 16, and a few
rows are all ones -- so that the positions of a query reach many different weights (uniform 0.4-density bits would give
every position weight 2); every fixture asserts on the checker's side which weights its queries reach."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import cases
from tests import findere_check as F
from tests import invalid_check as I
from tests import prevalence_check as V
from tests import weighted_check as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZS = (0, 1, 3, 7)
EDGES = (1, 2, 63, 64, 65, 128, 129, 1500)           # position counts n
THRESHOLDS = (0.0, 0.3, 0.8, 1.0)
LIMITS = (0, 1, 5)


def _graded(rng, sig, nbytes):
    k = np.arange(sig) % 17
    dens = np.where(k < 16, 2.0 ** -k.astype(np.float64), 0.0)
    bits = rng.random((sig, nbytes, 8)) < dens[:, None, None]
    m = np.packbits(bits, axis=2, bitorder="little").reshape(sig, nbytes)
    if sig >= 17:                            # a few rows everybody holds
        m[[3, sig // 2, sig - 2]] = 0xFF
    return m


SRC = O.random_sequence(6000, 77)            # the queries are cut from it


def _mask(m, first_doc, num_docs):
    return cases.mask_padding_docs(m, first_doc, num_docs)


def _plant(mats, sigs, page_docs, num_docs, k, num_hashes, planted=None):
    """documents that hold 90 / 60 / 35 % of the source's k-mers: scores on both sides of the thresholds (a small file: one
    document with 60 %, so that most positions stay rare)"""
    if planted is None:
        planted = {0: 0.9, num_docs // 2: 0.6, num_docs - 1: 0.35} if num_docs >= 16 else {0: 0.6}
    cases.plant(mats, sigs, page_docs, SRC, planted, k, 1, num_hashes)


def _classic(path, num_docs, sig, num_hashes, k, seed, mask=True, planted=None):
    rng = np.random.default_rng(seed)
    m = _graded(rng, sig, (num_docs + 7) // 8)
    if mask:
        m = _mask(m, 0, num_docs)
    _plant([m], [sig], 0, num_docs, k, num_hashes, planted)
    from oracle import construct as K
    K.write_classic(path, k, 1, ["doc_%05d" % i for i in range(num_docs)], sig, num_hashes, m)
    return path, F.FileBits(k, 1, num_hashes, [m], num_docs)


def _compact(path, num_docs, page_size, sigs, num_hashes, k, seed, mask=True):
    rng = np.random.default_rng(seed)
    page_docs = 8 * page_size
    mats = [_graded(rng, s, page_size) for s in sigs]
    if mask:
        mats = [_mask(m, p * page_docs, num_docs) for p, m in enumerate(mats)]
    _plant(mats, sigs, page_docs, num_docs, k, num_hashes)
    from oracle import construct as K
    K.write_compact(path, k, 1, page_size, [(s, num_hashes) for s in sigs], ["doc_%05d" % i for i in range(num_docs)], mats)
    return path, F.FileBits(k, 1, num_hashes, mats, num_docs)


@pytest.fixture(scope="module")
def src():
    return SRC


def _edge_queries(src, k, z, edges=EDGES):
    """one query per position count n, cut from the source at different places"""
    out = []
    for n in edges:
        ln = n + z + k - 1
        o = (37 * n) % (len(src) - ln)
        out.append(src[o:o + ln])
    return out


def _check(s, files, queries, z, mode="error", thresholds=THRESHOLDS, limits=LIMITS):
    """every threshold and limit of one batch against the checker; -> the set of weights the queries reach"""
    tabs = [W.tables(files, q, z, mode) for q in queries]
    want_total = np.array([[t[0] for t in tab] for tab in tabs], dtype=np.uint64).reshape(len(queries), len(files))
    for t in thresholds:
        for nr in limits:
            offs, hits, total = s.search_weighted_arrays(queries, t, nr)
            assert offs.dtype == np.uint64 and total.dtype == np.uint64 and len(offs) == len(queries) + 1
            assert np.array_equal(total, want_total), (z, mode, t, nr)
            rows = hits.tolist()
            for i in range(len(queries)):
                got = rows[int(offs[i]):int(offs[i + 1])]
                want = W.results_from(tabs[i], t, nr)
                assert got == want, (z, mode, t, nr, i, got[:4], want[:4])
            assert int(offs[-1]) == len(rows)
    return set().union(*[set(t[3].tolist()) for tab in tabs for t in tab])


def _sweep(gpu_lib, path, fb, src, zs=ZS, edges=EDGES):
    s = gpu_lib.Search(path)
    reached = set()
    for z in zs:
        s.set_findere(z)
        qs = _edge_queries(src, fb.term_size, z, edges)
        assert [fb.positions(q, z) for q in qs] == list(edges)
        reached |= _check(s, [fb], qs, z)                                       # a batch that mixes the lengths
        for q in qs:                                                            # ... and every position count alone
            _check(s, [fb], [q], z, thresholds=(0.0, 0.3), limits=(0, 1))
    s.close()
    return reached


def _max_weight(num_docs):
    return W.idf_weight(num_docs, 1)


@pytest.mark.parametrize("num_hashes", [1, 3])
@pytest.mark.parametrize("num_docs", [1, 7, 8, 9, 127, 129, 300, 1027])
def test_classic_layouts(gpu_lib, src, tmp_path, num_docs, num_hashes):
    """the tail bits of the last byte, the tail bytes of the last 16-byte chunk, rows narrower and wider than a wave"""
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), num_docs, 2003, num_hashes, 31, num_docs)
    reached = _sweep(gpu_lib, path, fb, src)
    # condition of the test: no weight, the rarest the file can have and all in between but one at the most; with one
    # hash function also the weight of a k-mer everybody holds (an all-ones row)
    top = _max_weight(num_docs)
    assert top in reached and reached <= set(range(top + 1)) and len(reached) >= top - 1 and (num_hashes != 1 or {0, 1} <= reached)


def test_cap_fixture_reaches_every_weight(gpu_lib, src, tmp_path):
    """D = 40 000: a singleton weighs 15 (the cap: log2(40 000) > 14); n = 4400 takes 15 n over 2^16, a plane-count boundary"""
    path, fb = _classic(str(tmp_path / "cap.cobs_classic"), 40000, 257, 1, 31, 11, planted={})
    s = gpu_lib.Search(path)
    qs = _edge_queries(src, 31, 0, (64, 1500, 4400))
    assert 15 * 4400 >= 2 ** 16 > 15 * 1500
    reached = _check(s, [fb], qs, 0, thresholds=(0.0, 0.3, 0.8), limits=(0, 5))
    assert reached == set(range(16))
    s.set_findere(3)
    _check(s, [fb], _edge_queries(src, 31, 3, (65, 1500)), 3, thresholds=(0.3,), limits=(0,))
    s.close()


@pytest.mark.parametrize("sigs", [[1, 2, 65, 4097], [1201, 997, 1500, 1103, 1301, 800]])
@pytest.mark.parametrize("page_size", [2, 8, 16, 200])
def test_compact_layouts(gpu_lib, src, tmp_path, page_size, sigs):
    """a last sub-index that is partly filled; narrow tiles whose lane groups walk different positions"""
    num_docs = len(sigs) * 8 * page_size - 5 * page_size - 3
    assert (len(sigs) - 1) * 8 * page_size < num_docs
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), num_docs, page_size, sigs, 1 if page_size != 8 else 2, 31, page_size)
    reached = _sweep(gpu_lib, path, fb, src)
    # (sub-indexes of 1 and 2 rows: every document of theirs holds every k-mer, no position is rare)
    assert len(reached) >= (2 if sigs[0] == 1 else 7)


def test_trailing_sub_index_of_padding(gpu_lib, src, tmp_path):
    path, fb = _compact(str(tmp_path / "t.cobs_compact"), 2 * 128 - 9, 16, [501, 703, 601], 1, 31, 5)
    assert (fb.doc_of_slot()[256:] < 0).all()
    assert len(_sweep(gpu_lib, path, fb, src, zs=(0, 3), edges=(1, 65, 300))) >= 4


def test_padding_slots_with_set_bits_neither_count_nor_come_back(gpu_lib, src, tmp_path):
    """files written WITHOUT masking the padding documents: their slots hold bits (the all-ones rows at least)"""
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 5, 301, 1, 31, 3, mask=False)
    q = src[:200]
    assert V.windows(fb, q, 0)[:, 5:].any()                         # (the padding slots would have counted)
    assert len(_sweep(gpu_lib, path, fb, src, zs=(0, 3), edges=(1, 64, 170))) >= 3
    # compact: the second sub-index partly filled, the third all padding, both with bits
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), 100, 8, [211, 307, 401], 2, 31, 4, mask=False)
    assert V.windows(fb, q, 0)[:, 100:128].any() and V.windows(fb, q, 0)[:, 128:].any()
    s = gpu_lib.Search(path)
    reached = set()
    for z in (0, 1):
        s.set_findere(z)
        reached |= _check(s, [fb], _edge_queries(src, 31, z, (1, 64, 170)), z)
        offs, hits, total = s.search_weighted_arrays(_edge_queries(src, 31, z, (170,)), 0.0, 0)
        assert len(hits) == 100 and int(hits["doc"].max()) == 99
    assert len(reached) >= 3                 # (two hashes: few windows of several k-mers are held by anybody)
    s.close()


def test_handle_over_two_files_of_different_term_size(gpu_lib, src, tmp_path):
    pa, fa = _classic(str(tmp_path / "a.cobs_classic"), 300, 2003, 1, 31, 1)
    pb, fb = _compact(str(tmp_path / "b.cobs_compact"), 150, 4, [499, 601, 701, 557, 811], 2, 20, 2)
    s = gpu_lib.Search([pa, pb])
    for z in ZS:
        s.set_findere(z)
        qs = _edge_queries(src, 31, z, (1, 2, 64, 65, 500))
        assert len(_check(s, [fa, fb], qs, z)) >= 5
    s.set_findere(0)
    q = _edge_queries(src, 31, 0, (500,))[0]
    res = s.search_weighted(q.decode(), 0.3, 5)                     # the list form of one query
    want = W.results([fa, fb], q, 0, 0.3, 5)
    tw = W.total_weights([fa, fb], q, 0)
    assert [(r.doc_name, r.score, r.total_weight) for r in res] == [("doc_%05d" % d, sc, tw[f]) for (f, d, sc) in want] and res
    pw = s.position_weights(q)
    assert len(pw) == 2 and all(np.array_equal(pw[f], W.weights(fl, q, 0)) and pw[f].dtype == np.uint8 for f, fl in enumerate([fa, fb]))
    s.close()


def test_several_device_passes_and_pool_overflow(gpu_lib, src, tmp_path):
    """the workspace limit cuts the call into passes, a small pool overflows and its pass is scanned again: same results"""
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), 700, 16, [1201, 997, 1500, 1103, 1301, 800], 1, 31, 3)
    rng = np.random.default_rng(41)
    queries = []
    for _ in range(39):
        ln = int(rng.integers(50, 151))
        o = int(rng.integers(0, len(src) - ln))
        queries.append(src[o:o + ln])
    queries.append(src[:1030])
    s = gpu_lib.Search(path, findere=3)
    s.weighted_ms()
    one = [s.search_weighted_arrays(queries, t, 0) for t in (0.0, 0.3)]
    t1 = s.weighted_ms()
    assert t1["passes"] == 2 and all(t1[k] > 0 for k in ("hash_ms", "prevalence_ms", "weights_ms", "scan_ms"))
    s.set_tuning("pass_bytes", 30000)
    many = [s.search_weighted_arrays(queries, t, 0) for t in (0.0, 0.3)]
    assert s.weighted_ms()["passes"] >= 6
    s.set_tuning("pass_bytes", 0)
    s.set_tuning("hit_cap", 7)                                      # the first pool holds 7 records
    small = [s.search_weighted_arrays(queries, t, 0) for t in (0.0, 0.3)]
    s.set_tuning("pass_bytes", 30000)
    both = [s.search_weighted_arrays(queries, t, 0) for t in (0.0, 0.3)]
    s.set_tuning("pass_bytes", 0)
    s.set_tuning("hit_cap", 0)
    for other in (many, small, both):
        for a, b in zip(one, other):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert len(one[0][1]) == 40 * 700 and 0 < len(one[1][1]) < 40 * 700
    assert len(_check(s, [fb], queries, 3, thresholds=(0.0, 0.3), limits=(0, 5))) >= 4
    # searches before and after on the same handle are not disturbed (the call shares their workspace)
    assert s.search_hits(queries[:5], 0.0, 3) == [F.results([fb], q, 3, 0.0, 3) for q in queries[:5]]
    s.close()


def test_miss_and_skip_agree_and_error_names_the_query(gpu_lib, src, tmp_path):
    from cobs_amd import _capi
    path, fb = _compact(str(tmp_path / "n.cobs_compact"), 300, 8, [901, 1003, 777, 1300, 950], 2, 31, 9)
    base = src[40:40 + 260]
    qs = [I.with_n(base, [o]) for o in (0, 130, len(base) - 1)] + [base, I.with_n(base, [7, 200]), b"N" * 100]
    got = {}
    for mode in I.MODES:
        s = gpu_lib.Search(path, invalid_bases=mode)
        for z in (0, 3):
            s.set_findere(z)
            assert len(_check(s, [fb], qs, z, mode)) >= 3
            got[mode, z] = [s.search_weighted_arrays(qs, t, 0) for t in (0.0, 0.3)]
            assert not got[mode, z][0][2][5].any()                  # all N: no weight at all ...
            o = got[mode, z][1][0]
            assert int(o[6]) == int(o[5])                           # ... and nothing returned above a threshold
        s.close()
    assert I.MODES == ("miss", "skip") or set(I.MODES) == {"miss", "skip"}
    for z in (0, 3):
        for a, b in zip(got["miss", z], got["skip", z]):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    s = gpu_lib.Search(path, findere=1)
    good = [src[:100], src[200:340], src[400:480]]
    bad_base = [good[0], good[1], good[2][:40] + b"N" + good[2][41:]]
    st, bad, offs, hits, total, msg = _raw_call(s, bad_base, 0.5, 0, 1000)
    assert st == _capi.ERR_INVALID_BASE and bad == 2 and "(query 2)" in msg
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.search_weighted(bad_base[2], 0.5)
    assert e.value.status == _capi.ERR_INVALID_BASE
    _check(s, [fb], good, 1, thresholds=(0.3,), limits=(0,))        # the handle still answers
    s.close()


def test_ties_are_cut_in_file_and_document_order(gpu_lib, src, tmp_path):
    """mostly all-ones rows: 1..9-position queries score the same in run after run of documents"""
    rng = np.random.default_rng(5)
    sig, num_docs = 499, 300
    m = np.full((sig, (num_docs + 7) // 8), 0xFF, dtype=np.uint8)
    for r in range(0, sig, 7):
        m[r] = np.packbits(rng.random((m.shape[1], 8)) < 0.5, axis=1, bitorder="little").reshape(-1)
    m = _mask(m, 0, num_docs)
    from oracle import construct as K
    path = str(tmp_path / "t.cobs_classic")
    K.write_classic(path, 31, 1, ["doc_%05d" % i for i in range(num_docs)], sig, 1, m)
    fb = F.FileBits(31, 1, 1, [m], num_docs)
    s = gpu_lib.Search(path)
    qs = _edge_queries(src, 31, 0, tuple(range(1, 10)))
    reached = _check(s, [fb], qs, 0)
    assert {1, 2} <= reached
    tied = 0
    for q in qs:
        full = W.results([fb], q, 0, 0.0, 0)
        tied += int(full[4][2] == full[5][2]) + int(full[0][2] == full[1][2])
    assert tied >= 9                                                # (the cuts at 1 and 5 fall inside runs of equal scores)
    s.close()


@pytest.mark.parametrize("z", [0, 3])
def test_identities_against_the_existing_calls(gpu_lib, oracle, z):
    """a procedural handle larger than the numpy restatement likes"""
    from cobs_amd import _capi
    lib = _capi.load()
    sigs = [20011, 30011, 25013, 40009, 35023, 45007]
    num_docs, page_size = 5000, 105
    s = gpu_lib.Search.synthetic("compact", sigs, num_docs, page_size=page_size, seed=5, findere=z)
    queries = [oracle.random_sequence(300 + 30 + z, 100 + i) for i in range(16)]
    text = oracle.random_sequence(400, 7)
    s.plant(text[:200], list(range(0, 5000, 2)), 1000, salt=1)     # some positions held by more than half of the documents,
    s.plant(text[150:], list(range(0, 5000, 7)), 900, salt=3)       # ... some by more than the random bits alone give
    s.plant(text[:360], [11, 12], 1000, salt=2)
    queries[5], queries[9] = text[:330 + z], text[50:380 + z]
    poffs, counts = s.prevalence_arrays(queries)
    w = np.array([lib.cobs_gpu_idf_weight(num_docs, int(c)) for c in counts], dtype=np.uint64)
    assert len(set(w.tolist())) >= 2
    offs, hits, total = s.search_weighted_arrays(queries, 0.0, 0)
    assert len(hits) == 16 * num_docs
    for i in range(16):
        seg = slice(int(poffs[i]), int(poffs[i + 1]))
        assert int(total[i, 0]) == int(w[seg].sum()), i
        assert int(hits["score"][int(offs[i]):int(offs[i + 1])].sum(dtype=np.uint64)) == int((w[seg] * counts[seg]).sum()), i
    # a hit's weighted score is the sum of the weights over the set bits of its hit_positions
    offs, hits, total = s.search_weighted_arrays(queries, 0.5, 20)
    assert int(offs[6]) - int(offs[5]) >= 2
    bo, bits = s.hit_positions(queries, offs, hits)
    for i in (5, 9):
        wq = w[int(poffs[i]):int(poffs[i + 1])]
        for h in range(int(offs[i]), int(offs[i + 1])):
            pos = gpu_lib.unpack_positions(bits[int(bo[h]):int(bo[h + 1])], len(wq))
            assert int(wq[pos].sum()) == int(hits["score"][h]), (i, h)
    s.close()


def _raw_call(s, queries, threshold, num_results, cap, null_offsets=False, lens=None):
    from cobs_amd import _capi
    lib = _capi.load()
    nq = len(queries)
    arr = (C.c_char_p * max(nq, 1))(*queries)
    lens = (C.c_size_t * max(nq, 1))(*(lens or [len(q) for q in queries]))
    hits = np.zeros(max(cap, 1), dtype=s.HIT_DTYPE)
    offs = np.full(nq + 1, 0xFFFF, dtype=np.uint64)
    total = np.zeros((nq, s.num_files), dtype=np.uint64)
    bad = C.c_size_t(12345)
    st = lib.cobs_gpu_search_weighted(s._h, arr, lens, nq, threshold, num_results,
                                      C.cast(hits.ctypes.data, C.POINTER(_capi.Hit)) if cap else None, cap,
                                      None if null_offsets else C.cast(offs.ctypes.data, C.POINTER(C.c_size_t)),
                                      C.cast(total.ctypes.data, C.POINTER(C.c_uint64)), C.byref(bad))
    return st, bad.value, offs, hits, total, lib.cobs_gpu_last_error().decode()


def test_refusals_come_back_before_any_device_work(gpu_lib, oracle, src, tmp_path):
    from cobs_amd import _capi
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 300, 2003, 1, 31, 1)
    s = gpu_lib.Search(path, findere=3)
    good = [src[:100], src[200:340], src[400:480]]
    s.weighted_ms()
    lib = _capi.load()
    # NULL arguments
    assert lib.cobs_gpu_search_weighted(s._h, None, None, 3, 0.5, 0, None, 0, None, None, None) == _capi.ERR_ARG
    assert _raw_call(s, good, 0.5, 0, 100, null_offsets=True)[0] == _capi.ERR_ARG
    offs = (C.c_size_t * 4)()
    assert lib.cobs_gpu_search_weighted(s._h, None, None, 3, 0.5, 0, None, 0, offs, None, None) == _capi.ERR_ARG
    arr = (C.c_char_p * 3)(*good)
    lens = (C.c_size_t * 3)(*[len(q) for q in good])
    assert lib.cobs_gpu_search_weighted(s._h, arr, lens, 3, 0.5, 0, None, 5, offs, None, None) == _capi.ERR_ARG      # cap without hits
    # a query that is too short names the query
    short = [good[0], good[1], src[:31 + 2]]
    st, bad, offs, hits, total, msg = _raw_call(s, short, 0.5, 0, 100)
    assert st == _capi.ERR_QUERY_TOO_SHORT and bad == 2 and str(31 + 3) in msg and "(query 2)" in msg
    # 69 905 positions are the most: 15 n stays below 2^20
    long_q = oracle.random_sequence(69906 + 30 + 3, 5)
    st, bad, offs, hits, total, msg = _raw_call(s, [good[0], long_q], 0.5, 0, 100)
    assert st == _capi.ERR_QUERY_TOO_LONG and bad == 1 and "(query 1)" in msg
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.search_weighted(long_q, 0.5)
    assert e.value.status == _capi.ERR_QUERY_TOO_LONG
    assert s.weighted_ms()["passes"] == 0                           # none of these reached the device
    # ... and 69 905 positions are served
    offs, hits, total = s.search_weighted_arrays([long_q[:-1]], 0.9, 3)
    assert int(total[0, 0]) > 0 and s.weighted_ms()["passes"] == 1
    # a result buffer that is too small: the needed size from the one scan that ran, then success
    want = [W.results([fb], q, 3, 0.3, 0) for q in good]
    need = sum(len(x) for x in want)
    assert need > 3
    st, bad, offs, hits, total, msg = _raw_call(s, good, 0.3, 0, 0)
    assert st == _capi.ERR_CAPACITY and int(offs[3]) == need and [int(offs[i + 1]) - int(offs[i]) for i in range(3)] == [len(x) for x in want]
    st, bad, offs, hits, total, msg = _raw_call(s, good, 0.3, 0, need - 1)
    assert st == _capi.ERR_CAPACITY and int(offs[3]) == need
    st, bad, offs, hits, total, msg = _raw_call(s, good, 0.3, 0, need)
    assert st == _capi.OK and hits[:need].tolist() == [h for x in want for h in x], msg
    s.close()
    # a handle with an HBM budget, one shard of several, the device list
    s = gpu_lib.Search(path, hbm_budget=256 << 20)
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.search_weighted(good[0], 0.5)
    assert e.value.status == _capi.ERR_UNSUPPORTED and "HBM budget" in str(e.value) and s.weighted_ms()["passes"] == 0
    s.close()
    s = gpu_lib.Search(path, shard_rank=0, shard_count=2)
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.search_weighted(good[0], 0.5)
    assert e.value.status == _capi.ERR_UNSUPPORTED and "shard" in str(e.value) and s.weighted_ms()["passes"] == 0
    s.close()
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        gpu_lib.MultiSearch.search_weighted_arrays(gpu_lib.MultiSearch.__new__(gpu_lib.MultiSearch), good)
    assert e.value.status == _capi.ERR_UNSUPPORTED


def _tool():
    return os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")


def test_cli_and_cpp_mirror_agree_with_the_arrays(gpu_lib, src, tmp_path):
    """cobs_gpu_query --weighted prints what ClassicSearch::search_weighted returns, in the shape of a plain query"""
    pa, fa = _classic(str(tmp_path / "a.cobs_classic"), 300, 2003, 1, 31, 1)
    pb, fb = _compact(str(tmp_path / "b.cobs_compact"), 150, 4, [499, 601, 701, 557, 811], 2, 20, 2)
    paths, files = [pa, pb], [fa, fb]
    queries = _edge_queries(src, 31, 3, (1, 64, 200)) + [I.with_n(src[100:300], [90])]
    qf = tmp_path / "q.fa"
    qf.write_text("".join(">q%d\n%s\n" % (i, q.decode()) for i, q in enumerate(queries)))
    index_args = ["-i", paths[0], "-i", paths[1]]
    for z, mode, t, nr in ((0, "miss", 0.3, 0), (3, "skip", 0.5, 5)):
        s = gpu_lib.Search(paths, findere=z, invalid_bases=mode)
        offs, hits, total = s.search_weighted_arrays(queries, t, nr)
        rows = hits.tolist()
        assert [rows[int(offs[i]):int(offs[i + 1])] for i in range(len(queries))] == [W.results(files, q, z, t, nr, mode) for q in queries]
        s.close()
        fl = (["--findere", str(z)] if z else []) + ["--invalid-bases", mode, "-t", str(t)] + (["-l", str(nr)] if nr else [])
        r = subprocess.run([_tool()] + index_args + fl + ["-f", str(qf), "--weighted"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        want = []
        for i in range(len(queries)):
            seg = rows[int(offs[i]):int(offs[i + 1])]
            want.append("*q%d\t%d" % (i, len(seg)))
            want += ["doc_%05d\t%d" % (d, sc) for (_f, d, sc) in seg]
        assert r.stdout.splitlines() == want and len(rows) > 0
    # a verbatim query: the result lines only
    q = queries[2]
    r = subprocess.run([_tool()] + index_args + ["--weighted", "-t", "0.3", q.decode()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["doc_%05d\t%d" % (d, sc) for (_f, d, sc) in W.results(files, q, 0, 0.3, 0)]
    for extra in (["--hbm-budget", "1"], ["-d", "0,1"], ["--sharded"], ["--prevalence"]):
        r = subprocess.run([_tool()] + index_args + extra + ["--weighted", q.decode()], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--weighted: not with" in r.stderr and r.stdout == ""


def test_timer_resets_on_read(gpu_lib, src, tmp_path):
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 129, 2003, 1, 31, 1)
    s = gpu_lib.Search(path)
    zero = {"hash_ms": 0.0, "prevalence_ms": 0.0, "weights_ms": 0.0, "scan_ms": 0.0, "passes": 0}
    assert s.weighted_ms() == zero
    s.search_weighted_arrays([src[:200], src[300:700]], 0.5)
    t = s.weighted_ms()
    assert t["passes"] == 1 and all(t[k] > 0 for k in ("hash_ms", "prevalence_ms", "weights_ms", "scan_ms"))
    assert s.weighted_ms() == zero
    s.close()
