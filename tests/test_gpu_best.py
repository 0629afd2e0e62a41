"""GPU: best-of-group search (cobs_gpu_search_best / Search.search_best) record for record against tests/best_check.py:
file, document, query, score, positions, ties and the order of every group.

Classic and compact layouts (padding documents, sub-indexes of 1, 2, 65 and 4097 rows), a handle over files of different
term size, every score width, group sizes around the split step and the wave, one group over all queries (partial states
and the merge kernel) and many small ones (one writer per cell), groups cut by a device pass at every member position,
ties built on purpose, thresholds, limits, findere, `miss` / `skip`, the selection pool's overflow, the caller's capacity,
every refusal, the call between the other call families, and device memory over repeated calls."""
import ctypes as C
import gc

import numpy as np
import pytest

from tests import best_check as B
from tests import cases
from tests import findere_check as F
from tests import groups_check as G
from tests import invalid_check as I
from tests import weighted_check as W

pytestmark = pytest.mark.gpu

THRESHOLDS = (0.0, 0.5, 0.8, 1.0)
LIMITS = (0, 1, 10)


def _classic(path, num_docs, sig, num_hashes, k, seed, planted=None, query=None):
    cases.make_classic(path, num_docs, sig, num_hashes, k, 1, 0.3, seed, planted=planted, query=query)
    return F.classic_file(path)


def _compact(path, num_docs, page_size, sigs, num_hashes, k, seed, planted=None, query=None):
    rng = np.random.default_rng(seed)
    page_docs = 8 * page_size
    mats = [cases.mask_padding_docs(cases.random_bits(rng, (s, page_size), 0.3), p * page_docs, num_docs)
            for p, s in enumerate(sigs)]
    if planted:
        cases.plant(mats, sigs, page_docs, query, planted, k, 1, num_hashes)
    from oracle import construct as K
    K.write_compact(path, k, 1, page_size, [(s, num_hashes) for s in sigs], ["doc_%05d" % i for i in range(num_docs)], mats)
    return F.FileBits(k, 1, num_hashes, mats, num_docs)


@pytest.fixture(scope="module")
def data(gpu_lib, oracle, tmp_path_factory):
    """index files with planted documents (two of them complete: every piece of src has the fraction 1 there)"""
    d = tmp_path_factory.mktemp("best")
    src = oracle.random_sequence(3000, 77)
    out = {"src": src}
    out["c1"] = (str(d / "c1.cobs_classic"), _classic(str(d / "c1.cobs_classic"), 300, 2003, 1, 31, 1,
                                                      planted={0: 1.0, 7: 1.0, 150: 0.8, 299: 0.5}, query=src))
    out["c3"] = (str(d / "c3.cobs_classic"), _classic(str(d / "c3.cobs_classic"), 200, 3001, 3, 31, 2,
                                                      planted={3: 1.0, 4: 1.0, 199: 0.9}, query=src))
    # 700 documents in 6 sub-indexes of 128: the last page ends in 68 padding documents
    out["p1"] = (str(d / "p1.cobs_compact"), _compact(str(d / "p1.cobs_compact"), 700, 16, [1201, 997, 1500, 1103, 1301, 800], 1,
                                                      31, 3, planted={1: 1.0, 130: 1.0, 500: 0.9, 699: 0.85}, query=src))
    out["p3"] = (str(d / "p3.cobs_compact"), _compact(str(d / "p3.cobs_compact"), 300, 8, [901, 1003, 777, 1300, 950], 3, 25, 4,
                                                      planted={0: 1.0, 1: 1.0, 299: 0.95}, query=src))
    out["tiny"] = (str(d / "tiny.cobs_compact"), _compact(str(d / "tiny.cobs_compact"), 60, 2, [1, 2, 65, 4097], 1, 31, 6,
                                                          planted={5: 1.0, 20: 1.0, 40: 0.9, 59: 1.0}, query=src))
    out["c2k20"] = (str(d / "c2k20.cobs_classic"), _classic(str(d / "c2k20.cobs_classic"), 150, 1499, 2, 20, 5,
                                                            planted={10: 1.0, 11: 0.9}, query=src))
    return out


def _reads(src, n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ln = int(rng.integers(lo, hi + 1))
        o = int(rng.integers(0, len(src) - ln))
        out.append(src[o:o + ln])
    return out


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def _lists(offs, hits):
    rows = hits.tolist()
    return [rows[int(offs[g]):int(offs[g + 1])] for g in range(len(offs) - 1)]


def _check(s, files, queries, offsets, z=0, mode="error", thresholds=THRESHOLDS, limits=LIMITS):
    """every record of every group equals the checker's; -> the records selected at a threshold > 0"""
    selected = 0
    for t in thresholds:
        want_full = B.results(files, queries, offsets, z, mode, t, 0)
        for lim in limits:
            offs, hits = s.search_best_arrays(queries, offsets, t, lim)
            want = [w[:lim] if lim else w for w in want_full]
            got = _lists(offs, hits)
            assert [len(g) for g in got] == [len(g) for g in want], (z, mode, t, lim)
            assert [tuple(r) for g in got for r in g] == [r for g in want for r in g], (z, mode, t, lim)
            selected += len(hits) if t > 0 else 0
    return selected


@pytest.mark.parametrize("name", ["c1", "c3", "p1", "p3", "tiny"])
def test_every_layout_threshold_and_limit(gpu_lib, oracle, data, name):
    path, fb = data[name]
    src = data["src"]
    queries = _reads(src, 14, 50, 150, 11) + [oracle.random_sequence(120, 5)]
    offsets = _offsets([0, 1, 2, 5, 0, 7, 0])               # (an empty group between two that are not)
    s = gpu_lib.Search(path)
    for z in (0, 1, 3):
        s.set_findere(z)
        assert _check(s, [fb], queries, offsets, z) > 0            # (the thresholds did select planted documents)
    # an exact tie at the cut: the two complete documents hold the group's longest member entirely, num_results = 1 keeps
    # the first
    s.set_findere(0)
    offs, hits = s.search_best_arrays(queries, offsets, 1.0, 0)
    full = _lists(offs, hits)[3]
    assert len(full) >= 2 and full[0][2:] == full[1][2:] and full[0][3] == full[0][4] and full[0][:2] < full[1][:2]
    offs, hits = s.search_best_arrays(queries, offsets, 1.0, 1)
    assert _lists(offs, hits)[3] == [full[0]] and _lists(offs, hits)[0] == []
    s.close()


def test_group_sizes_around_the_split_step_and_the_wave(gpu_lib, data):
    path, fb = data["c1"]
    sizes = [0, 1, 7, 8, 9, 63, 64, 65, 0]
    queries = _reads(data["src"], sum(sizes), 40, 60, 21)
    s = gpu_lib.Search(path)
    assert _check(s, [fb], queries, _offsets(sizes), 0, thresholds=(0.0, 0.5), limits=(0,)) > 0
    n = s.best_ms()
    assert n["passes"] == 1 and n["own_spans"] == 6 and n["pieces"] == 2 and n["split_groups"] == 1    # (65 = 64 + 1)
    s.close()


def test_one_group_over_all_queries_and_many_groups_of_two(gpu_lib, data):
    path, fb = data["p1"]
    queries = _reads(data["src"], 300, 40, 70, 31)
    s = gpu_lib.Search(path, findere=3)
    # one locus: the group's queries are split over work-groups that write partial states, the merge kernel folds them
    assert _check(s, [fb], queries, _offsets([300]), 3, thresholds=(0.0, 0.8), limits=(0, 10)) > 0
    n = s.best_ms()
    assert n["split_groups"] == 1 and n["pieces"] == 5 and n["own_spans"] == 0 and n["best_ms"] > 0 and n["select_ms"] > 0
    # 150 pairs: every cell of the state has one writer
    _check(s, [fb], queries, _offsets([2] * 150), 3, thresholds=(0.8,), limits=(0,))
    n = s.best_ms()
    assert n["own_spans"] == 150 and n["pieces"] == 0 and n["split_groups"] == 0
    # the mirror's objects and its group_size form
    want = B.results([fb], queries, _offsets([2] * 150), 3, "error", 0.8, 3)
    got = s.search_best(queries, group_size=2, threshold=0.8, num_results=3)
    assert [[(r.doc_name, r.file_no, r.doc, r.query, r.score, r.positions, r.ties) for r in g] for g in got] == \
           [[(s.doc_name(f, d), f, d, q, sc, p, t) for (f, d, q, sc, p, t) in g] for g in want]
    s.close()


def test_every_score_width(gpu_lib, data, oracle):
    path, fb = data["c1"]
    src = data["src"]
    s = gpu_lib.Search(path)
    reads = _reads(src, 6, 50, 200, 41)                                            # <= 255 terms: u8 rows
    mid = [src[:330], src[100:100 + 3000 - 100], src[7:7 + 1200]]                  # 300 .. 3000 terms: u16 rows
    long_q = oracle.random_sequence(66000, 99)                                     # u32 rows
    for queries, sizes in ((mid, [1, 2]), (reads[:2] + mid + reads[2:], [3, 0, 6]), ([long_q], [1]),
                           (reads[:3] + [long_q] + mid[:1], [2, 3])):
        _check(s, [fb], queries, _offsets(sizes), 0, thresholds=(0.0, 0.8), limits=(0, 10))
    # one group whose members come in passes of all three widths: the stored state is merged across them
    queries = reads[:3] + mid + [long_q] + reads[3:]
    s.set_tuning("pass_bytes", 3 * 304 + 1)
    p0 = s.host_passes
    _check(s, [fb], queries, _offsets([len(queries)]), 0, thresholds=(0.0, 0.8), limits=(0,))
    assert s.host_passes - p0 >= 2 * 5
    s.set_tuning("pass_bytes", 0)
    s.close()


def test_groups_cut_by_a_device_pass_at_every_member_position(gpu_lib, data):
    path, fb = data["c1"]
    src = data["src"]
    rng = np.random.default_rng(5)
    queries = [src[o:o + 100] for o in rng.integers(0, len(src) - 100, 16).tolist()]     # equal lengths: passes of equal size
    queries[9] = queries[6]                                                              # (a tie across a cut)
    offsets = _offsets([5, 7, 0, 4])
    s = gpu_lib.Search(path)
    one = [s.search_best_arrays(queries, offsets, t, 0) for t in (0.0, 0.8)]
    # 464 bytes of tables per query: passes of 1 (a cut at every member position), 2, 3 and 5 queries
    for per_pass in (1, 2, 3, 5):
        s.set_tuning("pass_bytes", 464 * per_pass + 8)
        for (o1, h1), t in zip(one, (0.0, 0.8)):
            p0 = s.host_passes
            o2, h2 = s.search_best_arrays(queries, offsets, t, 0)
            assert s.host_passes - p0 == -(-16 // per_pass) == s.best_ms()["passes"]
            assert np.array_equal(o1, o2) and np.array_equal(h1, h2), per_pass
    _check(s, [fb], queries, offsets, 0, thresholds=(0.0, 0.8), limits=(0, 1))
    s.set_tuning("pass_bytes", 0)
    s.close()


def test_ties_built_on_purpose(gpu_lib, data):
    path, fb = data["c1"]                          # documents 0 and 7 hold every k-mer of src
    src = data["src"]
    a, b = src[200:290], src[1000:1140]
    pieces = [src[50:50 + n] for n in (60, 140, 100, 139)]
    queries = [a, b, a] + pieces + [b, b]
    offsets = _offsets([3, 4, 2])
    s = gpu_lib.Search(path)
    for pass_bytes in (0, 200):                    # in one pass, and every member in a pass of its own
        s.set_tuning("pass_bytes", pass_bytes)
        p0 = s.host_passes
        _check(s, [fb], queries, offsets, 0, thresholds=(0.0, 1.0), limits=(0, 1))
        assert s.host_passes - p0 == 4 * (len(queries) if pass_bytes else 1)
        got = _lists(*s.search_best_arrays(queries, offsets, 1.0, 0))
        by_doc = [{(f, d): (q, sc, p, t) for (f, d, q, sc, p, t) in g} for g in got]
        # members of different length that a complete document holds entirely: all tie at 1, the longest wins
        assert by_doc[0][(0, 0)] == (1, 110, 110, 3) and by_doc[1][(0, 7)] == (4, 110, 110, 4)
        # two identical members: both are counted, the lower index wins
        assert by_doc[2][(0, 0)] == (7, 110, 110, 2)
        every = _lists(*s.search_best_arrays([a, a], [0, 2], 0.0, 0))[0]
        assert len(every) == 300 and all(q == 0 and t == 2 for (_f, _d, q, _s, _p, t) in every)
        # an exact tie at the num_results cut: the two complete documents carry the same record
        assert tuple(got[1][0][:2]) == (0, 0) and tuple(got[1][1][:2]) == (0, 7) and got[1][0][2:] == got[1][1][2:]
        assert _lists(*s.search_best_arrays(queries, offsets, 1.0, 1))[1] == [got[1][0]]
    s.set_tuning("pass_bytes", 0)
    s.close()


def test_two_files_of_different_term_size(gpu_lib, data):
    paths = [data["c1"][0], data["c2k20"][0], data["p3"][0]]
    files = [data["c1"][1], data["c2k20"][1], data["p3"][1]]
    queries = _reads(data["src"], 12, 50, 150, 51) + [data["src"][:900]]
    offsets = _offsets([2, 0, 10, 1])
    s = gpu_lib.Search(paths)
    for z in (0, 3):
        s.set_findere(z)
        assert _check(s, files, queries, offsets, z, limits=(0, 10)) > 0
    # the same member has another P in every file: the lane picked its file's
    rows = _lists(*s.search_best_arrays(queries, offsets, 0.0, 0))[3]
    assert {(f, p) for (f, _d, _q, _s, p, _t) in rows} == {(0, 900 - 31 + 1 - 3), (1, 900 - 20 + 1 - 3), (2, 900 - 25 + 1 - 3)}
    s.close()


@pytest.mark.parametrize("mode", ["miss", "skip"])
def test_invalid_bases(gpu_lib, data, mode):
    path, fb = data["c1"]
    src = data["src"]
    clean = _reads(src, 6, 60, 140, 61)
    with_n = [I.with_n(q, [10]) for q in clean[:3]] + [I.with_n(clean[3], [0, 40, 41]), I.with_n(clean[4], range(20, 30))]
    queries = clean + with_n + [b"N" * 80, b"N" * 45] + [b"N" * 70, src[300:400], b"N" * 60]
    offsets = _offsets([6, 5, 2, 0, 3])           # clean | reads with N | no valid position at all | empty | all-N beside a hit
    s = gpu_lib.Search(path, invalid_bases=mode)
    for z in (0, 3):
        s.set_findere(z)
        assert _check(s, [fb], queries, offsets, z, mode, limits=(0, 10)) > 0
    got = _lists(*s.search_best_arrays(queries, offsets, 0.0, 0))
    assert len(got[2]) == 300 and all(sc == 0 and t == 2 for (_f, _d, _q, sc, _p, t) in got[2])
    if mode == "skip":
        assert all(p == 0 and q == 11 for (_f, _d, q, _s, p, _t) in got[2])           # P = 0: the lower index
    # the all-N members never win over the member with a hit, and a group of them is never reported at a threshold > 0
    assert all(q == 14 for (_f, _d, q, sc, _p, _t) in got[4] if sc > 0) and any(sc > 0 for (_f, _d, _q, sc, _p, _t) in got[4])
    hit = _lists(*s.search_best_arrays(queries, offsets, 0.5, 0))
    assert hit[2] == [] and hit[4] and all(q == 14 for (_f, _d, q, _s, _p, _t) in hit[4])
    s.close()


def _raw_call(s, queries, offsets, t, lim, cap):
    from cobs_amd import _capi
    lib = _capi.load()
    nq, ng = len(queries), len(offsets) - 1
    arr = (C.c_char_p * max(nq, 1))(*queries)
    lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in queries])
    goffs = np.ascontiguousarray(offsets, dtype=np.uint64)
    hits = np.full(max(cap, 1) * 6, 0xA5A5A5A5, dtype=np.uint32).view(s.BEST_HIT_DTYPE)
    hoffs = np.zeros(ng + 1, dtype=np.uint64)
    bad = C.c_size_t(12345)
    st = lib.cobs_gpu_search_best(s._h, arr, lens, nq, C.cast(goffs.ctypes.data, C.POINTER(C.c_size_t)), ng, t, lim,
                                  C.cast(hits.ctypes.data, C.POINTER(_capi.BestHit)), cap,
                                  C.cast(hoffs.ctypes.data, C.POINTER(C.c_size_t)), C.byref(bad))
    return st, hoffs, hits, bad.value, lib.cobs_gpu_last_error().decode()


def test_pool_overflow_and_caller_capacity(gpu_lib, data):
    from cobs_amd import _capi
    path, fb = data["c1"]
    queries = _reads(data["src"], 20, 50, 120, 71)
    offsets = _offsets([4, 10, 6])
    s = gpu_lib.Search(path)
    want = [s.search_best_arrays(queries, offsets, t, 0) for t in (0.0, 0.5)]
    # a first pool guess that is too small: the selection runs again with the size the kernel reported
    s.set_tuning("hit_cap", 5)
    for (o1, h1), t in zip(want, (0.0, 0.5)):
        o2, h2 = s.search_best_arrays(queries, offsets, t, 0)
        assert np.array_equal(o1, o2) and np.array_equal(h1, h2) and len(h1) > 5
    _check(s, [fb], queries, offsets, 0, thresholds=(0.0, 0.5), limits=(0, 10))
    s.set_tuning("hit_cap", 0)
    # a caller's buffer that is too small: the needed sizes, nothing written; the second call succeeds
    need = len(want[1][1])
    st, hoffs, hits, _bad, msg = _raw_call(s, queries, offsets, 0.5, 0, need - 1)
    assert st == _capi.ERR_CAPACITY and int(hoffs[-1]) == need and np.array_equal(hoffs, want[1][0]), msg
    assert np.all(hits.view(np.uint32) == 0xA5A5A5A5)
    st, hoffs, hits, _bad, msg = _raw_call(s, queries, offsets, 0.5, 0, int(hoffs[-1]))
    assert st == _capi.OK and np.array_equal(hoffs, want[1][0]) and np.array_equal(hits[:need], want[1][1]), msg
    ms = s.best_ms()
    assert ms["best_ms"] > 0 and ms["select_ms"] > 0 and ms["order_ms"] >= 0
    s.close()


def test_refusals(gpu_lib, data):
    from cobs_amd import _capi
    path, fb = data["p1"]
    src = data["src"]
    good = [src[:100], src[200:340], src[400:480]]
    for kw, word in (({"hbm_budget": 256 << 20}, "budget"), ({"shard_rank": 0, "shard_count": 2}, "shard")):
        s = gpu_lib.Search(path, **kw)
        with pytest.raises(gpu_lib.CobsGpuError) as e:
            s.search_best(good, [0, 3])
        assert e.value.status == _capi.ERR_UNSUPPORTED and word in str(e.value)
        s.close()
    s = gpu_lib.Search(path, findere=3)
    for offsets in ([1, 3], [0, 2], [0, 2, 1, 3], [0, 4]):
        st, _o, _h, _b, msg = _raw_call(s, good, offsets, 0.5, 0, 100)
        assert st == _capi.ERR_ARG and "group_offsets" in msg, (offsets, msg)
    lib = _capi.load()
    assert lib.cobs_gpu_search_best(s._h, None, None, 3, None, 1, 0.0, 0, None, 0, None, None) == _capi.ERR_ARG
    p0 = s.host_passes
    st, _o, _h, bad, msg = _raw_call(s, [good[0], good[1], src[:31 + 2]], [0, 3], 0.5, 0, 100)
    assert st == _capi.ERR_QUERY_TOO_SHORT and bad == 2 and str(31 + 3) in msg and "(query 2)" in msg
    assert s.host_passes == p0                                             # (refused before anything was launched)
    st, _o, _h, bad, msg = _raw_call(s, [good[0], good[1][:50] + b"N" + good[1][51:], good[2]], [0, 1, 3], 0.5, 0, 100)
    assert st == _capi.ERR_INVALID_BASE and bad == 1 and "(query 1)" in msg
    # the handle still answers
    _check(s, [fb], good, [0, 1, 3], 3, thresholds=(0.8,), limits=(0,))
    s.close()


def test_between_the_other_call_families_on_one_handle(gpu_lib, data):
    """search -> search_best -> search_groups -> search_best -> search_weighted -> search_best: every result is checked"""
    paths = [data["c3"][0], data["p1"][0]]
    files = [data["c3"][1], data["p1"][1]]
    queries = _reads(data["src"], 11, 50, 150, 81) + [data["src"][:700]]
    offsets = _offsets([3, 0, 8, 1])
    s = gpu_lib.Search(paths, findere=1)

    def best():
        _check(s, files, queries, offsets, 1, thresholds=(0.0, 0.8), limits=(0, 10))

    so, sh = s.search_arrays(queries, 0.8, 0)
    rows = sh.tolist()
    for i, q in enumerate(queries):
        assert [tuple(r) for r in rows[int(so[i]):int(so[i + 1])]] == F.results(files, q, 1, 0.8, 0)
    best()
    want, want_p = G.results(files, queries, offsets, 1, "error", 0.8, 0.8, 0)
    go, gh, gp = s.search_groups_arrays(queries, offsets, 0.8, 0.8, 0)
    assert [tuple(r) for g in _lists(go, gh) for r in g] == [r for g in want for r in g] and np.array_equal(gp, want_p)
    best()
    wo, wh, _total = s.search_weighted_arrays(queries[:4], 0.5, 0)
    rows = wh.tolist()
    for i, q in enumerate(queries[:4]):
        assert rows[int(wo[i]):int(wo[i + 1])] == W.results(files, q, 1, 0.5, 0)
    best()
    s.close()


def test_no_device_memory_growth_over_repeated_calls(gpu_lib, data):
    import torch
    path, _fb = data["p1"]
    queries = _reads(data["src"], 80, 40, 90, 91)
    s = gpu_lib.Search(path)

    def cycle():
        s.search_best_arrays(queries, _offsets([80]), 0.0, 0)           # (partial states)
        s.search_best_arrays(queries, _offsets([8] * 10), 0.5, 3)
    cycle()
    gc.collect()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(20):
        cycle()
    gc.collect()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < (32 << 20), (free0, free1)
    s.close()
