"""GPU: grouped search (cobs_gpu_search_groups / Search.search_groups / search_paired / ClassicSearch::search_groups /
--group) record for record against tests/groups_check.py: file, document, sum, votes and order of every group, and P.

Classic and compact layouts (padding documents, sub-indexes of 1, 2, 65 and 4097 rows), a handle over files of different
term size, every score width, group sizes around the wave and the query-span split, one group over all queries (the
atomic path) and many small ones (the one-writer path), groups that span device passes, thresholds, limits and an exact
tie at the cut, findere, `miss` / `skip`, the selection pool's overflow, the caller's capacity, and every refusal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import cases
from tests import findere_check as F
from tests import groups_check as G
from tests import invalid_check as I

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = (0.0, 0.5, 0.8, 1.0)
READ_THRESHOLDS = (0.0, 0.8)
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
    """index files with planted documents (two of them complete: an exact tie at the top of every list)"""
    d = tmp_path_factory.mktemp("groups")
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


def _check(s, files, queries, offsets, z=0, mode="error", thresholds=THRESHOLDS, read_thresholds=READ_THRESHOLDS, limits=LIMITS):
    """every record of every group equals the checker's; -> the records selected at a threshold > 0"""
    selected = 0
    for t in thresholds:
        for rt in read_thresholds:
            want_full, want_p = G.results(files, queries, offsets, z, mode, t, rt, 0)
            for lim in limits:
                offs, hits, pos = s.search_groups_arrays(queries, offsets, t, rt, lim)
                want = [w[:lim] if lim else w for w in want_full]
                got = _lists(offs, hits)
                assert [tuple(r) for g in got for r in g] == [r for g in want for r in g], (z, mode, t, rt, lim)
                assert [len(g) for g in got] == [len(g) for g in want]
                assert np.array_equal(pos, want_p), (z, mode)
                selected += len(hits) if t > 0 else 0
    return selected


@pytest.mark.parametrize("name", ["c1", "c3", "p1", "p3", "tiny"])
def test_every_layout_threshold_read_threshold_and_limit(gpu_lib, oracle, data, name):
    path, fb = data[name]
    src = data["src"]
    queries = _reads(src, 14, 50, 150, 11) + [oracle.random_sequence(120, 5)]
    offsets = _offsets([0, 1, 2, 5, 0, 7, 0])
    s = gpu_lib.Search(path)
    for z in (0, 3):
        s.set_findere(z)
        assert _check(s, [fb], queries, offsets, z) > 0            # (the thresholds did select planted documents)
    # an exact tie at the cut: the two complete documents have the same sum, num_results = 1 keeps the first
    s.set_findere(0)
    offs, hits, _pos = s.search_groups_arrays(queries, offsets, 1.0, 0.8, 0)
    full = _lists(offs, hits)[3]
    assert len(full) >= 2 and full[0][2] == full[1][2] and (full[0][0], full[0][1]) < (full[1][0], full[1][1])
    offs, hits, _pos = s.search_groups_arrays(queries, offsets, 1.0, 0.8, 1)
    assert _lists(offs, hits)[3] == [full[0]]
    s.close()


def test_group_sizes_around_the_wave_and_the_span_split(gpu_lib, data):
    path, fb = data["c1"]
    sizes = [0, 1, 2, 63, 64, 65, 300, 0]
    queries = _reads(data["src"], sum(sizes), 40, 60, 21)
    s = gpu_lib.Search(path)
    assert _check(s, [fb], queries, _offsets(sizes), 0, thresholds=(0.0, 0.5), read_thresholds=(0.8,), limits=(0,)) > 0
    s.close()


def test_one_group_over_all_queries_and_many_groups_of_two(gpu_lib, data):
    path, fb = data["p1"]
    queries = _reads(data["src"], 300, 40, 70, 31)
    s = gpu_lib.Search(path, findere=3)
    # one sample: the group's queries are split over work-groups that combine with atomics
    assert _check(s, [fb], queries, _offsets([300]), 3, thresholds=(0.0, 0.8), limits=(0, 10)) > 0
    # 150 pairs: every accumulator cell has one writer
    offsets = _offsets([2] * 150)
    _check(s, [fb], queries, offsets, 3, thresholds=(0.8,), read_thresholds=(0.8,), limits=(0,))
    want, _p = G.results([fb], queries, offsets, 3, "error", 0.8, 0.8, 0)
    got = s.search_paired(queries[0::2], queries[1::2], 0.8, 0.8)
    assert [[(r.doc_name, r.score, r.votes) for r in g] for g in got] == \
           [[(s.doc_name(f, d), sc, v) for (f, d, sc, v) in g] for g in want]
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
        _check(s, [fb], queries, _offsets(sizes), 0, thresholds=(0.0, 0.8), read_thresholds=(0.8,), limits=(0, 10))
    s.close()


def test_groups_that_span_device_passes(gpu_lib, data):
    path, fb = data["c1"]
    src = data["src"]
    rng = np.random.default_rng(5)
    queries = [src[o:o + 100] for o in rng.integers(0, len(src) - 100, 60).tolist()]     # equal lengths: passes of equal size
    offsets = _offsets([6, 3, 21, 6, 24])
    s = gpu_lib.Search(path)
    one = [s.search_groups_arrays(queries, offsets, t, 0.8, 0) for t in (0.0, 0.8)]
    before = s.host_passes
    # 464 bytes of tables per query: passes of 6 queries (cuts at the end of group 0, inside group 2 three times, at the
    # start of group 3), of 4 and of 8
    for pass_bytes, passes in ((3000, 10), (2000, 15), (4000, 8)):
        s.set_tuning("pass_bytes", pass_bytes)
        for (o1, h1, p1), t in zip(one, (0.0, 0.8)):
            p0 = s.host_passes
            o2, h2, p2 = s.search_groups_arrays(queries, offsets, t, 0.8, 0)
            assert s.host_passes - p0 == passes
            assert np.array_equal(o1, o2) and np.array_equal(h1, h2) and np.array_equal(p1, p2), pass_bytes
    assert s.host_passes > before
    _check(s, [fb], queries, offsets, 0, thresholds=(0.0, 0.8), read_thresholds=(0.8,), limits=(0, 1))
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
    res, pos = s.search_groups(queries, offsets, 0.8, 0.8, return_positions=True)
    assert pos.shape == (4, 3) and int(pos[0, 0]) != int(pos[0, 1])                # per-file P
    want, want_p = G.results(files, queries, offsets, 3, "error", 0.8, 0.8, 0)
    assert [[(r.doc_name, r.score, r.votes) for r in g] for g in res] == \
           [[(s.doc_name(f, d), sc, v) for (f, d, sc, v) in g] for g in want]
    s.close()


@pytest.mark.parametrize("mode", ["miss", "skip"])
def test_invalid_bases(gpu_lib, data, mode):
    path, fb = data["c1"]
    src = data["src"]
    clean = _reads(src, 6, 60, 140, 61)
    with_n = [I.with_n(q, [10]) for q in clean[:3]] + [I.with_n(clean[3], [0, 40, 41]), I.with_n(clean[4], range(20, 30))]
    all_n = [b"N" * 80, b"N" * 45]
    queries = clean + with_n + all_n
    offsets = _offsets([6, 5, 2, 0, 1])           # clean | reads with N | no valid position at all | empty | one all-N read
    queries = queries + [b"N" * 60]
    s = gpu_lib.Search(path, invalid_bases=mode)
    for z in (0, 3):
        s.set_findere(z)
        assert _check(s, [fb], queries, offsets, z, mode, limits=(0, 10)) > 0
    offs, hits, pos = s.search_groups_arrays(queries, offsets, 0.5, 0.8, 0)
    if mode == "skip":
        assert int(pos[2, 0]) == 0 and int(pos[4, 0]) == 0
    assert _lists(offs, hits)[2] == [] and _lists(offs, hits)[4] == []              # P = 0 (or no score): nothing
    s.close()


def _raw_call(s, queries, offsets, t, rt, lim, cap):
    from cobs_amd import _capi
    lib = _capi.load()
    nq, ng = len(queries), len(offsets) - 1
    arr = (C.c_char_p * max(nq, 1))(*queries)
    lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in queries])
    goffs = np.ascontiguousarray(offsets, dtype=np.uint64)
    hits = np.full(max(cap, 1), 0xA5A5A5A5, dtype=np.uint32).repeat(4).view(s.GROUP_HIT_DTYPE)
    hoffs = np.zeros(ng + 1, dtype=np.uint64)
    bad = C.c_size_t(12345)
    st = lib.cobs_gpu_search_groups(s._h, arr, lens, nq, C.cast(goffs.ctypes.data, C.POINTER(C.c_size_t)), ng, t, rt, lim,
                                    C.cast(hits.ctypes.data, C.POINTER(_capi.GroupHit)), cap,
                                    C.cast(hoffs.ctypes.data, C.POINTER(C.c_size_t)), None, C.byref(bad))
    return st, hoffs, hits, bad.value, lib.cobs_gpu_last_error().decode()


def test_pool_overflow_and_caller_capacity(gpu_lib, data):
    from cobs_amd import _capi
    path, fb = data["c1"]
    queries = _reads(data["src"], 20, 50, 120, 71)
    offsets = _offsets([4, 10, 6])
    s = gpu_lib.Search(path)
    want = [s.search_groups_arrays(queries, offsets, t, 0.8, 0) for t in (0.0, 0.5)]
    # a first pool guess that is too small: the selection runs again with the size the kernel reported
    s.set_tuning("hit_cap", 5)
    for (o1, h1, _p), t in zip(want, (0.0, 0.5)):
        o2, h2, _p2 = s.search_groups_arrays(queries, offsets, t, 0.8, 0)
        assert np.array_equal(o1, o2) and np.array_equal(h1, h2) and len(h1) > 5
    _check(s, [fb], queries, offsets, 0, thresholds=(0.0, 0.5), read_thresholds=(0.8,), limits=(0, 10))
    s.set_tuning("hit_cap", 0)
    # a caller's buffer that is too small: the needed sizes, nothing written; the second call succeeds
    need = len(want[1][1])
    st, hoffs, hits, _bad, msg = _raw_call(s, queries, offsets, 0.5, 0.8, 0, need - 1)
    assert st == _capi.ERR_CAPACITY and int(hoffs[-1]) == need and np.array_equal(hoffs, want[1][0]), msg
    assert np.all(hits.view(np.uint32) == 0xA5A5A5A5)
    st, hoffs, hits, _bad, msg = _raw_call(s, queries, offsets, 0.5, 0.8, 0, int(hoffs[-1]))
    assert st == _capi.OK and np.array_equal(hoffs, want[1][0]) and np.array_equal(hits[:need], want[1][1]), msg
    ms = s.groups_ms()
    assert ms["accumulate_ms"] > 0 and ms["select_ms"] > 0 and ms["order_ms"] >= 0
    s.close()


def test_refusals(gpu_lib, data):
    from cobs_amd import _capi
    path, fb = data["p1"]
    src = data["src"]
    good = [src[:100], src[200:340], src[400:480]]
    for kw, word in (({"hbm_budget": 256 << 20}, "budget"), ({"shard_rank": 0, "shard_count": 2}, "shard")):
        s = gpu_lib.Search(path, **kw)
        with pytest.raises(gpu_lib.CobsGpuError) as e:
            s.search_groups(good, [0, 3])
        assert e.value.status == _capi.ERR_UNSUPPORTED and word in str(e.value)
        s.close()
    s = gpu_lib.Search(path, findere=3)
    for offsets in ([1, 3], [0, 2], [0, 2, 1, 3], [0, 4]):
        st, _o, _h, _b, msg = _raw_call(s, good, offsets, 0.5, 0.0, 0, 100)
        assert st == _capi.ERR_ARG and "group_offsets" in msg, (offsets, msg)
    lib = _capi.load()
    assert lib.cobs_gpu_search_groups(s._h, None, None, 3, None, 1, 0.0, 0.0, 0, None, 0, None, None, None) == _capi.ERR_ARG
    st, _o, _h, bad, msg = _raw_call(s, [good[0], good[1], src[:31 + 2]], [0, 3], 0.5, 0.0, 0, 100)
    assert st == _capi.ERR_QUERY_TOO_SHORT and bad == 2 and str(31 + 3) in msg and "(query 2)" in msg
    st, _o, _h, bad, msg = _raw_call(s, [good[0], good[1][:50] + b"N" + good[1][51:], good[2]], [0, 1, 3], 0.5, 0.0, 0, 100)
    assert st == _capi.ERR_INVALID_BASE and bad == 1 and "(query 1)" in msg
    # the handle still answers
    _check(s, [fb], good, [0, 1, 3], 3, thresholds=(0.8,), read_thresholds=(0.8,), limits=(0,))
    s.close()


def test_groups_of_one_are_the_search(gpu_lib, data):
    """threshold == read_threshold and one query per group: the group's records are that query's hits (queries with more
    than one hash in total: the reference's index-order rule does not come into it), every one with one vote"""
    paths = [data["c3"][0], data["p1"][0]]
    queries = _reads(data["src"], 10, 50, 150, 81) + [data["src"][:700]]
    s = gpu_lib.Search(paths)
    for z, mode in ((0, "error"), (3, "error"), (3, "skip")):
        s.set_findere(z)
        s.invalid_bases = mode
        qs = queries if mode == "error" else queries + [I.with_n(queries[0], [12])]
        for t in (0.0, 0.8, 1.0):
            so, sh = s.search_arrays(qs, t, 0)
            go, gh, _p = s.search_groups_arrays(qs, np.arange(len(qs) + 1), t, t, 0)
            assert np.array_equal(so, go)
            for col in ("file_no", "doc", "score"):
                assert np.array_equal(sh[col], gh[col]), (z, mode, t, col)
            assert np.all(gh["votes"] == 1)
    s.close()


def test_cli_groups(gpu_lib, data, tmp_path):
    tool = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")
    paths = [data["c1"][0], data["c2k20"][0]]
    files = [data["c1"][1], data["c2k20"][1]]
    queries = _reads(data["src"], 7, 50, 150, 91)
    fa = tmp_path / "reads.fa"
    fa.write_text("".join(">read%d\n%s\n" % (i, q.decode()) for i, q in enumerate(queries)))
    s = gpu_lib.Search(paths)
    base = [tool] + [a for p in paths for a in ("-i", p)] + ["-f", str(fa)]
    for group, sizes, t, rt, lim, z in (("2", [2, 2, 2, 1], 0.8, 0.8, 0, 0), ("all", [7], 0.5, 0.9, 5, 3), ("3", [3, 3, 1], 0.0, 0.0, 2, 0)):
        r = subprocess.run(base + ["--group", group, "-t", str(t), "--read-threshold", str(rt), "-l", str(lim), "--findere", str(z)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        offsets = _offsets(sizes)
        want, _p = G.results(files, queries, offsets, z, "error", t, rt, lim)
        text = ""
        for g, rows in enumerate(want):
            text += "*read%d\t%d\n" % (int(offsets[g]), len(rows))
            text += "".join("%s\t%d\t%d\n" % (s.doc_name(f, d), sc, v) for (f, d, sc, v) in rows)
        assert r.stdout == text, (group, r.stdout[:300])
    # without --group the output is what it was: one block per record, two columns
    r = subprocess.run(base + ["-t", "0.8"], capture_output=True, text=True, timeout=300)
    want = "".join("*read%d\t%d\n%s" % (i, len(res), "".join("%s\t%d\n" % (s.doc_name(f, d), sc) for f, d, sc in res))
                   for i, res in enumerate(F.results(files, q, 0, 0.8, 0) for q in queries))
    assert r.returncode == 0 and r.stdout == want
    s.close()
