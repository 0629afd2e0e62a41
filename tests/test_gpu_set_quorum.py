"""GPU: quorum scoring and per-set prevalence of the document sets (cobs_gpu_search_sets_quorum / cobs_gpu_set_prevalence,
Search.search_sets_quorum / set_prevalence, ClassicSearch::search_sets_quorum / set_prevalence, --sets-quorum /
--sets-profile) element by element against tests/set_quorum_check.py: for every labelled set of documents how many members
hold each position of a query, and the positions held by at least need = max(1, ceil(quorum * members)) of them.  Every
comparison is exact.

Classic rows from one byte to wider than a 16-byte chunk, compact sub-indexes of 2 and 16 row bytes and 1 to 4097 rows, a
last sub-index that is partly filled or all padding, padding slots that hold bits; on each of them the labellings of the set
search (every document its own set, one set of all, d % 5, runs of 37 that straddle chunk and sub-index borders, unlabelled
documents and unused set numbers), contiguous runs cut at slots 127 | 128 and inside a chunk, and round-robin over 129 sets
(128 records per column chunk); position counts at the borders of the lane groups; z = 0 and 2; the quorums, thresholds and
limits; the identities through the library itself; two files of which one is labelled, the invalid-bases policies, the
smallest pass, the wide table, relabelling, the capacity protocols, every refusal, the mirrors, the CLI, the timer and
device memory; rows of 71 column chunks under sets of 1000 to 9000 documents (8, 16, 32 and 64 lanes per position, the stride
loop, several position slabs), and more runs than one launch takes."""
import ctypes as C
import gc
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import invalid_check as I
from tests import set_quorum_check as Q
from tests.test_gpu_prevalence import _classic, _compact, _edge_queries      # the files the prevalence tests are built on
from tests.test_gpu_sets import _two_files, labelings

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 31, 32, 33, 64, 65, 200)                     # position counts n
ZS = (0, 2)
QUORUMS = (1e-9, 0.5, 0.95, 1.0)
THRESHOLDS = (0.0, 0.3, 0.9)
LIMITS = (0, 1, 3)


def quorum_labelings(num_docs):
    d = np.arange(num_docs)
    out = dict(labelings(num_docs))
    # contiguous runs cut at slots 127 | 128 and inside a chunk (at 50 and 200); set 1 is never used
    out["cuts"] = np.select([d < 50, d < 128, d < 200], [0, 2, 3], 4)
    # every column chunk of 128 slots holds 128 different sets: more records per chunk than any register batch
    out["rr129"] = d % 129
    return out


@pytest.fixture(scope="module")
def src(oracle):
    return oracle.random_sequence(3000, 77)


def _rows(hits):
    return np.stack([hits[f].astype(np.int64) for f in ("file_no", "set", "core", "any")], axis=1).reshape(-1, 4)


def _check(s, files, labs, queries, z, mode="error", quorums=QUORUMS, thresholds=THRESHOLDS, limits=LIMITS):
    offs, counts = s.set_prevalence_arrays(queries)
    want_offs, want = Q.segments(files, labs, queries, z, mode)
    assert offs.dtype == np.uint64 and counts.dtype == np.uint32
    assert np.array_equal(offs, want_offs), (z, mode, offs, want_offs)
    assert np.array_equal(counts, want), (z, mode, np.nonzero(counts != want)[0][:8])
    for quorum, t, k in itertools.product(quorums, thresholds, limits):
        offs, hits = s.search_sets_quorum_arrays(queries, quorum, t, k)
        want_offs, want = Q.arrays(files, labs, queries, z, quorum, t, k, mode)
        assert offs.dtype == np.uint64 and hits.dtype == s.SET_QUORUM_HIT_DTYPE
        assert np.array_equal(offs, want_offs), (z, quorum, t, k, offs, want_offs)
        got = _rows(hits)
        assert np.array_equal(got, want), (z, quorum, t, k, np.nonzero((got != want).any(axis=1))[0][:8])
    return counts


def _sweep(gpu_lib, path, fb, src, zs=ZS, ns=NS):
    s = gpu_lib.Search(path)
    for name, labels in quorum_labelings(fb.num_docs).items():
        s.set_doc_sets(labels)
        for z in zs:
            s.set_findere(z)
            qs = _edge_queries(src, fb.term_size, z, ns)
            assert [fb.positions(q, z) for q in qs] == list(ns)
            _check(s, [fb], [labels], qs, z)
    s.close()


@pytest.mark.parametrize("num_hashes", [1, 3])
@pytest.mark.parametrize("num_docs", [1, 9, 129, 300])
def test_classic_layouts(gpu_lib, src, tmp_path, num_docs, num_hashes):
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), num_docs, 2003, num_hashes, 31, num_docs)
    _sweep(gpu_lib, path, fb, src)


@pytest.mark.parametrize("sigs", [[1, 2, 65, 4097], [1201, 997, 1500, 1103, 1301, 800]])
@pytest.mark.parametrize("page_size", [2, 16])
def test_compact_layouts(gpu_lib, src, tmp_path, page_size, sigs):
    """a last sub-index that is partly filled; runs of 37 and the cuts span sub-index borders"""
    num_docs = len(sigs) * 8 * page_size - 5 * page_size - 3
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), num_docs, page_size, sigs, 1, 31, page_size)
    _sweep(gpu_lib, path, fb, src)


def test_trailing_sub_index_of_padding(gpu_lib, src, tmp_path):
    path, fb = _compact(str(tmp_path / "t.cobs_compact"), 2 * 128 - 9, 16, [501, 703, 601], 1, 31, 5)
    assert (fb.doc_of_slot()[256:] < 0).all()
    _sweep(gpu_lib, path, fb, src, ns=(1, 33, 200))


def test_padding_slots_with_set_bits_never_count(gpu_lib, src, tmp_path):
    """files written WITHOUT masking the padding documents: their slots hold random bits"""
    from tests import sets_check as S
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 5, 301, 1, 31, 3, mask=False)
    assert S.windows(fb, src[:200], 0)[:, 5:].any()
    _sweep(gpu_lib, path, fb, src, ns=(1, 33, 200))
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), 100, 8, [211, 307, 401], 2, 31, 4, mask=False)
    assert S.windows(fb, src[:200], 0)[:, 100:128].any() and S.windows(fb, src[:200], 0)[:, 128:].any()
    _sweep(gpu_lib, path, fb, src, ns=(1, 33, 200))


def wide_labelings(num_docs):
    """labellings of a page of 71 column chunks: runs of 8 to 71 records, so that the lanes of a position number 8, 16, 32
    and 64 and the longest run takes a second trip of the stride loop"""
    d = np.arange(num_docs)
    return {"one": np.zeros(num_docs, dtype=np.int64), "sets1000": d // 1000, "sets3000": d // 3000, "sets5000": d // 5000,
            "sparse": np.where(d % 4 == 1, -1, (d // 11) * 2)}


@pytest.mark.parametrize("z", ZS)
def test_wide_rows_every_lane_group_width_and_several_position_slabs(gpu_lib, src, tmp_path, z):
    """a classic file of 9000 documents: rows of 71 column chunks.  A set of 1000 documents is a run of 8 or 9 records (8 and
    16 lanes per position), of 3000 one of 24 or 25 (32 lanes), of 4000 / 5000 / 9000 one of 32 / 40 / 71 (64 lanes; 71: a
    second trip of the stride loop).  n = 2100 with 64 lanes per position is 2100 position groups: 66 slabs of work-groups."""
    num_docs = 9000
    path, fb = _classic(str(tmp_path / "w.cobs_classic"), num_docs, 2003, 1, 31, 17)
    ns = (1, 65, 200, 2100)
    qs = _edge_queries(src, 31, z, ns)
    assert [fb.positions(q, z) for q in qs] == list(ns)
    s = gpu_lib.Search(path, findere=z)
    seen = set()
    for name, labels in wide_labelings(num_docs).items():
        for c in Q.nonempty_sets(labels)[:12]:
            chunks = np.unique(np.nonzero(labels == c)[0] // 128)
            seen.add(min(64, 1 << int(np.ceil(np.log2(len(chunks))))))
            seen.add("loop" if len(chunks) > 64 else "once")
        s.set_doc_sets(labels)
        counts = _check(s, [fb], [labels], qs, z, quorums=(1e-9, 0.4), thresholds=(0.0, 0.3), limits=(0, 3))
        assert counts.any()
    assert seen >= {1, 8, 16, 32, 64, "loop", "once"}
    # the quorum bites on these fixtures: at z = 0 a set of 1000 has positions on both sides of need = 400
    if z == 0:
        core = [r[2] for r in Q.results([fb], [wide_labelings(num_docs)["sets1000"]], qs[3], 0, 0.4)]
        assert 0 < min(core) and max(core) < ns[3]
    s.close()


def test_more_runs_than_one_launch_takes(gpu_lib, src, tmp_path):
    """66 000 one-member sets in one page are 66 000 runs: the count kernel's grid takes 65 535 of them per launch, the rest
    go to a second launch that starts at run 65 535"""
    num_docs = 66000
    path, fb = _classic(str(tmp_path / "m.cobs_classic"), num_docs, 101, 1, 31, 23)
    qs = _edge_queries(src, 31, 0, (1, 33))
    labels = np.arange(num_docs)
    s = gpu_lib.Search(path)
    s.set_doc_sets(labels)
    counts = _check(s, [fb], [labels], qs, 0, quorums=(0.5,), thresholds=(0.0, 0.5), limits=(0, 3))
    tail = counts.reshape(-1)[-33 * (num_docs - 65535):]             # the cells of the second launch, query of 33 positions
    assert tail.any() and counts.max() == 1
    s.close()


def test_the_layout_tests_are_not_vacuous(src, tmp_path):
    """on the CHECKER's answer over the queries and labellings of the classic layouts: a set whose core at quorum 0.5 differs
    from both any and all, a count strictly between 0 and members, a set cut by a threshold, and a chunk with more records
    than a register batch"""
    between = partial = cut = False
    for num_docs in (9, 300):
        _path, fb = _classic(str(tmp_path / ("c%d.cobs_classic" % num_docs)), num_docs, 2003, 1, 31, num_docs)
        for labels in quorum_labelings(num_docs).values():
            mem = Q.members(labels)
            for z in ZS:
                for q in _edge_queries(src, 31, z, NS):
                    prof = Q.profile(fb, q, z, labels)
                    half, lo, hi = (Q.counts(fb, q, z, labels, x) for x in (0.5, 1e-9, 1.0))
                    for i, c in enumerate(Q.nonempty_sets(labels)):
                        between |= hi[c][0] < half[c][0] < lo[c][0]
                        partial |= bool(((prof[i] > 0) & (prof[i] < mem[c])).any())
                    for t in THRESHOLDS[1:]:
                        cut |= 0 < len(Q.results([fb], [labels], q, z, 0.5, t)) < len(Q.results([fb], [labels], q, z, 0.5, 0.0))
    assert between and partial and cut
    assert len(set(quorum_labelings(300)["rr129"][:128].tolist())) == 128


@pytest.mark.parametrize("z", ZS)
def test_identities_through_the_library(gpu_lib, src, tmp_path, z):
    """quorum = 1 is the set search's `all`, need = 1 its `any`; one set of all documents is the prevalence; the profile of a
    one-member set is the hit_positions bits of its document"""
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), 700, 16, [1201, 997, 1500, 1103, 1301, 800], 1, 31, 3)
    s = gpu_lib.Search(path, findere=z)
    qs = _edge_queries(src, 31, z, NS)
    for name, labels in quorum_labelings(700).items():
        s.set_doc_sets(labels)
        offs, ref = s.search_sets_arrays(qs, 0.0, "all")
        for quorum, col in ((1.0, "all"), (1e-9, "any")):
            qoffs, got = s.search_sets_quorum_arrays(qs, quorum)
            assert np.array_equal(offs, qoffs) and len(got)
            for i in range(len(qs)):
                a, b = ref[int(offs[i]):int(offs[i + 1])], got[int(offs[i]):int(offs[i + 1])]
                want = dict(zip(a["set"].tolist(), zip(a[col].tolist(), a["any"].tolist())))
                assert dict(zip(b["set"].tolist(), zip(b["core"].tolist(), b["any"].tolist()))) == want, (name, quorum, i)
    s.set_doc_sets(np.zeros(700, dtype=np.int64))
    poffs, prev = s.prevalence_arrays(qs)
    soffs, counts = s.set_prevalence_arrays(qs)
    assert np.array_equal(poffs, soffs) and np.array_equal(prev, counts) and prev.any()
    s.set_doc_sets(np.arange(700))
    hits = np.zeros(700, dtype=gpu_lib.Search.HIT_DTYPE)
    hits["doc"] = np.arange(700)
    for i in (1, 6):
        prof = s.set_prevalence(qs[i])[0]
        assert prof.shape == (700, NS[i]) and prof.max() == 1
        _bo, bits = s.hit_positions([qs[i]], [0, 700], hits)
        unpacked = np.unpackbits(np.ascontiguousarray(bits.reshape(700, -1)).view(np.uint8), axis=1, bitorder="little")[:, :NS[i]]
        assert np.array_equal(prof, unpacked), i
    s.close()


def test_two_files_of_different_term_size_one_labelled_and_the_invalid_bases_policies(gpu_lib, src, tmp_path):
    from cobs_amd import _capi
    paths, files = _two_files(tmp_path)
    labs = [None, quorum_labelings(150)["runs37"]]
    base = src[40:40 + 160]
    queries = [base, I.with_n(base, [0]), I.with_n(base, [70, 150]), b"N" * 80, src[500:500 + 64]]
    for mode in I.MODES:
        s = gpu_lib.Search(paths, invalid_bases=mode)
        s.set_doc_sets(labs[1], file_no=1)
        for z in ZS:
            s.set_findere(z)
            _check(s, files, labs, queries, z, mode=mode, limits=(0, 3))
        prof = s.set_prevalence(queries[2])
        assert prof[0].shape == (0, 0) and prof[1].shape == (5, files[1].positions(queries[2], ZS[-1]))
        s.close()
    assert 0 < Q.denominator(files[1], queries[2], 0, "skip") < Q.denominator(files[1], queries[2], 0, "miss")
    # under `error` both calls name the query, and the handle still answers; both files labelled now
    s = gpu_lib.Search(paths, findere=1)
    labs = [quorum_labelings(300)["mod5"], labs[1]]
    s.set_doc_sets(labs[0], file_no=0)
    s.set_doc_sets(labs[1], file_no=1)
    for call in (lambda: s.search_sets_quorum(queries[:3], 0.5), lambda: s.set_prevalence(queries[:3])):
        with pytest.raises(gpu_lib.CobsGpuError) as e:
            call()
        assert e.value.status == _capi.ERR_INVALID_BASE and "(query 1)" in str(e.value)
    good = [queries[0], queries[4]]
    _check(s, files, labs, good, 1, limits=(0,))
    res = s.search_sets_quorum(good[0], 0.3, 0.0, 2)                 # the list form of one query
    want = Q.results(files, labs, good[0], 1, 0.3, 0.0, 2)
    assert [(r.file_no, r.set, r.name, r.core, r.any) for r in res] == [(f, c, str(c), a, b) for (f, c, a, b) in want] and len(res) == 2
    s.close()


def test_smallest_pass_relabelling_and_clearing(gpu_lib, src, tmp_path):
    """the smallest workspace that admits every single query cuts the call into many passes: same arrays; one byte less is
    refused; labels are replaced and taken away between calls, and the inverse records follow"""
    from cobs_amd import _capi
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), 700, 16, [1201, 997, 1500, 1103, 1301, 800], 1, 31, 3)
    labs = quorum_labelings(700)
    rng = np.random.default_rng(41)
    queries = []
    for _ in range(12):
        ln = int(rng.integers(50, 151))
        o = int(rng.integers(0, len(src) - ln))
        queries.append(src[o:o + ln])
    s = gpu_lib.Search(path, findere=2)
    s.set_doc_sets(labs["runs37"])
    nsets, z = len(Q.nonempty_sets(labs["runs37"])), 2
    s.set_quorum_ms()
    offs, hits = s.search_sets_quorum_arrays(queries, 0.1, 0.2)
    soffs, counts = s.set_prevalence_arrays(queries)
    t = s.set_quorum_ms()
    assert t["passes"] == 2 and 0 < len(hits) < nsets * len(queries)
    want_offs, want = Q.arrays([fb], [labs["runs37"]], queries, z, 0.1, 0.2)
    assert np.array_equal(offs, want_offs) and np.array_equal(_rows(hits), want)
    assert np.array_equal(counts, Q.segments([fb], [labs["runs37"]], queries, z)[1])
    # 4 bytes per (set, position), and for the search a 16-byte record per set
    cells = max(nsets * fb.positions(q, z) for q in queries)
    for limit, call, want in ((4 * cells + 16 * nsets, lambda: s.search_sets_quorum_arrays(queries, 0.1, 0.2), (offs, hits)),
                              (4 * cells, lambda: s.set_prevalence_arrays(queries), (soffs, counts))):
        s.set_tuning("pass_bytes", limit)
        got = call()
        assert 3 <= s.set_quorum_ms()["passes"] <= len(queries)      # (two short queries may share a pass)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        s.set_tuning("pass_bytes", limit - 1)
        with pytest.raises(gpu_lib.CobsGpuError) as e:
            call()
        assert e.value.status == _capi.ERR_HIP and "do not fit the pass workspace" in str(e.value) and str(limit) in str(e.value)
        assert s.set_quorum_ms()["passes"] == 0
    s.set_tuning("pass_bytes", 0)
    # relabelling replaces the labels: the results follow the new ones (the set search in between builds its own records)
    for name in ("sparse", "rr129", "cuts"):
        s.set_doc_sets(labs[name])
        if name == "rr129":
            s.search_sets_arrays(queries[:2])
        _check(s, [fb], [labs[name]], queries[:5], z, quorums=(0.5,), thresholds=(0.0, 0.05), limits=(0, 3))
    # clearing: empty segments and no records, and the plain search is not disturbed
    assert s.set_doc_sets(None) == []
    offs, hits = s.search_sets_quorum_arrays(queries, 0.5)
    soffs, counts = s.set_prevalence_arrays(queries)
    assert not offs.any() and len(hits) == 0 and not soffs.any() and len(counts) == 0
    assert [p[0].shape for p in s.set_prevalence(queries[:2])] == [(0, 0), (0, 0)]
    from tests import findere_check as F
    assert s.search_hits(queries[:3], 0.0, 3) == [F.results([fb], q, z, 0.0, 3) for q in queries[:3]]
    s.set_doc_sets(labs["mod5"])
    _check(s, [fb], [labs["mod5"]], queries[:5], z, quorums=(0.95,), thresholds=(0.0,), limits=(0,))
    s.close()


def test_wide_table_gives_the_same_arrays(gpu_lib, src, tmp_path, monkeypatch):
    path, fb = _compact(str(tmp_path / "w.cobs_compact"), 300, 8, [901, 1003, 777, 1300, 950], 3, 31, 9)
    labels = quorum_labelings(300)["runs37"]
    qs = _edge_queries(src, 31, 2, NS)
    out = []
    for wide in (False, True):
        if wide:
            monkeypatch.setenv("COBS_GPU_IDX64", "1")
        s = gpu_lib.Search(path, findere=2)
        s.set_doc_sets(labels)
        out.append(s.search_sets_quorum_arrays(qs, 0.5) + s.set_prevalence_arrays(qs))
        _check(s, [fb], [labels], qs, 2, quorums=(0.5, 1.0), thresholds=(0.0, 0.3), limits=(0,))
        s.close()
    monkeypatch.delenv("COBS_GPU_IDX64")
    assert all(np.array_equal(a, b) for a, b in zip(out[0], out[1])) and len(out[0][1]) and out[0][3].any()


def _raw_search(s, queries, cap, quorum=0.5, threshold=0.0, num_results=0):
    from cobs_amd import _capi
    lib = _capi.load()
    nq = len(queries)
    arr = (C.c_char_p * max(nq, 1))(*queries)
    lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in queries])
    hits = np.zeros(max(cap, 1), dtype=s.SET_QUORUM_HIT_DTYPE)
    hits["any"] = 0xA5A5A5A5
    offs = np.full(nq + 1, 0xFFFF, dtype=np.uint64)
    bad = C.c_size_t(12345)
    st = lib.cobs_gpu_search_sets_quorum(s._h, arr, lens, nq, threshold, quorum, num_results,
                                         C.cast(hits.ctypes.data, C.POINTER(_capi.SetQuorumHit)) if cap else None, cap,
                                         C.cast(offs.ctypes.data, C.POINTER(C.c_size_t)), C.byref(bad))
    return st, bad.value, offs, hits, lib.cobs_gpu_last_error().decode()


def _raw_prevalence(s, queries, cap):
    from cobs_amd import _capi
    lib = _capi.load()
    nq = len(queries)
    arr = (C.c_char_p * max(nq, 1))(*queries)
    lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in queries])
    counts = np.full(max(cap, 1), 0xA5A5A5A5, dtype=np.uint32)
    offs = np.full(nq * s.num_files + 1, 0xFFFF, dtype=np.uint64)
    need, bad = C.c_size_t(777), C.c_size_t(12345)
    st = lib.cobs_gpu_set_prevalence(s._h, arr, lens, nq, C.cast(counts.ctypes.data, C.POINTER(C.c_uint32)) if cap else None, cap,
                                     C.cast(offs.ctypes.data, C.POINTER(C.c_size_t)), C.byref(need), C.byref(bad))
    return st, bad.value, offs, counts, need.value, lib.cobs_gpu_last_error().decode()


def test_refusals_and_capacity(gpu_lib, src, tmp_path):
    from cobs_amd import _capi
    lib = _capi.load()
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 300, 2003, 1, 31, 1)
    labels = quorum_labelings(300)["runs37"]
    s = gpu_lib.Search(path, findere=2)
    s.set_doc_sets(labels)
    good = [src[:100], src[200:340], src[400:480]]
    s.set_quorum_ms()
    # everything the host can refuse comes back before any device work
    for quorum in (0.0, -1.0, 1.5, float("nan")):
        st, bad, offs, hits, msg = _raw_search(s, good, 100, quorum=quorum)
        assert st == _capi.ERR_ARG and "quorum" in msg, quorum
    short = [good[0], good[1], src[:31 + 1]]
    st, bad, offs, hits, msg = _raw_search(s, short, 100)
    assert st == _capi.ERR_QUERY_TOO_SHORT and bad == 2 and str(31 + 2) in msg and "(query 2)" in msg
    st, bad, offs, counts, need, msg = _raw_prevalence(s, short, 100000)
    assert st == _capi.ERR_QUERY_TOO_SHORT and bad == 2 and "(query 2)" in msg
    assert lib.cobs_gpu_search_sets_quorum(s._h, None, None, 3, 0.0, 0.5, 0, None, 0, None, None) == _capi.ERR_ARG
    offs3 = (C.c_size_t * 4)()
    assert lib.cobs_gpu_search_sets_quorum(s._h, None, None, 3, 0.0, 0.5, 0, None, 0, offs3, None) == _capi.ERR_ARG
    assert lib.cobs_gpu_set_prevalence(s._h, None, None, 3, None, 0, offs3, None, None) == _capi.ERR_ARG
    arr = (C.c_char_p * 3)(*good)
    lens = (C.c_size_t * 3)(*[len(q) for q in good])
    assert lib.cobs_gpu_search_sets_quorum(s._h, arr, lens, 3, 0.0, 0.5, 0, None, 5, offs3, None) == _capi.ERR_ARG      # cap without hits
    assert lib.cobs_gpu_set_prevalence(s._h, arr, lens, 3, None, 5, offs3, None, None) == _capi.ERR_ARG
    assert lib.cobs_gpu_set_prevalence(s._h, arr, lens, 3, None, 0, None, None, None) == _capi.ERR_ARG
    # a query that is too long for the kernels' 32-bit position arithmetic: only the length is looked at, before any of the
    # text is read, so a claimed length over a short buffer asks for the refusal
    arr2 = (C.c_char_p * 2)(good[0], good[1])
    lens2 = (C.c_size_t * 2)(len(good[0]), 0xFFFFFFF0 - (1 << 20))
    offs5 = (C.c_size_t * 5)()
    bad = C.c_size_t(12345)
    assert lib.cobs_gpu_search_sets_quorum(s._h, arr2, lens2, 2, 0.0, 0.5, 0, None, 0, offs5, C.byref(bad)) == _capi.ERR_QUERY_TOO_LONG
    assert bad.value == 1 and b"(query 1)" in lib.cobs_gpu_last_error()
    bad = C.c_size_t(12345)
    assert lib.cobs_gpu_set_prevalence(s._h, arr2, lens2, 2, None, 0, offs5, None, C.byref(bad)) == _capi.ERR_QUERY_TOO_LONG
    assert bad.value == 1 and b"(query 1)" in lib.cobs_gpu_last_error()
    # (the remaining ERR_HIP, "out of device memory for the counts and records", needs a pass that exhausts the device's
    # memory below pass_bytes: not something a test may do on a shared machine; the refusal by pass_bytes stands in front of
    # it and is exercised in test_smallest_pass_relabelling_and_clearing)
    assert s.set_quorum_ms()["passes"] == 0
    # a buffer that is too small: the needed sizes, then the repeat
    want_offs, want = Q.arrays([fb], [labels], good, 2, 0.5)
    for cap in (0, 26):
        st, bad, offs, hits, msg = _raw_search(s, good, cap)
        assert st == _capi.ERR_CAPACITY and np.array_equal(offs, want_offs) and int(offs[3]) == 27 and np.all(hits["any"] == 0xA5A5A5A5), msg
    st, bad, offs, hits, msg = _raw_search(s, good, 27)
    assert st == _capi.OK and np.array_equal(offs, want_offs) and np.array_equal(_rows(hits), want), msg
    s.set_quorum_ms()
    want_offs, want = Q.segments([fb], [labels], good, 2)
    for cap in (0, len(want) - 1):
        st, bad, offs, counts, need, msg = _raw_prevalence(s, good, cap)
        assert st == _capi.ERR_CAPACITY and np.array_equal(offs, want_offs) and need == len(want) and np.all(counts == 0xA5A5A5A5), msg
    assert s.set_quorum_ms()["passes"] == 0                          # (the sizes are host arithmetic)
    st, bad, offs, counts, need, msg = _raw_prevalence(s, good, len(want))
    assert st == _capi.OK and np.array_equal(offs, want_offs) and need == len(want) and np.array_equal(counts, want), msg
    s.close()
    # a handle with an HBM budget, and one shard of two
    for kw, word in (({"hbm_budget": 256 << 20}, "HBM budget"), ({"shard_rank": 0, "shard_count": 2}, "shard")):
        s = gpu_lib.Search(path, **kw)
        s.set_doc_sets(labels)                                      # (the labels are kept; the calls are refused)
        for call in (lambda: s.search_sets_quorum(good, 0.5), lambda: s.set_prevalence(good)):
            with pytest.raises(gpu_lib.CobsGpuError) as e:
                call()
            assert e.value.status == _capi.ERR_UNSUPPORTED and word in str(e.value)
        assert s.set_quorum_ms()["passes"] == 0
        s.close()


def test_cli_and_cpp_mirror_agree_with_the_arrays(gpu_lib, src, tmp_path):
    """cobs_gpu_query --sets-quorum prints what ClassicSearch::search_sets_quorum returns -- per query its comment line with
    the number of sets, then set_name, core, any, members --, --sets-profile what ClassicSearch::set_prevalence returns"""
    tool = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")
    paths, files = _two_files(tmp_path)
    set_of = {"doc_%05d" % d: "lineage %02d" % (d // 37) for d in range(150) if d % 4 != 1}
    tsv = tmp_path / "sets.tsv"
    tsv.write_text("".join("%s\t%s\n" % kv for kv in set_of.items()))
    queries = _edge_queries(src, 31, 2, (1, 64, 200)) + [I.with_n(src[100:300], [90])]
    qf = tmp_path / "q.fa"
    qf.write_text("".join(">q%d\n%s\n" % (i, q.decode()) for i, q in enumerate(queries)))
    index_args = ["-i", paths[0], "-i", paths[1]]
    for z, mode, quorum, t, limit in ((0, "miss", 0.5, 0.05, 0), (2, "skip", 0.95, 0.0, 3)):
        s = gpu_lib.Search(paths, findere=z, invalid_bases=mode)
        names = [s.set_doc_sets({k: v for k, v in set_of.items() if k in set(s._names(f))}, file_no=f) for f in range(2)]
        members = [s.doc_sets(f)[1] for f in range(2)]
        res = s.search_sets_quorum(queries, quorum, t, limit)
        prof = s.set_prevalence(queries)
        labs = [np.array([-1 if d % 4 == 1 or d >= 150 else d // 37 for d in range(fb.num_docs)]) for fb in files]
        want = [Q.results(files, labs, q, z, quorum, t, limit, mode) for q in queries]
        assert [[(r.file_no, r.set, r.core, r.any) for r in rs] for rs in res] == want and any(want)
        for i, q in enumerate(queries):
            for f in range(2):
                assert np.array_equal(prof[i][f], Q.profile(files[f], q, z, labs[f], mode)), (i, f)
        s.close()
        fl = (["--findere", str(z)] if z else []) + ["--invalid-bases", mode, "--sets", str(tsv)]
        r = subprocess.run([tool] + index_args + fl + ["--sets-quorum", repr(quorum), "-t", str(t)] + (["-l", str(limit)] if limit else []) +
                           ["-f", str(qf)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        lines = iter(r.stdout.splitlines())
        for i, rs in enumerate(res):
            assert next(lines) == "*q%d\t%d" % (i, len(rs))
            for x in rs:
                assert next(lines) == "%s\t%d\t%d\t%d" % (names[x.file_no][x.set], x.core, x.any, members[x.file_no][x.set])
        assert next(lines, None) is None
        r = subprocess.run([tool] + index_args + fl + ["--sets-profile", "-f", str(qf)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        lines = iter(r.stdout.splitlines())
        for i in range(len(queries)):
            assert next(lines) == "*q%d\t%d" % (i, sum(int(np.count_nonzero(m)) for m in members))
            for f in range(2):
                for c, row in zip(np.nonzero(members[f])[0], prof[i][f]):
                    assert next(lines) == "%s\t%d\t%s" % (names[f][c], members[f][c], " ".join(map(str, row.tolist())))
        assert next(lines, None) is None
    # a verbatim query: the set lines only
    r = subprocess.run([tool] + index_args + ["--sets", str(tsv), "--sets-quorum", "1", "-t", "0", queries[2].decode()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and len(r.stdout.splitlines()) == 2 * 5 and all(len(ln.split("\t")) == 4 for ln in r.stdout.splitlines()), r.stderr
    r = subprocess.run([tool] + index_args + ["--sets", str(tsv), "--sets-profile", queries[2].decode()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and len(r.stdout.splitlines()) == 2 * 5, r.stderr


def test_timer_resets_on_read_and_no_device_memory_is_left(gpu_lib, src, tmp_path):
    import torch
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 129, 2003, 1, 31, 1)
    zero = {"hash_ms": 0.0, "count_ms": 0.0, "select_ms": 0.0, "order_ms": 0.0, "passes": 0}
    s = gpu_lib.Search(path)
    assert s.set_quorum_ms() == zero
    s.set_doc_sets(quorum_labelings(129)["mod5"])
    s.search_sets_quorum([src[:200], src[300:700]], 0.5)
    t = s.set_quorum_ms()
    assert t["hash_ms"] > 0 and t["count_ms"] > 0 and t["select_ms"] > 0 and t["order_ms"] >= 0 and t["passes"] == 1
    assert s.set_quorum_ms() == zero
    s.set_prevalence([src[:200]])
    t = s.set_quorum_ms()
    assert t["hash_ms"] > 0 and t["count_ms"] > 0 and t["order_ms"] == 0 and t["passes"] == 1
    assert s.set_quorum_ms() == zero and s.sets_ms()["passes"] == 0
    s.close()

    def cycle():
        s = gpu_lib.Search(path)
        s.set_doc_sets(quorum_labelings(129)["own"])
        s.search_sets_quorum_arrays([src[:200], src[300:700]], 0.5, 0.3)
        s.set_doc_sets(quorum_labelings(129)["runs37"])
        s.set_prevalence_arrays([src[:900]])
        s.search_sets_quorum_arrays([src[:900]], 0.95, 0.0, 2)
        s.close()
    cycle()
    gc.collect()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(10):
        cycle()
    gc.collect()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < (32 << 20), (free0, free1)
