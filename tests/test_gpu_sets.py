"""GPU: document sets (cobs_gpu_set_doc_sets / cobs_gpu_search_sets, Search.set_doc_sets / search_sets,
ClassicSearch::search_sets, --sets) bit for bit against tests/sets_check.py: for every labelled set of documents the
positions of a query that at least one member holds (any) and that every member holds (all).  Every comparison is exact.

Classic rows from one byte to wider than a 16-byte chunk, compact sub-indexes of 2 and 16 row bytes and 1 to 4097 rows, a
last sub-index that is partly filled or all padding, padding slots that hold bits; on each of them every document its own
set, one set of all, d % 5 (every chunk holds every set), runs of 37 (sets straddle chunk and sub-index borders) and a
labelling with unlabelled documents and unused set numbers; position counts at the borders of the bitmap words; z = 0
and 3; the thresholds, both keys, limits and ties; the identities of the definition on a procedural handle; two files of
which one is labelled, the invalid-bases policies, several device passes, relabelling, the wide table, every refusal, the
mirrors, the CLI, the timer and device memory."""
import ctypes as C
import gc
import os
import subprocess

import numpy as np
import pytest

from tests import invalid_check as I
from tests import sets_check as S
from tests.test_gpu_prevalence import _classic, _compact, _edge_queries      # the files the prevalence tests are built on

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 31, 32, 33, 64, 65, 100)                     # position counts n: the borders of the bitmap words
ZS = (0, 3)
# (threshold, rank_by, num_results)
COMBOS = ((0.0, "any", 0), (0.3, "any", 0), (1.0, "any", 0), (0.3, "all", 0), (1.0, "all", 1), (0.0, "all", 3), (0.3, "any", 1))


def labelings(num_docs):
    d = np.arange(num_docs)
    return {"own": d.copy(), "one": np.zeros(num_docs, dtype=np.int64), "mod5": d % 5, "runs37": d // 37,
            # every fourth document in no set, and only even set numbers in use
            "sparse": np.where(d % 4 == 1, -1, (d // 11) * 2)}


@pytest.fixture(scope="module")
def src(oracle):
    return oracle.random_sequence(3000, 77)


def _rows(hits):
    return np.stack([hits[f].astype(np.int64) for f in ("file_no", "set", "any", "all")], axis=1).reshape(-1, 4)


def _check(s, files, labs, queries, z, combos=COMBOS, mode="error"):
    for t, rank_by, k in combos:
        offs, hits = s.search_sets_arrays(queries, t, rank_by, k)
        want_offs, want = S.arrays(files, labs, queries, z, t, rank_by, k, mode)
        assert offs.dtype == np.uint64 and hits.dtype == s.SET_HIT_DTYPE
        assert np.array_equal(offs, want_offs), (z, t, rank_by, k, offs, want_offs)
        got = _rows(hits)
        assert np.array_equal(got, want), (z, t, rank_by, k, np.nonzero((got != want).any(axis=1))[0][:8])


def _sweep(gpu_lib, path, fb, src, zs=ZS, ns=NS):
    s = gpu_lib.Search(path)
    for name, labels in labelings(fb.num_docs).items():
        names = s.set_doc_sets(labels)
        assert len(names) == int(labels.max()) + 1
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
    """a last sub-index that is partly filled; lanes side by side along the position blocks for the narrow rows"""
    num_docs = len(sigs) * 8 * page_size - 5 * page_size - 3
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), num_docs, page_size, sigs, 1, 31, page_size)
    _sweep(gpu_lib, path, fb, src)


def test_trailing_sub_index_of_padding(gpu_lib, src, tmp_path):
    path, fb = _compact(str(tmp_path / "t.cobs_compact"), 2 * 128 - 9, 16, [501, 703, 601], 1, 31, 5)
    assert (fb.doc_of_slot()[256:] < 0).all()
    _sweep(gpu_lib, path, fb, src, ns=(1, 33, 100))


def test_padding_slots_with_set_bits_never_take_part(gpu_lib, src, tmp_path):
    """files written WITHOUT masking the padding documents: their slots hold random bits"""
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 5, 301, 1, 31, 3, mask=False)
    assert S.windows(fb, src[:200], 0)[:, 5:].any()
    _sweep(gpu_lib, path, fb, src, ns=(1, 33, 100))
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), 100, 8, [211, 307, 401], 2, 31, 4, mask=False)
    assert S.windows(fb, src[:200], 0)[:, 100:128].any() and S.windows(fb, src[:200], 0)[:, 128:].any()
    _sweep(gpu_lib, path, fb, src, ns=(1, 33, 100))


def test_the_layout_tests_are_not_vacuous(src, tmp_path):
    """on the CHECKER's answer over the queries and labellings of the classic layouts: a multi-member set with all > 0, a
    set with 0 < any < n, a set with all < any, and ties in the key"""
    multi_all = partial_any = all_below_any = ties = False
    for num_docs in (9, 300):
        _path, fb = _classic(str(tmp_path / ("c%d.cobs_classic" % num_docs)), num_docs, 2003, 1, 31, num_docs)
        for labels in labelings(num_docs).values():
            members = np.bincount(labels[labels >= 0])
            for z in ZS:
                for q in _edge_queries(src, 31, z, NS):
                    n = fb.positions(q, z)
                    got = S.counts(fb, q, z, labels)
                    for c, (a, b) in got.items():
                        multi_all |= members[c] > 1 and b > 0
                        partial_any |= 0 < a < n
                        all_below_any |= b < a
                    ties |= len({a for a, _b in got.values()}) < len(got)
    assert multi_all and partial_any and all_below_any and ties


@pytest.mark.parametrize("z", ZS)
def test_identities_on_a_procedural_handle(gpu_lib, oracle, z):
    """larger than the numpy restatement likes: one-member sets against the scan, one set of all against the prevalence,
    sets of 7 against the OR and the AND of their members' hit_positions words"""
    sigs = [20011, 30011, 25013, 40009, 35023, 45007]
    num_docs, page_size = 5000, 105
    s = gpu_lib.Search.synthetic("compact", sigs, num_docs, page_size=page_size, seed=5, findere=z)
    n = 300
    queries = [oracle.random_sequence(n + 30 + z, 100 + i) for i in range(6)]
    text = oracle.random_sequence(400, 7)
    s.plant(text, list(range(0, 5000, 7)), 900, salt=1)              # one member of every set of 7 holds most of the text
    s.plant(text, list(range(21)), 1000, salt=2)                     # ... and three sets hold it whole
    queries[1], queries[4] = text[:n + 30 + z], text[50:50 + n + 30 + z]

    def by_set(labels, nsets):
        s.set_doc_sets(labels)
        offs, hits = s.search_sets_arrays(queries)
        assert offs.tolist() == [nsets * i for i in range(len(queries) + 1)]
        out = np.zeros((len(queries), nsets, 2), dtype=np.int64)
        for i in range(len(queries)):
            seg = hits[int(offs[i]):int(offs[i + 1])]
            assert sorted(seg["set"].tolist()) == list(range(nsets)) and not seg["file_no"].any()
            out[i, seg["set"], 0], out[i, seg["set"], 1] = seg["any"], seg["all"]
        return out
    own = by_set(np.arange(num_docs), num_docs)
    for i, q in enumerate(queries):
        score = s.counts(q)[:num_docs].astype(np.int64)
        assert np.array_equal(own[i, :, 0], score) and np.array_equal(own[i, :, 1], score), i
    assert own[1].max() == n
    one = by_set(np.zeros(num_docs, dtype=np.int64), 1)
    offs, counts = s.prevalence_arrays(queries)
    for i in range(len(queries)):
        seg = counts[int(offs[i]):int(offs[i + 1])]
        assert one[i, 0].tolist() == [int((seg > 0).sum()), int((seg == num_docs).sum())], i
    assert one[1, 0, 0] == n
    sevens = by_set(np.arange(num_docs) // 7, 715)
    hits = np.zeros(num_docs, dtype=gpu_lib.Search.HIT_DTYPE)
    hits["doc"] = np.arange(num_docs)
    starts = np.arange(0, num_docs, 7)
    for i in (1, 3):
        _bo, bits = s.hit_positions([queries[i]], [0, num_docs], hits)
        words = bits.reshape(num_docs, -1)
        pop = lambda w: np.unpackbits(np.ascontiguousarray(w).view(np.uint8), axis=1).sum(axis=1)      # noqa: E731
        assert np.array_equal(sevens[i, :, 0], pop(np.bitwise_or.reduceat(words, starts, axis=0))), i
        assert np.array_equal(sevens[i, :, 1], pop(np.bitwise_and.reduceat(words, starts, axis=0))), i
    assert sevens[1, :3, 1].tolist() == [n, n, n] and sevens[1, 3:, 1].max() < n and sevens[3, :, 1].max() < sevens[3, :, 0].min()
    s.close()


def _two_files(tmp_path):
    pa, fa = _classic(str(tmp_path / "a.cobs_classic"), 300, 2003, 1, 31, 1)
    pb, fb = _compact(str(tmp_path / "b.cobs_compact"), 150, 4, [499, 601, 701, 557, 811], 2, 20, 2)
    return [pa, pb], [fa, fb]


def test_two_files_of_different_term_size_one_labelled_and_the_invalid_bases_policies(gpu_lib, src, tmp_path):
    from cobs_amd import _capi
    paths, files = _two_files(tmp_path)
    labs = [None, labelings(150)["runs37"]]
    base = src[40:40 + 160]
    queries = [base, I.with_n(base, [0]), I.with_n(base, [70, 150]), b"N" * 80, src[500:500 + 64]]
    for mode in I.MODES:
        s = gpu_lib.Search(paths, invalid_bases=mode)
        s.set_doc_sets(labs[1], file_no=1)
        assert s.doc_sets(0)[0] == [] and len(s.doc_sets(0)[1]) == 0 and len(s.doc_sets(1)[1]) == 5
        for z in ZS:
            s.set_findere(z)
            _check(s, files, labs, queries, z, mode=mode)
        s.close()
    assert 0 < S.denominator(files[1], queries[2], 0, "skip") < S.denominator(files[1], queries[2], 0, "miss")
    # under `error` the call names the query, and the handle still answers; both files labelled now
    s = gpu_lib.Search(paths, findere=1)
    labs = [labelings(300)["mod5"], labs[1]]
    s.set_doc_sets(labs[0], file_no=0)
    s.set_doc_sets(labs[1], file_no=1)
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.search_sets(queries[:3])
    assert e.value.status == _capi.ERR_INVALID_BASE and "(query 1)" in str(e.value)
    good = [queries[0], queries[4]]
    _check(s, files, labs, good, 1)
    res = s.search_sets(good[0], 0.3, "any", 2)                      # the list form of one query
    want = S.results(files, labs, good[0], 1, 0.3, "any", 2)
    assert [(r.file_no, r.set, r.name, r.any, r.all) for r in res] == [(f, c, str(c), a, b) for (f, c, a, b) in want] and len(res) == 2
    s.close()


def test_passes_relabelling_and_clearing(gpu_lib, src, tmp_path):
    """the workspace limit cuts the call into passes: same arrays; the searches around it are not disturbed; labels are
    replaced and taken away between calls"""
    from tests import findere_check as F
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), 700, 16, [1201, 997, 1500, 1103, 1301, 800], 1, 31, 3)
    rng = np.random.default_rng(41)
    queries = []
    for _ in range(39):
        ln = int(rng.integers(50, 151))
        o = int(rng.integers(0, len(src) - ln))
        queries.append(src[o:o + ln])
    queries.append(src[:1030])
    labs = labelings(700)
    s = gpu_lib.Search(path, findere=3)
    before = s.search_hits(queries[:5], 0.0, 3)
    assert before == [F.results([fb], q, 3, 0.0, 3) for q in queries[:5]]
    s.set_doc_sets(labs["runs37"])
    s.sets_ms()
    offs, hits = s.search_sets_arrays(queries, 0.3)
    assert s.sets_ms()["passes"] == 1
    s.set_tuning("pass_bytes", 30000)
    offs2, hits2 = s.search_sets_arrays(queries, 0.3)
    assert s.sets_ms()["passes"] >= 3
    assert np.array_equal(offs, offs2) and np.array_equal(hits, hits2)
    # the bitmaps of a single query that do not fit: an error with a message, before any device work
    s.set_tuning("pass_bytes", 2000)
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.search_sets_arrays(queries, 0.3)
    from cobs_amd import _capi
    assert e.value.status == _capi.ERR_HIP and "do not fit the pass workspace" in str(e.value) and s.sets_ms()["passes"] == 0
    s.set_tuning("pass_bytes", 0)
    want_offs, want = S.arrays([fb], [labs["runs37"]], queries, 3, 0.3)
    assert np.array_equal(offs, want_offs) and np.array_equal(_rows(hits), want)
    assert s.search_hits(queries[:5], 0.0, 3) == before
    # relabelling replaces the labels; doc_sets reports them
    names = s.set_doc_sets(labs["sparse"])
    got_names, members = s.doc_sets()
    assert got_names == names and np.array_equal(members, np.bincount(labs["sparse"][labs["sparse"] >= 0], minlength=len(names)))
    assert (members == 0).any()
    _check(s, [fb], [labs["sparse"]], queries[:6], 3, combos=COMBOS[:3])
    named = s.set_doc_sets({"doc_%05d" % d: "clade_%c" % "ba"[d % 2] for d in range(0, 700, 3)})
    assert named == ["clade_a", "clade_b"]
    lab = np.full(700, -1)
    lab[0:700:3] = [1 - (d % 2) for d in range(0, 700, 3)]
    _check(s, [fb], [lab], queries[:6], 3, combos=COMBOS[:3])
    assert [r.name for r in s.search_sets(queries[0])] == ["clade_%c" % "ab"[r[1]] for r in S.results([fb], [lab], queries[0], 3)]
    # clearing: nothing comes back, and the plain search is as before
    assert s.set_doc_sets(None) == [] and s.doc_sets()[0] == []
    offs, hits = s.search_sets_arrays(queries, 0.0)
    assert not offs.any() and len(hits) == 0
    assert s.search_hits(queries[:5], 0.0, 3) == before
    s.close()


def test_wide_table_gives_the_same_arrays(gpu_lib, src, tmp_path, monkeypatch):
    path, fb = _compact(str(tmp_path / "w.cobs_compact"), 300, 8, [901, 1003, 777, 1300, 950], 3, 31, 9)
    labels = labelings(300)["runs37"]
    qs = _edge_queries(src, 31, 3, NS)
    out = []
    for wide in (False, True):
        if wide:
            monkeypatch.setenv("COBS_GPU_IDX64", "1")
        s = gpu_lib.Search(path, findere=3)
        s.set_doc_sets(labels)
        out.append(s.search_sets_arrays(qs, 0.0))
        _check(s, [fb], [labels], qs, 3, combos=COMBOS[:2])
        s.close()
    monkeypatch.delenv("COBS_GPU_IDX64")
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and len(out[0][1])


def _raw_search(s, queries, cap, threshold=0.0, rank_by=0, num_results=0):
    from cobs_amd import _capi
    lib = _capi.load()
    nq = len(queries)
    arr = (C.c_char_p * max(nq, 1))(*queries)
    lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in queries])
    hits = np.zeros(max(cap, 1), dtype=s.SET_HIT_DTYPE)
    hits["any"] = 0xA5A5A5A5
    offs = np.full(nq + 1, 0xFFFF, dtype=np.uint64)
    bad = C.c_size_t(12345)
    st = lib.cobs_gpu_search_sets(s._h, arr, lens, nq, threshold, rank_by, num_results,
                                  C.cast(hits.ctypes.data, C.POINTER(_capi.SetHit)) if cap else None, cap,
                                  C.cast(offs.ctypes.data, C.POINTER(C.c_size_t)), C.byref(bad))
    return st, bad.value, offs, hits, lib.cobs_gpu_last_error().decode()


def test_refusals_and_capacity(gpu_lib, src, tmp_path):
    from cobs_amd import _capi
    lib = _capi.load()
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 300, 2003, 1, 31, 1)
    labels = labelings(300)["runs37"]
    s = gpu_lib.Search(path, findere=3)
    u32 = lambda a: C.cast(np.ascontiguousarray(a, dtype=np.uint32).ctypes.data, C.POINTER(C.c_uint32))      # noqa: E731
    # the label validation: nothing is kept of a refused labelling
    lab = labels.astype(np.uint32)
    assert lib.cobs_gpu_set_doc_sets(s._h, 0, u32(lab), 299, 9) == _capi.ERR_ARG and b"document count" in lib.cobs_gpu_last_error()
    assert lib.cobs_gpu_set_doc_sets(s._h, 0, u32(lab), 300, 8) == _capi.ERR_ARG and b"document 296" in lib.cobs_gpu_last_error()
    assert lib.cobs_gpu_set_doc_sets(s._h, 1, u32(lab), 300, 9) == _capi.ERR_ARG
    assert s.doc_sets()[0] == [] and len(s.doc_sets()[1]) == 0
    with_none = lab.copy()
    with_none[7] = 0xFFFFFFFF
    assert lib.cobs_gpu_set_doc_sets(s._h, 0, u32(with_none), 300, 9) == _capi.OK
    n, members = C.c_uint32(0), (C.c_uint32 * 9)()
    assert lib.cobs_gpu_get_doc_sets(s._h, 0, C.byref(n), members, 8) == _capi.ERR_CAPACITY and n.value == 9
    assert lib.cobs_gpu_get_doc_sets(s._h, 0, C.byref(n), members, 9) == _capi.OK and list(members) == [36] + [37] * 7 + [4]
    s.set_doc_sets(labels)
    good = [src[:100], src[200:340], src[400:480]]
    s.sets_ms()
    # everything the host can refuse comes back before any device work
    st, bad, offs, hits, msg = _raw_search(s, good, 100, rank_by=2)
    assert st == _capi.ERR_ARG and "rank_by" in msg
    short = [good[0], good[1], src[:31 + 2]]
    st, bad, offs, hits, msg = _raw_search(s, short, 100)
    assert st == _capi.ERR_QUERY_TOO_SHORT and bad == 2 and str(31 + 3) in msg and "(query 2)" in msg
    assert lib.cobs_gpu_search_sets(s._h, None, None, 3, 0.0, 0, 0, None, 0, None, None) == _capi.ERR_ARG
    offs3 = (C.c_size_t * 4)()
    assert lib.cobs_gpu_search_sets(s._h, None, None, 3, 0.0, 0, 0, None, 0, offs3, None) == _capi.ERR_ARG
    arr = (C.c_char_p * 3)(*good)
    lens = (C.c_size_t * 3)(*[len(q) for q in good])
    assert lib.cobs_gpu_search_sets(s._h, arr, lens, 3, 0.0, 0, 0, None, 5, offs3, None) == _capi.ERR_ARG      # cap without hits
    assert s.sets_ms()["passes"] == 0
    # a buffer that is too small: the needed sizes, then the repeat
    want_offs, want = S.arrays([fb], [labels], good, 3)
    for cap in (0, 26):
        st, bad, offs, hits, msg = _raw_search(s, good, cap)
        assert st == _capi.ERR_CAPACITY and np.array_equal(offs, want_offs) and int(offs[3]) == 27 and np.all(hits["any"] == 0xA5A5A5A5), msg
    st, bad, offs, hits, msg = _raw_search(s, good, 27)
    assert st == _capi.OK and np.array_equal(offs, want_offs) and np.array_equal(_rows(hits), want), msg
    s.close()
    # a handle with an HBM budget, and one shard of two
    for kw, word in (({"hbm_budget": 256 << 20}, "HBM budget"), ({"shard_rank": 0, "shard_count": 2}, "shard")):
        s = gpu_lib.Search(path, **kw)
        s.set_doc_sets(labels)                                      # (the labels are kept; the search is refused)
        with pytest.raises(gpu_lib.CobsGpuError) as e:
            s.search_sets(good)
        assert e.value.status == _capi.ERR_UNSUPPORTED and word in str(e.value)
        assert s.sets_ms()["passes"] == 0
        s.close()


def test_cli_and_cpp_mirror_agree_with_the_arrays(gpu_lib, src, tmp_path):
    """cobs_gpu_query --sets prints what ClassicSearch::search_sets returns: per query its comment line with the number of
    sets, then set_name, any, all"""
    tool = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")
    paths, files = _two_files(tmp_path)
    set_of = {"doc_%05d" % d: "lineage %02d" % (d // 37) for d in range(150) if d % 4 != 1}
    tsv = tmp_path / "sets.tsv"
    tsv.write_text("".join("%s\t%s\n" % kv for kv in set_of.items()))
    queries = _edge_queries(src, 31, 3, (1, 64, 200)) + [I.with_n(src[100:300], [90])]
    qf = tmp_path / "q.fa"
    qf.write_text("".join(">q%d\n%s\n" % (i, q.decode()) for i, q in enumerate(queries)))
    index_args = ["-i", paths[0], "-i", paths[1]]
    for z, mode, by, t, limit in ((0, "miss", "any", 0.3, 0), (3, "skip", "all", 0.01, 3)):
        s = gpu_lib.Search(paths, findere=z, invalid_bases=mode)
        names = [s.set_doc_sets({k: v for k, v in set_of.items() if k in set(s._names(f))}, file_no=f) for f in range(2)]
        res = s.search_sets(queries, t, by, limit)
        labs = [np.array([-1 if d % 4 == 1 or d >= 150 else d // 37 for d in range(fb.num_docs)]) for fb in files]
        want = [S.results(files, labs, q, z, t, by, limit, mode) for q in queries]
        assert [[(r.file_no, r.set, r.any, r.all) for r in rs] for rs in res] == want and any(want)
        s.close()
        fl = (["--findere", str(z)] if z else []) + ["--invalid-bases", mode, "--sets", str(tsv), "--sets-by", by, "-t", str(t)]
        fl += ["-l", str(limit)] if limit else []
        r = subprocess.run([tool] + index_args + fl + ["-f", str(qf)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        lines = iter(r.stdout.splitlines())
        for i, rs in enumerate(res):
            assert next(lines) == "*q%d\t%d" % (i, len(rs))
            for x in rs:
                assert next(lines) == "%s\t%d\t%d" % (names[x.file_no][x.set], x.any, x.all)
        assert next(lines, None) is None
    # a verbatim query: the set lines only; a name the index does not hold is an error that names it
    r = subprocess.run([tool] + index_args + ["--sets", str(tsv), "-t", "0", queries[2].decode()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and len(r.stdout.splitlines()) == 2 * 5, r.stderr
    tsv.write_text("doc_00000\ta\ndoc_99999\tb\n")
    r = subprocess.run([tool] + index_args + ["--sets", str(tsv), queries[2].decode()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "no document named doc_99999" in r.stderr and r.stdout == ""


def test_timer_resets_on_read_and_no_device_memory_is_left(gpu_lib, src, tmp_path):
    import torch
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 129, 2003, 1, 31, 1)
    zero = {"hash_ms": 0.0, "presence_ms": 0.0, "select_ms": 0.0, "order_ms": 0.0, "passes": 0}
    s = gpu_lib.Search(path)
    assert s.sets_ms() == zero
    s.set_doc_sets(labelings(129)["mod5"])
    s.search_sets([src[:200], src[300:700]])
    t = s.sets_ms()
    assert t["hash_ms"] > 0 and t["presence_ms"] > 0 and t["select_ms"] > 0 and t["order_ms"] >= 0 and t["passes"] == 1
    assert s.sets_ms() == zero
    s.close()

    def cycle():
        s = gpu_lib.Search(path)
        s.set_doc_sets(labelings(129)["own"])
        s.search_sets_arrays([src[:200], src[300:700]], 0.3)
        s.set_doc_sets(labelings(129)["runs37"])
        s.search_sets_arrays([src[:900]], 0.0, "all", 2)
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
