"""GPU: the per-position presence of every hit (cobs_gpu_hit_positions / Search.hit_positions / search_positions /
ClassicSearch::search_positions / --positions) bit for bit against tests/positions_check.py: position p of a query is
set in a document when its terms p .. p + z are all present there; the popcount of a hit's words is the hit's score.

Both index kinds, H = 1 and H > 1, several term sizes, a handle over files of different term size, every findere z,
thresholds and limits, every word edge of the output, reads and long queries, pairs that are no hits, sub-indexes of
1, 2, 65 and 4097 rows, several device passes, and every error the call refuses on the host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import cases
from tests import findere_check as F
from tests import positions_check as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZS = (0, 1, 3, 7)
THRESHOLDS = (0.0, 0.8, 1.0)
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
    """index files with planted matches (so that thresholds 0.8 / 1.0 select something) and their bits"""
    d = tmp_path_factory.mktemp("positions")
    src = oracle.random_sequence(3000, 77)
    out = {}
    out["c1"] = (str(d / "c1.cobs_classic"), _classic(str(d / "c1.cobs_classic"), 300, 2003, 1, 31, 1,
                                                      planted={0: 1.0, 7: 0.95, 150: 0.8}, query=src))
    out["c3"] = (str(d / "c3.cobs_classic"), _classic(str(d / "c3.cobs_classic"), 200, 3001, 3, 31, 2,
                                                      planted={3: 1.0, 199: 0.9}, query=src))
    out["p1"] = (str(d / "p1.cobs_compact"), _compact(str(d / "p1.cobs_compact"), 700, 16, [1201, 997, 1500, 1103, 1301, 800], 1,
                                                      31, 3, planted={1: 1.0, 500: 0.9}, query=src))
    out["p3"] = (str(d / "p3.cobs_compact"), _compact(str(d / "p3.cobs_compact"), 300, 8, [901, 1003, 777, 1300, 950], 3, 25, 4,
                                                      planted={0: 1.0, 299: 0.95}, query=src))
    out["c2k20"] = (str(d / "c2k20.cobs_classic"), _classic(str(d / "c2k20.cobs_classic"), 150, 1499, 2, 20, 5,
                                                            planted={10: 1.0}, query=src))
    # sub-indexes of 1, 2, 65 and 4097 rows: the zero row right behind a single row, the fast modulo at its edges
    out["tiny"] = (str(d / "tiny.cobs_compact"), _compact(str(d / "tiny.cobs_compact"), 60, 2, [1, 2, 65, 4097], 1, 31, 6,
                                                          planted={5: 1.0, 20: 1.0, 40: 0.9, 59: 1.0}, query=src))
    out["tiny2"] = (str(d / "tiny2.cobs_compact"), _compact(str(d / "tiny2.cobs_compact"), 64, 2, [4097, 65, 2, 1], 2, 31, 7,
                                                            planted={0: 0.9, 63: 1.0}, query=src))
    out["src"] = src
    return out


def _reads(src, n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ln = int(rng.integers(lo, hi + 1))
        o = int(rng.integers(0, len(src) - ln))
        out.append(src[o:o + ln])
    return out


def _rand(n, seed):
    from oracle import oracle as O
    return O.random_sequence(n, seed)


def _check_pairs(files, queries, z, offsets, hits, bit_offsets, bits):
    """every hit's words equal the checker's (so bits >= n are zero) and their popcount is the hit's score"""
    assert len(offsets) == len(queries) + 1 and len(bit_offsets) == len(hits) + 1 and int(offsets[-1]) == len(hits)
    assert int(bit_offsets[0]) == 0 and int(bit_offsets[-1]) == len(bits) and bits.dtype == np.uint64
    rows = hits.tolist()
    for qi, q in enumerate(queries):
        for i in range(int(offsets[qi]), int(offsets[qi + 1])):
            f, d, sc = rows[i]
            pos = P.positions(files, q, z, f, d)
            got = bits[int(bit_offsets[i]):int(bit_offsets[i + 1])]
            assert len(got) == (len(pos) + 63) // 64, (qi, f, d, z)
            assert np.array_equal(got, P.pack(pos)), (qi, f, d, z)
            assert P.popcount(got) == sc, (qi, f, d, z, sc)


def _check_search(s, files, queries, z, thresholds=THRESHOLDS, limits=LIMITS):
    selected = 0
    for t in thresholds:
        for lim in limits:
            offs, hits = s.search_arrays(queries, t, lim)
            o2, h2, bo, bits = s.search_positions(queries, t, lim)
            assert np.array_equal(o2, offs) and np.array_equal(h2, hits), (z, t, lim)
            assert [h2.tolist()[int(o2[i]):int(o2[i + 1])] for i in range(len(queries))] == \
                   [F.results(files, q, z, t, lim) for q in queries]
            _check_pairs(files, queries, z, o2, h2, bo, bits)
            selected += len(h2) if t > 0 else 0
    return selected


@pytest.mark.parametrize("name", ["c1", "c3", "p1", "p3", "c2k20", "tiny", "tiny2"])
def test_every_layout_z_threshold_and_limit(gpu_lib, data, name):
    path, fb = data[name]
    src = data["src"]
    k = fb.term_size
    queries = _reads(src, 8, 50, 150, 11) + [src[100:100 + 1000 + k - 1], src[5:5 + 400], _rand(300, 5)]
    s = gpu_lib.Search(path)
    for z in ZS:
        s.set_findere(z)
        assert _check_search(s, [fb], queries, z) > 0          # (the thresholds did select planted documents)
    s.close()


def test_handle_over_two_files_of_different_term_size(gpu_lib, data):
    paths = [data["c1"][0], data["p3"][0]]
    files = [data["c1"][1], data["p3"][1]]
    src = data["src"]
    queries = _reads(src, 6, 50, 150, 21) + [src[:900]]
    s = gpu_lib.Search(paths)
    for z in ZS:
        s.set_findere(z)
        assert _check_search(s, files, queries, z) > 0
    s.close()
    # three files, the middle one with another term size
    s = gpu_lib.Search([data["p1"][0], data["c2k20"][0], data["c3"][0]], findere=3)
    _check_search(s, [data["p1"][1], data["c2k20"][1], data["c3"][1]], queries, 3, limits=(0, 10))
    s.close()


@pytest.mark.parametrize("name", ["c1", "p3"])
def test_position_counts_at_every_word_edge(gpu_lib, data, name):
    path, fb = data[name]
    src = data["src"]
    s = gpu_lib.Search(path)
    for z in ZS:
        s.set_findere(z)
        queries = []
        for n in (1, 2, 63, 64, 65, 127, 128, 129, 1000):
            ln = n + z + fb.term_size - 1
            o = (37 * n) % (len(src) - ln)
            queries.append(src[o:o + ln])
        assert [fb.positions(q, z) for q in queries] == [1, 2, 63, 64, 65, 127, 128, 129, 1000]
        _check_search(s, [fb], queries, z, limits=(0, 10))
        for q in queries:                                       # and one query per call
            _check_search(s, [fb], [q], z, thresholds=(0.8,), limits=(0,))
    s.close()


def test_query_above_65535_terms(gpu_lib, data):
    """32-bit scores, more than 1024 words per pair"""
    path, fb = data["c1"]
    q = _rand(66000 + 30 + 7, 91)
    s = gpu_lib.Search(path)
    for z in (0, 7):
        s.set_findere(z)
        assert fb.positions(q, z) > 65535
        _check_search(s, [fb], [q], z, thresholds=(0.0,), limits=(10,))
        _check_search(s, [fb], [data["src"][:200], q, data["src"][50:130]], z, thresholds=(0.0,), limits=(3,))
    s.close()


def test_reads_and_mixed_lengths(gpu_lib, data):
    """a batch of 50-150 bp reads (the multi-query form of the scan produced the hits) and a batch mixing lengths"""
    path, fb = data["p1"]
    src = data["src"]
    reads = _reads(src, 60, 50, 150, 31)
    mixed = _reads(src, 10, 50, 150, 32) + [src[:1030], src[7:7 + 2600], _rand(38, 1), src[300:300 + 517]]
    s = gpu_lib.Search(path)
    for z in ZS:
        s.set_findere(z)
        assert _check_search(s, [fb], reads, z, limits=(0, 10)) > 0
        assert _check_search(s, [fb], mixed, z, limits=(0, 10)) > 0
    s.close()


def test_pairs_that_are_no_hits(gpu_lib, data):
    """hit_positions takes any (file, document) pairs: documents with score 0, document 0, the last document of a compact
    file whose last sub-index is not full (no padding document is asked about), every document of a sub-index"""
    paths = [data["p1"][0], data["c3"][0]]
    files = [data["p1"][1], data["c3"][1]]
    src = data["src"]
    queries = [_rand(120, 3), src[40:40 + 300], _rand(31 + 7, 4)]
    s = gpu_lib.Search(paths)
    for z in ZS:
        s.set_findere(z)
        pairs = [[(0, 0), (0, 699), (0, 1), (0, 127), (0, 128), (0, 500), (1, 0), (1, 199), (1, 3)],
                 [(1, d) for d in (199, 0, 100)] + [(0, d) for d in range(640, 700)],
                 [(0, 699), (1, 7)]]
        offsets = np.cumsum([0] + [len(p) for p in pairs]).astype(np.uint64)
        hits = np.zeros(int(offsets[-1]), dtype=gpu_lib.Search.HIT_DTYPE)
        flat = [fd for p in pairs for fd in p]
        hits["file_no"] = [f for f, _ in flat]
        hits["doc"] = [d for _, d in flat]
        hits["score"] = 0xFFFFFFFF                                # ignored
        bo, bits = s.hit_positions(queries, offsets, hits)
        zero = 0
        rows = hits.tolist()
        for qi, q in enumerate(queries):
            for i in range(int(offsets[qi]), int(offsets[qi + 1])):
                f, d, _ = rows[i]
                pos = P.positions(files, q, z, f, d)
                assert np.array_equal(bits[int(bo[i]):int(bo[i + 1])], P.pack(pos)), (z, qi, f, d)
                zero += int(pos.sum() == 0)
        assert zero > 0 or z == 0                                 # (some pair did have score 0)
    # a query without pairs between two that have some, and one that is too short but is not asked about
    s.set_findere(0)
    qs = [src[:100], b"ACGT", src[100:220]]
    offsets = np.array([0, 1, 1, 2], dtype=np.uint64)
    hits = np.zeros(2, dtype=gpu_lib.Search.HIT_DTYPE)
    hits["doc"] = [1, 500]
    bo, bits = s.hit_positions(qs, offsets, hits)
    assert np.array_equal(bits[:int(bo[1])], P.pack(P.positions(files, qs[0], 0, 0, 1)))
    assert np.array_equal(bits[int(bo[1]):], P.pack(P.positions(files, qs[2], 0, 0, 500)))
    s.close()


def test_several_device_passes(gpu_lib, data):
    """the workspace limit of the search call cuts the positions call into passes as well: same words"""
    path, fb = data["p1"]
    src = data["src"]
    queries = _reads(src, 30, 50, 150, 41) + [src[:1030]]
    s = gpu_lib.Search(path, findere=3)
    offs, hits = s.search_arrays(queries, 0.0, 10)
    s.positions_ms()
    bo, bits = s.hit_positions(queries, offs, hits)
    one = s.positions_ms()
    assert one["passes"] == 1 and one["presence_ms"] > 0 and one["hash_ms"] > 0
    s.set_tuning("pass_bytes", 20000)
    bo2, bits2 = s.hit_positions(queries, offs, hits)
    assert s.positions_ms()["passes"] > 3
    assert np.array_equal(bo, bo2) and np.array_equal(bits, bits2)
    _check_pairs([fb], queries, 3, offs, hits, bo2, bits2)
    s.set_tuning("pass_bytes", 0)
    # searches before and after on the same handle are not disturbed (the call shares their workspace)
    assert s.search_hits(queries, 0.8, 0) == [F.results([fb], q, 3, 0.8, 0) for q in queries]
    for _ in range(3):                                          # (a single query: the captured-graph path)
        assert s.search_hits(queries[:1], 0.0, 5) == [F.results([fb], queries[0], 3, 0.0, 5)]
        o, h, b1, w1 = s.search_positions(queries[:1], 0.0, 5)
        _check_pairs([fb], queries[:1], 3, o, h, b1, w1)
    s.close()


def test_empty_hit_list(gpu_lib, data):
    path, fb = data["c1"]
    s = gpu_lib.Search(path)
    queries = [_rand(200, 8), _rand(90, 9)]
    s.positions_ms()
    offs, hits, bo, bits = s.search_positions(queries, 1.0, 0)
    assert offs.tolist() == [0, 0, 0] and len(hits) == 0 and bo.tolist() == [0] and len(bits) == 0 and bits.dtype == np.uint64
    bo, bits = s.hit_positions([], [0], np.zeros(0, dtype=gpu_lib.Search.HIT_DTYPE))
    assert bo.tolist() == [0] and len(bits) == 0
    assert s.positions_ms()["passes"] == 0                      # no device work
    s.close()


def _raw_call(s, queries, offsets, hits, cap_words):
    from cobs_amd import _capi
    lib = _capi.load()
    nq = len(queries)
    arr = (C.c_char_p * max(nq, 1))(*queries)
    lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in queries])
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    bits = np.full(max(cap_words, 1), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    bo = np.zeros(len(hits) + 1, dtype=np.uint64)
    need, bad = C.c_size_t(0), C.c_size_t(12345)
    st = lib.cobs_gpu_hit_positions(s._h, arr, lens, nq, C.cast(hits.ctypes.data, C.POINTER(_capi.Hit)),
                                    C.cast(offs.ctypes.data, C.POINTER(C.c_size_t)),
                                    C.cast(bits.ctypes.data, C.POINTER(C.c_uint64)), cap_words,
                                    C.cast(bo.ctypes.data, C.POINTER(C.c_size_t)), C.byref(need), C.byref(bad))
    return st, need.value, bad.value, bo, bits, lib.cobs_gpu_last_error().decode()


def test_errors_are_statuses_refused_before_any_launch(gpu_lib, data):
    from cobs_amd import _capi
    path, fb = data["c1"]
    src = data["src"]
    s = gpu_lib.Search(path, findere=3)
    good = [src[:100], src[200:340], src[400:480]]
    offs, hits = s.search_arrays(good, 0.0, 4)
    words = sum((len(q) - 31 + 1 - 3 + 63) // 64 for q in good) * 4
    # too small a buffer: the needed size, offsets filled, nothing written; the second call succeeds
    s.positions_ms()
    st, need, bad, bo, bits, msg = _raw_call(s, good, offs, hits, words - 1)
    assert st == _capi.ERR_CAPACITY and need == words and int(bo[-1]) == words, msg
    assert np.all(bits == 0xA5A5A5A5A5A5A5A5) and s.positions_ms()["passes"] == 0
    st, need, bad, bo, bits, msg = _raw_call(s, good, offs, hits, need)
    assert st == _capi.OK and need == words, msg
    _check_pairs([fb], good, 3, offs, hits, bo, bits[:words])
    # an invalid base / a query that is too short name the query
    s.positions_ms()
    bad_base = [good[0], good[1][:50] + b"N" + good[1][51:], good[2]]
    st, need, bad, bo, bits, msg = _raw_call(s, bad_base, offs, hits, words)
    assert st == _capi.ERR_INVALID_BASE and bad == 1 and "(query 1)" in msg
    short = [good[0], good[1], src[:31 + 2]]
    st, need, bad, bo, bits, msg = _raw_call(s, short, offs, hits, words)
    assert st == _capi.ERR_QUERY_TOO_SHORT and bad == 2 and str(31 + 3) in msg and "(query 2)" in msg
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.hit_positions(short, offs, hits)
    assert e.value.status == _capi.ERR_QUERY_TOO_SHORT
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.search_positions(bad_base, 0.0, 4)
    assert e.value.status == _capi.ERR_INVALID_BASE
    # a document / file number out of range, descending offsets, NULL arguments
    for field, value in (("doc", 300), ("doc", 0xFFFFFFFF), ("file_no", 1)):
        h2 = hits.copy()
        h2[field][5] = value
        st, need, bad, bo, bits, msg = _raw_call(s, good, offs, h2, words)
        assert st == _capi.ERR_ARG, (field, value, msg)
    st = _raw_call(s, good, np.array([0, 4, 2, 12], dtype=np.uint64), hits, words)[0]
    assert st == _capi.ERR_ARG
    lib = _capi.load()
    assert lib.cobs_gpu_hit_positions(s._h, None, None, 3, None, None, None, 0, None, None, None) == _capi.ERR_ARG
    assert s.positions_ms()["passes"] == 1                      # only the call with the invalid base reached the device (K1 finds it)
    # the handle still answers
    o, h, b1, w1 = s.search_positions(good, 0.8, 0)
    _check_pairs([fb], good, 3, o, h, b1, w1)
    s.close()


def test_handles_whose_rows_are_not_all_resident_refuse(gpu_lib, data):
    from cobs_amd import _capi
    path, fb = data["p1"]
    queries = [data["src"][:100]]
    for kw in ({"hbm_budget": 256 << 20}, {"shard_rank": 0, "shard_count": 2}):
        s = gpu_lib.Search(path, **kw)
        hits = np.zeros(2, dtype=gpu_lib.Search.HIT_DTYPE)      # documents 0 and 1
        hits["doc"] = [0, 1]
        with pytest.raises(gpu_lib.CobsGpuError) as e:
            s.hit_positions(queries, [0, 2], hits)
        assert e.value.status == _capi.ERR_UNSUPPORTED and "resident" in str(e.value)
        s.close()
    s = gpu_lib.Search(path, hbm_budget=256 << 20)
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.search_positions(queries, 0.0, 3)
    assert e.value.status == _capi.ERR_UNSUPPORTED
    s.close()


def test_one_query_convenience(gpu_lib, data):
    path, fb = data["c3"]
    q = data["src"][30:30 + 200]
    s = gpu_lib.Search(path, findere=1)
    res = s.search_with_positions(q, 0.8)
    want = F.results([fb], q, 1, 0.8, 0)
    assert [(r.doc_name, r.score) for r, _ in res] == [(s.doc_name(f, d), sc) for f, d, sc in want] and len(want) >= 2
    for (r, pos), (f, d, sc) in zip(res, want):
        assert pos.dtype == bool and np.array_equal(pos, P.positions([fb], q, 1, f, d)) and int(pos.sum()) == sc
    s.close()


def test_cpp_mirror(gpu_lib, data, tmp_path):
    exe = str(tmp_path / "positions_api")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "positions_api.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "cobs_amd"), "-lcobs_gpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "cobs_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    paths = [data["c1"][0], data["p3"][0]]
    files = [data["c1"][1], data["p3"][1]]
    q = data["src"][60:60 + 230]
    s = gpu_lib.Search(paths)
    for z, t, lim in ((0, 0.8, 0), (3, 0.0, 10), (7, 1.0, 0), (1, 0.0, 1)):
        r = subprocess.run([exe, str(z), str(t), str(lim), q.decode()] + paths, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        want = F.results(files, q, z, t, lim)
        lines = r.stdout.strip().splitlines()
        assert lines[-1] == "search %d" % len(want) and len(lines) == len(want) + 1 and len(want) >= 1
        for ln, (f, d, sc) in zip(lines, want):
            name, score, words = ln.split("\t")
            assert (name, int(score)) == (s.doc_name(f, d), sc)
            got = np.array([int(w, 16) for w in words.split(",")], dtype=np.uint64)
            assert np.array_equal(got, P.pack(P.positions(files, q, z, f, d))), (z, t, lim, f, d)
    s.close()
    r = subprocess.run([exe, "0", "0.8", "0", q[:20].decode()] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and r.stdout.startswith("error 3 ")          # COBS_GPU_ERR_QUERY_TOO_SHORT, thrown


def _tool():
    return os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")


def test_cli_positions(gpu_lib, data, tmp_path):
    paths = [data["c1"][0], data["p3"][0]]
    files = [data["c1"][1], data["p3"][1]]
    queries = _reads(data["src"], 5, 60, 150, 81) + [_rand(200, 3), data["src"][:700]]
    qf = tmp_path / "q.fa"
    qf.write_text("".join(">q%d\n%s\n" % (i, q.decode()) for i, q in enumerate(queries)))
    index_args = ["-i", paths[0], "-i", paths[1]]
    for z in (0, 3):
        s = gpu_lib.Search(paths, findere=z)
        for extra in (["-t", "0.8"], ["-t", "0", "-l", "10"], ["-t", "1.0", "-l", "1"], []):
            fl = ["--findere", str(z)] if z else []
            t = float(extra[1]) if extra else 0.8
            lim = int(extra[3]) if len(extra) > 2 else 0
            r = subprocess.run([_tool()] + index_args + fl + ["-f", str(qf)] + extra + ["--positions"], capture_output=True,
                               text=True, timeout=300)
            assert r.returncode == 0, r.stderr
            want, plain, ones = [], [], 0
            for i, q in enumerate(queries):
                res = F.results(files, q, z, t, lim)
                assert [(x.doc_name, x.score) for x in s.search(q, t, lim)] == [(s.doc_name(f, d), sc) for f, d, sc in res]
                want.append("*q%d\t%d" % (i, len(res)))
                plain.append(want[-1])
                for f, d, sc in res:
                    bits = "".join("1" if b else "0" for b in P.positions(files, q, z, f, d))
                    assert len(bits) == len(q) - files[f].term_size + 1 - z and bits.count("1") == sc
                    want.append("%s\t%d\t%s" % (s.doc_name(f, d), sc, bits))
                    plain.append("%s\t%d" % (s.doc_name(f, d), sc))
                    ones += 1
            assert r.stdout.splitlines() == want and ones > 0
            # without the flag: the output as it was
            r0 = subprocess.run([_tool()] + index_args + fl + ["-f", str(qf)] + extra, capture_output=True, text=True, timeout=300)
            assert r0.returncode == 0 and r0.stdout.splitlines() == plain
        # a verbatim query
        q = queries[-1]
        r = subprocess.run([_tool()] + index_args + (["--findere", str(z)] if z else []) + ["--positions", q.decode()],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        res = F.results(files, q, z, 0.8, 0)
        assert r.stdout.splitlines() == ["%s\t%d\t%s" % (s.doc_name(f, d), sc, "".join("1" if b else "0" for b in
                                                                                       P.positions(files, q, z, f, d)))
                                         for f, d, sc in res] and len(res) >= 1
        s.close()
    # refused with a clear message where the rows are not resident on one GPU
    for extra in (["-d", "0,1"], ["--hbm-budget", "1"], ["--sharded"]):
        r = subprocess.run([_tool()] + index_args + extra + ["--positions", queries[0].decode()], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 1 and "--positions: not with" in r.stderr and r.stdout == ""
