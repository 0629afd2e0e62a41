"""GPU: query prevalence (cobs_gpu_prevalence / Search.prevalence / ClassicSearch::prevalence / --prevalence) count for
count against tests/prevalence_check.py: for every position of a query the REAL documents in which its terms p .. p + z are
all present.  Every comparison is exact.

Classic rows from one byte to wider than a wave pass, compact sub-indexes of 2 to 200 row bytes and 1 to 4097 rows, a last
sub-index that is partly filled or all padding, padding slots that hold bits, H = 1 and H > 1, several term sizes, a handle
over files of different term size, every findere z at every edge of the position count, the invalid-bases policies,
several device passes, the identities against the scan and the presence kernel on a procedural handle, shards cut inside
a sub-index, every refusal, the mirrors, the CLI and the timer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import cases
from tests import findere_check as F
from tests import invalid_check as I
from tests import prevalence_check as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZS = (0, 1, 3, 7)
EDGES = (1, 2, 63, 64, 65, 128, 129, 1500)           # position counts n


def _classic(path, num_docs, sig, num_hashes, k, seed, mask=True):
    rng = np.random.default_rng(seed)
    m = cases.random_bits(rng, (sig, (num_docs + 7) // 8), 0.4)
    if mask:
        m = cases.mask_padding_docs(m, 0, num_docs)
    from oracle import construct as K
    K.write_classic(path, k, 1, ["doc_%05d" % i for i in range(num_docs)], sig, num_hashes, m)
    return path, F.FileBits(k, 1, num_hashes, [m], num_docs)


def _compact(path, num_docs, page_size, sigs, num_hashes, k, seed, mask=True):
    rng = np.random.default_rng(seed)
    page_docs = 8 * page_size
    mats = [cases.random_bits(rng, (s, page_size), 0.4) for s in sigs]
    if mask:
        mats = [cases.mask_padding_docs(m, p * page_docs, num_docs) for p, m in enumerate(mats)]
    from oracle import construct as K
    K.write_compact(path, k, 1, page_size, [(s, num_hashes) for s in sigs], ["doc_%05d" % i for i in range(num_docs)], mats)
    return path, F.FileBits(k, 1, num_hashes, mats, num_docs)


@pytest.fixture(scope="module")
def src(oracle):
    return oracle.random_sequence(3000, 77)


def _edge_queries(src, k, z, edges=EDGES):
    """one query per position count n, cut from the source at different places"""
    out = []
    for n in edges:
        ln = n + z + k - 1
        o = (37 * n) % (len(src) - ln)
        out.append(src[o:o + ln])
    return out


def _check(s, files, queries, z, mode="error", ranges=None):
    offs, counts = s.prevalence_arrays(queries)
    want_offs, want = V.segments(files, queries, z, mode, ranges)
    assert counts.dtype == np.uint32 and offs.dtype == np.uint64
    assert np.array_equal(offs, want_offs), (z, mode)
    assert np.array_equal(counts, want), (z, mode, np.nonzero(counts != want)[0][:8])
    return counts


def _sweep(gpu_lib, path, fb, src, zs=ZS, edges=EDGES):
    s = gpu_lib.Search(path)
    total = 0
    for z in zs:
        s.set_findere(z)
        qs = _edge_queries(src, fb.term_size, z, edges)
        assert [fb.positions(q, z) for q in qs] == list(edges)
        total += int(_check(s, [fb], qs, z).sum())                 # a batch that mixes the lengths
        _check(s, [fb], qs[:1], z)                                  # ... and one query alone, n = 1
    s.close()
    return total


@pytest.mark.parametrize("num_hashes", [1, 3])
@pytest.mark.parametrize("num_docs", [1, 7, 8, 9, 127, 129, 300, 1027])
def test_classic_layouts(gpu_lib, src, tmp_path, num_docs, num_hashes):
    """the tail bits of the last byte, the tail bytes of the last 16-byte chunk, rows narrower and wider than a wave pass"""
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), num_docs, 2003, num_hashes, 31, num_docs)
    assert _sweep(gpu_lib, path, fb, src) > 0


@pytest.mark.parametrize("sigs", [[1, 2, 65, 4097], [1201, 997, 1500, 1103, 1301, 800]])
@pytest.mark.parametrize("page_size", [2, 8, 16, 200])
def test_compact_layouts(gpu_lib, src, tmp_path, page_size, sigs):
    """a last sub-index that is partly filled; lanes side by side along the positions for the narrow rows"""
    num_docs = len(sigs) * 8 * page_size - 5 * page_size - 3
    assert (len(sigs) - 1) * 8 * page_size < num_docs
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), num_docs, page_size, sigs, 1 if page_size != 8 else 2, 31, page_size)
    assert _sweep(gpu_lib, path, fb, src, edges=(1, 2, 63, 64, 65, 128, 129, 700)) > 0


def test_trailing_sub_index_of_padding(gpu_lib, src, tmp_path):
    path, fb = _compact(str(tmp_path / "t.cobs_compact"), 2 * 128 - 9, 16, [501, 703, 601], 1, 31, 5)
    assert (fb.doc_of_slot()[256:] < 0).all()
    assert _sweep(gpu_lib, path, fb, src, zs=(0, 3), edges=(1, 65, 300)) > 0


def test_padding_slots_with_set_bits_are_not_counted(gpu_lib, src, tmp_path):
    """files written WITHOUT masking the padding documents: their slots hold random bits"""
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 5, 301, 1, 31, 3, mask=False)
    q = src[:200]
    assert V.windows(fb, q, 0)[:, 5:].any()                         # (the padding slots would have counted)
    assert _sweep(gpu_lib, path, fb, src, zs=(0, 3), edges=(1, 64, 170)) > 0
    # compact: the second sub-index partly filled, the third all padding, both with bits everywhere
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), 100, 8, [211, 307, 401], 2, 31, 4, mask=False)
    assert V.windows(fb, q, 0)[:, 100:128].any() and V.windows(fb, q, 0)[:, 128:].any()
    s = gpu_lib.Search(path)
    for z in (0, 3):
        s.set_findere(z)
        counts = _check(s, [fb], _edge_queries(src, 31, z, (1, 64, 170)), z)
        assert counts.max() <= 100
    s.close()


@pytest.mark.parametrize("k", [15, 20, 25, 31])
def test_term_sizes(gpu_lib, src, tmp_path, k):
    path, fb = _compact(str(tmp_path / "k.cobs_compact"), 300, 8, [901, 1003, 777, 1300, 950], 3, k, k)
    assert _sweep(gpu_lib, path, fb, src, zs=(0, 3), edges=(1, 64, 129, 400)) > 0


def test_handle_over_two_files_of_different_term_size(gpu_lib, src, tmp_path):
    """the segments of a query have different lengths per file"""
    pa, fa = _classic(str(tmp_path / "a.cobs_classic"), 300, 2003, 1, 31, 1)
    pb, fb = _compact(str(tmp_path / "b.cobs_compact"), 150, 4, [499, 601, 701, 557, 811], 2, 20, 2)
    s = gpu_lib.Search([pa, pb])
    for z in ZS:
        s.set_findere(z)
        qs = _edge_queries(src, 31, z, (1, 2, 64, 65, 500))
        offs, _counts = s.prevalence_arrays(qs)
        assert int(offs[2]) - int(offs[1]) == int(offs[1]) - int(offs[0]) + 11
        _check(s, [fa, fb], qs, z)
        per = s.prevalence(qs)                                      # the list form: one array per file
        assert len(per) == len(qs) and all(len(p) == 2 for p in per)
        assert np.array_equal(per[3][1], V.prevalence(fb, qs[3], z)) and per[3][1].dtype == np.uint32
        one = s.prevalence(qs[2].decode())                          # a single str query: that query's list
        assert len(one) == 2 and np.array_equal(one[0], V.prevalence(fa, qs[2], z))
    s.close()


@pytest.mark.parametrize("mode", I.MODES)
def test_invalid_bases_read_zero(gpu_lib, src, tmp_path, mode):
    path, fb = _compact(str(tmp_path / "n.cobs_compact"), 300, 8, [901, 1003, 777, 1300, 950], 2, 31, 9)
    base = src[40:40 + 260]
    s = gpu_lib.Search(path, invalid_bases=mode)
    for z in (0, 3):
        s.set_findere(z)
        qs = [I.with_n(base, [o]) for o in (0, 130, len(base) - 1)] + [base, I.with_n(base, [7, 200]), b"N" * 100]
        offs, counts = s.prevalence_arrays(qs)
        _check(s, [fb], qs, z, mode)
        for i, q in enumerate(qs):
            bad = ~I.position_valid(fb, q, z)
            seg = counts[int(offs[i]):int(offs[i + 1])]
            assert len(seg) == len(bad) and not seg[bad].any() and (i == 3 or bad.any())
        assert counts[int(offs[3]):int(offs[4])].sum() > 0
    s.close()


def _raw_call(s, queries, cap, null_offsets=False):
    from cobs_amd import _capi
    lib = _capi.load()
    nq = len(queries)
    arr = (C.c_char_p * max(nq, 1))(*queries)
    lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in queries])
    counts = np.full(max(cap, 1), 0xA5A5A5A5, dtype=np.uint32)
    offs = np.full(nq * s.num_files + 1, 0xFFFF, dtype=np.uint64)
    need, bad = C.c_size_t(0), C.c_size_t(12345)
    st = lib.cobs_gpu_prevalence(s._h, arr, lens, nq, C.cast(counts.ctypes.data, C.POINTER(C.c_uint32)) if cap else None, cap,
                                 None if null_offsets else C.cast(offs.ctypes.data, C.POINTER(C.c_size_t)),
                                 C.byref(need), C.byref(bad))
    return st, need.value, bad.value, offs, counts, lib.cobs_gpu_last_error().decode()


def test_invalid_base_under_error_names_the_query(gpu_lib, src, tmp_path):
    from cobs_amd import _capi
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 129, 2003, 1, 31, 1)
    s = gpu_lib.Search(path, findere=1)
    good = [src[:100], src[200:340], src[400:480]]
    cells = sum(len(q) - 31 + 1 - 1 for q in good)
    bad_base = [good[0], good[1], good[2][:40] + b"N" + good[2][41:]]
    st, need, bad, offs, counts, msg = _raw_call(s, bad_base, cells)
    assert st == _capi.ERR_INVALID_BASE and bad == 2 and "(query 2)" in msg
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.prevalence(bad_base)
    assert e.value.status == _capi.ERR_INVALID_BASE
    _check(s, [fb], good, 1)                                        # the handle still answers
    s.close()


def test_several_device_passes(gpu_lib, src, tmp_path):
    """the workspace limit of the search call cuts the call into passes: same counts"""
    path, fb = _compact(str(tmp_path / "p.cobs_compact"), 700, 16, [1201, 997, 1500, 1103, 1301, 800], 1, 31, 3)
    rng = np.random.default_rng(41)
    queries = []
    for _ in range(39):
        ln = int(rng.integers(50, 151))
        o = int(rng.integers(0, len(src) - ln))
        queries.append(src[o:o + ln])
    queries.append(src[:1030])
    s = gpu_lib.Search(path, findere=3)
    s.prevalence_ms()
    offs, counts = s.prevalence_arrays(queries)
    one = s.prevalence_ms()
    assert one["passes"] == 1 and one["kernel_ms"] > 0 and one["hash_ms"] > 0
    s.set_tuning("pass_bytes", 30000)
    offs2, counts2 = s.prevalence_arrays(queries)
    assert s.prevalence_ms()["passes"] >= 3
    assert np.array_equal(offs, offs2) and np.array_equal(counts, counts2)
    s.set_tuning("pass_bytes", 0)
    want_offs, want = V.segments([fb], queries, 3)
    assert np.array_equal(offs, want_offs) and np.array_equal(counts, want)
    # searches before and after on the same handle are not disturbed (the call shares their workspace)
    assert s.search_hits(queries[:5], 0.0, 3) == [F.results([fb], q, 3, 0.0, 3) for q in queries[:5]]
    _check(s, [fb], queries[:3], 3)
    s.close()


@pytest.mark.parametrize("z", [0, 3])
def test_identities_against_the_scan_and_the_presence_kernel(gpu_lib, oracle, z):
    """a procedural handle larger than the numpy restatement likes: the sum over the positions is the sum over the real
    documents of the score row; a position's count is the number of documents whose hit_positions bit is set"""
    sigs = [20011, 30011, 25013, 40009, 35023, 45007]
    num_docs, page_size = 5000, 105
    s = gpu_lib.Search.synthetic("compact", sigs, num_docs, page_size=page_size, seed=5, findere=z)
    assert s.total_counts == 6 * 8 * page_size >= num_docs
    queries = [oracle.random_sequence(300 + 30 + z, 100 + i) for i in range(64)]
    text = oracle.random_sequence(400, 7)
    s.plant(text, list(range(0, 5000, 7)), 900, salt=1)             # some positions widely held, beyond the random bits
    queries[5], queries[40] = text[:330 + z], text[50:380 + z]
    offs, counts = s.prevalence_arrays(queries)
    assert len(counts) == 64 * 300 and counts.max() <= num_docs and counts[int(offs[5]):int(offs[6])].min() > 100
    for i, q in enumerate(queries):
        assert int(counts[int(offs[i]):int(offs[i + 1])].sum(dtype=np.uint64)) == int(s.counts(q)[:num_docs].sum(dtype=np.uint64)), i
    hits = np.zeros(num_docs, dtype=gpu_lib.Search.HIT_DTYPE)
    hits["doc"] = np.arange(num_docs)
    for i in (5, 17):
        bo, bits = s.hit_positions([queries[i]], [0, num_docs], hits)
        words = bits.reshape(num_docs, -1)
        for p in (0, 1, 63, 64, 150, 299):
            assert int(((words[:, p // 64] >> np.uint64(p % 64)) & np.uint64(1)).sum()) == int(counts[int(offs[i]) + p]), (i, p)
    s.close()


@pytest.mark.parametrize("kind", ["compact", "classic"])
def test_shards_add_up(gpu_lib, src, tmp_path, kind):
    """one shard of several answers for the documents of its own slots; a cut falls inside a sub-index"""
    if kind == "compact":
        path, fb = _compact(str(tmp_path / "s.cobs_compact"), 6 * 8 * 48 - 7, 48, [300, 900, 200, 1500, 400, 650], 1, 31, 4)
        page_docs = 8 * 48
    else:
        path, fb = _classic(str(tmp_path / "s.cobs_classic"), 1027, 2003, 2, 31, 4)
        page_docs = fb.slots
    z = 1
    queries = _edge_queries(src, 31, z, (1, 64, 65, 300))
    s = gpu_lib.Search(path, findere=z)
    _whole_offs, whole = s.prevalence_arrays(queries)
    s.close()
    inside = 0
    for count in (2, 3):
        for mode in (0, 1, 2):
            total = np.zeros_like(whole)
            pos = 0
            for rank in range(count):
                s = gpu_lib.Search(path, shard_rank=rank, shard_count=count, shard_mode=mode, findere=z)
                i = s.info(0)
                assert int(i.slot_begin) == pos, (count, mode, rank)
                inside += int(int(i.slot_begin) % page_docs != 0)
                total += _check(s, [fb], queries, z, ranges=[(int(i.slot_begin), int(i.slot_count))])
                pos += int(i.slot_count)
                s.close()
            assert pos == fb.slots and np.array_equal(total, whole), (count, mode)
    assert inside > 0


def test_refusals_come_back_before_any_device_work(gpu_lib, src, tmp_path):
    from cobs_amd import _capi
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 300, 2003, 1, 31, 1)
    s = gpu_lib.Search(path, findere=3)
    good = [src[:100], src[200:340], src[400:480]]
    cells = sum(len(q) - 31 + 1 - 3 for q in good)
    s.prevalence_ms()
    # a capacity of 0 (counts NULL) and one that is too small: the needed size and the offsets, nothing written
    st, need, bad, offs, counts, msg = _raw_call(s, good, 0)
    assert st == _capi.ERR_CAPACITY and need == cells and offs.tolist() == [0, 67, 67 + 107, cells], msg
    st, need, bad, offs, counts, msg = _raw_call(s, good, cells - 1)
    assert st == _capi.ERR_CAPACITY and need == cells and int(offs[-1]) == cells and np.all(counts == 0xA5A5A5A5)
    # a query that is too short names the query
    short = [good[0], good[1], src[:31 + 2]]
    st, need, bad, offs, counts, msg = _raw_call(s, short, cells)
    assert st == _capi.ERR_QUERY_TOO_SHORT and bad == 2 and str(31 + 3) in msg and "(query 2)" in msg
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.prevalence(short)
    assert e.value.status == _capi.ERR_QUERY_TOO_SHORT
    # NULL arguments
    lib = _capi.load()
    assert lib.cobs_gpu_prevalence(s._h, None, None, 3, None, 0, None, None, None) == _capi.ERR_ARG
    assert _raw_call(s, good, cells, null_offsets=True)[0] == _capi.ERR_ARG
    offs = (C.c_size_t * 4)()
    assert lib.cobs_gpu_prevalence(s._h, None, None, 3, None, 0, offs, None, None) == _capi.ERR_ARG
    arr = (C.c_char_p * 3)(*good)
    lens = (C.c_size_t * 3)(*[len(q) for q in good])
    assert lib.cobs_gpu_prevalence(s._h, arr, lens, 3, None, cells, offs, None, None) == _capi.ERR_ARG      # cap without counts
    assert s.prevalence_ms()["passes"] == 0                         # none of these reached the device
    st, need, bad, offs, counts, msg = _raw_call(s, good, cells)
    assert st == _capi.OK and need == cells, msg
    assert np.array_equal(counts[:cells], V.segments([fb], good, 3)[1])
    s.close()
    # a handle with an HBM budget
    s = gpu_lib.Search(path, hbm_budget=256 << 20)
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.prevalence(good)
    assert e.value.status == _capi.ERR_UNSUPPORTED and "HBM budget" in str(e.value)
    assert s.prevalence_ms()["passes"] == 0
    s.close()


def _tool():
    return os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")


def test_cli_and_cpp_mirror_agree_with_the_arrays(gpu_lib, src, tmp_path):
    """cobs_gpu_query --prevalence prints what ClassicSearch::prevalence returns: per query its comment line, then per
    file file_no, num_docs, n and the n counts"""
    pa, fa = _classic(str(tmp_path / "a.cobs_classic"), 300, 2003, 1, 31, 1)
    pb, fb = _compact(str(tmp_path / "b.cobs_compact"), 150, 4, [499, 601, 701, 557, 811], 2, 20, 2)
    paths, files = [pa, pb], [fa, fb]
    queries = _edge_queries(src, 31, 3, (1, 64, 200)) + [I.with_n(src[100:300], [90])]
    qf = tmp_path / "q.fa"
    qf.write_text("".join(">q%d\n%s\n" % (i, q.decode()) for i, q in enumerate(queries)))
    index_args = ["-i", paths[0], "-i", paths[1]]
    for z, mode in ((0, "miss"), (3, "skip")):
        s = gpu_lib.Search(paths, findere=z, invalid_bases=mode)
        offs, counts = s.prevalence_arrays(queries)
        want_offs, want = V.segments(files, queries, z, mode)
        assert np.array_equal(offs, want_offs) and np.array_equal(counts, want)
        s.close()
        fl = (["--findere", str(z)] if z else []) + ["--invalid-bases", mode]
        r = subprocess.run([_tool()] + index_args + fl + ["-f", str(qf), "--prevalence"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == 3 * len(queries)
        for i, q in enumerate(queries):
            assert lines[3 * i] == "*q%d\t2" % i
            for f in range(2):
                file_no, num_docs, n, cs = lines[3 * i + 1 + f].split("\t")
                seg = counts[int(offs[2 * i + f]):int(offs[2 * i + f + 1])]
                assert (int(file_no), int(num_docs), int(n)) == (f, files[f].num_docs, len(seg))
                assert np.array_equal(np.array([int(c) for c in cs.split(" ")], dtype=np.uint32), seg), (z, i, f)
    # a verbatim query: the file lines only
    q = queries[2]
    r = subprocess.run([_tool()] + index_args + ["--prevalence", q.decode()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 2
    for f in range(2):
        file_no, num_docs, n, cs = lines[f].split("\t")
        assert int(file_no) == f and np.array_equal(np.array([int(c) for c in cs.split(" ")], dtype=np.uint32), V.prevalence(files[f], q, 0))
    # refused with a clear message where the rows are not resident on one GPU
    for extra in (["--hbm-budget", "1"], ["-d", "0,1"], ["--sharded"]):
        r = subprocess.run([_tool()] + index_args + extra + ["--prevalence", q.decode()], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--prevalence: not with" in r.stderr and r.stdout == ""


def test_timer_resets_on_read(gpu_lib, src, tmp_path):
    path, fb = _classic(str(tmp_path / "c.cobs_classic"), 129, 2003, 1, 31, 1)
    s = gpu_lib.Search(path)
    assert s.prevalence_ms() == {"kernel_ms": 0.0, "hash_ms": 0.0, "passes": 0}
    s.prevalence([src[:200], src[300:700]])
    t = s.prevalence_ms()
    assert t["kernel_ms"] > 0 and t["hash_ms"] > 0 and t["passes"] == 1
    assert s.prevalence_ms() == {"kernel_ms": 0.0, "hash_ms": 0.0, "passes": 0}
    s.close()
