"""GPU: findere scoring (cobs_gpu_set_findere / Search(findere=z) / --findere) bit for bit against the numpy restatement
of tests/findere_check.py: a position p of a query scores in a document when its terms p .. p + z are all present there
(every term: all H bits set), thresholds are ceil(threshold * (T - z)), ordering as COBS orders.

Every result path (counts, search, search_arrays, search_view, the device-resident batches, the sharded calls and the
CLI), both index kinds, H = 1 and H > 1, several term sizes, reads (the multi-query scan), long queries (16- and 32-bit
scores) and every block / virtual-wave boundary of the scan's contiguous block ranges."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cases
from tests import findere_check as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZS = (1, 2, 3, 7)


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
    d = tmp_path_factory.mktemp("findere")
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


def _check_counts(s, files, queries, z):
    for q in queries:
        np.testing.assert_array_equal(s.counts(q), F.counts(files, q, z))


def _check_results(s, files, queries, z, thresholds=(0.0, 0.8, 1.0), limits=(0, 1, 10), view=True):
    for t in thresholds:
        for lim in limits:
            want = [F.results(files, q, z, t, lim) for q in queries]
            got = s.search_hits(queries, t, lim)
            assert got == want, (z, t, lim)
            offs, hits = s.search_arrays(queries, t, lim)
            rows = hits.tolist()
            assert [rows[int(offs[i]):int(offs[i + 1])] for i in range(len(queries))] == want
            if view:
                offs, hits = s.search_view(queries, t, lim)
                rows = hits.tolist()
                assert [rows[int(offs[i]):int(offs[i + 1])] for i in range(len(queries))] == want
            one = s.search(queries[0], t, lim)
            assert [(r.doc_name, r.score) for r in one] == [(s.doc_name(f, d), sc) for (f, d, sc) in want[0]]


def _check_batch(s, files, queries, z):
    b = gpu_lib_batch(s)
    b.set_queries(queries)
    b.run_hits(0.8)
    b.sync()
    for i, q in enumerate(queries):
        assert b.hits_host(i) == F.results(files, q, z, 0.8, 0)
    for keep in (True, False):
        b.run_topk(0.0, 10, keep_counts=keep)
        b.sync()
        for i, q in enumerate(queries):
            assert b.hits_host(i, 10) == F.results(files, q, z, 0.0, 10)
    b.run(0.0)
    b.sync()
    for i, q in enumerate(queries):
        np.testing.assert_array_equal(b.counts_host(i), F.counts(files, q, z))
    b.close()


def gpu_lib_batch(s):
    import cobs_amd
    return cobs_amd.Batch(s)


@pytest.mark.parametrize("name", ["c1", "c3", "p1", "p3", "c2k20"])
def test_every_result_path_reads_and_long_queries(gpu_lib, data, name):
    path, fb = data[name]
    src = data["src"]
    reads = _reads(src, 12, 40, 150, 11)
    longq = [src[100:100 + 1000 + fb.term_size - 1], src[5:5 + 1200], gpu_lib_rand(1030, 5)]
    s = gpu_lib.Search(path)
    assert s.findere == 0
    for z in ZS:
        s.set_findere(z)
        assert s.findere == z
        _check_counts(s, [fb], reads + longq, z)
        _check_results(s, [fb], reads, z)
        _check_results(s, [fb], longq, z, thresholds=(0.0, 0.8), limits=(0, 10))
        _check_batch(s, [fb], reads[:6] + longq[:1], z)
    s.close()


def gpu_lib_rand(n, seed):
    from oracle import oracle as O
    return O.random_sequence(n, seed)


def test_multi_file_handle_with_different_term_sizes(gpu_lib, data):
    paths = [data["c1"][0], data["p3"][0], data["c2k20"][0]]
    files = [data["c1"][1], data["p3"][1], data["c2k20"][1]]
    src = data["src"]
    queries = _reads(src, 8, 45, 150, 21) + [src[:900]]
    s = gpu_lib.Search(paths, findere=3)
    assert s.findere == 3
    for z in (3, 7, 1):
        s.set_findere(z)
        _check_counts(s, files, queries, z)
        _check_results(s, files, queries, z, limits=(0, 10))
        _check_batch(s, files, queries[:4], z)
    s.close()


@pytest.mark.parametrize("mq", [-1, 0, 1])
def test_reads_through_each_scan_form(gpu_lib, data, mq):
    """100-bp reads are the multi-query form of the scan (lane groups of a wave serve different queries); forced on /
    off / automatic, every wave count"""
    path, fb = data["p1"]
    reads = _reads(data["src"], 40, 40, 150, 31 + mq)
    s = gpu_lib.Search(path)
    s.set_tuning("mq", mq)
    for waves in (0, 1, 2, 4):
        s.set_tuning("waves", waves)
        for z in (2, 7):
            s.set_findere(z)
            want = [F.results([fb], q, z, 0.0, 0) for q in reads]
            assert s.search_hits(reads, 0.0, 0) == want
            assert s.search_hits(reads, 0.8, 0) == [F.results([fb], q, z, 0.8, 0) for q in reads]
    s.close()


def test_block_and_wave_boundaries(gpu_lib, data):
    """T - z = 0..7 mod 8 at several block counts, under 1, 2 and 4 waves per group and every tile width: every way a
    contiguous block range and its primed window can start and end"""
    for name in ("c1", "c3"):
        path, fb = data[name]
        s = gpu_lib.Search(path)
        src = data["src"]
        for z in (1, 3, 7):
            s.set_findere(z)
            qs = []
            for m in (0, 1, 3, 9, 40):
                for r in range(8):
                    n = 8 * m + r                                  # T - z
                    if n < 1:
                        continue
                    ln = n + z + fb.term_size - 1
                    o = (37 * m + 11 * r) % (len(src) - ln)
                    qs.append(src[o:o + ln])
            want = [F.counts([fb], q, z) for q in qs]
            for waves in (1, 2, 4):
                s.set_tuning("waves", waves)
                for tw in (0, 4, 64):
                    s.set_tuning("tile_w", tw)
                    b = gpu_lib.Batch(s)
                    b.set_queries(qs)
                    b.run(0.0)
                    b.sync()
                    for i in range(len(qs)):
                        np.testing.assert_array_equal(b.counts_host(i), want[i], err_msg="%s z %d waves %d tile %d query %d" %
                                                      (name, z, waves, tw, i))
                    b.close()
            s.set_tuning("waves", 0)
            s.set_tuning("tile_w", 0)
        s.close()


def test_query_above_65535_terms(gpu_lib, data):
    """32-bit scores"""
    path, fb = data["c1"]
    q = gpu_lib_rand(66000 + 30 + 7, 91)
    s = gpu_lib.Search(path, findere=7)
    np.testing.assert_array_equal(s.counts(q), F.counts([fb], q, 7))
    assert s.search_hits([q], 0.0, 10) == [F.results([fb], q, 7, 0.0, 10)]
    s.close()


def test_short_queries(gpu_lib, data):
    from cobs_amd import _capi
    path, fb = data["c1"]
    s = gpu_lib.Search(path)
    for z in ZS:
        s.set_findere(z)
        q = data["src"][50:50 + 31 + z]
        c = s.counts(q)
        assert c.max() <= 1
        np.testing.assert_array_equal(c, F.counts([fb], q, z))
        assert s.search_hits([q], 1.0, 0) == [F.results([fb], q, z, 1.0, 0)]
        with pytest.raises(gpu_lib.CobsGpuError) as e:
            s.search(q[:-1])
        assert e.value.status == _capi.ERR_QUERY_TOO_SHORT and str(31 + z) in str(e.value)
        with pytest.raises(gpu_lib.CobsGpuError) as e:
            s.search_arrays([data["src"][:200], q[:-1]])
        assert e.value.status == _capi.ERR_QUERY_TOO_SHORT
    # a batch samples z when it RUNS: queries set at z = 0, run at z = 3
    s.set_findere(0)
    b = gpu_lib.Batch(s)
    b.set_queries([data["src"][:32]])
    s.set_findere(3)
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        b.run(0.0)
    assert e.value.status == _capi.ERR_QUERY_TOO_SHORT
    s.set_findere(0)
    b.run(0.0)
    b.sync()
    np.testing.assert_array_equal(b.counts_host(0), F.counts([fb], data["src"][:32], 0))
    b.close()
    with pytest.raises(ValueError):
        s.set_findere(8)
    assert s.findere == 0
    s.close()


def test_z0_through_the_setter_is_the_plain_search(gpu_lib, data, oracle):
    path, fb = data["p3"]
    queries = _reads(data["src"], 10, 40, 150, 41) + [data["src"][:1000]]
    a = gpu_lib.Search(path)
    b = gpu_lib.Search(path)
    b.set_findere(5)
    b.set_findere(0)
    ix = oracle.Index.open(path)
    for q in queries:
        np.testing.assert_array_equal(F.counts([fb], q, 0), ix.counts(q))          # the restatement's anchor
    for t, lim in ((0.0, 0), (0.8, 0), (0.0, 10)):
        assert a.search_hits(queries, t, lim) == b.search_hits(queries, t, lim)
    ba, bb = gpu_lib.Batch(a), gpu_lib.Batch(b)
    for bt in (ba, bb):
        bt.set_queries(queries)
        bt.run(0.0)
        bt.sync()
    for i in range(len(queries)):
        np.testing.assert_array_equal(ba.counts_host(i), bb.counts_host(i))
    ba.close()
    bb.close()
    a.close()
    b.close()


def test_graph_shape_class_holds_z(gpu_lib, data):
    """a single query is captured into a graph the second time its shape comes along; z is part of the shape"""
    path, fb = data["c1"]
    q = data["src"][200:200 + 130]
    s = gpu_lib.Search(path)
    r0 = F.results([fb], q, 0, 0.0, 10)
    r3 = F.results([fb], q, 3, 0.0, 10)
    assert r0 != r3
    for _ in range(3):
        assert [(x.doc_name, x.score) for x in s.search(q, 0.0, 10)] == [(s.doc_name(f, d), sc) for f, d, sc in r0]
    replays = s.graph_replays
    s.set_findere(3)
    for _ in range(3):
        assert [(x.doc_name, x.score) for x in s.search(q, 0.0, 10)] == [(s.doc_name(f, d), sc) for f, d, sc in r3]
    s.set_findere(0)
    assert [(x.doc_name, x.score) for x in s.search(q, 0.0, 10)] == [(s.doc_name(f, d), sc) for f, d, sc in r0]
    assert s.graph_replays > replays        # (the graphs did replay: the check above is not vacuous)
    s.close()


def test_planted_documents(gpu_lib):
    import cobs_amd
    sig, D = 4099, 1500
    s = cobs_amd.Search.synthetic("classic", [sig], D, seed=9)
    text = gpu_lib_rand(600, 123)
    s.plant(text, [5, 700], keep_permille=1000)
    s.plant(text, [1499], keep_permille=900, salt=3)
    rows = s.read_rows(0, 0, 0, sig)
    fb = F.FileBits(31, 1, 1, [rows], D)
    T = len(text) - 30
    for z in ZS:
        s.set_findere(z)
        c = s.counts(text)
        assert c[5] == T - z and c[700] == T - z
        np.testing.assert_array_equal(c, F.counts([fb], text, z))
        assert s.search_hits([text], 0.8, 0) == [F.results([fb], text, z, 0.8, 0)]
    s.close()


def test_stated_effect_on_unrelated_documents(gpu_lib):
    import cobs_amd
    s = cobs_amd.Search.synthetic("classic", [1 << 20], 4000, seed=3)
    qs = [gpu_lib_rand(1030, 500 + i) for i in range(8)]
    means = {}
    for z in (0, 3):
        s.set_findere(z)
        c = np.stack([s.counts(q)[:4000] for q in qs]).astype(np.float64)
        means[z] = c.mean() / (1000 - z)
    assert 0.25 < means[0] < 0.35, means
    assert means[3] < 0.02, means
    s.close()


def test_hbm_budget_handle_refuses(gpu_lib, data, oracle):
    from cobs_amd import _capi
    path, fb = data["p1"]
    s = gpu_lib.Search(path, hbm_budget=256 << 20)
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.set_findere(3)
    assert e.value.status == _capi.ERR_UNSUPPORTED
    lib = _capi.load()
    assert lib.cobs_gpu_set_findere(s._h, 8) == _capi.ERR_ARG
    s.set_findere(0)
    assert s.findere == 0
    queries = _reads(data["src"], 6, 40, 150, 51)
    ix = oracle.Index.open(path)
    for q in queries:
        np.testing.assert_array_equal(s.counts(q), ix.counts(q))
    assert s.search_hits(queries, 0.0, 10) == [F.results([fb], q, 0, 0.0, 10) for q in queries]
    s.close()
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        gpu_lib.Search(path, hbm_budget=256 << 20, findere=2)
    assert e.value.status == _capi.ERR_UNSUPPORTED


def test_sharded_one_rank(gpu_lib, data, comm_one_rank):
    paths = [data["c1"][0], data["p3"][0]]
    files = [data["c1"][1], data["p3"][1]]
    queries = _reads(data["src"], 6, 40, 150, 61) + [data["src"][:700]]
    s = gpu_lib.Search(paths, findere=3)
    for t, lim in ((0.0, 0), (0.8, 0), (0.0, 10)):
        want = [F.results(files, q, 3, t, lim) for q in queries]
        assert s.sharded_search_hits(comm_one_rank, queries, t, lim) == want
    s.close()


_RANKS_SCRIPT = r"""
import os, sys, numpy as np
sys.path.insert(0, %(root)r)
import cobs_amd
paths = %(paths)r
queries = [bytes(q) for q in %(queries)r]
single = cobs_amd.Search(paths)
for z in (3, 7):
    single.set_findere(z)
    m = cobs_amd.MultiSearch(paths, [0] * %(ranks)d, findere=z)
    assert m.findere == z
    for r in range(%(ranks)d):
        assert m.shard(r).findere == z
    for t, lim in ((0.0, 0), (0.8, 0), (0.0, 10), (1.0, 1)):
        assert m.search_hits(queries, t, lim) == single.search_hits(queries, t, lim), (z, t, lim)
    m.set_findere(0)
    assert m.search_hits(queries, 0.0, 10) == cobs_amd.Search(paths).search_hits(queries, 0.0, 10)
    m.close()
print("ok")
"""


@pytest.fixture(scope="module")
def mock_library(gpu_lib):
    r = subprocess.run(["bash", os.path.join(ROOT, "tests", "mock_rccl", "build.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    lib = os.path.join(ROOT, "cobs_amd", "libmockrccl.so")
    assert os.path.exists(lib)
    return lib


@pytest.mark.parametrize("ranks", [2, 3])
def test_device_list_handle_over_ranks_sharing_the_gpu(mock_library, data, ranks):
    paths = [data["p1"][0], data["c3"][0]]
    queries = [list(q) for q in _reads(data["src"], 6, 40, 150, 71)] + [list(data["src"][:600])]
    code = _RANKS_SCRIPT % {"root": ROOT, "paths": paths, "queries": queries, "ranks": ranks}
    pre = ":".join([mock_library] + [p for p in os.environ.get("LD_PRELOAD", "").split(":") if p])
    env = dict(os.environ, LD_PRELOAD=pre)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-6000:]
    assert "[mock rccl]" not in r.stderr, r.stderr[-6000:]


def _tool():
    return os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")


def test_cli_query_and_benchmark_fpr(gpu_lib, data, tmp_path):
    path, fb = data["c1"]
    queries = _reads(data["src"], 5, 60, 150, 81) + [gpu_lib_rand(200, 3)]
    qf = tmp_path / "q.fa"
    qf.write_text("".join(">q%d\n%s\n" % (i, q.decode()) for i, q in enumerate(queries)))
    s = gpu_lib.Search(path, findere=3)
    for extra in (["-t", "0.8"], ["-t", "0", "-l", "10"], ["-t", "0.3"]):
        r = subprocess.run([_tool(), "-i", path, "--findere", "3", "-f", str(qf)] + extra, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        t = float(extra[1])
        lim = int(extra[3]) if len(extra) > 2 else 0
        want = []
        for i, q in enumerate(queries):
            res = s.search(q, t, lim)
            want.append("*q%d\t%d" % (i, len(res)))
            want += ["%s\t%d" % (x.doc_name, x.score) for x in res]
        assert r.stdout.strip().splitlines() == want
    s.close()
    fpr = {}
    for z in (0, 3):
        r = subprocess.run([_tool(), "benchmark-fpr", path, "-k", "300", "-q", "40", "-w", "2", "--seed", "5",
                            "--findere", str(z)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        line = r.stdout.strip().splitlines()[0]
        kv = dict(f.split("=", 1) for f in line.split()[1:])
        assert kv["findere"] == str(z)
        fpr[z] = float(kv["fpr"])
    assert fpr[3] < fpr[0] / 10 and 0.2 < fpr[0] < 0.4, fpr
