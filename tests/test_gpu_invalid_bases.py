"""GPU: the invalid-bases policy (cobs_gpu_set_invalid_bases / Search(invalid_bases=...) / --invalid-bases) bit for bit
against the numpy restatement of tests/invalid_check.py.

`error` keeps failing the call with the first bad query; under `miss` and `skip` a k-mer that holds a character outside
ACGT names the zero row in K1's table, so every result path, findere, hit positions, budgeted handles and the device
list follow; `skip` takes its thresholds from the valid positions K1 counts (ceil(t * V), at least 1), on the device.
tests/test_invalid_bases_cpu.py checks on the CPU that the query sets below hold what the tests here need (a query with
V = 0, one with V = T, the miss-versus-skip document, the replay pair, the alignment cases)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cases
from tests import findere_check as F
from tests import invalid_check as V
from cobs_amd.search import unpack_positions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTED_FULL = 0          # the document of "c1" that holds every k-mer of the source text


def _gpu(fn):
    return pytest.mark.gpu(fn)


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


def _classic(path, num_docs, sig, num_hashes, k, seed, planted=None, query=None):
    cases.make_classic(path, num_docs, sig, num_hashes, k, 1, 0.3, seed, planted=planted, query=query)
    return F.classic_file(path)


def build_files(d, oracle):
    """index files with planted matches (thresholds 0.8 / 1.0 select something) and their bits"""
    src = oracle.random_sequence(3000, 77)
    j = lambda n: os.path.join(d, n)
    out = {"src": src}
    out["c1"] = (j("c1.cobs_classic"), _classic(j("c1.cobs_classic"), 300, 2003, 1, 31, 1,
                                                planted={PLANTED_FULL: 1.0, 7: 0.95, 150: 0.8}, query=src))
    out["c3"] = (j("c3.cobs_classic"), _classic(j("c3.cobs_classic"), 200, 3001, 3, 31, 2, planted={3: 1.0, 199: 0.9}, query=src))
    out["p1"] = (j("p1.cobs_compact"), _compact(j("p1.cobs_compact"), 700, 16, [1201, 997, 1500, 1103, 1301, 800], 1, 31, 3,
                                                planted={1: 1.0, 500: 0.9}, query=src))
    out["p3"] = (j("p3.cobs_compact"), _compact(j("p3.cobs_compact"), 300, 8, [901, 1003, 777, 1300, 950], 3, 25, 4,
                                                planted={0: 1.0, 299: 0.95}, query=src))
    out["c2k20"] = (j("c2k20.cobs_classic"), _classic(j("c2k20.cobs_classic"), 150, 1499, 2, 20, 5, planted={10: 1.0}, query=src))
    return out


def batch_queries(src, k, z=0):
    """the placement edges, reads of 50 - 110 characters (the multi-query scan) and queries of more than 255 terms (16-bit
    scores), with and without invalid characters"""
    qs = V.placement_queries(src, k, z)
    rng = np.random.default_rng(1000 + k + z)
    for i in range(8):
        ln = int(rng.integers(50, 111))
        o = int(rng.integers(0, len(src) - ln))
        q = src[o:o + ln]
        if i % 4 != 3:
            q = V.with_n(q, [int(x) for x in rng.integers(0, ln, size=1 + i % 3)])
        qs.append(q)
    long_q = src[200:200 + 400 + k]
    qs.append(V.with_n(long_q, [0, 77, 78, 300, len(long_q) - 1]))
    qs.append(long_q)
    return qs


def miss_vs_skip_query(src):
    return V.with_n(src[500:730], [60, 150])


def replay_queries(src):
    base = src[900:1030]
    return V.with_n(base, [10]), V.with_n(base, [40, 90])


def alignment_queries(src):
    """k = 31: the k-mer at offset a = 0 .. 3 (every alignment of the loader's first byte) with an N directly behind it"""
    return [V.with_n(src[1200:1300], [31 + a]) for a in range(4)]


@pytest.fixture(scope="module")
def data(gpu_lib, oracle, tmp_path_factory):
    return build_files(str(tmp_path_factory.mktemp("invalid")), oracle)


def _first_bad(fb, queries):
    for i, q in enumerate(queries):
        if not V.char_valid(fb, q).all():
            return i
    return None


def _check_results(s, files, queries, z, mode, thresholds=(0.0, 0.8, 1.0), limits=(0, 1, 10)):
    for t in thresholds:
        for lim in limits:
            want = [V.results(files, q, z, mode, t, lim) for q in queries]
            assert s.search_hits(queries, t, lim) == want, (mode, z, t, lim)
            offs, hits = s.search_arrays(queries, t, lim)
            rows = hits.tolist()
            assert [rows[int(offs[i]):int(offs[i + 1])] for i in range(len(queries))] == want
            offs, hits = s.search_view(queries, t, lim)
            rows = hits.tolist()
            assert [rows[int(offs[i]):int(offs[i + 1])] for i in range(len(queries))] == want
    for qi in (1, len(queries) - 2):          # the single-query call (captured into a graph the second time)
        for t in thresholds:
            want = V.results(files, queries[qi], z, mode, t, 10)
            for _ in range(2):
                one = s.search(queries[qi], t, 10)
                assert [(r.doc_name, r.score) for r in one] == [(s.doc_name(f, d), sc) for (f, d, sc) in want], (mode, t, qi)


def _check_batch(gpu_lib, s, files, queries, z, mode):
    b = gpu_lib.Batch(s)
    b.set_queries(queries)
    for t in (0.8, 1.0):
        b.run_hits(t)
        b.sync()
        for i, q in enumerate(queries):
            assert b.hits_host(i) == V.results(files, q, z, mode, t, 0), (mode, t, i)
    for keep in (True, False):
        for t in (0.0, 0.8):
            b.run_topk(t, 10, keep_counts=keep)
            b.sync()
            for i, q in enumerate(queries):
                assert b.hits_host(i, 10) == V.results(files, q, z, mode, t, 10), (mode, keep, t, i)
    for t in (0.0, 0.8):
        b.run(t)
        b.sync()
        for i, q in enumerate(queries):
            np.testing.assert_array_equal(b.counts_host(i), V.counts(files, q, z))
            assert b.hits_host(i) == V.results(files, q, z, mode, t, 0), (mode, t, i)
    for f, fb in enumerate(files):
        np.testing.assert_array_equal(b.scored_positions(f), [V.valid_positions(fb, q, z) for q in queries])
    b.close()


@_gpu
@pytest.mark.parametrize("name", ["c1", "c3", "p1", "p3", "c2k20"])
def test_modes_on_every_result_path(gpu_lib, data, name):
    from cobs_amd import _capi
    path, fb = data[name]
    queries = batch_queries(data["src"], fb.term_size)
    s = gpu_lib.Search(path)
    assert s.invalid_bases == "error"
    bad = _first_bad(fb, queries)
    assert bad is not None and bad > 0
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.search_arrays(queries, 0.0, 10)
    assert e.value.status == _capi.ERR_INVALID_BASE and "(query %d)" % bad in str(e.value)
    b = gpu_lib.Batch(s)
    b.set_queries(queries)
    b.run(0.0)
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        b.sync()
    assert e.value.status == _capi.ERR_INVALID_BASE and "(query %d)" % bad in str(e.value)
    b.close()
    for mode in V.MODES:
        s.invalid_bases = mode
        assert s.invalid_bases == mode
        for q in queries:
            np.testing.assert_array_equal(s.counts(q), V.counts([fb], q, 0))
        _check_results(s, [fb], queries, 0, mode)
        _check_batch(gpu_lib, s, [fb], queries, 0, mode)
    # back to the default: the call fails again, naming the same query
    s.invalid_bases = "error"
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.search_hits(queries, 0.8, 0)
    assert e.value.status == _capi.ERR_INVALID_BASE and "(query %d)" % bad in str(e.value)
    b = gpu_lib.Batch(s)
    b.set_queries(queries[:1])
    b.run(0.0)
    b.sync()
    np.testing.assert_array_equal(b.scored_positions(0), [fb.positions(queries[0], 0)])
    b.close()
    s.close()


@_gpu
def test_clean_batch_is_identical_in_all_modes(gpu_lib, data):
    path, fb = data["p1"]
    src = data["src"]
    queries = [src[o:o + ln] for o, ln in ((0, 31), (40, 77), (300, 110), (1000, 500), (5, 64))]
    got = {}
    for mode in ("error", "miss", "skip"):
        s = gpu_lib.Search(path, invalid_bases=mode)
        got[mode] = [s.search_hits(queries, t, lim) for t in (0.0, 0.8, 1.0) for lim in (0, 1, 10)]
        got[mode].append([s.counts(q).tolist() for q in queries])
        b = gpu_lib.Batch(s)
        b.set_queries(queries)
        b.run_hits(0.8)
        b.sync()
        got[mode].append([b.hits_host(i) for i in range(len(queries))])
        got[mode].append(b.scored_positions(0).tolist())
        b.close()
        s.close()
    assert got["error"] == got["miss"] == got["skip"]
    assert got["error"][0] == [F.results([fb], q, 0, 0.0, 0) for q in queries]
    assert got["error"][-1] == [fb.positions(q, 0) for q in queries]


@_gpu
def test_k31_loader_alignments_and_the_byte_behind_a_kmer(gpu_lib, data):
    path, fb = data["c1"]
    queries = alignment_queries(data["src"])
    # (a query's text starts at a multiple of 8 on the device: term a sits at alignment a of the loader)
    s = gpu_lib.Search(path, invalid_bases="skip")
    b = gpu_lib.Batch(s)
    b.set_queries(queries)
    b.run(0.0)
    b.sync()
    for a, q in enumerate(queries):
        np.testing.assert_array_equal(b.counts_host(a), V.counts([fb], q, 0))
        # the k-mer in front of the N counts, in the document that holds every k-mer of the text
        assert int(b.counts_host(a)[PLANTED_FULL]) == V.valid_positions(fb, q, 0) == len(q) - 30 - 31
    np.testing.assert_array_equal(b.scored_positions(0), [V.valid_positions(fb, q, 0) for q in queries])
    b.close()
    offs, hits, bit_offsets, bits = s.search_positions(queries, 0.8, 0)
    for a, q in enumerate(queries):
        for h in range(int(offs[a]), int(offs[a + 1])):
            f, d, sc = hits.tolist()[h]
            got = unpack_positions(bits[int(bit_offsets[h]):int(bit_offsets[h + 1])], len(q) - 30)
            np.testing.assert_array_equal(got, V.position_bits(fb, q, 0, d))
            assert not got[a + 1:a + 32].any() and (got[a] or d != PLANTED_FULL)
    s.close()


@_gpu
@pytest.mark.parametrize("name,z", [("c1", 1), ("p3", 3), ("c3", 3)])
def test_findere_validity_spans_k_plus_z(gpu_lib, data, name, z):
    path, fb = data[name]
    queries = batch_queries(data["src"], fb.term_size, z)
    s = gpu_lib.Search(path, findere=z)
    for mode in V.MODES:
        s.invalid_bases = mode
        for q in queries:
            np.testing.assert_array_equal(s.counts(q), V.counts([fb], q, z))
        _check_results(s, [fb], queries, z, mode, thresholds=(0.0, 0.8), limits=(0, 10))
        _check_batch(gpu_lib, s, [fb], queries, z, mode)
        # hit positions: an invalid position reads 0, the popcount is the score
        offs, hits, bit_offsets, bits = s.search_positions(queries, 0.8, 0)
        rows = hits.tolist()
        assert [rows[int(offs[i]):int(offs[i + 1])] for i in range(len(queries))] == [V.results([fb], q, z, mode, 0.8, 0) for q in queries]
        assert len(rows) > 0
        docs = fb.doc_of_slot()
        for i, q in enumerate(queries):
            for h in range(int(offs[i]), int(offs[i + 1])):
                f, d, sc = rows[h]
                words = bits[int(bit_offsets[h]):int(bit_offsets[h + 1])]
                got = unpack_positions(words, fb.positions(q, z))
                slot = int(np.nonzero(docs == d)[0][0])
                np.testing.assert_array_equal(got, V.position_bits(fb, q, z, slot))
                assert int(got.sum()) == sc and not got[~V.position_valid(fb, q, z)].any()
    s.close()


@_gpu
def test_miss_versus_skip(gpu_lib, data):
    path, fb = data["c1"]
    q = miss_vs_skip_query(data["src"])
    alln = b"N" * 230
    v = V.valid_positions(fb, q, 0)
    s = gpu_lib.Search(path, invalid_bases="miss")
    got = s.search_hits([q, alln], 0.8, 0)
    assert PLANTED_FULL not in [d for (_f, d, _s) in got[0]] and got[1] == []
    assert got == [V.results([fb], x, 0, "miss", 0.8, 0) for x in (q, alln)]
    s.invalid_bases = "skip"
    got = s.search_hits([q, alln], 0.8, 0)
    assert (0, PLANTED_FULL, v) in got[0] and got[1] == []
    assert got == [V.results([fb], x, 0, "skip", 0.8, 0) for x in (q, alln)]
    everything = s.search_hits([alln], 0.0, 0)[0]
    assert len(everything) == fb.num_docs and all(sc == 0 for (_f, _d, sc) in everything)
    for mode in V.MODES:                     # every limit and threshold, both as a batch of two and one by one
        s.invalid_bases = mode
        _check_results(s, [fb], [q, alln, q[:100], alln[:40]], 0, mode)
    s.close()


@_gpu
def test_graph_replay_gets_each_query_its_own_threshold(gpu_lib, data):
    path, fb = data["c1"]
    qa, qb = replay_queries(data["src"])
    s = gpu_lib.Search(path, invalid_bases="skip")
    want = {q: V.results([fb], q, 0, "skip", 0.8, 0) for q in (qa, qb)}
    replays = s.graph_replays
    for q in (qa, qb, qa, qb, qb, qa):
        got = s.search(q, 0.8)
        assert [(r.doc_name, r.score) for r in got] == [(s.doc_name(f, d), sc) for (f, d, sc) in want[q]]
    assert s.graph_replays > replays         # (the graph did replay: the check above is not vacuous)
    for lim in (1, 10):
        for q in (qa, qb, qa, qb):
            assert s.search_hits([q], 0.8, lim) == [V.results([fb], q, 0, "skip", 0.8, lim)]
    # the policy is part of the shape class: the same shape under miss and error
    s.invalid_bases = "miss"
    for q in (qa, qb, qa):
        assert s.search_hits([q], 0.8, 0) == [V.results([fb], q, 0, "miss", 0.8, 0)]
    s.invalid_bases = "error"
    for _ in range(3):
        with pytest.raises(gpu_lib.CobsGpuError):
            s.search(qa, 0.8)
    clean = data["src"][900:1030]
    assert s.search_hits([clean], 0.8, 0) == [F.results([fb], clean, 0, 0.8, 0)]
    s.close()


@_gpu
def test_counts_after_a_captured_search_names_the_invalid_query(gpu_lib, data):
    """the pair the call-sequence walk found (tests/test_gpu_call_sequence.py: search_small -> counts): a search captured
    into a graph leaves a run in the batch's timer ring whose events were recorded inside the capture; booking the timers
    of the next plain pass failed over them and replaced the message of cobs_gpu_counts' invalid base with a HIP error"""
    from cobs_amd import _capi
    path, fb = data["c1"]
    clean = data["src"][900:1030]
    s = gpu_lib.Search(path)
    replays = s.graph_replays
    for _ in range(3):                                  # candidate, capture, replay
        assert s.search_hits([clean], 0.8, 0) == [F.results([fb], clean, 0, 0.8, 0)]
    assert s.graph_replays > replays
    s.timers(reset=True)
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.counts(V.with_n(clean, [40]))
    assert e.value.status == _capi.ERR_INVALID_BASE and "Invalid DNA base pair" in str(e.value) and "(query 0)" in str(e.value)
    assert np.array_equal(s.counts(clean), F.counts([fb], clean, 0))        # the handle still answers
    # ... and the plain passes behind the captured one are booked (only they have a hashing time of their own)
    t = s.timers()
    assert t["hashes"] > 0 and t["scan"] > 0, t
    s.close()


@_gpu
def test_multi_file_handle(gpu_lib, data):
    names = ("c1", "p3", "c2k20")
    paths, files = [data[n][0] for n in names], [data[n][1] for n in names]
    queries = batch_queries(data["src"], 31)
    for mode in V.MODES:
        s = gpu_lib.Search(paths, invalid_bases=mode)
        _check_results(s, files, queries, 0, mode, limits=(0, 10))
        _check_batch(gpu_lib, s, files, queries, 0, mode)
        s.close()


@_gpu
@pytest.mark.parametrize("fetch", ["whole", "fetch"])
def test_budgeted_handle(gpu_lib, data, tmp_path, fetch):
    """a streamed file: chunks copied whole and chunks fetched row by row both read an invalid k-mer as the zero row"""
    ps, D = 96, 5 * 8 * 96 - 11
    src = data["src"]
    path = str(tmp_path / "st.cobs_compact")
    fb = _compact(path, D, ps, [700, 1500, 5000, 900, 2600], 2, 31, 6, planted={0: 1.0, D - 1: 0.95, 2500: 0.85}, query=src)
    queries = [V.with_n(src[:700], [5, 300, 301]), V.with_n(src[100:180], [40]), b"N" * 64, src[50:350], V.with_n(src[7:120], [0, 112])]
    s = gpu_lib.Search(path, hbm_budget=400 * 1024)
    if fetch == "fetch":
        s.set_tuning("row_fetch_alpha", 0)
    else:
        s.set_tuning("row_fetch", 0)
    for mode in V.MODES:
        s.invalid_bases = mode
        for q in queries[:3]:
            np.testing.assert_array_equal(s.counts(q), V.counts([fb], q, 0))
        for t, lim in ((0.0, 10), (0.8, 0), (0.8, 3), (1.0, 0)):
            assert s.search_hits(queries, t, lim) == [V.results([fb], q, 0, mode, t, lim) for q in queries], (mode, t, lim)
        b = gpu_lib.Batch(s)
        b.set_queries(queries)
        b.run_hits(0.8)
        b.sync()
        for i, q in enumerate(queries):
            assert b.hits_host(i) == V.results([fb], q, 0, mode, 0.8, 0)
        np.testing.assert_array_equal(b.scored_positions(0), [V.valid_positions(fb, q, 0) for q in queries])
        b.close()
    fetched, whole = s.stream_counters()
    assert (fetched > 0) if fetch == "fetch" else (fetched == 0 and whole > 0)
    s.close()


@_gpu
def test_sharded_one_rank(gpu_lib, data, comm_one_rank):
    paths, files = [data["c1"][0], data["p3"][0]], [data["c1"][1], data["p3"][1]]
    queries = batch_queries(data["src"], 31)
    for mode in V.MODES:
        s = gpu_lib.Search(paths, invalid_bases=mode)
        for t, lim in ((0.0, 0), (0.8, 0), (0.0, 10), (0.8, 1)):
            assert s.sharded_search_hits(comm_one_rank, queries, t, lim) == [V.results(files, q, 0, mode, t, lim) for q in queries]
        s.close()


_RANKS_SCRIPT = r"""
import os, sys, numpy as np
sys.path.insert(0, %(root)r)
import cobs_amd
paths = %(paths)r
queries = [bytes(q) for q in %(queries)r]
m = cobs_amd.MultiSearch(paths, [0] * %(ranks)d)
assert m.invalid_bases == "error"
try:
    m.search_hits(queries, 0.8, 0)
    raise SystemExit("the default policy answered a query with an N")
except cobs_amd.CobsGpuError as e:
    assert "Invalid DNA base pair" in str(e), e
for mode in ("miss", "skip"):
    single = cobs_amd.Search(paths, invalid_bases=mode)
    m.invalid_bases = mode
    assert m.invalid_bases == mode
    for r in range(%(ranks)d):
        assert m.shard(r).invalid_bases == mode
    for t, lim in ((0.0, 0), (0.8, 0), (0.0, 10), (1.0, 1), (0.8, 3)):
        assert m.search_hits(queries, t, lim) == single.search_hits(queries, t, lim), (mode, t, lim)
    single.close()
m2 = cobs_amd.MultiSearch(paths, [0] * %(ranks)d, invalid_bases="skip")
assert m2.invalid_bases == "skip"
m2.close()
m.close()
print("ok")
"""


@_gpu
def test_device_list_over_two_ranks_sharing_the_gpu(gpu_lib, data):
    r = subprocess.run(["bash", os.path.join(ROOT, "tests", "mock_rccl", "build.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    mock = os.path.join(ROOT, "cobs_amd", "libmockrccl.so")
    paths = [data["p1"][0], data["c3"][0]]
    queries = [list(q) for q in batch_queries(data["src"], 31)]
    code = _RANKS_SCRIPT % {"root": ROOT, "paths": paths, "queries": queries, "ranks": 2}
    pre = ":".join([mock] + [p for p in os.environ.get("LD_PRELOAD", "").split(":") if p])
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=dict(os.environ, LD_PRELOAD=pre))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-6000:]
    assert "[mock rccl]" not in r.stderr, r.stderr[-6000:]
    # ... whose single-device side is the checker's
    fbs = [data["p1"][1], data["c3"][1]]
    s = gpu_lib.Search(paths, invalid_bases="skip")
    qs = batch_queries(data["src"], 31)
    assert s.search_hits(qs, 0.8, 3) == [V.results(fbs, q, 0, "skip", 0.8, 3) for q in qs]
    s.close()


@_gpu
def test_cli(gpu_lib, data, tmp_path):
    path, fb = data["c1"]
    tool = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")
    queries = batch_queries(data["src"], 31)[:14] + [miss_vs_skip_query(data["src"])]
    qf = tmp_path / "q.fa"
    qf.write_text("".join(">q%d\n%s\n" % (i, q.decode()) for i, q in enumerate(queries)))
    r = subprocess.run([tool, "-i", path, "-f", str(qf), "-t", "0.8"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "Invalid DNA base pair" in r.stderr
    for mode, extra in (("skip", ["-t", "0.8"]), ("miss", ["-t", "0.8"]), ("skip", ["-t", "0", "-l", "10"])):
        r = subprocess.run([tool, "-i", path, "--invalid-bases", mode, "-f", str(qf)] + extra, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        t = float(extra[1])
        lim = int(extra[3]) if len(extra) > 2 else 0
        want = []
        for i, q in enumerate(queries):
            res = V.results([fb], q, 0, mode, t, lim)
            want.append("*q%d\t%d" % (i, len(res)))
            want += ["doc_%05d\t%d" % (d, sc) for (_f, d, sc) in res]
        assert r.stdout.strip().splitlines() == want, mode
    r = subprocess.run([tool, "benchmark-fpr", path, "-k", "100", "-q", "20", "-w", "2", "--seed", "5", "--invalid-bases", "skip"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("RESULT name=benchmark"), r.stderr
