"""CPU: the grouped-search checker (tests/groups_check.py) anchored on the oracle, and what the new entry points and
their mirrors promise without a device.

At z = 0 and all-ACGT queries a group's sum is the sum of the oracle's search scores of its queries and its votes are
the number of the oracle's hits at read_threshold: the checker adds nothing of its own but the grouping."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import cases
from tests import findere_check as F
from tests import groups_check as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("groups_cpu")
    src = oracle.random_sequence(1500, 77)
    a = cases.make_classic(str(d / "a.cobs_classic"), 120, 1009, 3, 31, 1, 0.3, 5, planted={0: 1.0, 77: 0.9}, query=src)
    b = cases.make_classic(str(d / "b.cobs_classic"), 90, 1201, 1, 25, 1, 0.3, 6, planted={3: 1.0, 89: 0.85}, query=src)
    return src, [a, b], [F.classic_file(a), F.classic_file(b)]


def _reads(src, n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ln = int(rng.integers(lo, hi + 1))
        o = int(rng.integers(0, len(src) - ln))
        out.append(src[o:o + ln])
    return out


def test_sums_and_votes_are_the_oracle_scores_and_hits_grouped(files, oracle):
    src, paths, fbs = files
    ixs = [oracle.Index.open(p) for p in paths]
    queries = _reads(src, 9, 40, 140, 3) + [oracle.random_sequence(80, 9)]
    offsets = [0, 0, 1, 3, 10, 10]
    for rt in (0.0, 0.8):
        sums, votes, P = G.totals(fbs, queries, offsets, 0, "error", rt)
        for g in range(len(offsets) - 1):
            want_sum = [np.zeros(fb.slots, dtype=np.uint64) for fb in fbs]
            want_votes = [np.zeros(fb.slots, dtype=np.uint64) for fb in fbs]
            want_p = [0, 0]
            for q in queries[offsets[g]:offsets[g + 1]]:
                for f, d, _name, sc in oracle.search(ixs, q, 0.0, 0):
                    want_sum[f][d] += sc
                for f, d, _name, sc in oracle.search(ixs, q, rt, 0):
                    want_votes[f][d] += 1
                for f, fb in enumerate(fbs):
                    want_p[f] += len(q) - fb.term_size + 1
            for f, fb in enumerate(fbs):
                real = fb.doc_of_slot() >= 0
                np.testing.assert_array_equal(sums[f][g][real], want_sum[f][:fb.num_docs])
                np.testing.assert_array_equal(votes[f][g][real], want_votes[f][:fb.num_docs])
                assert int(P[g, f]) == want_p[f]
    # a group of one query at threshold == read_threshold is that query's search (total hash count > 1)
    for t in (0.0, 0.8, 1.0):
        res, _P = G.results(fbs, queries, list(range(len(queries) + 1)), 0, "error", t, t, 0)
        for q, r in zip(queries, res):
            assert [(f, d, s) for (f, d, s, _v) in r] == [(f, d, s) for (f, d, _n, s) in oracle.search(ixs, q, t, 0)]
            assert all(v == 1 for (_f, _d, _s, v) in r)


def test_thresholds_order_and_limits_of_the_checker(files):
    src, _paths, fbs = files
    queries = _reads(src, 6, 60, 120, 5)
    offsets = [0, 0, 6]
    res, P = G.results(fbs, queries, offsets, 0, "error", 0.0, 0.0, 0)
    assert res[0] and all(s == 0 and v == 0 for (_f, _d, s, v) in res[0])          # an empty group: every real document, nothing
    assert len(res[1]) == 120 + 90 and all(v == 6 for (_f, _d, _s, v) in res[1])   # read_threshold <= 0: |g| votes
    assert res[1] == sorted(res[1], key=lambda h: (-h[2], h[0], h[1]))
    assert P[0].tolist() == [0, 0]
    assert G.results(fbs, queries, offsets, 0, "error", 0.5, 0.0, 0)[0][0] == []   # P = 0 returns nothing at threshold > 0
    top = G.results(fbs, queries, offsets, 0, "error", 0.0, 0.8, 3)[0][1]
    assert top == res_votes(fbs, queries, offsets)[:3]
    full = G.results(fbs, queries, offsets, 0, "error", 1.0, 0.8, 0)[0][1]
    assert {(f, d) for (f, d, _s, _v) in full} == {(0, 0), (1, 3)}                 # the fully planted documents
    assert G.group_threshold(0.8, 0) == 1 and G.group_threshold(0.0, 10) == 0 and G.group_threshold(0.25, 10) == 3


def res_votes(fbs, queries, offsets):
    return G.results(fbs, queries, offsets, 0, "error", 0.0, 0.8, 0)[0][1]


def test_symbols_are_exported_bound_and_refuse_null():
    from cobs_amd import _capi
    lib = _capi.load()
    batch_h = open(os.path.join(ROOT, "include", "cobs_gpu_batch.h")).read()
    diag_h = open(os.path.join(ROOT, "include", "cobs_gpu_diag.h")).read()
    base_h = open(os.path.join(ROOT, "include", "cobs_gpu.h")).read()
    assert "cobs_gpu_search_groups(" in batch_h and "cobs_gpu_groups_ms(" in diag_h
    assert "cobs_gpu_search_groups" not in base_h and "cobs_gpu_groups_ms" not in base_h
    for name in ("cobs_gpu_search_groups", "cobs_gpu_groups_ms"):
        assert hasattr(lib, name) and name in _capi.SYMBOLS
    assert C.sizeof(_capi.GroupHit) == 16
    goffs = (C.c_size_t * 2)(0, 0)
    hoffs = (C.c_size_t * 2)(7, 7)
    bad = C.c_size_t(0)
    # no handle (one cannot be opened without a device): an argument error, not a crash
    st = lib.cobs_gpu_search_groups(None, None, None, 0, goffs, 1, 0.0, 0.0, 0, None, 0, hoffs, None, C.byref(bad))
    assert st == _capi.ERR_ARG and b"NULL" in lib.cobs_gpu_last_error()
    assert lib.cobs_gpu_search_groups(None, None, None, 0, None, 0, 0.0, 0.0, 0, None, 0, None, None, None) == _capi.ERR_ARG
    ms = (C.c_double * 3)()
    assert lib.cobs_gpu_groups_ms(None, C.byref(ms)) == _capi.ERR_ARG


def test_python_mirrors_exist_and_nothing_runs_without_a_device(golden_dir):
    import torch

    import cobs_amd
    import cobs_index
    from cobs_amd import _capi
    sig = inspect.signature(cobs_amd.Search.search_groups)
    assert list(sig.parameters) == ["self", "queries", "group_offsets", "threshold", "read_threshold", "num_results",
                                    "return_positions"]
    assert [sig.parameters[n].default for n in ("threshold", "read_threshold", "num_results", "return_positions")] == \
           [0.0, 0.0, 0, False]
    assert list(inspect.signature(cobs_amd.Search.search_paired).parameters)[:3] == ["self", "reads1", "reads2"]
    r = cobs_amd.GroupResult("d", 3, 2)
    assert (r.doc_name, r.score, r.votes) == ("d", 3, 2) and r == cobs_index.GroupResult("d", 3, 2)
    assert cobs_index.Search.search_groups is cobs_amd.Search.search_groups
    assert list(inspect.signature(cobs_amd.Search.search).parameters) == ["self", "query", "threshold", "num_results"]
    s = cobs_amd.Search(None, _handle=C.c_void_p())           # no handle: the library refuses
    with pytest.raises(cobs_amd.CobsGpuError) as e:
        s.search_groups_arrays([b"ACGT" * 10], [0, 1])
    assert e.value.status == _capi.ERR_ARG
    with pytest.raises(ValueError):
        s.search_paired([b"ACGT" * 10], [])
    if not torch.cuda.is_available():
        with pytest.raises(cobs_amd.CobsGpuError) as e:
            cobs_amd.Search(os.path.join(golden_dir, "c1.cobs_classic")).search_groups([b"A" * 40], [0, 1])
        assert e.value.status == _capi.ERR_NO_DEVICE


def test_cli_names_the_flags():
    tool = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")
    r = subprocess.run([tool, "-h"], capture_output=True, text=True, timeout=60)
    assert "--group" in r.stderr and "--read-threshold" in r.stderr
    r = subprocess.run([tool, "-i", "x.cobs_classic", "--group", "0", "-f", "q.fa"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--group" in r.stderr
