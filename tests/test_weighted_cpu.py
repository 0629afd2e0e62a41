"""CPU: cobs_gpu_idf_weight through the loaded library against the checker's restatement, the weighted checker
(tests/weighted_check.py) anchored on the oracle with all weights forced to 1, its identity against the prevalence checker,
and what the new entry points and their mirrors promise without a device."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import cases
from tests import findere_check as F
from tests import prevalence_check as V
from tests import weighted_check as W
from tests.test_positions_cpu import _read_compact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS = (1, 2, 3, 7, 8, 16383, 16384, 16385, 2 ** 32 - 1)


def _counts_for(D):
    cs = {0, 1, 2, D // 2, D // 2 + 1, D - 1, D}
    for j in range(0, 40):                       # every power-of-two boundary c * 2^j = D, and D +- 1
        for d in (D - 1, D, D + 1):
            if d % (1 << j) == 0:
                cs.add(d >> j)
            cs.add((d >> j) + 1)
            cs.add(d >> j)
    return sorted(c for c in cs if 0 <= c <= D)


def test_idf_weight_of_the_library_is_the_definition():
    from cobs_amd import _capi
    lib = _capi.load()
    assert "cobs_gpu_idf_weight" in _capi.SYMBOLS
    seen = set()
    for D in DS:
        last = None
        for c in _counts_for(D):
            got = lib.cobs_gpu_idf_weight(D, c)
            assert got == W.idf_weight(D, c), (D, c, got)
            assert 0 <= got <= 15 and (got == 0) == (c == 0)
            if c:
                # the definition, once more: the largest j <= 14 with c * 2^j <= D
                j = got - 1
                assert c * 2 ** j <= D and (j == 14 or c * 2 ** (j + 1) > D), (D, c)
                assert last is None or got <= last, (D, c)          # non-increasing in c
                last = got
            seen.add(got)
    assert seen == set(range(16))
    assert lib.cobs_gpu_idf_weight(16384, 1) == 15 and lib.cobs_gpu_idf_weight(16383, 1) == 14
    assert lib.cobs_gpu_idf_weight(100, 51) == 1 and lib.cobs_gpu_idf_weight(100, 50) == 2
    # dense sweep of small collections
    for D in range(1, 70):
        ws = [lib.cobs_gpu_idf_weight(D, c) for c in range(D + 1)]
        assert ws == [W.idf_weight(D, c) for c in range(D + 1)]
        assert all(a >= b for a, b in zip(ws[1:], ws[2:]))


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("weighted_cpu")
    src = oracle.random_sequence(600, 77)
    a = cases.make_classic(str(d / "a.cobs_classic"), 120, 1009, 3, 31, 1, 0.3, 5, planted={0: 1.0, 77: 0.9}, query=src)
    b = cases.make_compact(str(d / "b.cobs_compact"), 200, 8, [701, 1009, 853, 977], 1, 25, 1, 0.3, 6,
                           planted={3: 1.0, 199: 0.85}, query=src)
    return src, [a, b], [F.classic_file(a), _read_compact(b)]


def test_all_ones_weights_give_the_oracle(files, oracle):
    """weights forced to 1: the checker's scores are the oracle's counts and its results the oracle's, z = 0"""
    src, paths, fbs = files
    for path, fb in zip(paths, fbs):
        ix = oracle.Index.open(path)
        for q in (src[:100], src[200:560], oracle.random_sequence(80, 5)):
            ones = np.ones(fb.positions(q, 0), dtype=np.uint8)
            np.testing.assert_array_equal(W.scores(fb, q, 0, weights=ones), np.asarray(ix.counts(q)).astype(np.uint64))
            for t in (0.0, 0.3, 0.8, 1.0):
                for nr in (0, 1, 5):
                    assert W.results([fb], q, 0, t, nr, weights=[ones]) == cases.oracle_results([ix], q, t, nr), (path, t, nr)


def test_scores_add_up_to_weight_times_count(files):
    src, paths, fbs = files
    reached = set()
    for z in (0, 1, 3, 7):
        for q in (src[:31 + 7], src[10:10 + 95], src[:500]):
            for fb in fbs:
                w = W.weights(fb, q, z)
                c = V.prevalence(fb, q, z)
                real = fb.doc_of_slot() >= 0
                assert w.dtype == np.uint8 and len(w) == fb.positions(q, z) and ((w == 0) == (c == 0)).all()
                sc = W.scores(fb, q, z)
                assert int(sc[real].sum()) == int((w.astype(np.uint64) * c).sum())
                assert W.total_weights([fb], q, z) == [int(w.sum())]
                reached |= set(w.tolist())
    assert len(reached) >= 4             # (the planted documents and the random bits give different weights)


def test_thresholds():
    assert W.thresholds(0.0, 100) == 0 and W.thresholds(-1.0, 100) == 0
    assert W.thresholds(0.8, 0) == 1 and W.thresholds(1e-9, 5) == 1
    assert W.thresholds(0.8, 10) == 8 and W.thresholds(0.3, 11) == 4 and W.thresholds(1.0, 15000) == 15000


def test_miss_and_skip_are_the_same(files):
    from tests import invalid_check as I
    src, paths, fbs = files
    q = I.with_n(src[50:250], [100])
    for z in (0, 3):
        a = W.results(fbs[:1], q, z, 0.3, 0, "miss")
        assert a == W.results(fbs[:1], q, z, 0.3, 0, "skip")
        assert W.total_weights(fbs[:1], q, z, "miss") == W.total_weights(fbs[:1], q, z, "skip")
        bad = ~I.position_valid(fbs[0], q, z)
        assert bad.any() and not W.weights(fbs[0], q, z, "miss")[bad].any()


def test_symbols_are_exported_bound_and_refuse_null():
    from cobs_amd import _capi
    lib = _capi.load()
    for name, header in (("cobs_gpu_idf_weight", "cobs_gpu_batch.h"), ("cobs_gpu_search_weighted", "cobs_gpu_batch.h"),
                         ("cobs_gpu_weighted_ms", "cobs_gpu_diag.h")):
        assert hasattr(lib, name) and name in _capi.SYMBOLS
        assert name + "(" in open(os.path.join(ROOT, "include", header)).read()
        assert name not in open(os.path.join(ROOT, "include", "cobs_gpu.h")).read()
    text = open(os.path.join(ROOT, "include", "cobs_gpu_batch.h")).read()
    assert "SAME result" in text                 # miss and skip: the header says so
    offs = (C.c_size_t * 1)(7)
    bad = C.c_size_t(0)
    # no handle: an argument error, not a crash (a handle cannot be opened without a device)
    st = lib.cobs_gpu_search_weighted(None, None, None, 0, 0.5, 0, None, 0, offs, None, C.byref(bad))
    assert st == _capi.ERR_ARG and b"NULL" in lib.cobs_gpu_last_error()
    ms = (C.c_double * 5)()
    assert lib.cobs_gpu_weighted_ms(None, C.byref(ms)) == _capi.ERR_ARG


def test_python_mirrors_exist_with_their_parameter_names():
    import cobs_amd
    import cobs_index
    from cobs_amd import _capi
    S = cobs_amd.Search
    assert list(inspect.signature(S.search_weighted).parameters) == ["self", "query", "threshold", "num_results"]
    assert list(inspect.signature(S.search_weighted_arrays).parameters) == ["self", "queries", "threshold", "num_results"]
    assert list(inspect.signature(S.position_weights).parameters) == ["self", "query"]
    assert list(inspect.signature(S.search).parameters) == ["self", "query", "threshold", "num_results"]
    assert cobs_index.Search.search_weighted is S.search_weighted
    r = cobs_amd.WeightedResult("d", 7, 30)
    assert (r.doc_name, r.score, r.total_weight) == ("d", 7, 30) and isinstance(r, cobs_amd.SearchResult)
    with pytest.raises(cobs_amd.CobsGpuError) as e:           # the device list is refused by the mirror
        cobs_amd.MultiSearch.search_weighted_arrays(cobs_amd.MultiSearch.__new__(cobs_amd.MultiSearch), [b"ACGT" * 10])
    assert e.value.status == _capi.ERR_UNSUPPORTED and "device-list" in str(e.value)


def test_cli_names_the_flag_and_its_refusals():
    tool = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")
    r = subprocess.run([tool, "-h"], capture_output=True, text=True, timeout=60)
    assert "--weighted" in r.stderr
    for extra in (["-d", "0,1"], ["--hbm-budget", "1"], ["--sharded"], ["--prevalence"]):
        r = subprocess.run([tool, "-i", "nowhere.cobs_classic"] + extra + ["--weighted", "ACGT" * 10], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 1 and "--weighted: not with" in r.stderr and r.stdout == ""
