"""CPU: cobs_gpu_covered_bases through the loaded library against the checker (tests/coverage_check.py), the checker's two
restatements against each other, the checker anchored on the oracle at z = 0 (its set-position counts are the oracle's
scores; the coverage obeys the bounds of the definition), and what the new entry points and their mirrors promise
without a device."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import cases
from tests import coverage_check as G
from tests import findere_check as F
from tests import invalid_check as I
from tests import positions_check as P
from tests import prevalence_check as V
from tests.test_positions_cpu import _read_compact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 2, 63, 64, 65, 128, 129, 1500)
SPANS = (1, 3, 31, 32, 38, 64, 255)


def _lib_covered(lib, words, n, span):
    w = np.ascontiguousarray(words, dtype=np.uint64)
    return int(lib.cobs_gpu_covered_bases(C.cast(w.ctypes.data, C.POINTER(C.c_uint64)), n, span))


def test_covered_bases_of_the_library_is_the_definition():
    from cobs_amd import _capi
    import cobs_amd
    lib = _capi.load()
    assert "cobs_gpu_covered_bases" in _capi.SYMBOLS
    rng = np.random.default_rng(3)
    seen_partial = 0
    for n in NS:
        for span in SPANS:
            for dens in (0.0, 0.01, 0.05, 0.3, 0.9, 1.0):
                bits = rng.random(n) < dens
                if dens == 0.01 and n > 2:
                    bits[:] = False
                    bits[[0, n - 1]] = True                      # the two ends alone
                want = G.covered_bases(bits, span)
                words = P.pack(bits).astype(np.uint64)
                assert len(words) == (n + 63) // 64
                assert _lib_covered(lib, words, n, span) == want, (n, span, dens)
                # garbage at or beyond n in the last word is ignored
                dirty = words.copy()
                if n % 64:
                    dirty[-1] |= np.uint64(((1 << 64) - 1) ^ ((1 << (n % 64)) - 1))
                    assert int(dirty[-1]) != int(words[-1])
                assert _lib_covered(lib, dirty, n, span) == want, (n, span, dens)
                assert cobs_amd.covered_bases(dirty, n, span) == want
                s = int(bits.sum())
                if s:
                    assert s + span - 1 <= want <= min(n + span - 1, s * span)
                    seen_partial += int(want < n + span - 1)
                else:
                    assert want == 0
    assert seen_partial > 50
    # by hand: positions 0 and 5 of 10, span 3 -> bases 0..2 and 5..7; positions 0 and 2 -> bases 0..4
    assert _lib_covered(lib, [0b100001], 10, 3) == 6 and _lib_covered(lib, [0b101], 10, 3) == 5
    assert _lib_covered(lib, [0b1000000000], 10, 3) == 3          # the last position: the tail bases n .. n + span - 2
    assert lib.cobs_gpu_covered_bases(None, 10, 3) == 0 and _lib_covered(lib, [1], 0, 3) == 0
    with pytest.raises(ValueError):
        cobs_amd.covered_bases([1], 65, 3)


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("coverage_cpu")
    src = oracle.random_sequence(600, 77)
    b = cases.make_compact(str(d / "b.cobs_compact"), 200, 8, [701, 1009, 853, 977], 1, 25, 1, 0.3, 6,
                           planted={3: 1.0, 199: 0.85}, query=src)
    return src, b, _read_compact(b)


def _anchor(oracle, path, fb, queries, full=None):
    ix = oracle.Index.open(path)
    docs = fb.doc_of_slot()
    for q in queries:
        (length, cov, _docs, s), = G.tables([fb], q, 0)
        score = np.asarray(ix.counts(q)).astype(np.uint64)
        np.testing.assert_array_equal(s, score)                  # the checker's set positions are the oracle's score
        span = G.span_of(fb, 0)
        assert length == len(q) == fb.positions(q, 0) + span - 1
        for slot in range(fb.slots):
            si, ci = int(s[slot]), int(cov[slot])
            if si:
                assert si + span - 1 <= ci <= min(length, si * span), (path, slot)
            else:
                assert ci == 0
        if full is not None and q is queries[0]:
            slot = int(np.nonzero(docs == full)[0][0])
            assert int(s[slot]) == fb.positions(q, 0) and int(cov[slot]) == len(q)
        np.testing.assert_array_equal(G.coverage(fb, q, 0), cov)
    return ix


def test_anchored_on_the_oracle_on_the_golden_files(golden_dir, oracle):
    q = b"AGTCAACGCTAAGGCATTTCCCCCCTGCCTCCTGCCTGCTGCCAAGCCCT"
    for name, fb in (("c1.cobs_classic", F.classic_file(os.path.join(golden_dir, "c1.cobs_classic"))),
                     ("c1.cobs_compact", _read_compact(os.path.join(golden_dir, "c1.cobs_compact")))):
        _anchor(oracle, os.path.join(golden_dir, name), fb, [q, oracle.random_sequence(90, 3)])


def test_anchored_on_the_oracle_on_a_compact_fixture(files, oracle):
    src, path, fb = files
    _anchor(oracle, path, fb, [src[:100], src[200:560], oracle.random_sequence(80, 5)], full=3)
    # the results at z = 0 with every position set are the oracle's hits with coverage L: document 3 leads
    res = G.results([fb], src[:100], 0, 0.8, 0)
    assert res[0] == (0, 3, 100)


def test_the_two_restatements_agree(files):
    src, path, fb = files
    partial = 0
    for z in (0, 1, 3, 7):
        for q in (src[:25 + z], src[:25 + z + 1], src[10:10 + 95], src[300:460]):
            for mode in ("error", "miss"):
                qq = q if mode == "error" or len(q) < 60 else I.with_n(q, [len(q) // 2])
                a, b = G.coverage(fb, qq, z, mode), G.coverage_by_bases(fb, qq, z, mode)
                np.testing.assert_array_equal(a, b)
                partial += int(((a > 0) & (a < len(qq))).sum())
                # every slot: covered_bases of its positions vector
                win = V.windows(fb, qq, z, mode)
                for slot in (0, 3, 199, 255):
                    assert G.covered_bases(win[:, slot], fb.term_size + z) == int(a[slot])
    assert partial > 100


def test_thresholds():
    assert G.thresholds(0.0, 100) == 0 and G.thresholds(-1.0, 100) == 0
    assert G.thresholds(1e-9, 5) == 1 and G.thresholds(0.8, 100) == 80 and G.thresholds(0.3, 11) == 4
    assert G.thresholds(1.0, 1 << 19) == 1 << 19


def test_miss_and_skip_are_the_same_and_an_n_is_never_covered(files):
    src, path, fb = files
    q = I.with_n(src[50:250], [100])
    for z in (0, 3):
        assert G.results([fb], q, z, 0.3, 0, "miss") == G.results([fb], q, z, 0.3, 0, "skip")
        cov = G.covered(fb, q, z, "miss")
        assert not cov[100].any() and cov[99, 3] and cov[101, 3]          # the planted document: all but that base
        assert int(G.coverage(fb, q, z, "miss")[3]) == len(q) - 1


def test_symbols_are_exported_bound_and_refuse_null():
    from cobs_amd import _capi
    lib = _capi.load()
    for name, header in (("cobs_gpu_covered_bases", "cobs_gpu_batch.h"), ("cobs_gpu_search_coverage", "cobs_gpu_batch.h"),
                         ("cobs_gpu_coverage_ms", "cobs_gpu_diag.h")):
        assert hasattr(lib, name) and name in _capi.SYMBOLS
        assert name + "(" in open(os.path.join(ROOT, "include", header)).read()
        assert name not in open(os.path.join(ROOT, "include", "cobs_gpu.h")).read()
    text = open(os.path.join(ROOT, "include", "cobs_gpu_batch.h")).read()
    assert "s + span - 1 <= coverage <= min(L, s * span)" in text
    assert "the two policies give the SAME result here" in text      # miss and skip: the header says so
    offs = (C.c_size_t * 1)(7)
    bad = C.c_size_t(0)
    # no handle: an argument error, not a crash (a handle cannot be opened without a device)
    st = lib.cobs_gpu_search_coverage(None, None, None, 0, 0.5, 0, None, 0, offs, C.byref(bad))
    assert st == _capi.ERR_ARG and b"NULL" in lib.cobs_gpu_last_error()
    ms = (C.c_double * 3)()
    assert lib.cobs_gpu_coverage_ms(None, C.byref(ms)) == _capi.ERR_ARG


def test_no_handle_without_a_device(golden_dir):
    """(on a host with a GPU the handle opens; tests/test_gpu_coverage.py takes over there)"""
    import torch
    import cobs_amd
    from cobs_amd import _capi
    if not torch.cuda.is_available():
        with pytest.raises(cobs_amd.CobsGpuError) as e:
            cobs_amd.Search(os.path.join(golden_dir, "c1.cobs_classic")).search_coverage("ACGT" * 20, 0.8)
        assert e.value.status == _capi.ERR_NO_DEVICE


def test_python_mirrors_exist_with_their_parameter_names():
    import cobs_amd
    import cobs_index
    from cobs_amd import _capi
    S = cobs_amd.Search
    assert list(inspect.signature(S.search_coverage).parameters) == ["self", "query", "threshold", "num_results"]
    assert list(inspect.signature(S.search_coverage_arrays).parameters) == ["self", "queries", "threshold", "num_results"]
    assert list(inspect.signature(S.coverage_ms).parameters) == ["self"]
    assert list(inspect.signature(cobs_amd.covered_bases).parameters) == ["words", "n", "span"]
    assert list(inspect.signature(S.search).parameters) == ["self", "query", "threshold", "num_results"]
    assert cobs_index.Search.search_coverage is S.search_coverage and "covered_bases" in cobs_amd.__all__
    with pytest.raises(cobs_amd.CobsGpuError) as e:           # the device list is refused by the mirror
        cobs_amd.MultiSearch.search_coverage_arrays(cobs_amd.MultiSearch.__new__(cobs_amd.MultiSearch), [b"ACGT" * 10])
    assert e.value.status == _capi.ERR_UNSUPPORTED and "device-list" in str(e.value)
    text = open(os.path.join(ROOT, "include", "cobs_gpu_search.hpp")).read()
    assert "void search_coverage(" in text and "inline uint64_t covered_bases(" in text


def test_cli_names_the_flag_and_its_refusals():
    tool = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")
    r = subprocess.run([tool, "-h"], capture_output=True, text=True, timeout=60)
    assert "--coverage" in r.stderr
    for extra in (["-d", "0,1"], ["--hbm-budget", "1"], ["--sharded"], ["--prevalence"], ["--weighted"], ["--group", "2"],
                  ["--sets", "nowhere.tsv"]):
        r = subprocess.run([tool, "-i", "nowhere.cobs_classic"] + extra + ["--coverage", "ACGT" * 10], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 1 and "--coverage: not with" in r.stderr and r.stdout == "", (extra, r.stderr)
