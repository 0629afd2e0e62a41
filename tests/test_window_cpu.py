"""CPU: cobs_gpu_best_window through the loaded library against the checker (tests/window_check.py), the checker's two
restatements against each other, the checker anchored on the oracle (with W >= n at z = 0 its best window is the oracle's
score), the identities of the definition on random bitmaps, the conditions of the GPU structure fixture on the checker
alone, and what the new entry points and their mirrors promise without a device."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import findere_check as F
from tests import positions_check as P
from tests import prevalence_check as V
from tests import window_check as B
from tests.test_gpu_window import structure
from tests.test_positions_cpu import _read_compact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 63, 64, 65, 1000)


def _windows_for(n):
    return tuple(sorted({1, 2, 63, 64, 65, n - 1, n, n + 1, 4095} - {0}))


def _lib_best(lib, words, n, W):
    w = np.ascontiguousarray(words, dtype=np.uint64)
    start = C.c_size_t(777)
    best = int(lib.cobs_gpu_best_window(C.cast(w.ctypes.data, C.POINTER(C.c_uint64)), n, W, C.byref(start)))
    assert int(lib.cobs_gpu_best_window(C.cast(w.ctypes.data, C.POINTER(C.c_uint64)), n, W, None)) == best   # start may be NULL
    return best, int(start.value)


def test_best_window_of_the_library_is_the_definition():
    from cobs_amd import _capi
    import cobs_amd
    lib = _capi.load()
    assert "cobs_gpu_best_window" in _capi.SYMBOLS
    rng = np.random.default_rng(5)
    partial = 0
    for n in NS:
        for W in _windows_for(n):
            for dens in (0.0, 0.02, 0.1, 0.3, 0.6, 0.9, 1.0):
                bits = rng.random(n) < dens
                want = B.best_window(bits, W)
                w = min(W, n)
                if dens == 1.0:
                    assert want == (w, 0)                                # all ones: a full window, the first start
                if dens == 0.0:
                    assert want == (0, 0)
                words = P.pack(bits).astype(np.uint64)
                assert len(words) == (n + 63) // 64
                assert _lib_best(lib, words, n, W) == want, (n, W, dens)
                # garbage at or beyond n in the last word is ignored
                dirty = words.copy()
                if n % 64:
                    dirty[-1] |= np.uint64(((1 << 64) - 1) ^ ((1 << (n % 64)) - 1))
                    assert int(dirty[-1]) != int(words[-1])
                assert _lib_best(lib, dirty, n, W) == want, (n, W, dens)
                assert cobs_amd.best_window(dirty, n, W) == want and cobs_amd.best_window(bits, n, W) == want
                partial += int(0 < want[0] < min(w, int(bits.sum())))
    assert partial > 20
    # a tie: two equal windows, the first start wins; by hand
    assert _lib_best(lib, [0b0110000110], 10, 2) == (2, 1)
    assert _lib_best(lib, [0b1000010000], 10, 3) == (1, 2)
    assert _lib_best(lib, [0b1110000111], 10, 4) == (3, 0) and _lib_best(lib, [0b1110000110], 10, 4) == (3, 6)
    assert _lib_best(lib, [0b1110000111], 10, 10) == (6, 0) and _lib_best(lib, [0b1110000111], 10, 4000) == (6, 0)
    # n = 0 and NULL words give 0
    start = C.c_size_t(9)
    assert lib.cobs_gpu_best_window(None, 10, 3, C.byref(start)) == 0 and start.value == 0
    assert _lib_best(lib, [1], 0, 3) == (0, 0)
    with pytest.raises(ValueError):
        cobs_amd.best_window([1], 65, 3)


def test_the_two_restatements_agree():
    rng = np.random.default_rng(9)
    partial = 0
    for n in (1, 2, 7, 8, 9, 40, 70):
        for dens in (0.1, 0.5, 0.9):
            win = rng.random((n, 12)) < dens
            win[:, 0] = False
            win[:, 1] = True
            for W in sorted({1, 2, 7, 8, 9, n - 1, n, n + 1, 4095} - {0}):
                a, b = B.best(win, W), B.best_by_slots(win, W)
                np.testing.assert_array_equal(a, b)
                w = min(W, n)
                assert a[0] == 0 and a[1] == w
                for slot in range(12):
                    assert B.best_window(win[:, slot], W)[0] == int(a[slot])
                    s0 = B.best_window(win[:, slot], W)[1]
                    assert int(win[s0:s0 + w, slot].sum()) == int(a[slot])
                    assert all(int(win[s:s + w, slot].sum()) < int(a[slot]) for s in range(s0))      # the first start
                partial += int(((a > 0) & (a < np.minimum(w, win.sum(axis=0)))).sum())
    assert partial > 100


def test_identities_on_random_bitmaps():
    rng = np.random.default_rng(13)
    for n in (1, 5, 64, 200, 1000):
        win = rng.random((n, 40)) < rng.random(40)[None, :]
        score = win.sum(axis=0)
        prev = np.zeros(40, dtype=np.int64)
        for W in (1, 2, 3, 7, 8, 50, 63, 64, 65, 199, 200, 201, 999, 1000, 1001, 4095):
            b = B.best(win, W)
            assert (b >= prev).all()                                         # non-decreasing in W
            assert (b <= np.minimum(min(W, n), score)).all()
            if W >= n:
                np.testing.assert_array_equal(b, score)                      # the plain search's score
            if W == 1:
                np.testing.assert_array_equal(b, (score > 0).astype(np.int64))
            prev = b


def test_thresholds():
    assert B.thresholds(0.0, 100) == 0 and B.thresholds(-1.0, 100) == 0
    assert B.thresholds(1e-9, 5) == 1 and B.thresholds(0.8, 100) == 80 and B.thresholds(0.3, 11) == 4
    assert B.thresholds(1.0, 4095) == 4095 and B.thresholds(0.5, 1) == 1


def test_anchored_on_the_oracle_on_the_golden_files(golden_dir, oracle):
    """W >= n, z = 0, all-ACGT queries: best is the oracle's count; smaller windows stay below it"""
    q = b"AGTCAACGCTAAGGCATTTCCCCCCTGCCTCCTGCCTGCTGCCAAGCCCT"
    seen = 0
    for name, fb in (("c1.cobs_classic", F.classic_file(os.path.join(golden_dir, "c1.cobs_classic"))),
                     ("c1.cobs_compact", _read_compact(os.path.join(golden_dir, "c1.cobs_compact")))):
        ix = oracle.Index.open(os.path.join(golden_dir, name))
        for qq in (q, oracle.random_sequence(90, 3)):
            score = np.asarray(ix.counts(qq)).astype(np.int64)
            n = fb.positions(qq, 0)
            for W in (n, n + 1, 4095):
                (w, b, _docs, s), = B.tables([fb], qq, 0, W)
                assert w == n
                np.testing.assert_array_equal(b, score)
                np.testing.assert_array_equal(s, score)
            (w, b, _docs, s), = B.tables([fb], qq, 0, 5)
            assert w == 5 and (b <= np.minimum(5, score)).all() and ((b > 0) == (score > 0)).all()
            seen += int((score > 0).sum())
        # the results at W >= n are the oracle's hits in the window search's order
        res = B.results([fb], q, 0, 4095, 0.5, 0)
        want = sorted(((f, d, sc) for (f, d, _n, sc) in oracle.search([ix], q, 0.5, 0)), key=lambda r: (-r[2], r[0], r[1]))
        assert res == want
    assert seen > 0


@pytest.mark.parametrize("z", [0, 3])
def test_structure_fixture_reaches_what_it_is_for(z):
    """the non-vacuity conditions of tests/test_gpu_window.py's structure fixture, on the checker alone"""
    _path, fb, q = structure(None, z)
    win = V.windows(fb, q, z)
    assert win.shape[0] == 600 - z
    b, score = B.structure_conditions(win, fb.doc_of_slot())
    assert (score[18:] == 0).all()                                          # every set position is planted
    # (d): the run crosses every default segment boundary (multiples of 100) and every forced one
    assert win[:, 3].all() and win[395:405, 8].all() and win[390:410, 13].all()


def test_symbols_are_exported_bound_and_refuse_null():
    from cobs_amd import _capi
    lib = _capi.load()
    for name, header in (("cobs_gpu_best_window", "cobs_gpu_batch.h"), ("cobs_gpu_search_window", "cobs_gpu_batch.h"),
                         ("cobs_gpu_window_ms", "cobs_gpu_diag.h")):
        assert hasattr(lib, name) and name in _capi.SYMBOLS
        assert name + "(" in open(os.path.join(ROOT, "include", header)).read()
        assert name not in open(os.path.join(ROOT, "include", "cobs_gpu.h")).read()
    text = open(os.path.join(ROOT, "include", "cobs_gpu_batch.h")).read()
    assert "best <= min(w, score of the plain search)" in text
    assert "4095" in text
    offs = (C.c_size_t * 1)(7)
    bad = C.c_size_t(0)
    # no handle: an argument error, not a crash (a handle cannot be opened without a device)
    st = lib.cobs_gpu_search_window(None, None, None, 0, 100, 0.5, 0, None, 0, offs, C.byref(bad))
    assert st == _capi.ERR_ARG and b"NULL" in lib.cobs_gpu_last_error()
    ms = (C.c_double * 3)()
    assert lib.cobs_gpu_window_ms(None, C.byref(ms)) == _capi.ERR_ARG


def test_no_handle_without_a_device(golden_dir):
    """(on a host with a GPU the handle opens; tests/test_gpu_window.py takes over there)"""
    import torch
    import cobs_amd
    from cobs_amd import _capi
    if not torch.cuda.is_available():
        with pytest.raises(cobs_amd.CobsGpuError) as e:
            cobs_amd.Search(os.path.join(golden_dir, "c1.cobs_classic")).search_window("ACGT" * 20, 10, 0.8)
        assert e.value.status == _capi.ERR_NO_DEVICE


def test_python_mirrors_exist_with_their_parameter_names():
    import cobs_amd
    import cobs_index
    from cobs_amd import _capi
    S = cobs_amd.Search
    assert list(inspect.signature(S.search_window).parameters) == ["self", "query", "window", "threshold", "num_results"]
    assert list(inspect.signature(S.search_window_arrays).parameters) == ["self", "queries", "window", "threshold", "num_results"]
    assert list(inspect.signature(S.window_ms).parameters) == ["self"]
    assert list(inspect.signature(cobs_amd.best_window).parameters) == ["bits_or_words", "n", "window"]
    assert list(inspect.signature(S.search).parameters) == ["self", "query", "threshold", "num_results"]
    assert cobs_index.Search.search_window is S.search_window and "best_window" in cobs_amd.__all__
    with pytest.raises(cobs_amd.CobsGpuError) as e:           # the device list is refused by the mirror
        cobs_amd.MultiSearch.search_window_arrays(cobs_amd.MultiSearch.__new__(cobs_amd.MultiSearch), [b"ACGT" * 10], 5)
    assert e.value.status == _capi.ERR_UNSUPPORTED and "device-list" in str(e.value)
    text = open(os.path.join(ROOT, "include", "cobs_gpu_search.hpp")).read()
    assert "void search_window(" in text and "inline uint32_t best_window(" in text


def test_cli_names_the_flag_and_its_refusals():
    tool = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")
    r = subprocess.run([tool, "-h"], capture_output=True, text=True, timeout=60)
    assert "--window N" in r.stderr
    for extra in (["-d", "0,1"], ["--hbm-budget", "1"], ["--sharded"], ["--prevalence"], ["--weighted"], ["--coverage"],
                  ["--group", "2"], ["--sets", "nowhere.tsv"], ["--sets", "nowhere.tsv", "--sets-quorum", "0.5"],
                  ["--sets", "nowhere.tsv", "--sets-profile"]):
        r = subprocess.run([tool, "-i", "nowhere.cobs_classic"] + extra + ["--window", "100", "ACGT" * 10], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 1 and "--window: not with" in r.stderr and r.stdout == "", (extra, r.stderr)
    for n in ("0", "4096", "x", "-3"):
        r = subprocess.run([tool, "-i", "nowhere.cobs_classic", "--window", n, "ACGT" * 10], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 1 and "--window: a number of positions, 1 .. 4095" in r.stderr and r.stdout == "", (n, r.stderr)
