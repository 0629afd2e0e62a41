"""CPU: the best-of-group checker (tests/best_check.py) anchored on the oracle, the associativity of its merge, and what
the new entry points and their mirrors promise without a device.

At z = 0 and all-ACGT queries a one-member group's best record carries the oracle's score of every document; a real
group's score / positions is the maximum of its members' oracle fractions and `query` attains it: the checker adds
nothing of its own but the choice."""
import ctypes as C
import inspect
import itertools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import best_check as B
from tests import cases
from tests import findere_check as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("best_cpu")
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


def test_best_records_are_the_oracle_scores_and_their_largest_fraction(files, oracle):
    src, paths, fbs = files
    ixs = [oracle.Index.open(p) for p in paths]
    queries = _reads(src, 9, 40, 140, 3) + [oracle.random_sequence(80, 9)]
    want = []                                   # per query, per file: the oracle's score of every document
    for q in queries:
        sc = [np.zeros(fb.num_docs, dtype=np.int64) for fb in fbs]
        for f, d, _name, s in oracle.search(ixs, q, 0.0, 0):
            sc[f][d] = s
        want.append(sc)
    # one-member groups: the best record's score is the oracle's score, for every document
    res = B.results(fbs, queries, list(range(len(queries) + 1)), 0, "error", 0.0, 0)
    for q, recs in enumerate(res):
        assert len(recs) == sum(fb.num_docs for fb in fbs)
        for (f, d, bq, s, P, t) in recs:
            assert (bq, s, P, t) == (q, int(want[q][f][d]), len(queries[q]) - fbs[f].term_size + 1, 1)
    # real groups: score / positions is the maximum of the members' oracle fractions, and `query` attains it
    offsets = [0, 0, 1, 3, 10, 10]
    res = B.results(fbs, queries, offsets, 0, "error", 0.0, 0)
    assert res[0] == [] and res[4] == []        # a group without members reports nothing
    for g in (1, 2, 3):
        members = range(offsets[g], offsets[g + 1])
        assert len(res[g]) == sum(fb.num_docs for fb in fbs)
        for (f, d, bq, s, P, t) in res[g]:
            fr = {q: Fraction(int(want[q][f][d]), len(queries[q]) - fbs[f].term_size + 1) for q in members}
            assert bq in members and Fraction(s, P) == max(fr.values()) == fr[bq] and s == int(want[bq][f][d])
            assert t == sum(1 for q in members if fr[q] == fr[bq]) >= 1
        assert res[g] == sorted(res[g], key=lambda h: (-Fraction(h[3], h[4]), -h[3], h[0], h[1]))
    # thresholds and limits: the planted-complete documents are what a full-length member finds at 1.0
    full = B.results(fbs, queries, offsets, 0, "error", 1.0, 0)[3]
    assert {(f, d) for (f, d, *_r) in full} >= {(0, 0), (1, 3)} and all(s == P for (_f, _d, _q, s, P, _t) in full)
    assert B.results(fbs, queries, offsets, 0, "error", 0.0, 3)[3] == res[3][:3]
    assert B.threshold_of(0.8, 0) == 1 and B.threshold_of(0.0, 10) == 0 and B.threshold_of(0.25, 10) == 3


def test_the_vectorised_cells_are_the_literal_definition(files):
    src, _paths, fbs = files
    queries = _reads(src, 7, 40, 90, 8) + [src[100:170], src[100:170], b"N" * 60]
    offsets = [0, 3, 3, 10]
    for mode, z in (("error", 0), ("skip", 1), ("miss", 1)):
        qs = queries if mode != "error" else queries[:-1] + [src[5:65]]
        per_file = B.cells(fbs, qs, offsets, z, mode)
        for fb, (bs, bp, bq, bt) in zip(fbs, per_file):
            sc = [B.G.scores(fb, q, z, mode) for q in qs]
            P = [B.G.positions_of(fb, q, z, mode) for q in qs]
            for g in range(3):
                for slot in range(0, fb.slots, 7):
                    members = [(int(sc[q][slot]), int(P[q]), q) for q in range(offsets[g], offsets[g + 1])]
                    assert B.best_of(members) == (int(bs[g, slot]), int(bp[g, slot]), int(bq[g, slot]), int(bt[g, slot]))
    assert int(B.cells(fbs, queries, offsets, 1, "skip")[0][1][2].min()) > 0       # the all-N member (P = 0) is never the best


def _fold(members):
    st = B.EMPTY
    for m in members:
        st = B.merge(st, (m[0], m[1], m[2], 1))
    return st


def test_the_merge_is_associative_under_every_cut():
    cells = {
        "random": [(3, 10, 0), (5, 12, 1), (2, 4, 2), (7, 20, 3), (1, 2, 4), (6, 12, 5)],
        "equal fraction, different length": [(5, 10, 0), (10, 20, 1), (1, 2, 2), (20, 40, 3), (3, 7, 4)],
        "identical members": [(4, 9, 0), (4, 9, 1), (4, 9, 2), (2, 9, 3), (4, 9, 4)],
        "all zero": [(0, 10, 0), (0, 20, 1), (0, 0, 2), (0, 5, 3)],
        "P = 0 beside hits": [(0, 0, 0), (3, 10, 1), (0, 0, 2), (6, 20, 3), (0, 7, 4)],
        "large": [(4000000000, 4100000000, 0), (2000000000, 2050000000, 1), (4000000001, 4100000001, 2)],
    }
    for name, members in cells.items():
        want = B.best_of(members)
        n = len(members)
        assert _fold(members) == want, name
        for i, j in itertools.combinations_with_replacement(range(n + 1), 2):
            a, b, c = _fold(members[:i]), _fold(members[i:j]), _fold(members[j:])
            assert B.merge(B.merge(a, b), c) == B.merge(a, B.merge(b, c)) == want, (name, i, j)
            assert B.merge(c, B.merge(b, a)) == want and B.merge(B.merge(a, c), b) == want, (name, i, j)
        assert B.merge(B.EMPTY, want) == B.merge(want, B.EMPTY) == want
    assert B.best_of(cells["equal fraction, different length"]) == (20, 40, 3, 4)          # the longest wins, all tie
    assert B.best_of(cells["identical members"]) == (4, 9, 0, 4)                           # the lowest index wins
    assert B.best_of(cells["all zero"]) == (0, 10, 0, 4)
    assert B.best_of(cells["P = 0 beside hits"]) == (6, 20, 3, 2)                          # P = 0 ties with no hit


def test_symbols_are_exported_bound_and_refuse_null(tmp_path):
    from cobs_amd import _capi
    lib = _capi.load()
    batch_h = open(os.path.join(ROOT, "include", "cobs_gpu_batch.h")).read()
    diag_h = open(os.path.join(ROOT, "include", "cobs_gpu_diag.h")).read()
    base_h = open(os.path.join(ROOT, "include", "cobs_gpu.h")).read()
    assert "cobs_gpu_search_best(" in batch_h and "cobs_gpu_best_ms(" in diag_h and "cobs_gpu_best" not in base_h
    for name in ("cobs_gpu_search_best", "cobs_gpu_best_ms", "cobs_gpu_best_counts"):
        assert hasattr(lib, name) and name in _capi.SYMBOLS
    assert C.sizeof(_capi.BestHit) == 24 and [f[0] for f in _capi.BestHit._fields_] == ["file_no", "doc", "query", "score", "positions", "ties"]
    assert lib.cobs_gpu_abi_version() == 2
    goffs = (C.c_size_t * 2)(0, 0)
    hoffs = (C.c_size_t * 2)(7, 7)
    bad = C.c_size_t(0)
    # no handle (one cannot be opened without a device): an argument error, not a crash
    st = lib.cobs_gpu_search_best(None, None, None, 0, goffs, 1, 0.0, 0, None, 0, hoffs, C.byref(bad))
    assert st == _capi.ERR_ARG and b"NULL" in lib.cobs_gpu_last_error()
    assert lib.cobs_gpu_search_best(None, None, None, 0, None, 0, 0.0, 0, None, 0, None, None) == _capi.ERR_ARG
    ms = (C.c_double * 3)()
    assert lib.cobs_gpu_best_ms(None, C.byref(ms)) == _capi.ERR_ARG
    n = (C.c_uint64 * 4)()
    assert lib.cobs_gpu_best_counts(None, C.byref(n)) == _capi.ERR_ARG
    # the header still compiles as C99 and as C++17
    inc = os.path.join(ROOT, "include")
    probe = "cobs_gpu_best_hit h; h.ties = 1; return (int)h.ties == 0 || sizeof h != 24;"
    c = tmp_path / "best.c"
    c.write_text('#include "cobs_gpu_batch.h"\n#include "cobs_gpu_diag.h"\nint main(void) { %s }\n' % probe)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, "-fsyntax-only", str(c)])
    cpp = tmp_path / "best.cpp"
    cpp.write_text('#include "cobs_gpu_search.hpp"\nint main() { cobs_gpu::ClassicSearch::BestResult r{}; %s }\n'
                   % probe.replace("return", "return r.ties != 0 ||"))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", inc, "-fsyntax-only", str(cpp)])


def test_python_mirrors_exist_and_nothing_runs_without_a_device(golden_dir):
    import torch

    import cobs_amd
    import cobs_index
    from cobs_amd import _capi
    sig = inspect.signature(cobs_amd.Search.search_best)
    assert list(sig.parameters) == ["self", "queries", "group_offsets", "threshold", "num_results", "group_size"]
    assert [sig.parameters[n].default for n in ("group_offsets", "threshold", "num_results", "group_size")] == [None, 0.0, 0, None]
    assert list(inspect.signature(cobs_amd.Search.search_best_arrays).parameters) == list(sig.parameters)
    r = cobs_amd.BestResult("d", 1, 2, 3, 4, 5, 6)
    assert (r.doc_name, r.file_no, r.doc, r.query, r.score, r.positions, r.ties) == ("d", 1, 2, 3, 4, 5, 6)
    assert r == cobs_index.BestResult("d", 1, 2, 3, 4, 5, 6) and r != cobs_amd.BestResult("d", 1, 2, 3, 4, 5, 7)
    assert cobs_index.Search.search_best is cobs_amd.Search.search_best and hasattr(cobs_amd.Search, "best_ms")
    assert cobs_amd.Search.BEST_HIT_DTYPE.itemsize == 24
    s = cobs_amd.Search(None, _handle=C.c_void_p())           # no handle: the library refuses
    with pytest.raises(cobs_amd.CobsGpuError) as e:
        s.search_best_arrays([b"ACGT" * 10], [0, 1])
    assert e.value.status == _capi.ERR_ARG
    with pytest.raises(ValueError):
        s.search_best([b"ACGT" * 10])                         # neither offsets nor a size
    with pytest.raises(ValueError):
        s.search_best([b"ACGT" * 10], [0, 1], group_size=1)
    with pytest.raises(ValueError):
        s.search_best([b"ACGT" * 10], group_size=0)
    with pytest.raises(cobs_amd.CobsGpuError) as e:           # the device list is refused by the mirror
        cobs_amd.MultiSearch.search_best_arrays(object.__new__(cobs_amd.MultiSearch), [b"ACGT" * 10], [0, 1])
    assert e.value.status == _capi.ERR_UNSUPPORTED and "device-list" in str(e.value)
    if not torch.cuda.is_available():
        with pytest.raises(cobs_amd.CobsGpuError) as e:
            cobs_amd.Search(os.path.join(golden_dir, "c1.cobs_classic")).search_best([b"A" * 40], [0, 1])
        assert e.value.status == _capi.ERR_NO_DEVICE


def test_cli_names_the_flags_and_refuses_combinations():
    tool = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")
    r = subprocess.run([tool, "-h"], capture_output=True, text=True, timeout=60)
    assert "--best N" in r.stderr and "--best-by-name SEP" in r.stderr
    base = [tool, "-i", "x.cobs_classic", "-f", "q.fa"]
    for extra in (["--best", "0"], ["--best", "x"], ["--best", "3", "--best-by-name", "_"], ["--best-by-name", "__"],
                  ["--best", "3", "--group", "2"], ["--best", "3", "--weighted"], ["--best", "all", "--coverage"],
                  ["--best", "3", "--window", "20"], ["--best", "3", "--prevalence"], ["--best", "3", "--positions"],
                  ["--best-by-name", "_", "--fpr-adjust"], ["--best", "3", "--sets", "s.tsv"], ["--best", "3", "--hbm-budget", "1"],
                  ["--best", "3", "-d", "0,1"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--best" in r.stderr and r.stdout == "", extra
    r = subprocess.run([tool, "-i", "x.cobs_classic", "--best", "3", "ACGT"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--best" in r.stderr
