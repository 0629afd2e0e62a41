"""CPU: the set-quorum checker (tests/set_quorum_check.py) anchored on the oracle -- with one-member sets and z = 0, core == any
== the oracle's score row for every quorum --, on the prevalence checker with one set of all documents and with the sum over
a full labelling, and on the document-set checker at quorum 1 and at need = 1; the need rule against exact rational
arithmetic; and what the new entry points and their mirrors promise without a device: the symbols, the struct, the refusals
that need no handle, the Python mirrors and the flags the CLI refuses."""
import ctypes as C
import inspect
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import prevalence_check as V
from tests import set_quorum_check as Q
from tests import sets_check as S
from tests.test_positions_cpu import _read_compact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")
QUORUMS = (1e-9, 0.5, 0.95, 1.0)
GOLDEN_QUERY = b"AGTCAACGCTAAGGCATTTCCCCCCTGCCTCCTGCCTGCTGCCAAGCCCT"


@pytest.fixture(scope="module")
def golden(golden_dir, oracle):
    path = os.path.join(golden_dir, "c1.cobs_compact")
    return path, _read_compact(path), [GOLDEN_QUERY, oracle.random_sequence(90, 3)]


def test_one_member_sets_are_the_oracles_score_row(golden, oracle):
    path, fb, queries = golden
    ix = oracle.Index.open(path)
    slots = Q.slot_of_doc(fb)
    own = np.arange(fb.num_docs)
    for q in queries:
        row = np.asarray(ix.counts(q))
        prof = Q.profile(fb, q, 0, own)
        assert prof.shape == (fb.num_docs, fb.positions(q, 0)) and prof.max() <= 1
        for quorum in QUORUMS:
            got = Q.counts(fb, q, 0, own, quorum)
            assert sorted(got) == list(range(fb.num_docs))
            for d in range(fb.num_docs):
                assert got[d] == (int(row[slots[d]]), int(row[slots[d]])), (d, quorum)
    assert np.asarray(ix.counts(GOLDEN_QUERY)).max() == 20


def test_one_set_of_all_and_the_sum_over_a_full_labelling_are_the_prevalence(golden):
    _path, fb, queries = golden
    d = np.arange(fb.num_docs)
    for z in (0, 2):
        for q in queries:
            prev = V.prevalence(fb, q, z)
            one = Q.profile(fb, q, z, np.zeros(fb.num_docs, dtype=np.int64))
            assert one.shape == (1, len(prev)) and np.array_equal(one[0], prev)
            for labels in (d % 3, d // 2, d):
                assert np.array_equal(Q.profile(fb, q, z, labels).sum(axis=0), prev)
            # unlabelled documents leave the sum
            part = np.where(d % 2 == 0, d % 3, -1)
            rest = np.where(d % 2 == 1, 0, -1)
            assert np.array_equal(Q.profile(fb, q, z, part).sum(axis=0) + Q.profile(fb, q, z, rest).sum(axis=0), prev)


def test_quorum_one_is_all_and_need_one_is_any(golden):
    _path, fb, queries = golden
    d = np.arange(fb.num_docs)
    seen_diff = False
    for z in (0, 2):
        for q in queries:
            for labels in (d % 3, d // 2, np.zeros(fb.num_docs, dtype=np.int64), np.where(d % 4 == 1, -1, (d // 3) * 2)):
                ref = S.counts(fb, q, z, labels)                       # {set: (any, all)}
                hi = Q.counts(fb, q, z, labels, 1.0)
                lo = Q.counts(fb, q, z, labels, 1e-9)
                assert sorted(hi) == sorted(ref) == sorted(lo)
                for c, (a, b) in ref.items():
                    assert hi[c] == (b, a) and lo[c] == (a, a), (z, c)
                    seen_diff |= a != b
    assert seen_diff


def test_threshold_rule_and_ordering(golden):
    _path, fb, queries = golden
    q = queries[0]
    labels = np.arange(fb.num_docs) // 2
    every = Q.results([fb, fb], [labels, None], q, 0, 0.5)
    assert len(every) == len(Q.nonempty_sets(labels)) and {r[0] for r in every} == {0}       # a file without labels contributes nothing
    assert every == sorted(every, key=lambda r: (-r[2], -r[3], r[0], r[1]))
    n = fb.positions(q, 0)
    for t in (0.1, 0.3, 0.9):
        thr = max(1, int(np.ceil(t * n)))
        assert Q.results([fb], [labels], q, 0, 0.5, t) == [r for r in every if r[2] >= thr]
    assert Q.results([fb], [labels], q, 0, 0.5, 1e-9) == [r for r in every if r[2] >= 1]      # at least 1
    assert Q.results([fb], [labels], q, 0, 0.5, 0.0, 3) == every[:3]
    offs, rows = Q.arrays([fb], [labels], queries, 0, 0.5, 0.1)
    assert offs.tolist() == [0, len(Q.results([fb], [labels], queries[0], 0, 0.5, 0.1)), len(rows)] and rows.shape[1] == 4
    soffs, seg = Q.segments([fb, fb], [labels, None], queries, 0)
    assert soffs.tolist()[:3] == [0, len(Q.nonempty_sets(labels)) * n, len(Q.nonempty_sets(labels)) * n] and len(seg) == soffs[-1]


# (members, quorum) for which ceil of the DOUBLE product differs from ceil of the exact rational product, among the grid
# below: none -- every product of the grid that is an integer in exact arithmetic is that integer in double too.  The
# definition is the double rule all the same; the last test case pins one product off the grid where the two part.
DOUBLE_RULE_WINS = ()


def test_need_against_exact_rational_arithmetic():
    differ = []
    for m in (1, 2, 3, 19, 20, 21, 100, 128, 129):
        for text in ("0.5", "0.9", "0.95", "0.99", "1.0"):
            got = Q.need(float(text), m)
            assert got == max(1, math.ceil(float(text) * m)) and 1 <= got <= m
            exact = max(1, math.ceil(Fraction(text) * m))
            if got != exact:
                differ.append((m, text))
            else:
                assert got == exact
    assert tuple(differ) == DOUBLE_RULE_WINS
    assert [Q.need(0.95, m) for m in (1, 19, 20, 21, 100, 128, 129)] == [1, 19, 19, 20, 95, 122, 123]
    assert [Q.need(1e-9, m) for m in (1, 129, 10 ** 6)] == [1, 1, 1] and Q.need(1.0, 129) == 129
    # 0.07 * 100 is 7.000000000000001 in double: the double rule says 8, exact arithmetic 7
    assert Q.need(0.07, 100) == 8 and math.ceil(Fraction("0.07") * 100) == 7


def test_symbols_are_exported_bound_and_refuse_without_a_handle():
    from cobs_amd import _capi
    lib = _capi.load()
    for name, header in (("cobs_gpu_search_sets_quorum", "cobs_gpu_batch.h"), ("cobs_gpu_set_prevalence", "cobs_gpu_batch.h"),
                         ("cobs_gpu_set_quorum_ms", "cobs_gpu_diag.h")):
        assert hasattr(lib, name) and name in _capi.SYMBOLS
        assert name + "(" in open(os.path.join(ROOT, "include", header)).read()
        assert name not in open(os.path.join(ROOT, "include", "cobs_gpu.h")).read()
    assert C.sizeof(_capi.SetQuorumHit) == 16
    assert [f[0] for f in _capi.SetQuorumHit._fields_] == ["file_no", "set", "core", "any"]
    assert "typedef struct cobs_gpu_set_quorum_hit { uint32_t file_no, set, core, any; }" in open(os.path.join(ROOT, "include", "cobs_gpu_batch.h")).read()
    # no handle: an argument error, not a crash (a handle cannot be opened without a device)
    offs = (C.c_size_t * 1)(0)
    bad = C.c_size_t(0)
    assert lib.cobs_gpu_search_sets_quorum(None, None, None, 0, 0.0, 0.5, 0, None, 0, offs, C.byref(bad)) == _capi.ERR_ARG
    assert b"NULL" in lib.cobs_gpu_last_error()
    assert lib.cobs_gpu_search_sets_quorum(None, None, None, 0, 0.0, 0.5, 0, None, 0, None, None) == _capi.ERR_ARG
    for quorum in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert lib.cobs_gpu_search_sets_quorum(None, None, None, 0, 0.0, quorum, 0, None, 0, offs, C.byref(bad)) == _capi.ERR_ARG
        assert b"quorum" in lib.cobs_gpu_last_error(), quorum
    need = C.c_size_t(0)
    assert lib.cobs_gpu_set_prevalence(None, None, None, 0, None, 0, offs, C.byref(need), C.byref(bad)) == _capi.ERR_ARG
    assert lib.cobs_gpu_set_prevalence(None, None, None, 0, None, 0, None, None, None) == _capi.ERR_ARG
    ms = (C.c_double * 5)()
    assert lib.cobs_gpu_set_quorum_ms(None, C.byref(ms)) == _capi.ERR_ARG


def test_python_mirrors_exist():
    import cobs_amd
    import cobs_index
    from cobs_amd import _capi
    params = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert params(cobs_amd.Search.search_sets_quorum) == ["self", "query", "quorum", "threshold", "num_results"]
    assert params(cobs_amd.Search.search_sets_quorum_arrays) == ["self", "queries", "quorum", "threshold", "num_results"]
    assert params(cobs_amd.Search.set_prevalence) == ["self", "query"]
    assert params(cobs_amd.Search.set_prevalence_arrays) == ["self", "queries"]
    assert inspect.signature(cobs_amd.Search.search_sets_quorum).parameters["threshold"].default == 0.0
    assert callable(cobs_amd.Search.set_quorum_ms)
    assert cobs_index.SetQuorumResult is cobs_amd.SetQuorumResult and cobs_amd.Search.SET_QUORUM_HIT_DTYPE.itemsize == 16
    assert cobs_amd.Search.SET_QUORUM_HIT_DTYPE.names == ("file_no", "set", "core", "any")
    r = cobs_amd.SetQuorumResult(1, 2, "ecoli", 30, 44)
    assert (r.file_no, r.set, r.name, r.core, r.any) == (1, 2, "ecoli", 30, 44) and r == cobs_amd.SetQuorumResult(1, 2, "ecoli", 30, 44)
    assert r != cobs_amd.SetQuorumResult(1, 2, "ecoli", 30, 45)
    for call in (lambda m: m.search_sets_quorum_arrays([b"ACGT" * 10], 0.5), lambda m: m.set_prevalence_arrays([b"ACGT" * 10]),
                 lambda m: m.search_sets_quorum(b"ACGT" * 10, 0.5), lambda m: m.set_prevalence(b"ACGT" * 10)):      # the device list is refused
        with pytest.raises(cobs_amd.CobsGpuError) as e:
            call(cobs_amd.MultiSearch.__new__(cobs_amd.MultiSearch))
        assert e.value.status == _capi.ERR_UNSUPPORTED and "device-list" in str(e.value)


def test_cli_refuses_the_flags_before_it_opens_the_index(tmp_path):
    r = subprocess.run([TOOL, "-h"], capture_output=True, text=True, timeout=60)
    assert "--sets-quorum X" in r.stderr and "--sets-profile" in r.stderr
    good = tmp_path / "good.tsv"
    good.write_text("doc_00000\tecoli\ndoc_00001\tecoli\ndoc_00002\tk pneumoniae\n")

    def run(*args):
        r = subprocess.run([TOOL, "-i", "nowhere.cobs_classic"] + list(args) + ["ACGT" * 10], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and r.stdout == ""
        return r.stderr
    # well-formed flags get as far as the index
    for ok in (["--sets-quorum", "0.95"], ["--sets-quorum", "1"], ["--sets-quorum", "1e-9", "-t", "0.5", "-l", "3"], ["--sets-profile"]):
        err = run("--sets", str(good), *ok)
        assert "--sets" not in err and "nowhere.cobs_classic" in err, (ok, err)
    assert "--sets-quorum: needs --sets" in run("--sets-quorum", "0.5")
    assert "--sets-profile: needs --sets" in run("--sets-profile")
    for bad in ("0", "-0.5", "1.5", "nan", "most", "0.5x", ""):
        assert "--sets-quorum: a number in (0, 1]" in run("--sets", str(good), "--sets-quorum", bad), bad
    assert "--sets-quorum: not with" in run("--sets", str(good), "--sets-quorum", "0.5", "--sets-profile")
    assert "--sets-quorum: not with" in run("--sets", str(good), "--sets-quorum", "0.5", "--sets-by", "all")
    assert "--sets-profile: not with" in run("--sets", str(good), "--sets-profile", "--sets-by", "all")
    for new in (["--sets-quorum", "0.5"], ["--sets-profile"]):
        for extra in (["--positions"], ["--prevalence"], ["--weighted"], ["--group", "2"], ["--fpr-adjust"], ["--sharded"], ["-d", "0,1"],
                      ["--hbm-budget", "1"]):
            assert "--sets: not with" in run("--sets", str(good), *new, *extra), (new, extra)
        assert "--coverage: not with" in run("--sets", str(good), *new, "--coverage")
