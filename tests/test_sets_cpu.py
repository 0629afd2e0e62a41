"""CPU: the document-set checker (tests/sets_check.py) anchored on the oracle -- with one-member sets and z = 0, any == all ==
the oracle's score row -- and on the prevalence checker with one set of all documents; its threshold rule and ordering;
and what the new entry points and their mirrors promise without a device: the symbols, the struct, the refusals that need
no handle, the label conversion of the Python mirror, the .tsv parser of the CLI and the flags it refuses."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import cases
from tests import findere_check as F
from tests import invalid_check as I
from tests import prevalence_check as V
from tests import sets_check as S
from tests.test_positions_cpu import _read_compact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("sets_cpu")
    src = oracle.random_sequence(1500, 77)
    a = cases.make_classic(str(d / "a.cobs_classic"), 120, 1009, 3, 31, 1, 0.3, 5, planted={0: 1.0, 77: 0.9, 78: 1.0}, query=src)
    b = cases.make_compact(str(d / "b.cobs_compact"), 200, 8, [701, 1009, 853, 977], 1, 25, 1, 0.3, 6,
                           planted={3: 1.0, 4: 0.9, 199: 0.85}, query=src)
    return src, [a, b], [F.classic_file(a), _read_compact(b)]


def test_one_member_sets_are_the_oracles_score_row(files, golden_dir, oracle):
    src, paths, fbs = files
    todo = [(p, fb, [src[:120], oracle.random_sequence(90, 3)]) for p, fb in zip(paths, fbs)]
    q = b"AGTCAACGCTAAGGCATTTCCCCCCTGCCTCCTGCCTGCTGCCAAGCCCT"
    todo.append((os.path.join(golden_dir, "c1.cobs_classic"), F.classic_file(os.path.join(golden_dir, "c1.cobs_classic")), [q]))
    todo.append((os.path.join(golden_dir, "c1.cobs_compact"), _read_compact(os.path.join(golden_dir, "c1.cobs_compact")), [q]))
    for path, fb, queries in todo:
        ix = oracle.Index.open(path)
        slots = S.slot_of_doc(fb)
        for q in queries:
            row = np.asarray(ix.counts(q))
            got = S.counts(fb, q, 0, np.arange(fb.num_docs))
            assert sorted(got) == list(range(fb.num_docs))
            for d in range(fb.num_docs):
                assert got[d] == (int(row[slots[d]]), int(row[slots[d]])), (path, d)


def test_one_set_of_all_documents_agrees_with_the_prevalence_checker(files):
    src, _paths, fbs = files
    for fb in fbs:
        for z in (0, 3):
            for q in (src[:31 + 7], src[10:10 + 95], src[:700]):
                prev = V.prevalence(fb, q, z)
                got = S.counts(fb, q, z, np.zeros(fb.num_docs, dtype=np.int64))
                assert got == {0: (int((prev > 0).sum()), int((prev == fb.num_docs).sum()))}


def test_identities_of_the_definition(files):
    """all <= min and max <= any over the members' scores, any <= n; unlabelled documents and unused numbers do not exist"""
    src, _paths, fbs = files
    rng = np.random.default_rng(3)
    for fb in fbs:
        slots = S.slot_of_doc(fb)
        labels = rng.integers(-1, 9, fb.num_docs)
        labels[labels == 4] = 5                                      # set 4 has no member
        for z in (0, 3):
            q = src[40:40 + 150]
            sc = fb.scores(q, z)
            got = S.counts(fb, q, z, labels)
            assert sorted(got) == sorted(set(labels[labels >= 0].tolist())) and 4 not in got and -1 not in got
            for c, (a, b) in got.items():
                member_scores = sc[slots[labels == c]]
                assert b <= member_scores.min() and member_scores.max() <= a <= fb.positions(q, z)
    # planted neighbours share most of the source: a two-member set with all > 0 and all < any
    a, b = S.counts(fbs[0], src[:700], 0, np.where(np.isin(np.arange(120), (77, 78)), 0, -1))[0]
    assert 0 < b < a <= 670


def test_threshold_rule_and_ordering(files):
    src, _paths, fbs = files
    q = src[100:100 + 130]
    labelings = [np.arange(120) // 7, None]
    every = S.results(fbs, labelings, q, 0, 0.0)
    assert len(every) == 18 and {r[0] for r in every} == {0}          # a file without labels contributes nothing
    assert every == sorted(every, key=lambda r: (-r[2], -r[3], r[0], r[1]))
    by_all = S.results(fbs, labelings, q, 0, 0.0, "all")
    assert by_all == sorted(every, key=lambda r: (-r[3], -r[2], r[0], r[1])) and by_all != every
    n = fbs[0].positions(q, 0)
    for t in (0.3, 0.77, 1.0):
        thr = max(1, int(np.ceil(t * n)))
        assert S.results(fbs, labelings, q, 0, t) == [r for r in every if r[2] >= thr]
        assert S.results(fbs, labelings, q, 0, t, "all") == [r for r in by_all if r[3] >= thr]
    assert S.results(fbs, labelings, q, 0, 1e-9, "all") == [r for r in by_all if r[3] >= 1]      # at least 1
    assert S.results(fbs, labelings, q, 0, 0.0, "any", 3) == every[:3]
    # skip: the denominator is the valid positions, and a query without one returns nothing
    qn = I.with_n(q, [50])
    v = I.valid_positions(fbs[0], qn, 0)
    assert S.denominator(fbs[0], qn, 0, "skip") == v < n == S.denominator(fbs[0], qn, 0, "miss")
    assert S.results(fbs, labelings, b"N" * 60, 0, 0.5, mode="skip") == []
    offs, rows = S.arrays(fbs, labelings, [q, qn], 0, 0.3, mode="skip")
    assert offs.tolist() == [0, len(S.results(fbs, labelings, q, 0, 0.3, mode="skip")), len(rows)] and rows.shape[1] == 4


def test_symbols_are_exported_bound_and_refuse_without_a_handle():
    from cobs_amd import _capi
    lib = _capi.load()
    for name, header in (("cobs_gpu_set_doc_sets", "cobs_gpu_batch.h"), ("cobs_gpu_get_doc_sets", "cobs_gpu_batch.h"),
                         ("cobs_gpu_search_sets", "cobs_gpu_batch.h"), ("cobs_gpu_sets_ms", "cobs_gpu_diag.h")):
        assert hasattr(lib, name) and name in _capi.SYMBOLS
        assert name + "(" in open(os.path.join(ROOT, "include", header)).read()
        assert name not in open(os.path.join(ROOT, "include", "cobs_gpu.h")).read()
    assert C.sizeof(_capi.SetHit) == 16
    assert (_capi.NO_SET, _capi.SETS_BY_ANY, _capi.SETS_BY_ALL) == (0xFFFFFFFF, 0, 1)
    text = open(os.path.join(ROOT, "include", "cobs_gpu_batch.h")).read()
    assert "#define COBS_GPU_NO_SET 0xFFFFFFFFu" in text and "#define COBS_GPU_SETS_BY_ALL 1u" in text
    # no handle: an argument error, not a crash (a handle cannot be opened without a device)
    labels = (C.c_uint32 * 2)(0, 1)
    assert lib.cobs_gpu_set_doc_sets(None, 0, labels, 2, 2) == _capi.ERR_ARG and b"NULL" in lib.cobs_gpu_last_error()
    n = C.c_uint32(7)
    assert lib.cobs_gpu_get_doc_sets(None, 0, C.byref(n), None, 0) == _capi.ERR_ARG
    offs = (C.c_size_t * 1)(0)
    bad = C.c_size_t(0)
    assert lib.cobs_gpu_search_sets(None, None, None, 0, 0.0, 0, 0, None, 0, offs, C.byref(bad)) == _capi.ERR_ARG
    assert lib.cobs_gpu_search_sets(None, None, None, 0, 0.0, 7, 0, None, 0, None, None) == _capi.ERR_ARG
    ms = (C.c_double * 5)()
    assert lib.cobs_gpu_sets_ms(None, C.byref(ms)) == _capi.ERR_ARG


def test_python_mirrors_exist_and_convert_labels():
    import cobs_amd
    import cobs_index
    from cobs_amd import _capi
    assert list(inspect.signature(cobs_amd.Search.set_doc_sets).parameters) == ["self", "labels", "file_no"]
    assert list(inspect.signature(cobs_amd.Search.search_sets).parameters) == ["self", "queries", "threshold", "rank_by", "num_results"]
    assert list(inspect.signature(cobs_amd.Search.search_sets_arrays).parameters) == ["self", "queries", "threshold", "rank_by", "num_results"]
    assert inspect.signature(cobs_amd.Search.search_sets).parameters["rank_by"].default == "any"
    for name in ("doc_sets", "sets_ms"):
        assert callable(getattr(cobs_amd.Search, name))
    assert cobs_index.SetResult is cobs_amd.SetResult and cobs_amd.Search.SET_HIT_DTYPE.itemsize == 16
    r = cobs_amd.SetResult(1, 2, "ecoli", 30, 4)
    assert (r.file_no, r.set, r.name, r.any, r.all) == (1, 2, "ecoli", 30, 4) and r == cobs_amd.SetResult(1, 2, "ecoli", 30, 4)
    names = ["d0", "d1", "d2", "d3"]
    arr, sets = cobs_amd.doc_set_labels([2, -1, 0, 2], names)
    assert arr.dtype == np.uint32 and arr.tolist() == [2, _capi.NO_SET, 0, 2] and sets == ["0", "1", "2"]
    arr, sets = cobs_amd.doc_set_labels(np.array([0, 0xFFFFFFFF, 1, 1], dtype=np.uint32), names)
    assert arr.tolist() == [0, _capi.NO_SET, 1, 1] and sets == ["0", "1"]
    arr, sets = cobs_amd.doc_set_labels({"d3": "salmonella", "d0": "ecoli", "d2": "ecoli"}, names)
    assert sets == ["ecoli", "salmonella"] and arr.tolist() == [0, _capi.NO_SET, 0, 1]
    assert cobs_amd.doc_set_labels([-1, -1, -1, -1], names)[1] == []
    with pytest.raises(ValueError) as e:
        cobs_amd.doc_set_labels({"d0": "a", "nobody": "b"}, names)
    assert "nobody" in str(e.value)
    for bad in ([0, 1, 2], [0, -2, 0, 0], [0.5, 1, 2, 3], [[0, 1], [2, 3]]):
        with pytest.raises(ValueError):
            cobs_amd.doc_set_labels(bad, names)
    for call in (lambda m: m.set_doc_sets([0]), lambda m: m.search_sets_arrays([b"ACGT" * 10])):      # the device list is refused
        with pytest.raises(cobs_amd.CobsGpuError) as e:
            call(cobs_amd.MultiSearch.__new__(cobs_amd.MultiSearch))
        assert e.value.status == _capi.ERR_UNSUPPORTED and "not additive" in str(e.value)


def test_cli_parses_the_tsv_and_refuses_flags_before_it_opens_the_index(tmp_path):
    r = subprocess.run([TOOL, "-h"], capture_output=True, text=True, timeout=60)
    assert "--sets FILE.tsv" in r.stderr and "--sets-by" in r.stderr
    good = tmp_path / "good.tsv"
    good.write_text("doc_00000\tecoli\ndoc_00001\tecoli\n\ndoc_00002\tk pneumoniae\r\ndoc_00000\tecoli\n")

    def run(*args):
        r = subprocess.run([TOOL, "-i", "nowhere.cobs_classic"] + list(args) + ["ACGT" * 10], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and r.stdout == ""
        return r.stderr
    # a well-formed file gets as far as the index
    assert "--sets" not in run("--sets", str(good))
    assert "could not open" in run("--sets", str(tmp_path / "missing.tsv"))
    for text, line in (("doc_00000 ecoli\n", 1), ("doc_00000\tecoli\nno_tab_here\n", 2), ("doc_00000\t\n", 1), ("\tecoli\n", 1),
                       ("doc_00000\tecoli\textra\n", 1)):
        bad = tmp_path / "bad.tsv"
        bad.write_text(text)
        err = run("--sets", str(bad))
        assert "--sets: line %d of" % line in err and "document name<TAB>set name" in err, err
    twice = tmp_path / "twice.tsv"
    twice.write_text("doc_00000\tecoli\ndoc_00001\tecoli\ndoc_00000\tsalmonella\n")
    err = run("--sets", str(twice))
    assert "--sets: line 3 of" in err and "doc_00000 is already in set ecoli" in err
    assert "--sets-by: any or all" in run("--sets", str(good), "--sets-by", "most")
    assert "--sets-by: needs --sets" in run("--sets-by", "all")
    for extra in (["--positions"], ["--prevalence"], ["--weighted"], ["--group", "2"], ["--fpr-adjust"], ["--sharded"], ["-d", "0,1"],
                  ["--hbm-budget", "1"]):
        assert "--sets: not with" in run("--sets", str(good), *extra), extra
