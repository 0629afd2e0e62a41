"""CPU: the filter-fill checker anchored on the oracle's hashes, the C surface of cobs_gpu_doc_bits, and the host
arithmetic of the FPR adjustment (cobs_amd.fpr_adjust) against the checker's formulas."""
import ctypes as C
import itertools
import os

import numpy as np

from tests import cases, fill_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _expect_bits(ix, docs_by_name):
    """distinct hash % S_p over the terms and hash functions of every document, in the file's document order"""
    sigs = fill_check.doc_sigs(ix)
    out = []
    for d, name in enumerate(ix["names"]):
        h = docs_by_name[name].hashes.reshape(-1)
        out.append(len(np.unique(h % np.uint64(sigs[d]))) if h.size else 0)
    return np.array(out, dtype=np.uint64)


def test_checker_equals_distinct_rows_of_the_golden_documents(golden_dir, oracle, construct):
    for name in ("c1.cobs_classic", "c1.cobs_compact"):
        ix = fill_check.read_index(os.path.join(golden_dir, name))
        docs = construct.fasta_dir_docs(os.path.join(golden_dir, "fasta"), ix["term_size"], ix["canonicalize"], ix["num_hashes"])
        by_name = {d.name: d for d in docs}
        assert sorted(by_name) == sorted(ix["names"])
        bits = fill_check.bits_of_mats(ix["mats"])
        n = len(ix["names"])
        assert np.array_equal(bits[:n], _expect_bits(ix, by_name)), name
        assert not bits[n:].any()                   # padding slots of a well-formed file
        assert bits[:n].all()


def test_checker_equals_distinct_rows_of_the_survey_probe_files(oracle, construct, tmp_path):
    pc, pk, q, names, _scores = cases.survey_probe_files(oracle, construct, tmp_path)
    hashes, good = oracle.term_hashes(q, 31, 1, 3)
    by_name = {names[j]: construct.Doc(names[j], names[j], 0, 0, hashes[np.arange(0, 270, j + 1)]) for j in range(20)}
    for path in (pc, pk):
        ix = fill_check.read_index(path)
        assert ix["names"] == names and ix["num_hashes"] == 3
        bits = fill_check.bits_of_file(path)
        assert np.array_equal(bits[:20], _expect_bits(ix, by_name)), path
        assert not bits[20:].any()
    assert fill_check.read_index(pk)["sigs"] == [3001, 4001, 5003]
    # fill and fpr follow from the counts
    ix = fill_check.read_index(pc)
    assert fill_check.doc_fill(pc)[0] == int(fill_check.bits_of_file(pc)[0]) / 5003
    assert fill_check.doc_fpr(pc)[3] == fill_check.doc_fill(pc)[3] ** 3


def test_surface():
    from cobs_amd import _capi
    inc = os.path.join(ROOT, "include")
    batch_h = open(os.path.join(inc, "cobs_gpu_batch.h")).read()
    diag_h = open(os.path.join(inc, "cobs_gpu_diag.h")).read()
    base_h = open(os.path.join(inc, "cobs_gpu.h")).read()
    assert "cobs_gpu_doc_bits(" in batch_h and "cobs_gpu_doc_bits_ms(" in diag_h
    assert "cobs_gpu_doc_bits" not in base_h
    for name in ("cobs_gpu_doc_bits", "cobs_gpu_doc_bits_ms"):
        assert name in _capi.SYMBOLS
    lib = _capi.load()
    need = C.c_size_t(77)
    assert lib.cobs_gpu_doc_bits(None, 0, None, 0, C.byref(need)) == _capi.ERR_ARG
    assert need.value == 0
    assert lib.cobs_gpu_doc_bits(None, 0, None, 0, None) == _capi.ERR_ARG
    ms = (C.c_double * 4)()
    assert lib.cobs_gpu_doc_bits_ms(None, C.byref(ms)) == _capi.ERR_ARG
    import cobs_amd
    import cobs_index
    assert cobs_index.fpr_adjust is cobs_amd.fpr_adjust
    for m in ("doc_bits", "doc_fill", "doc_fpr", "search_adjusted"):
        assert hasattr(cobs_amd.Search, m)


def test_fpr_adjust_equals_the_checkers_formulas():
    import cobs_amd
    sig = 1 << 53                 # fills of 0, one bit, 0.3, 1 - 2^-52 ... exactly representable numerators
    fills = [0, 1, int(0.3 * sig), sig - 2, sig]
    assert (sig - 2) / sig == 1.0 - 2.0 ** -52
    n = 0
    for bits, H, z, P, frac in itertools.product(fills, (1, 2, 3), (0, 3, 7), (0, 1, 270, 1000, 100000), (0.0, 0.1, 0.5, 1.0)):
        s = int(P * frac)
        want = fill_check.adjust(s, P, bits, sig, H, z)
        e, a = cobs_amd.fpr_adjust(s, P, bits, sig, H, z)
        for got, w in ((e, want["expected_fp"]), (a, want["adjusted"])):
            assert got == got and got >= 0.0                      # never NaN, never negative
            assert abs(got - w) <= 1e-12 * abs(w), (bits, H, z, P, s, got, w)
        if want["q"] >= 1.0:
            assert a == 0.0
        n += 1
    assert n == 5 * 3 * 3 * 5 * 4
    # a saturated filter says nothing; an empty one leaves the score as it is
    assert cobs_amd.fpr_adjust(50, 100, sig, sig, 1, 0) == (100.0, 0.0)
    assert cobs_amd.fpr_adjust(50, 100, 0, sig, 2, 3) == (0.0, 50.0)
    # arrays broadcast
    e, a = cobs_amd.fpr_adjust(np.array([10, 90]), 100, np.array([3, 9]), 10, 1, 0)
    assert np.allclose(e, [30.0, 90.0]) and a[0] == 0.0 and a[1] == 0.0
    e, a = cobs_amd.fpr_adjust(np.array([65.0]), 100, np.array([3]), 10, 1, 0)
    assert abs(a[0] - 50.0) < 1e-9
