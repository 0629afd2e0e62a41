"""CPU: the prevalence checker (tests/prevalence_check.py) anchored on the oracle at z = 0, its identities against the
findere / positions / invalid-bases checkers, and what the new entry point and its mirrors promise without a device.

prevalence[p] = the real documents in which position p of a query is set.  At z = 0 that is the number of real documents
for which the oracle scores the single-k-mer query q[p:p+k] with 1 (all H bits set), and the sum over p is the sum over
the real documents of oracle.Index.counts(q)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from tests import cases
from tests import findere_check as F
from tests import invalid_check as I
from tests import positions_check as P
from tests import prevalence_check as V
from tests.test_positions_cpu import _read_compact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _anchor(oracle, path, fb, queries):
    ix = oracle.Index.open(path)
    real = fb.doc_of_slot() >= 0
    assert int(real.sum()) == fb.num_docs
    k = fb.term_size
    for q in queries:
        prev = V.prevalence(fb, q, 0)
        assert prev.dtype == np.uint32 and len(prev) == len(q) - k + 1
        for p in range(len(prev)):
            one = np.asarray(ix.counts(q[p:p + k]))
            assert set(np.unique(one)) <= {0, 1}
            assert int(prev[p]) == int((one[real] == 1).sum()), (path, p)
        assert int(prev.sum()) == int(np.asarray(ix.counts(q))[real].sum())


def test_anchored_on_the_oracle_on_the_golden_files(golden_dir, oracle):
    q = b"AGTCAACGCTAAGGCATTTCCCCCCTGCCTCCTGCCTGCTGCCAAGCCCT"
    for name, fb in (("c1.cobs_classic", F.classic_file(os.path.join(golden_dir, "c1.cobs_classic"))),
                     ("c1.cobs_compact", _read_compact(os.path.join(golden_dir, "c1.cobs_compact")))):
        _anchor(oracle, os.path.join(golden_dir, name), fb, [q, oracle.random_sequence(90, 3)])


def test_anchored_on_the_oracle_on_a_hand_built_compact_file(tmp_path, oracle):
    """three hashes, a last sub-index that is partly filled, planted documents (so that some positions are widely held)"""
    src = oracle.random_sequence(400, 77)
    path = cases.make_compact(str(tmp_path / "h.cobs_compact"), 150, 8, [701, 1009, 853], 3, 25, 1, 0.5, 6,
                              planted={3: 1.0, 70: 1.0, 149: 0.9}, query=src)
    fb = _read_compact(path)
    _anchor(oracle, path, fb, [src[:120], oracle.random_sequence(60, 9)])
    assert V.prevalence(fb, src[:120], 0).min() >= 2          # documents 3 and 70 hold every k-mer of the source


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("prevalence_cpu")
    src = oracle.random_sequence(1500, 77)
    a = cases.make_classic(str(d / "a.cobs_classic"), 120, 1009, 3, 31, 1, 0.3, 5, planted={0: 1.0, 77: 0.9}, query=src)
    b = cases.make_compact(str(d / "b.cobs_compact"), 200, 8, [701, 1009, 853, 977], 1, 25, 1, 0.3, 6,
                           planted={3: 1.0, 199: 0.85}, query=src)
    return src, [F.classic_file(a), _read_compact(b)]


def test_identities_for_every_z(files):
    """the sum over the positions is the sum over the real documents of the scores; a position's count is the number of
    hits whose positions bit is set; a shard's slot ranges add up"""
    src, fbs = files
    queries = [src[:31 + 7], src[10:10 + 95], src[:700]]
    for z in (0, 1, 3, 7):
        for q in queries:
            for fi, fb in enumerate(fbs):
                prev = V.prevalence(fb, q, z)
                docs = fb.doc_of_slot()
                assert len(prev) == fb.positions(q, z)
                assert int(prev.sum()) == int(fb.scores(q, z)[docs >= 0].sum())
                per_doc = np.array([P.positions(fbs, q, z, fi, int(d)) for d in docs[docs >= 0]])
                np.testing.assert_array_equal(prev, per_doc.sum(axis=0))
                cut = [0, 40, 41, fb.slots]
                parts = [V.prevalence(fb, q, z, "error", a, b - a) for a, b in zip(cut, cut[1:])]
                np.testing.assert_array_equal(prev, np.sum(parts, axis=0))
    offs, counts = V.segments(fbs, queries, 3)
    assert len(offs) == len(queries) * 2 + 1 and int(offs[-1]) == len(counts) and counts.dtype == np.uint32
    np.testing.assert_array_equal(counts[int(offs[3]):int(offs[4])], V.prevalence(fbs[1], queries[1], 3))


def test_padding_slots_never_count(oracle):
    """a file whose padding slots hold bits: the count stops at the last real document"""
    rng = np.random.default_rng(1)
    m = cases.random_bits(rng, (301, 1), 0.9)
    fb = F.FileBits(31, 1, 1, [m], 5)
    q = oracle.random_sequence(100, 4)
    prev = V.prevalence(fb, q, 0)
    assert prev.max() <= 5 and V.windows(fb, q, 0)[:, 5:].any()
    mats = [cases.random_bits(rng, (s, 8), 0.9) for s in (101, 203, 307)]
    fb = F.FileBits(31, 1, 1, mats, 100)                     # the third sub-index is padding only
    assert V.prevalence(fb, q, 0).max() <= 100 and V.windows(fb, q, 0)[:, 128:].any()


def test_invalid_positions_read_zero(files):
    src, fbs = files
    fb = fbs[0]
    k = fb.term_size
    base = src[50:50 + 200]
    for z in (0, 3):
        n = len(base) - k + 1 - z
        for o in (0, 100, len(base) - 1):
            q = I.with_n(base, [o])
            for mode in I.MODES:
                prev = V.prevalence(fb, q, z, mode)
                bad = ~I.position_valid(fb, q, z)
                assert len(prev) == n and bad.any() and not prev[bad].any()
                np.testing.assert_array_equal(prev[~bad], V.prevalence(fb, base, z)[~bad])
                assert int(prev.sum()) == int(I.scores(fb, q, z)[fb.doc_of_slot() >= 0].sum())


def test_symbols_are_exported_bound_and_refuse_null():
    from cobs_amd import _capi
    lib = _capi.load()
    for name, header in (("cobs_gpu_prevalence", "cobs_gpu_batch.h"), ("cobs_gpu_prevalence_ms", "cobs_gpu_diag.h")):
        assert hasattr(lib, name) and name in _capi.SYMBOLS
        assert name + "(" in open(os.path.join(ROOT, "include", header)).read()
        assert name not in open(os.path.join(ROOT, "include", "cobs_gpu.h")).read()
    offs = (C.c_size_t * 1)(0)
    need, bad = C.c_size_t(7), C.c_size_t(0)
    # no handle: an argument error, not a crash (a handle cannot be opened without a device)
    st = lib.cobs_gpu_prevalence(None, None, None, 0, None, 0, offs, C.byref(need), C.byref(bad))
    assert st == _capi.ERR_ARG and b"NULL" in lib.cobs_gpu_last_error()
    assert lib.cobs_gpu_prevalence(None, None, None, 0, None, 0, None, None, None) == _capi.ERR_ARG
    ms = (C.c_double * 3)()
    assert lib.cobs_gpu_prevalence_ms(None, C.byref(ms)) == _capi.ERR_ARG


def test_python_mirrors_exist_with_their_parameter_names():
    import cobs_amd
    import cobs_index
    from cobs_amd import _capi
    assert list(inspect.signature(cobs_amd.Search.prevalence).parameters) == ["self", "queries"]
    assert list(inspect.signature(cobs_amd.Search.prevalence_arrays).parameters) == ["self", "queries"]
    assert cobs_index.Search.prevalence is cobs_amd.Search.prevalence
    assert list(inspect.signature(cobs_amd.Search.search).parameters) == ["self", "query", "threshold", "num_results"]
    with pytest.raises(cobs_amd.CobsGpuError) as e:           # the device list is refused by the mirror
        cobs_amd.MultiSearch.prevalence_arrays(cobs_amd.MultiSearch.__new__(cobs_amd.MultiSearch), [b"ACGT" * 10])
    assert e.value.status == _capi.ERR_UNSUPPORTED and "ask the shards" in str(e.value)


def test_cli_names_the_flag_and_refuses_it_with_a_budget():
    import subprocess
    tool = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")
    r = subprocess.run([tool, "-h"], capture_output=True, text=True, timeout=60)
    assert "--prevalence" in r.stderr
    for extra in (["-d", "0,1"], ["--hbm-budget", "1"], ["--sharded"]):
        r = subprocess.run([tool, "-i", "nowhere.cobs_classic"] + extra + ["--prevalence", "ACGT" * 10], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 1 and "--prevalence: not with" in r.stderr and r.stdout == ""
