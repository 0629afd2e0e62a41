"""CPU: the invalid-bases checker (tests/invalid_check.py) against the oracle, the conditions the GPU fixtures of
tests/test_gpu_invalid_bases.py rely on, and the entry points' argument checks that need no device.

A k-mer that holds a character outside ACGT is absent from every document (`miss`), and its positions also leave the
threshold's denominator (`skip`).  Cutting a query at its invalid characters gives all-ACGT segments: the `miss` counts
of the query are the sum of the plain counts of its segments, which the oracle (z = 0) and findere_check (z > 0) compute
without knowing about the policy."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import cases
from tests import findere_check as F
from tests import invalid_check as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _queries(oracle, k, z=0):
    src = oracle.random_sequence(600, 31)
    qs = V.placement_queries(src, k, z)
    rng = np.random.default_rng(7)
    for i in range(6):                               # random Ns, dense and sparse
        q = bytearray(oracle.random_sequence(int(rng.integers(k + z, 400)), 200 + i))
        for o in rng.integers(0, len(q), size=int(rng.integers(1, 6))):
            q[int(o)] = ord("N")
        qs.append(bytes(q))
    return qs


@pytest.mark.parametrize("kind,num_hashes,k", [("classic", 1, 31), ("classic", 3, 31), ("classic", 2, 20), ("compact", 3, 25)])
def test_miss_counts_are_the_sum_over_acgt_segments(oracle, tmp_path, kind, num_hashes, k):
    if kind == "classic":
        p = cases.make_classic(str(tmp_path / "a.cobs_classic"), 300, 1009, num_hashes, k, 1, 0.3, 5)
        fb = F.classic_file(p)
    else:
        from tests import test_gpu_invalid_bases as G
        p = str(tmp_path / "a.cobs_compact")
        fb = G._compact(p, 300, 16, [701, 1009, 853], num_hashes, k, 6)
    ix = oracle.Index.open(p)
    seen_zero = seen_full = False
    for q in _queries(oracle, k):
        want = np.zeros(fb.slots, dtype=np.uint32)
        v = 0
        for seg in V.segments(fb, q, k):
            want += ix.counts(seg)
            v += len(seg) - k + 1
        np.testing.assert_array_equal(V.counts([fb], q, 0), want)
        assert V.valid_positions(fb, q, 0) == v
        seen_zero |= v == 0
        seen_full |= v == len(q) - k + 1
        for z in (1, 3):
            if len(q) < k + z:
                continue
            want = np.zeros(fb.slots, dtype=np.uint32)
            v = 0
            for seg in V.segments(fb, q, k + z):
                want += F.counts([fb], seg, z)
                v += len(seg) - k + 1 - z
            np.testing.assert_array_equal(V.counts([fb], q, z), want)
            assert V.valid_positions(fb, q, z) == v
            assert int(V.counts([fb], q, z).max()) <= v
    assert seen_zero and seen_full


def test_threshold_rules():
    class Fixed:
        term_size, canonicalize, num_hashes = 4, 1, 1

        def positions(self, q, z):
            return len(q) - 4 + 1 - z

    fb = Fixed()
    q = b"ACGTACGTNACGTACG"                           # T = 13; terms 5 .. 8 hold the N: V = 9
    assert V.valid_positions(fb, q, 0) == 9
    assert V.valid_positions(fb, q, 2) == 3 + 2       # windows of 6 characters
    assert V.threshold("miss", 0.8, fb, q, 0) == 11 and V.threshold("skip", 0.8, fb, q, 0) == 8
    assert V.threshold("miss", 1.0, fb, q, 0) == 13 and V.threshold("skip", 1.0, fb, q, 0) == 9
    assert V.threshold("miss", 0.0, fb, q, 0) == 0 and V.threshold("skip", 0.0, fb, q, 0) == 0
    alln = b"N" * 16
    assert V.valid_positions(fb, alln, 0) == 0
    assert V.threshold("skip", 0.8, fb, alln, 0) == 1 and V.threshold("skip", 0.0, fb, alln, 0) == 0
    assert V.threshold("miss", 0.8, fb, alln, 0) == 11
    # lower case and other letters are invalid; a file that does not canonicalize takes every byte
    assert V.valid_positions(fb, b"ACGTaCGTACGT", 0) == 5
    fb.canonicalize = 0
    assert V.valid_positions(fb, b"ACGTaCGTNNNN", 0) == 9


def test_gpu_fixture_conditions(oracle, tmp_path):
    """what tests/test_gpu_invalid_bases.py takes for granted about its queries"""
    from tests import test_gpu_invalid_bases as G
    d = G.build_files(str(tmp_path), oracle)
    src = d["src"]
    for name, z in (("c1", 0), ("c3", 0), ("p1", 0), ("p3", 0), ("c2k20", 0), ("c1", 1), ("p3", 3)):
        fb = d[name][1]
        qs = G.batch_queries(src, fb.term_size, z)
        vs = [V.valid_positions(fb, q, z) for q in qs]
        assert 0 in vs
        assert any(v == fb.positions(q, z) for v, q in zip(vs, qs))
        assert any(0 < v < fb.positions(q, z) for v, q in zip(vs, qs))
        assert all(len(q) >= fb.term_size + z for q in qs)
    # miss versus skip: the planted 1.0 document holds every valid k-mer of the query; two Ns take V below 0.8 T
    fb = d["c1"][1]
    q = G.miss_vs_skip_query(src)
    T = len(q) - 30
    v = V.valid_positions(fb, q, 0)
    assert len(q) == 230 and v < 0.8 * T and v == T - 62
    doc = G.PLANTED_FULL
    assert int(V.scores(fb, q, 0)[doc]) == v
    assert (0, doc, v) in V.results([fb], q, 0, "skip", 0.8)
    assert doc not in [h[1] for h in V.results([fb], q, 0, "miss", 0.8)]
    alln = b"N" * 230
    assert V.results([fb], alln, 0, "skip", 0.8) == [] and len(V.results([fb], alln, 0, "skip", 0.0)) == fb.num_docs
    # graph replay: equal lengths, different thresholds under skip
    qa, qb = G.replay_queries(src)
    assert len(qa) == len(qb)
    assert V.threshold("skip", 0.8, fb, qa, 0) != V.threshold("skip", 0.8, fb, qb, 0)
    assert V.results([fb], qa, 0, "skip", 0.8) != V.results([fb], qb, 0, "skip", 0.8)
    # the k = 31 loader: an N directly behind a k-mer, at every alignment of the k-mer's first byte
    for q in G.alignment_queries(src):
        n = q.index(b"N")
        assert n >= 31 and V.run_valid(fb, q, 31)[n - 31] and not V.run_valid(fb, q, 31)[n - 30]


def test_abi_argument_checks_without_a_device():
    from cobs_amd import _capi
    lib = _capi.load()
    m = C.c_uint32(99)
    for mode in (0, 1, 2, 3):
        assert lib.cobs_gpu_set_invalid_bases(None, mode) == _capi.ERR_ARG
        assert lib.cobs_gpu_multi_set_invalid_bases(None, mode) == _capi.ERR_ARG
    assert lib.cobs_gpu_get_invalid_bases(None, C.byref(m)) == _capi.ERR_ARG
    assert lib.cobs_gpu_multi_get_invalid_bases(None, C.byref(m)) == _capi.ERR_ARG
    assert lib.cobs_gpu_batch_scored_positions(None, 0, None) == _capi.ERR_ARG
    assert m.value == 99


def test_python_surface_without_a_device():
    import inspect

    import cobs_amd
    import cobs_index
    from cobs_amd import _capi
    for fn in (cobs_amd.Search.__init__, cobs_amd.Search.synthetic, cobs_amd.MultiSearch.__init__):
        assert inspect.signature(fn).parameters["invalid_bases"].default == "error"
    assert cobs_index.Search is cobs_amd.Search
    assert callable(cobs_amd.Batch.scored_positions)
    s = cobs_amd.Search(None, _handle=C.c_void_p())          # no handle: Python checks the name, the library the handle
    for bad in ("ignore", 3, -1, None):
        with pytest.raises(ValueError):
            s.invalid_bases = bad
    with pytest.raises(cobs_amd.CobsGpuError) as e:
        s.invalid_bases = "skip"
    assert e.value.status == _capi.ERR_ARG
    with pytest.raises(cobs_amd.CobsGpuError):
        _ = s.invalid_bases


def test_cli_flag_is_named_and_checked():
    tool = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")
    r = subprocess.run([tool, "-h"], capture_output=True, text=True, timeout=60)
    assert "--invalid-bases error|miss|skip" in r.stderr
    for bad in ("ignore", "2", ""):
        r = subprocess.run([tool, "-i", "none.cobs_classic", "--invalid-bases", bad, "ACGT"], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 1 and "--invalid-bases: error, miss or skip" in r.stderr
