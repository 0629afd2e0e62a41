"""CPU: the positions checker (tests/positions_check.py) against the findere checker and the oracle, the word packing,
and what the new entry point and its Python mirrors promise without a device.

A hit's positions are the per-term presence of its query in ONE document, windowed by findere z; their popcount is the
score the search reports for the hit.  At z = 0 that is the COBS count, which oracle.Index.counts computes independently."""
import ctypes as C
import inspect
import os
import struct

import numpy as np
import pytest

from tests import cases
from tests import findere_check as F
from tests import positions_check as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read_compact(path):
    """a compact index file -> FileBits (the layout oracle/construct.py's compact_header writes)"""
    raw = open(path, "rb").read()
    assert raw[:18] == b"COBS:COMPACT_INDEX"
    _ver, k, canon, nparams, ndocs, page_size = struct.unpack_from("<IIBIIQ", raw, 18)
    pos = 18 + struct.calcsize("<IIBIIQ")
    params = [struct.unpack_from("<QQ", raw, pos + 16 * i) for i in range(nparams)]
    pos += 16 * nparams
    for _ in range(ndocs):
        pos = raw.index(b"\n", pos) + 1
    pos += (page_size - ((pos + 13) % page_size)) % page_size
    assert raw[pos:pos + 13] == b"COMPACT_INDEX"
    pos += 13
    mats = []
    for s, _h in params:
        mats.append(np.frombuffer(raw, dtype=np.uint8, count=s * page_size, offset=pos).reshape(s, page_size))
        pos += s * page_size
    assert pos == len(raw) and len({h for _s, h in params}) == 1
    return F.FileBits(k, canon, params[0][1], mats, ndocs)


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("positions_cpu")
    src = oracle.random_sequence(1500, 77)
    a = cases.make_classic(str(d / "a.cobs_classic"), 120, 1009, 3, 31, 1, 0.3, 5, planted={0: 1.0, 77: 0.9}, query=src)
    b = cases.make_compact(str(d / "b.cobs_compact"), 200, 8, [701, 1009, 853, 977], 1, 25, 1, 0.3, 6,
                           planted={3: 1.0, 199: 0.85}, query=src)
    return src, [F.classic_file(a), _read_compact(b)]


def test_popcount_of_the_positions_is_the_search_score(files):
    src, fbs = files
    queries = [src[:31 + 7], src[10:10 + 95], src[200:200 + 31 + 127], src[:1030]]
    for z in (0, 1, 3, 7):
        for q in queries:
            for t in (0.0, 0.8, 1.0):
                res = F.results(fbs, q, z, t, 0)
                assert t or len(res) == 320
                for f, d, sc in res:
                    pos = P.positions(fbs, q, z, f, d)
                    assert pos.dtype == bool and len(pos) == len(q) - fbs[f].term_size + 1 - z
                    assert int(pos.sum()) == sc == P.popcount(P.pack(pos))
    # the window by hand: positions at z are the AND of z + 1 shifted copies of the z = 0 positions
    q = queries[2]
    p0 = P.positions(fbs, q, 0, 0, 77)
    for z in (1, 3, 7):
        n = len(p0) - z
        want = np.all([p0[j:j + n] for j in range(z + 1)], axis=0)
        np.testing.assert_array_equal(P.positions(fbs, q, z, 0, 77), want)


def test_positions_at_z0_are_the_oracle_counts_on_the_golden_files(golden_dir, oracle):
    q = b"AGTCAACGCTAAGGCATTTCCCCCCTGCCTCCTGCCTGCTGCCAAGCCCT"
    for name, fb in (("c1.cobs_classic", F.classic_file(os.path.join(golden_dir, "c1.cobs_classic"))),
                     ("c1.cobs_compact", _read_compact(os.path.join(golden_dir, "c1.cobs_compact")))):
        ix = oracle.Index.open(os.path.join(golden_dir, name))
        for qq in (q, oracle.random_sequence(200, 3)):
            counts = ix.counts(qq)
            docs = fb.doc_of_slot()
            assert (docs >= 0).sum() == fb.num_docs
            for slot in np.nonzero(docs >= 0)[0]:
                assert int(P.positions([fb], qq, 0, 0, int(docs[slot])).sum()) == int(counts[slot]), (name, slot)
            assert F.results([fb], qq, 0) == [(f, d, s) for (f, d, _n, s) in oracle.search(ix, qq)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128])
def test_packing_round_trip(n):
    from cobs_amd.search import unpack_positions
    rng = np.random.default_rng(n)
    for pos in (rng.random(n) < 0.5, np.ones(n, dtype=bool), np.zeros(n, dtype=bool)):
        w = P.pack(pos)
        assert w.dtype == np.uint64 and len(w) == (n + 63) // 64
        np.testing.assert_array_equal(P.unpack(w, n), pos)
        np.testing.assert_array_equal(unpack_positions(w, n), pos)         # the product's own unpacking agrees
        assert P.popcount(w) == int(pos.sum())
        for p in range(n):
            assert bool((int(w[p // 64]) >> (p % 64)) & 1) == bool(pos[p])
        assert int(w[-1]) >> ((n - 1) % 64 + 1) == 0                       # bits >= n of the last word are zero


def test_symbol_is_exported_bound_and_refuses_null():
    from cobs_amd import _capi
    lib = _capi.load()
    assert hasattr(lib, "cobs_gpu_hit_positions") and "cobs_gpu_hit_positions" in _capi.SYMBOLS
    text = open(os.path.join(ROOT, "include", "cobs_gpu_batch.h")).read()
    assert "cobs_gpu_hit_positions(" in text
    assert "cobs_gpu_hit_positions" not in open(os.path.join(ROOT, "include", "cobs_gpu.h")).read()
    offs = (C.c_size_t * 2)(0, 0)
    boffs = (C.c_size_t * 1)(0)
    need, bad = C.c_size_t(7), C.c_size_t(0)
    # no handle: an argument error, not a crash (a handle cannot be opened without a device)
    st = lib.cobs_gpu_hit_positions(None, None, None, 0, None, offs, None, 0, boffs, C.byref(need), C.byref(bad))
    assert st == _capi.ERR_ARG and b"NULL" in lib.cobs_gpu_last_error()
    st = lib.cobs_gpu_hit_positions(None, None, None, 0, None, None, None, 0, None, None, None)
    assert st == _capi.ERR_ARG
    ms = (C.c_double * 3)()
    assert lib.cobs_gpu_positions_ms(None, C.byref(ms)) == _capi.ERR_ARG


def test_python_mirrors_exist_with_their_parameter_names():
    import cobs_amd
    import cobs_index
    from cobs_amd import _capi
    assert list(inspect.signature(cobs_amd.Search.hit_positions).parameters) == ["self", "queries", "offsets", "hits"]
    sig = inspect.signature(cobs_amd.Search.search_positions)
    assert list(sig.parameters) == ["self", "queries", "threshold", "num_results"]
    assert sig.parameters["threshold"].default == 0.0 and sig.parameters["num_results"].default == 0
    assert cobs_index.Search.search_positions is cobs_amd.Search.search_positions
    # Search.search keeps the reference's signature
    assert list(inspect.signature(cobs_amd.Search.search).parameters) == ["self", "query", "threshold", "num_results"]
    s = cobs_amd.Search(None, _handle=C.c_void_p())           # no handle: the library refuses
    with pytest.raises(cobs_amd.CobsGpuError) as e:
        s.hit_positions([b"ACGT" * 10], [0, 1], np.zeros(1, dtype=cobs_amd.Search.HIT_DTYPE))
    assert e.value.status == _capi.ERR_ARG
    with pytest.raises(ValueError):
        s.hit_positions([b"ACGT" * 10], [0], np.zeros(0, dtype=cobs_amd.Search.HIT_DTYPE))


def test_cli_names_the_flag():
    import subprocess
    tool = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")
    r = subprocess.run([tool, "-h"], capture_output=True, text=True, timeout=60)
    assert "--positions" in r.stderr
