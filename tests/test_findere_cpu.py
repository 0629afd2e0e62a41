"""CPU: the findere checker against the oracle, and the findere entry points' argument checks that need no device.

findere (Robidou & Peterlongo, SPIRE 2021): with z > 0 a query position scores in a document only when its z + 1
consecutive k-mers are all present there.  tests/findere_check.py restates the windowed score in numpy; at z = 0 it
must be the COBS count, which oracle.Index.counts computes independently."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import cases
from tests import findere_check as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compact_file(path, num_docs, page_size, sigs, num_hashes, term_size, seed):
    rng = np.random.default_rng(seed)
    page_docs = 8 * page_size
    mats = [cases.mask_padding_docs(cases.random_bits(rng, (s, page_size), 0.3), p * page_docs, num_docs)
            for p, s in enumerate(sigs)]
    from oracle import construct as K
    names = ["doc_%05d" % i for i in range(num_docs)]
    K.write_compact(path, term_size, 1, page_size, [(s, num_hashes) for s in sigs], names, mats)
    return F.FileBits(term_size, 1, num_hashes, mats, num_docs)


@pytest.mark.parametrize("kind,num_hashes,term_size", [("classic", 1, 31), ("classic", 3, 31), ("classic", 2, 20),
                                                       ("compact", 1, 31), ("compact", 3, 25)])
def test_checker_at_z0_is_the_oracle_count(oracle, tmp_path, kind, num_hashes, term_size):
    if kind == "classic":
        p = cases.make_classic(str(tmp_path / "a.cobs_classic"), 300, 1009, num_hashes, term_size, 1, 0.3, 5)
        fb = F.classic_file(p)
    else:
        p = str(tmp_path / "a.cobs_compact")
        fb = _compact_file(p, 300, 16, [701, 1009, 853], num_hashes, term_size, 6)
    ix = oracle.Index.open(p)
    for n, length in enumerate([term_size, term_size + 1, 40, 77, 150, 300]):
        q = oracle.random_sequence(length, 100 + n)
        want = ix.counts(q)
        got = F.counts([fb], q, 0)
        assert got.shape == want.shape
        np.testing.assert_array_equal(got, want)
        # a window never scores more than a single term: the findere score is monotone in z
        prev = got
        for z in (1, 2, 3, 7):
            if length - term_size + 1 - z < 1:
                break
            cur = F.counts([fb], q, z)
            assert np.all(cur <= prev)
            prev = cur


def test_checker_windows_by_hand():
    """presence patterns with known window counts: the restatement itself, on a hand-made presence matrix"""
    class Fixed(F.FileBits):
        def __init__(self, P):
            self._P = P
            self.slots = P.shape[1]

        def presence(self, q):
            return self._P

    P = np.array([[1, 1, 0, 1], [1, 1, 1, 1], [1, 0, 1, 1], [0, 1, 1, 1], [1, 1, 1, 1]], dtype=bool)   # [T = 5, 4 docs]
    f = Fixed(P)
    assert F.counts([f], b"", 0).tolist() == [4, 4, 4, 5]
    assert F.counts([f], b"", 1).tolist() == [2, 2, 3, 4]
    assert F.counts([f], b"", 2).tolist() == [1, 0, 2, 3]
    assert F.counts([f], b"", 4).tolist() == [0, 0, 0, 1]


def test_abi_argument_checks_without_a_device():
    from cobs_amd import _capi
    lib = _capi.load()
    z = C.c_uint32(99)
    assert lib.cobs_gpu_set_findere(None, 0) == _capi.ERR_ARG
    assert lib.cobs_gpu_set_findere(None, 3) == _capi.ERR_ARG
    assert lib.cobs_gpu_set_findere(None, 8) == _capi.ERR_ARG
    assert lib.cobs_gpu_get_findere(None, C.byref(z)) == _capi.ERR_ARG
    assert lib.cobs_gpu_multi_set_findere(None, 1) == _capi.ERR_ARG
    assert lib.cobs_gpu_multi_get_findere(None, C.byref(z)) == _capi.ERR_ARG
    assert z.value == 99


def test_python_surface_without_a_device():
    import inspect

    import cobs_amd
    from cobs_amd import _capi
    # appended keywords: every existing positional call keeps its meaning
    ps = list(inspect.signature(cobs_amd.Search.__init__).parameters)
    assert ps[-1] == "findere" and ps[:7] == ["self", "path", "device", "shard_rank", "shard_count", "hbm_budget",
                                             "shard_mode"]
    assert list(inspect.signature(cobs_amd.Search.synthetic).parameters)[-1] == "findere"
    assert inspect.signature(cobs_amd.Search.__init__).parameters["findere"].default == 0
    s = cobs_amd.Search(None, _handle=C.c_void_p())          # no handle: the library refuses, Python checks z first
    with pytest.raises(ValueError):
        s.set_findere(8)
    with pytest.raises(ValueError):
        s.set_findere(-1)
    with pytest.raises(cobs_amd.CobsGpuError) as e:
        s.set_findere(2)
    assert e.value.status == _capi.ERR_ARG
    with pytest.raises(cobs_amd.CobsGpuError):
        _ = s.findere


def test_cli_flag_is_named_and_checked():
    tool = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")
    if not os.path.exists(tool):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cobs_amd", "csrc"), "-j8"], stdout=subprocess.DEVNULL)
    r = subprocess.run([tool, "-h"], capture_output=True, text=True, timeout=60)
    assert "--findere Z" in r.stderr
    for bad in ("8", "-1", "x"):
        r = subprocess.run([tool, "-i", "none.cobs_classic", "--findere", bad, "ACGT"], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 1 and "--findere: 0 .. 7" in r.stderr
