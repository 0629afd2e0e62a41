"""CPU: the document-similarity checker on a hand-written matrix, cobs_gpu_jaccard_estimate through the loaded library
against the checker's restatement, its exact cases and refusals, the C surface of cobs_gpu_doc_shared_bits, and the
estimate against the true Jaccard index of documents with a planted share of common k-mers."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import similarity_check as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_checker_on_a_hand_written_matrix():
    # 5 rows x 16 documents; byte 0 = documents 0..7 (bit d), byte 1 = documents 8..15
    m = np.array([[0b00000111, 0b10000000],      # row 0: documents 0 1 2 15
                  [0b00000101, 0b10000001],      # row 1: 0 2 8 15
                  [0b00000010, 0b00000001],      # row 2: 1 8
                  [0b10000001, 0b00000000],      # row 3: 0 7
                  [0b00000100, 0b10000000]],     # row 4: 2 15
                 dtype=np.uint8)
    got = SC.shared_of_mat(m, [0, 2, 15, 3])
    assert got.dtype == np.uint64 and got.shape == (4, 16)
    #                 d: 0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15
    assert got[0].tolist() == [3, 1, 2, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 2]      # document 0: rows 0 1 3
    assert got[1].tolist() == [2, 1, 3, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 3]      # document 2: rows 0 1 4
    assert got[2].tolist() == [2, 1, 3, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 3]      # document 15: rows 0 1 4 (a copy of 2)
    assert got[3].tolist() == [0] * 16                                              # document 3: no bit
    ix = dict(mats=[m], sigs=[5], num_hashes=1, names=["d%d" % i for i in range(16)])
    assert [r.tolist() for r in SC.shared_of_index(ix, [15, 0])] == [got[2].tolist(), got[0].tolist()]
    # two sub-indexes of one byte each: document 9 is slot 1 of sub-index 1
    ix2 = dict(mats=[m[:, :1], m[:, 1:]], sigs=[5, 5], num_hashes=1, names=["d%d" % i for i in range(16)])
    assert SC.shared_of_index(ix2, [8])[0].tolist() == [2, 0, 0, 0, 0, 0, 0, 1]
    assert SC.shared_of_index(ix2, [2])[0].tolist() == [2, 1, 3, 0, 0, 0, 0, 0]
    # the estimate: documents 2 and 15 are copies (Jaccard 1), 0 and 2 share 2 of 4 union bits
    assert SC.estimate(5, 1, 3, 3, 3)[:4] == (1.0, 1.0, 1.0, 1.0)
    assert SC.estimate(5, 1, 3, 3, 2)[0] == 0.5
    assert [r[0] for r in SC.similar(ix, 2)][:2] == ["d15", "d0"]
    assert [(a, b) for a, b, *_ in SC.all_pairs(ix, 0.99)] == [(2, 15)]


def _lib_estimate(lib, sig, H, a, b, c):
    out = (C.c_double * 5)()
    st = lib.cobs_gpu_jaccard_estimate(sig, H, a, b, c, C.byref(out))
    return st, tuple(out)


def test_jaccard_estimate_of_the_library_is_the_definition():
    """over a grid of (sig, H, a, b, c): within 1e-12 * max(1, n(t_or)) of the restatement -- a handful of double
    operations, each under one ulp, scaled by the union because n_inter is a difference of terms of that size"""
    from cobs_amd import _capi
    import cobs_amd
    assert "cobs_gpu_jaccard_estimate" in _capi.SYMBOLS
    lib = _capi.load()
    n = 0
    for sig in (1, 2, 64, 1000, 4099, 1 << 20, (1 << 40) + 7):
        for H in (1, 2, 3, 7):
            vals = sorted(v for v in {0, 1, 2, sig // 3, sig // 2, sig - 1, sig} if 0 <= v <= sig)
            for a in vals:
                for b in vals:
                    lo = max(0, a + b - sig)                    # two columns of sig rows share at least this much
                    for c in sorted({lo, min(a, b), (lo + min(a, b)) // 2, min(lo + 1, min(a, b))}):
                        st, got = _lib_estimate(lib, sig, H, a, b, c)
                        assert st == _capi.OK, (sig, H, a, b, c)
                        want = SC.estimate(sig, H, a, b, c)
                        if a + b - c == sig:
                            assert got[0] == want[0] and all(math.isnan(v) for v in got[1:]), (sig, H, a, b, c)
                        else:
                            tol = 1e-12 * max(1.0, SC.n_of(a + b - c, sig, H))
                            assert all(abs(g - w) <= tol for g, w in zip(got, want)), (sig, H, a, b, c, got, want)
                        assert cobs_amd.jaccard_estimate(sig, H, a, b, c)[0] == got[0]
                        n += 1
    assert n > 1500              # (the grid did not collapse)


def test_jaccard_estimate_exact_cases():
    from cobs_amd import _capi
    lib = _capi.load()
    for sig, H, a in ((1000, 1, 200), (4099, 3, 1), (1 << 30, 2, 12345678), (77, 1, 76)):
        st, got = _lib_estimate(lib, sig, H, a, a, a)
        assert st == _capi.OK and got[:4] == (1.0, 1.0, 1.0, 1.0) and got[4] == SC.n_of(a, sig, H)
    # independent filters: 1 - t_or / S = (1 - a / S)(1 - b / S), so n(a) + n(b) = n(t_or)
    st, got = _lib_estimate(lib, 1000, 1, 200, 300, 60)
    assert st == _capi.OK and abs(got[1]) <= 1e-12 and got[0] == 60 / 440
    # empty documents: every denominator is zero
    assert _lib_estimate(lib, 1000, 1, 0, 0, 0) == (_capi.OK, (0.0, 0.0, 0.0, 0.0, 0.0))
    st, got = _lib_estimate(lib, 1000, 1, 0, 10, 0)
    assert st == _capi.OK and got[:4] == (0.0, 0.0, 0.0, 0.0)
    # a subset: containment of the smaller in the larger is 1 (n_inter is a difference: to rounding)
    st, got = _lib_estimate(lib, 100000, 1, 1000, 5000, 1000)
    assert st == _capi.OK and abs(got[2] - 1.0) <= 1e-12 and got[2] <= 1.0 and 0.15 < got[1] < 0.25 and 0.15 < got[3] < 0.25
    # the saturated filter
    for a, b, c in ((1000, 1000, 1000), (600, 500, 100), (1000, 0, 0)):
        st, got = _lib_estimate(lib, 1000, 2, a, b, c)
        assert st == _capi.OK and got[0] == c / 1000 and all(math.isnan(v) for v in got[1:])


def test_jaccard_estimate_refusals():
    from cobs_amd import _capi
    import cobs_amd
    lib = _capi.load()
    for args in ((0, 1, 0, 0, 0), (1000, 0, 10, 10, 5), (1000, 1, 10, 20, 11), (1000, 1, 20, 10, 11), (1000, 1, 1001, 10, 5),
                 (1000, 1, 10, 1001, 5)):
        st, _ = _lib_estimate(lib, *args)
        assert st == _capi.ERR_ARG, args
        with pytest.raises(cobs_amd.CobsGpuError) as e:
            cobs_amd.jaccard_estimate(*args)
        assert e.value.status == _capi.ERR_ARG
    assert lib.cobs_gpu_jaccard_estimate(1000, 1, 10, 10, 5, None) == _capi.ERR_ARG


def test_surface():
    from cobs_amd import _capi
    import cobs_amd
    inc = os.path.join(ROOT, "include")
    batch_h = open(os.path.join(inc, "cobs_gpu_batch.h")).read()
    diag_h = open(os.path.join(inc, "cobs_gpu_diag.h")).read()
    assert "cobs_gpu_doc_shared_bits(" in batch_h and "cobs_gpu_jaccard_estimate(" in batch_h
    assert "cobs_gpu_similarity_ms(" in diag_h and "#define COBS_GPU_ABI_VERSION 2" in open(os.path.join(inc, "cobs_gpu.h")).read()
    for name in ("cobs_gpu_doc_shared_bits", "cobs_gpu_jaccard_estimate", "cobs_gpu_similarity_ms"):
        assert name in _capi.SYMBOLS
    lib = _capi.load()
    need = C.c_size_t(77)
    refs = (C.c_uint32 * 1)(0)
    assert lib.cobs_gpu_doc_shared_bits(None, 0, refs, 1, None, None, 0, C.byref(need)) == _capi.ERR_ARG and need.value == 0
    ms = (C.c_double * 4)()
    assert lib.cobs_gpu_similarity_ms(None, C.byref(ms)) == _capi.ERR_ARG
    for m in ("doc_shared_bits", "similar_documents", "similarity_ms"):
        assert hasattr(cobs_amd.Search, m)
    assert "jaccard_estimate" in cobs_amd.__all__
    # the kernel constants the GPU test names
    hpp = open(os.path.join(ROOT, "cobs_amd", "csrc", "similarity_kernels.hpp")).read()
    assert "constexpr int kSimRefs = 8;" in hpp and "constexpr int kSimPlanes = 12;" in hpp
    assert "constexpr uint32_t kSimBlockRows = 8;" in hpp
    assert "constexpr uint32_t kSimFlushBlocks = ((1u << kSimPlanes) - 1u) / kSimBlockRows;" in hpp


PLANTED_TOLERANCE = 0.0204               # Jaccard: twice the worst deviation measured (test_estimate_against_planted_truth)
PLANTED_TOLERANCE_CONTAINMENT = 0.0283   # containment, either way: twice the worst deviation measured


def planted_deviation(construct, seed, n_common=3000, n_own=3000, H=3):
    """|estimated - true| Jaccard of two documents of n_common + n_own random k-mers (their 64-bit hashes), n_common of
    them common to both, in a classic matrix sized as `cobs classic-construct` sizes it (false positive rate 0.3)"""
    rng = np.random.default_rng(seed)
    h = rng.integers(0, 1 << 63, size=(n_common + 2 * n_own, H), dtype=np.uint64)
    a = construct.Doc("a", "a", 0, n_common + n_own, h[:n_common + n_own])
    b = construct.Doc("b", "b", 0, n_common + n_own, np.concatenate([h[:n_common], h[n_common + n_own:]]))
    sig = construct.calc_signature_size(n_common + n_own, H, 0.3)
    m = construct.build_matrix([a, b], sig, 1)
    sh = SC.shared_of_mat(m, [0])[0]
    bits_b = int(SC.shared_of_mat(m, [1])[0][1])
    est = SC.estimate(sig, H, int(sh[0]), bits_b, int(sh[1]))
    true = n_common / (n_common + 2 * n_own)
    return abs(est[1] - true), est, true


def test_estimate_against_planted_truth(construct):
    """two documents of 6000 k-mers that share 3000 (true Jaccard 1/3), H = 3, S for a false positive rate of 0.3: over
    the seeds 0..19 the worst deviation from the truth, measured on the CPU through the checker only, was 0.010177 for the estimated
    Jaccard and 0.014129 for the two containments (true value 1/2); each tolerance is twice its figure: 0.0204 and 0.0283"""
    dev, est, true = planted_deviation(construct, 100)          # a seed outside the measured ones
    assert dev <= PLANTED_TOLERANCE, (dev, est, true)
    assert abs(est[2] - 0.5) <= PLANTED_TOLERANCE_CONTAINMENT and abs(est[3] - 0.5) <= PLANTED_TOLERANCE_CONTAINMENT
