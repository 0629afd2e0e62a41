"""GPU: shared filter bits of documents (cobs_gpu_doc_shared_bits / Search.doc_shared_bits / similar_documents).  Every
case is exact integer equality with the numpy checker (tests/similarity_check.py) over ALL cells of every reference."""
import ctypes as C

import numpy as np
import pytest

from oracle import construct as K
from tests import cases, fill_check
from tests import similarity_check as SC

pytestmark = pytest.mark.gpu

M = 8                       # references of one panel (similarity_kernels.hpp: kSimRefs)
NP = 12                     # the kernel's bit planes per reference (kSimPlanes)
BLOCK = 8                   # rows of a carry-save block (kSimBlockRows)
SLAB = ((1 << NP) - 1) // BLOCK * BLOCK      # 4088: the longest slab a lane counts (kSimFlushBlocks blocks)


def _write_classic(path, m, num_docs, H=1, k=31):
    K.write_classic(path, k, 1, ["doc_%05d" % i for i in range(num_docs)], m.shape[0], H, m)
    return path


def _matrix(rng, S, D, density):
    row = (D + 7) // 8
    if density >= 1.0:
        m = np.full((S, row), 0xFF, dtype=np.uint8)
    else:
        m = cases.random_bits(rng, (S, row), density)
    return cases.mask_padding_docs(m, 0, D)


def _knobs(monkeypatch, side):
    if side == "1":
        monkeypatch.setenv("COBS_GPU_SIM_SIDE", "1")
        monkeypatch.setenv("COBS_GPU_SIM_GROUPS", "1")


def _same(got, want):
    return len(got) == len(want) and all(g.dtype == np.uint64 and np.array_equal(g, w) for g, w in zip(got, want))


def _raw(s, refs, file_no=0, cap=None, fill=0):
    """the C call as it is -> (status, offsets, shared, needed); cap None: sized by a first call"""
    from cobs_amd import _capi
    lib = _capi.load()
    r = np.ascontiguousarray(refs, dtype=np.uint32)
    offs = np.full(len(r) + 1, 0xABCD, dtype=np.uint64)
    need = C.c_size_t(12345)
    rp, op = r.ctypes.data_as(C.POINTER(C.c_uint32)), offs.ctypes.data_as(C.POINTER(C.c_uint64))
    if cap is None:
        st = lib.cobs_gpu_doc_shared_bits(s._h, file_no, rp, len(r), op, None, 0, C.byref(need))
        if st != _capi.OK:
            return st, offs, None, need.value
        cap = need.value
    out = np.full(cap, fill, dtype=np.uint64)
    st = lib.cobs_gpu_doc_shared_bits(s._h, file_no, rp, len(r), op, out.ctypes.data_as(C.POINTER(C.c_uint64)), cap, C.byref(need))
    return st, offs, out, need.value


ROW_COUNTS = [1, 2, 7, 8, 9, 63, 64, 65, SLAB - 1, SLAB, SLAB + 1, (1 << NP) - 1, 1 << NP, (1 << NP) + 1, 3 * (1 << NP) + 5]


@pytest.mark.parametrize("side", ["0", "1"])
def test_row_counts_around_every_boundary(gpu_lib, tmp_path, monkeypatch, side):
    """S around the block size, the slab length and 2^NP, all-ones (every cell of a real document must equal S: a lost
    carry or a dropped flush shows) and density 0.3.  side=1: one lane walks every row of a slab and the launch aims at ONE
    work-group, so these small matrices reach full-length slabs (4088 rows per lane) and slab boundaries; side=0: the
    geometry as shipped"""
    _knobs(monkeypatch, side)
    rng = np.random.default_rng(5)
    D, refs = 100, [0, 99, 37]
    for S in ROW_COUNTS:
        for density in (1.0, 0.3):
            m = _matrix(rng, S, D, density)
            p = _write_classic(cases.tmp(tmp_path, "s%d_%d.cobs_classic" % (S, int(density * 10))), m, D)
            s = gpu_lib.Search(p)
            got = s.doc_shared_bits(refs)
            assert _same(got, SC.shared_of_mat(m, refs)), (S, density)
            if density >= 1.0:
                assert all((g[:D] == S).all() and not g[D:].any() for g in got)
            s.close()


@pytest.mark.parametrize("side", ["0", "1"])
def test_wide_rows_around_the_slab_boundaries(gpu_lib, tmp_path, monkeypatch, side):
    """rows of 64 words and more take the kernel variant whose waves lie in one row (the reference bytes in scalar
    registers): D = 2100 is two column tiles, the second with two live lanes"""
    _knobs(monkeypatch, side)
    rng = np.random.default_rng(15)
    D, refs = 2100, [0, 2099, 2047, 2048, 1001]
    for S in (9, SLAB, SLAB + 1, 2 * SLAB + 3):
        for density in (1.0, 0.3):
            m = _matrix(rng, S, D, density)
            p = _write_classic(cases.tmp(tmp_path, "w%d_%d.cobs_classic" % (S, int(density * 10))), m, D)
            s = gpu_lib.Search(p)
            got = s.doc_shared_bits(refs)
            assert _same(got, SC.shared_of_mat(m, refs)), (S, density)
            if density >= 1.0:
                assert all((g[:D] == S).all() and not g[D:].any() for g in got)
            s.close()


@pytest.mark.parametrize("D", [1, 7, 8, 9, 127, 128, 129, 1000, 12544])
def test_classic_widths(gpu_lib, tmp_path, D):
    """partial last byte, partial last word, padded pitch, several column tiles; references: the first, the last, a bit 7
    of a byte, and documents 127 / 128 where D allows"""
    rng = np.random.default_rng(D)
    S = 333 if D < 2000 else 77
    m = _matrix(rng, S, D, 0.3)
    p = _write_classic(cases.tmp(tmp_path, "w.cobs_classic"), m, D)
    refs = sorted({r for r in (0, D - 1, 7, 127, 128) if r < D})
    s = gpu_lib.Search(p)
    got = s.doc_shared_bits(refs)
    assert all(len(g) == s.info(0).counts_size == 8 * ((D + 7) // 8) for g in got)
    assert _same(got, SC.shared_of_mat(m, refs))


@pytest.mark.parametrize("n_refs", [1, M - 1, M, M + 1, 2 * M + 3])
def test_panels(gpu_lib, tmp_path, n_refs):
    """references beyond one panel, with duplicates and in descending order; one sweep per panel of M"""
    rng = np.random.default_rng(n_refs)
    S, D = 1500, 300
    m = _matrix(rng, S, D, 0.3)
    p = _write_classic(cases.tmp(tmp_path, "p.cobs_classic"), m, D)
    refs = [int(r) for r in rng.integers(0, D, size=n_refs)]
    if n_refs > 2:
        refs[-1] = refs[0]                          # a duplicate
    refs = sorted(refs, reverse=True)
    s = gpu_lib.Search(p)
    assert s.similarity_ms()["sweeps"] == 0
    got = s.doc_shared_bits(refs)
    assert _same(got, SC.shared_of_mat(m, refs))
    ms = s.similarity_ms()
    assert ms["sweeps"] == (n_refs + M - 1) // M and ms["bytes_read"] == ms["sweeps"] * m.size
    assert ms["sweep_ms"] > 0 and ms["extract_ms"] > 0
    assert s.similarity_ms()["sweeps"] == 0         # reset on read


def test_planted_structure(gpu_lib, tmp_path):
    rng = np.random.default_rng(21)
    S, D = 5003, 300
    cols = (rng.random((S, 8 * ((D + 7) // 8))) < 0.3).astype(np.uint8)
    cols[:, D:] = 0
    cols[:, 10] = cols[:, 3]                        # a copy
    cols[:, 21] &= 1 - cols[:, 20]                  # a disjoint pair
    cols[:, 30] &= cols[:, 31]                      # a subset
    cols[:, 40] = 0                                 # an all-zero document
    cols[:, 41] = 1                                 # an all-ones document
    m = np.packbits(cols, axis=1, bitorder="little")
    p = _write_classic(cases.tmp(tmp_path, "pl.cobs_classic"), m, D)
    s = gpu_lib.Search(p)
    bits = s.doc_bits()
    got = np.stack(s.doc_shared_bits(list(range(D))))
    assert np.array_equal(got, SC.shared_of_mat(m, range(D)))
    assert got[3, 10] == bits[3] == bits[10] and np.array_equal(got[3], got[10])
    assert got[20, 21] == 0 and bits[20] and bits[21]
    assert got[30, 31] == bits[30] and bits[30] < bits[31]
    assert not got[40].any() and bits[40] == 0
    assert np.array_equal(got[41], bits)
    assert np.array_equal(got[:, :D], got[:, :D].T)                 # shared(a, b) == shared(b, a)
    assert np.array_equal(np.diagonal(got), bits[:D])               # shared(a, a) == bits(a)
    # the mirror over it
    ix = fill_check.read_index(p)
    for ref, kw in ((3, {}), (30, dict(min_jaccard=0.05)), ("doc_00031", dict(num_results=7)), (41, {}), (40, {})):
        want = SC.similar(ix, ix["names"].index(ref) if isinstance(ref, str) else ref, **kw)
        res = s.similar_documents(ref, **kw)
        assert [(r[0], r[4]) for r in res] == [(w[0], w[4]) for w in want], ref
        for r, w in zip(res, want):
            assert all((a != a and b != b) or abs(a - b) <= 1e-12 for a, b in zip(r[1:4], w[1:4])), (ref, r, w)
    assert s.similar_documents(3)[0][:2] == ("doc_00010", 1.0)
    assert all(r[1] != r[1] for r in s.similar_documents(41))       # the saturated filter estimates nothing


@pytest.mark.parametrize("ps", [1, 2, 16, 200])
def test_compact_page_sizes(gpu_lib, tmp_path, ps):
    """sub-indexes of different S_p, a DENSE one between sparse ones, the last page holding padding documents, references
    from several pages in one call"""
    from cobs_amd import _capi
    sigs = [501, 97, 4099, 64, 1300][:5 if ps < 200 else 3]
    dens = [0.05, 1.0, 0.05, 0.9, 0.3]
    P = len(sigs)
    per = 8 * ps
    D = (P - 1) * per + max(1, per - 5)
    rng = np.random.default_rng(ps)
    mats = [cases.mask_padding_docs(np.full((s, ps), 0xFF, dtype=np.uint8) if d >= 1.0 else cases.random_bits(rng, (s, ps), d),
                                    i * per, D) for i, (s, d) in enumerate(zip(sigs, dens))]
    p = cases.tmp(tmp_path, "c.cobs_compact")
    K.write_compact(p, 31, 1, ps, [(s, 1) for s in sigs], ["doc_%05d" % i for i in range(D)], mats)
    refs = [D - 1, 0, per, 2 * per + min(per - 1, 7), per - 1, (P - 1) * per, per + per // 2, 0]
    s = gpu_lib.Search(p)
    st, offs, out, need = _raw(s, refs)
    assert st == _capi.OK and need == len(refs) * per and offs.tolist() == [i * per for i in range(len(refs) + 1)]
    want = SC.shared_of_file(p, refs)
    assert _same([out[i * per:(i + 1) * per] for i in range(len(refs))], want)
    assert _same(s.doc_shared_bits(refs), want)
    pad = D - (P - 1) * per                         # real documents of the last page
    assert pad < per and not out[:per][pad:].any()  # (refs[0] is a document of the last page: its padding cells are 0)
    assert (out[2 * per:3 * per] == 97).all()       # the dense sub-index: every pair shares every row
    st, _offs, _out, need = _raw(s, [0, D])         # a padding slot is no document
    assert st == _capi.ERR_ARG and need == 0
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.doc_shared_bits([P * per - 1])
    assert e.value.status == _capi.ERR_ARG


def test_files_sequencing_and_memory(gpu_lib, oracle, tmp_path):
    import gc

    import torch
    pa = cases.make_classic(cases.tmp(tmp_path, "a.cobs_classic"), 300, 700, 3, 31, 1, 0.3, 1)
    pb = cases.make_compact(cases.tmp(tmp_path, "b.cobs_compact"), 700, 32, [400, 900, 650], 1, 20, 1, 0.2, 2)
    s = gpu_lib.Search([pa, pb])
    refs_b, refs_a = [699, 3, 256, 300, 511], [299, 0]
    want_b, want_a = SC.shared_of_file(pb, refs_b), SC.shared_of_file(pa, refs_a)
    q = oracle.random_sequence(300, 5)
    hits0 = s.search_hits([q], 0.0, 7)
    assert _same(s.doc_shared_bits(refs_b, 1), want_b)
    bits0 = s.doc_bits(1)
    assert np.array_equal(bits0, fill_check.bits_of_file(pb))
    assert _same(s.doc_shared_bits(refs_b, 1), want_b) and _same(s.doc_shared_bits(refs_a), want_a)
    assert s.search_hits([q], 0.0, 7) == hits0 and np.array_equal(s.doc_bits(1), bits0)
    # 20 more calls on the handle: device memory stays where it is
    gc.collect()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(20):
        assert _same(s.doc_shared_bits(refs_b, 1), want_b)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < (8 << 20), (free0, free1)


def test_refusals(gpu_lib, tmp_path):
    from cobs_amd import _capi
    p = cases.make_classic(cases.tmp(tmp_path, "r.cobs_classic"), 100, 50, 1, 31, 1, 0.3, 1)
    s = gpu_lib.Search(p)
    lib = _capi.load()
    # the sizing call succeeds, fills offsets and runs nothing
    st, offs, _out, need = _raw(s, [5, 6])
    assert st == _capi.OK and need == 208 and offs.tolist() == [0, 104, 208]
    assert s.similarity_ms()["sweeps"] == 1                               # (_raw's second call ran the panel)
    r = (C.c_uint32 * 2)(5, 6)
    need = C.c_size_t(0)
    assert lib.cobs_gpu_doc_shared_bits(s._h, 0, r, 2, None, None, 0, C.byref(need)) == _capi.OK and need.value == 208
    # a buffer that is too small is left alone
    st, offs, out, n = _raw(s, [5, 6], cap=207, fill=0x5A5A)
    assert st == _capi.ERR_CAPACITY and n == 208 and offs.tolist() == [0, 104, 208] and (out == 0x5A5A).all()
    assert lib.cobs_gpu_doc_shared_bits(s._h, 0, r, 2, None, None, 300, C.byref(need)) == _capi.ERR_CAPACITY
    assert s.similarity_ms()["sweeps"] == 0                               # nothing ran
    # arguments
    assert lib.cobs_gpu_doc_shared_bits(s._h, 1, r, 2, None, None, 0, C.byref(need)) == _capi.ERR_ARG and need.value == 0
    assert lib.cobs_gpu_doc_shared_bits(s._h, 0, None, 2, None, None, 0, C.byref(need)) == _capi.ERR_ARG
    assert lib.cobs_gpu_doc_shared_bits(None, 0, r, 2, None, None, 0, C.byref(need)) == _capi.ERR_ARG
    assert _raw(s, [5, 100])[0] == _capi.ERR_ARG                          # slots 100..103 are padding
    st, offs, _out, need = _raw(s, [])
    assert st == _capi.OK and need == 0 and offs.tolist() == [0]
    assert s.doc_shared_bits([]) == []
    assert s.similarity_ms()["sweeps"] == 0
    # handles whose rows or columns are not all resident
    big = cases.make_classic(cases.tmp(tmp_path, "big.cobs_classic"), 5000, 300, 1, 31, 1, 0.3, 3)
    for kw in (dict(hbm_budget=128 * 1024), dict(shard_rank=0, shard_count=2), dict(shard_rank=1, shard_count=2, shard_mode=1)):
        h = gpu_lib.Search(big, **kw)
        with pytest.raises(gpu_lib.CobsGpuError) as e:
            h.doc_shared_bits([5])
        assert e.value.status == _capi.ERR_UNSUPPORTED, kw
        h.close()
    m = gpu_lib.MultiSearch(p, [0])
    for call in (lambda: m.doc_shared_bits([5]), lambda: m.similar_documents(5)):
        with pytest.raises(gpu_lib.CobsGpuError) as e:
            call()
        assert e.value.status == _capi.ERR_UNSUPPORTED
    m.close()
    assert _same(s.doc_shared_bits([5]), SC.shared_of_file(p, [5]))
