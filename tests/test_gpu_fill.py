"""GPU: per-document filter fill (cobs_gpu_doc_bits / Search.doc_bits / doc_fill / doc_fpr / search_adjusted).  Every case
is exact integer equality with the numpy checker (tests/fill_check.py) over ALL slots of the handle."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import construct as K
from tests import cases, fill_check

pytestmark = pytest.mark.gpu

NP = 12                     # the kernel's bit planes (fill_kernels.hpp: kFillPlanes)
BLOCK = 8                   # rows of a carry-save block
SLAB = ((1 << NP) - 1) // BLOCK * BLOCK      # 4088: the longest slab a lane counts


def _write_classic(path, m, num_docs, H=1, k=31):
    names = ["doc_%05d" % i for i in range(num_docs)]
    K.write_classic(path, k, 1, names, m.shape[0], H, m)
    return path


def _matrix(rng, S, D, density):
    row = (D + 7) // 8
    if density >= 1.0:
        m = np.full((S, row), 0xFF, dtype=np.uint8)
    else:
        m = cases.random_bits(rng, (S, row), density)
    return cases.mask_padding_docs(m, 0, D)


ROW_COUNTS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, SLAB - 1, SLAB, SLAB + 1, (1 << NP) - 1, 1 << NP, (1 << NP) + 1,
              3 * (1 << NP) + 5]


@pytest.mark.parametrize("side", ["0", "1"])
def test_row_counts_around_every_boundary(gpu_lib, tmp_path, monkeypatch, side):
    """S around the block size, the slab length and 2^NP, all-ones (every count must equal S: a lost carry or a dropped
    flush shows) and density 0.3.  side=1: one lane walks every row of a slab and the launch aims at ONE work-group, so
    these small matrices reach full-length slabs (4088 rows per lane, the most the planes hold) and slab boundaries;
    side=0: the geometry as shipped (rows side by side in a work-group)."""
    if side == "1":
        monkeypatch.setenv("COBS_GPU_FILL_SIDE", "1")
        monkeypatch.setenv("COBS_GPU_FILL_GROUPS", "1")
    rng = np.random.default_rng(5)
    D = 100
    for S in ROW_COUNTS:
        for density in (1.0, 0.3):
            m = _matrix(rng, S, D, density)
            p = _write_classic(cases.tmp(tmp_path, "s%d_%d.cobs_classic" % (S, int(density * 10))), m, D)
            want = fill_check.bits_of_file(p)
            s = gpu_lib.Search(p)
            got = s.doc_bits()
            assert got.dtype == np.uint64 and np.array_equal(got, want), (S, density)
            if density >= 1.0:
                assert (got[:D] == S).all() and not got[D:].any()
            s.close()


@pytest.mark.parametrize("side", ["0", "1"])
def test_zero_and_one_columns_among_random_ones(gpu_lib, tmp_path, monkeypatch, side):
    if side == "1":
        monkeypatch.setenv("COBS_GPU_FILL_SIDE", "1")
        monkeypatch.setenv("COBS_GPU_FILL_GROUPS", "1")
    rng = np.random.default_rng(6)
    S, D = 3 * (1 << NP) + 5, 300
    m = _matrix(rng, S, D, 0.3)
    m[:, 17] &= np.uint8(~(1 << 3) & 0xFF)          # document 139: no bit
    m[:, 20] |= np.uint8(1 << 6)                    # document 166: every bit
    p = _write_classic(cases.tmp(tmp_path, "zo.cobs_classic"), m, D)
    got = gpu_lib.Search(p).doc_bits()
    assert np.array_equal(got, fill_check.bits_of_file(p))
    assert got[139] == 0 and got[166] == S


@pytest.mark.parametrize("groups,side,D", [("1", None, 100), ("1", None, 1000), ("1", "4", 1000), ("3", None, 5000)])
def test_many_blocks_per_lane_with_rows_side_by_side(gpu_lib, tmp_path, monkeypatch, groups, side, D):
    """the walk the full-size index takes: SEVERAL rows side by side in a work-group (ly > 1) and many blocks per lane,
    i.e. a row stride of 8 x ly over many iterations.  The launch aims at one (or three) work-groups, so a matrix of
    12 293 rows gives a lane 7 (D = 100: ly = 256), 49 (D = 1000: ly = 32), 385 (ly = 4) or 86 (D = 5000: ly = 6, three slabs
    that end inside the matrix) iterations; all-ones and random"""
    monkeypatch.setenv("COBS_GPU_FILL_GROUPS", groups)
    if side:
        monkeypatch.setenv("COBS_GPU_FILL_SIDE", side)
    rng = np.random.default_rng(D)
    S = 3 * (1 << NP) + 5
    for density in (1.0, 0.3):
        p = _write_classic(cases.tmp(tmp_path, "mb%d.cobs_classic" % int(density * 10)), _matrix(rng, S, D, density), D)
        got = gpu_lib.Search(p).doc_bits()
        assert np.array_equal(got, fill_check.bits_of_file(p)), density
        if density >= 1.0:
            assert (got[:D] == S).all() and not got[D:].any()


@pytest.mark.parametrize("D", [1, 7, 8, 9, 127, 128, 129, 1000, 12544])
def test_classic_widths(gpu_lib, tmp_path, D):
    """partial last byte, partial last 16-byte chunk, padded pitch, several column tiles"""
    rng = np.random.default_rng(D)
    S = 333 if D < 2000 else 77
    p = _write_classic(cases.tmp(tmp_path, "w.cobs_classic"), _matrix(rng, S, D, 0.3), D)
    s = gpu_lib.Search(p)
    got = s.doc_bits()
    assert len(got) == s.info(0).counts_size == 8 * ((D + 7) // 8)
    assert np.array_equal(got, fill_check.bits_of_file(p))


@pytest.mark.parametrize("ps", [1, 2, 16, 200])
def test_compact_page_sizes(gpu_lib, tmp_path, ps):
    """sub-indexes of different S_p, a DENSE one between sparse ones (a neighbour's rows or the zero row being counted
    shows), the last page holding padding documents"""
    sigs = [501, 97, 4099, 64, 1300][:5 if ps < 200 else 3]
    dens = [0.05, 1.0, 0.05, 0.9, 0.3]
    P = len(sigs)
    D = (P - 1) * 8 * ps + max(1, 8 * ps - 5)
    rng = np.random.default_rng(ps)
    mats = [cases.mask_padding_docs(np.full((s, ps), 0xFF, dtype=np.uint8) if d >= 1.0 else cases.random_bits(rng, (s, ps), d),
                                    i * 8 * ps, D) for i, (s, d) in enumerate(zip(sigs, dens))]
    p = cases.tmp(tmp_path, "c.cobs_compact")
    K.write_compact(p, 31, 1, ps, [(s, 1) for s in sigs], ["doc_%05d" % i for i in range(D)], mats)
    got = gpu_lib.Search(p).doc_bits()
    want = fill_check.bits_of_file(p)
    assert np.array_equal(got, want)
    assert (got[8 * ps:16 * ps] == 97).all() and not got[D:].any()


def test_hashes_files_and_file_no(gpu_lib, tmp_path):
    pa = cases.make_classic(cases.tmp(tmp_path, "a.cobs_classic"), 300, 700, 3, 31, 1, 0.3, 1)
    pb = cases.make_compact(cases.tmp(tmp_path, "b.cobs_compact"), 700, 32, [400, 900, 650], 1, 20, 1, 0.2, 2)
    s = gpu_lib.Search([pa, pb])
    assert np.array_equal(s.doc_bits(1), fill_check.bits_of_file(pb))
    assert np.array_equal(s.doc_bits(0), fill_check.bits_of_file(pa))
    assert np.array_equal(s.doc_bits(), fill_check.bits_of_file(pa))
    # the mirrors over the real documents
    for f, p in ((0, pa), (1, pb)):
        assert np.array_equal(s.doc_fill(f), np.array(fill_check.doc_fill(p)))
        assert np.allclose(s.doc_fpr(f), np.array(fill_check.doc_fpr(p)), rtol=1e-12, atol=0)
        assert len(s.doc_fill(f)) == s.info(f).num_docs


@pytest.mark.parametrize("kind", ["classic", "compact"])
def test_shards_return_their_slice(gpu_lib, tmp_path, kind):
    if kind == "classic":
        p = cases.make_classic(cases.tmp(tmp_path, "sh.cobs_classic"), 5000, 300, 1, 31, 1, 0.3, 3)
    else:
        p = cases.make_compact(cases.tmp(tmp_path, "sh.cobs_compact"), 6 * 8 * 48 - 7, 48, [300, 900, 200, 1500, 400, 650], 1, 31, 1, 0.3, 4)
    want = fill_check.bits_of_file(p)
    for count in (2, 3, 5):
        for mode in (0, 1, 2):
            pos = 0
            for rank in range(count):
                s = gpu_lib.Search(p, shard_rank=rank, shard_count=count, shard_mode=mode)
                i = s.info(0)
                got = s.doc_bits()
                assert int(i.slot_begin) == pos and len(got) == int(i.slot_count), (count, mode, rank)
                assert np.array_equal(got, want[pos:pos + len(got)]), (count, mode, rank)
                pos += len(got)
                s.close()
            assert pos == len(want)              # the slices tile the file


def _bits_from_rows(s, file_no=0):
    i = s.info(file_no)
    mats = [s.read_rows(file_no, pg, 0, s.signature_size(file_no, pg)) for pg in range(int(i.num_pages))]
    return fill_check.bits_of_mats(mats), mats


def test_synthetic_and_built_in_place(gpu_lib, golden_dir):
    for kind, sigs, D, ps in (("classic", [5003], 1000, 0), ("compact", [1201, 3001, 700], 3 * 8 * 24 - 9, 24)):
        s = gpu_lib.Search.synthetic(kind, sigs, D, page_size=ps, seed=3)
        want, _ = _bits_from_rows(s)
        got = s.doc_bits()
        assert np.array_equal(got, want) and got[:D].all() and not got[D:].any()
    s = gpu_lib.build_search(os.path.join(golden_dir, "fasta"))
    want, _ = _bits_from_rows(s)
    assert np.array_equal(s.doc_bits(), want) and want[:int(s.info(0).num_docs)].all()
    assert np.array_equal(want, fill_check.bits_of_file(os.path.join(golden_dir, "c1.cobs_classic")))


def _budget_case(gpu_lib, oracle, path, budget, layout_check):
    want = fill_check.bits_of_file(path)
    q = oracle.random_sequence(300, 5)
    res = gpu_lib.Search(path)
    s = gpu_lib.Search(path, hbm_budget=budget)
    assert layout_check(s.stream_layout(0)), s.stream_layout(0)
    before = s.search_hits([q], 0.0, 7)
    c_before = s.counts(q)
    assert s.doc_bits_ms()["passes"] == 0
    got = s.doc_bits()
    assert np.array_equal(got, want) and np.array_equal(got, res.doc_bits())
    ms = s.doc_bits_ms()
    ix = fill_check.read_index(path)
    assert ms["passes"] == 1 and ms["bytes_read"] == sum(m.size for m in ix["mats"])       # every row byte read once
    # the stream buffers are left in a state the next pass is correct from
    assert s.search_hits([q], 0.0, 7) == before and np.array_equal(s.counts(q), c_before)
    assert np.array_equal(s.counts(q), res.counts(q))
    assert np.array_equal(s.doc_bits(), want) and s.doc_bits_ms()["passes"] == 1
    return s


@pytest.mark.parametrize("no_pin", ["0", "1"])
def test_hbm_budgets(gpu_lib, oracle, tmp_path, monkeypatch, no_pin):
    if no_pin == "1":
        monkeypatch.setenv("COBS_GPU_NO_PIN", "1")
    ps, D = 96, 5 * 8 * 96 - 11
    # whole-slice chunks and (H = 3) column slices: the 5000-row sub-index exceeds a 200 KB buffer
    pc = cases.make_compact(cases.tmp(tmp_path, "b3.cobs_compact"), D, ps, [700, 1500, 5000, 900, 2600], 3, 31, 1, 0.3, 6)
    _budget_case(gpu_lib, oracle, pc, 400 * 1024, lambda lay: lay[1] > 0 and lay[2] > 1 and lay[3] == 0)
    # row ranges: one sub-index of 12 000 rows x 40 bytes through ~16 KB buffers, about 30 ranges
    monkeypatch.setenv("COBS_GPU_ROW_RANGE_MIN", "48")
    pr = cases.make_classic(cases.tmp(tmp_path, "rr.cobs_classic"), 320, 12000, 1, 31, 1, 0.3, 7)
    _budget_case(gpu_lib, oracle, pr, 32 * 1024, lambda lay: 25 <= lay[3] <= 40)
    # ... and the same file by columns
    monkeypatch.setenv("COBS_GPU_ROW_RANGES", "0")
    pk = cases.make_classic(cases.tmp(tmp_path, "cs.cobs_classic"), 4003, 3001, 1, 31, 1, 0.3, 8)
    _budget_case(gpu_lib, oracle, pk, 600 * 1024, lambda lay: lay[2] > 1 and lay[3] == 0)
    monkeypatch.delenv("COBS_GPU_ROW_RANGES")
    # resident and streamed chunks mixed in one file: small stream buffers, the rest of the budget keeps slices
    monkeypatch.setenv("COBS_GPU_STREAM_BUF_KIB", "64")
    pm = cases.make_compact(cases.tmp(tmp_path, "mx.cobs_compact"), D, ps, [700, 1500, 5000, 900, 2600], 1, 31, 1, 0.3, 9)
    s = _budget_case(gpu_lib, oracle, pm, 700 * 1024, lambda lay: lay[0] > 0 and (lay[1] + lay[2] + lay[3]) > 0)
    ms = s.doc_bits_ms()
    assert ms["kernel_ms"] > 0 and ms["pcie_ms"] > 0


def test_budgeted_synthetic(gpu_lib):
    sigs = [4001, 6007, 9001, 12007]
    ps, D = 256, 4 * 8 * 256 - 100
    a = gpu_lib.Search.synthetic("compact", sigs, D, page_size=ps, seed=9)
    b = gpu_lib.Search.synthetic("compact", sigs, D, page_size=ps, seed=9, hbm_budget=5 * 1024 * 1024)
    want, _ = _bits_from_rows(a)
    assert np.array_equal(a.doc_bits(), want) and np.array_equal(b.doc_bits(), want)


def test_cache_and_plant(gpu_lib, oracle):
    s = gpu_lib.Search.synthetic("compact", [2001, 3001], 2 * 8 * 16 - 3, page_size=16, seed=4)
    a = s.doc_bits()
    assert s.doc_bits_ms()["passes"] == 1
    assert np.array_equal(s.doc_bits(), a) and s.doc_bits_ms()["passes"] == 1       # served from the cache
    text = oracle.random_sequence(800, 3)
    s.plant(text, [3, 200], 1000)
    b = s.doc_bits()
    want, _ = _bits_from_rows(s)
    assert s.doc_bits_ms()["passes"] == 2
    assert np.array_equal(b, want) and not np.array_equal(a, b)
    changed = np.nonzero(a != b)[0].tolist()
    assert changed == [3, 200] and (b[changed] > a[changed]).all()


def test_refusals(gpu_lib, tmp_path):
    from cobs_amd import _capi
    p = cases.make_classic(cases.tmp(tmp_path, "r.cobs_classic"), 100, 50, 1, 31, 1, 0.3, 1)
    s = gpu_lib.Search(p)
    lib = _capi.load()
    need = C.c_size_t(0)
    buf = (C.c_uint64 * 8)()
    assert lib.cobs_gpu_doc_bits(s._h, 0, buf, 8, C.byref(need)) == _capi.ERR_CAPACITY
    assert need.value == 104 and s.doc_bits_ms()["passes"] == 0                       # nothing ran
    assert lib.cobs_gpu_doc_bits(s._h, 0, None, 0, C.byref(need)) == _capi.ERR_CAPACITY and need.value == 104
    assert lib.cobs_gpu_doc_bits(s._h, 1, buf, 8, C.byref(need)) == _capi.ERR_ARG and need.value == 0
    assert s.doc_bits_ms()["passes"] == 0
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        s.doc_bits(5)
    assert e.value.status == _capi.ERR_ARG
    m = gpu_lib.MultiSearch(p, [0])
    with pytest.raises(gpu_lib.CobsGpuError) as e:
        m.doc_bits()
    assert e.value.status == _capi.ERR_UNSUPPORTED
    assert np.array_equal(m.shard(0).doc_bits(), fill_check.bits_of_file(p))
    m.close()


@pytest.mark.parametrize("z,mode", [(0, "error"), (3, "error"), (0, "skip"), (2, "skip")])
def test_search_adjusted_orders_a_dense_and_a_sparse_document(gpu_lib, oracle, z, mode):
    """two documents hold the same share of the query's k-mers; one of them is a saturated-looking filter (dense), the
    other sparse: equal raw evidence is worth less in the dense one, and the mirror says so exactly as the checker does"""
    S, D = 20011, 64
    s = gpu_lib.Search.synthetic("classic", [S], D, seed=11, findere=z, invalid_bases=mode)
    q = oracle.random_sequence(400, 21)
    noise = [oracle.random_sequence(3000, 100 + i) for i in range(12)]
    for t in noise:                      # document 5 becomes dense
        s.plant(t, [5], 1000, salt=1)
        s.plant(t, [6], 1000, salt=1)    # ... and so does document 6
    s.plant(q, [5, 9], 1000, salt=2)     # 5 (dense) and 9 (sparse) hold every k-mer of the query: equal raw scores
    s.plant(q, [6, 10], 500, salt=3)     # 6 (dense) and 10 (sparse) hold about half of them
    query = q if mode == "error" else q[:100] + b"N" + q[101:]
    res = {r.doc_name: r for r in s.search_adjusted(query, 0.0, 0)}
    plain = {r.doc_name: r.score for r in s.search(query)}
    bits, _ = _bits_from_rows(s)
    assert np.array_equal(s.doc_bits(), bits)
    k = 31
    T = len(query) - k + 1
    P = T - z
    if mode == "skip":                   # valid positions: those whose k + z characters miss the N
        P = sum(1 for p in range(T - z) if not (p <= 100 < p + k + z))
    names = [s.doc_name(0, d) for d in range(D)]
    for d in range(D):
        r = res[names[d]]
        assert r.score == plain[names[d]]
        want = fill_check.adjust(r.score, P, int(bits[d]), S, 1, z)
        assert abs(r.expected_fp - want["expected_fp"]) <= 1e-12 * abs(want["expected_fp"])
        assert abs(r.adjusted - want["adjusted"]) <= 1e-12 * abs(want["adjusted"])
    dense, sparse = res[names[5]], res[names[9]]
    assert dense.score == sparse.score == P
    assert bits[5] > bits[9] and dense.expected_fp > sparse.expected_fp
    # equal raw scores, full evidence: both estimate P; an unrelated document estimates about 0
    assert abs(dense.adjusted - P) < 1e-6 and abs(sparse.adjusted - P) < 1e-6
    # partial evidence: the checker's order of the dense and the sparse document is the mirror's
    w6 = fill_check.adjust(res[names[6]].score, P, int(bits[6]), S, 1, z)["adjusted"]
    w10 = fill_check.adjust(res[names[10]].score, P, int(bits[10]), S, 1, z)["adjusted"]
    assert w6 != w10 and (res[names[6]].adjusted < res[names[10]].adjusted) == (w6 < w10)
    assert res[names[6]].expected_fp > res[names[10]].expected_fp
    others = [res[names[d]].adjusted for d in range(D) if d not in (5, 6, 9, 10)]
    assert max(others) < 0.25 * P
