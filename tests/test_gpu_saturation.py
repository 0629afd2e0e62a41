"""GPU: every bit-sliced counter at its largest value, with the query length on both sides of every plane boundary
(tests/saturation.py tables the boundaries beside their source lines).  Documents that hold every row score the maximum
whatever k, H or z; a document that misses one term of the query scores just below.  Every comparison is exact: whole
score rows against the oracle, the special documents against the analytic values (tests/test_saturation_cpu.py holds
the numpy checkers against the same values without a GPU).  Every alternate path asserts the witness that it was
taken -- stats()["table_bytes"], Batch.scan_geometry(), the handle's findere -- so a silent fall-back fails."""
import numpy as np
import pytest

from tests import best_check as BC
from tests import coverage_check as CC
from tests import groups_check as G
from tests import prevalence_check as V
from tests import saturation as S
from tests import set_quorum_check as Q
from tests import sets_check as SC
from tests import weighted_check as W
from tests import window_check as B

pytestmark = pytest.mark.gpu

SMALL_T = [T for T in S.PLAIN_T if T <= S.SMALL_T]


@pytest.fixture(scope="module")
def world(tmp_path_factory, oracle):
    return S.build(tmp_path_factory.mktemp("saturation"), S.SMALL_INDEXES + ("narrow_h3", "narrow_k248"))


@pytest.fixture(scope="module")
def oracles(world, oracle):
    return {n: oracle.Index.open(ix.path) for n, ix in world.items()}


def _rows(offs, hits, i=0):
    return [tuple(r) for r in hits.tolist()[int(offs[i]):int(offs[i + 1])]]


def _want_row(ix, oix, q, z):
    """the whole score row: the oracle's at z = 0 (any length), the numpy checker's under findere"""
    return oix.counts(q) if z == 0 else ix.fb.scores(q, z)


def _plain(gpu, oracle, s, ix, oix, T, z=0, mixed=False, paths=True, rank=True, witness=None, run_witness=None):
    """one T-term query through every reader of the planes.  witness(batch) is asked after the first and the last run,
    run_witness(batch, kind) after every run, kind = "rows", "hits" or "topk" """
    def ran(kind):
        if run_witness:
            run_witness(b, kind)

    q = ix.query(T)
    P = T - z
    docs = ix.fb.doc_of_slot()
    special = S.plain_special(ix, T, z)
    queries = S.mixed_batch(ix, T) if mixed else [q]
    at = queries.index(q)
    rows = [_want_row(ix, oix, qq, z) for qq in queries]
    assert {d: int(rows[at][d]) for d in special} == special                # (the reference reaches the analytic values)
    b = gpu.Batch(s)
    b.set_queries(queries)
    b.run(0.0)
    b.sync()
    ran("rows")
    if witness:
        witness(b)
    assert b.counts_device()[1] == S.score_bytes(T), (ix.name, T)
    assert list(b.scored_positions(0)) == [len(qq) - ix.k + 1 - z for qq in queries]
    for i in range(len(queries)):
        assert np.array_equal(b.counts_host(i), rows[i]), (ix.name, T, z, i)
    if paths:
        nb = max(len(qq) for qq in queries) - ix.k + 2
        h = b.score_histogram(nb)
        real = docs >= 0
        want_h = np.zeros(nb, dtype=np.uint64)
        for r in rows:
            want_h += np.bincount(np.asarray(r)[real].astype(np.int64), minlength=nb).astype(np.uint64)
        assert np.array_equal(h, want_h) and int(h[P]) >= len(ix.full)                  # the bin at the top
        for t, bound in zip(S.thresholds(P), (P, P - 1)):
            want = S.hits_of(special, bound)
            assert want == S.hits_of_row(rows[at], docs, bound) and want[0][2] == P and (bound == P or want[-1][2] == P - 1)
            b.run(t)
            b.sync()
            ran("rows")
            assert b.hits_host(at) == want, (ix.name, T, z, t, "rows kept")
            b.run_hits(t)
            b.sync()
            ran("hits")
            assert b.hits_host(at) == want, (ix.name, T, z, t, "hits only")
        nfull = len(S.hits_of(special, P))
        for k in (1, nfull, nfull + 2):
            b.run_topk(0.0, k, keep_counts=False)
            b.sync()
            ran("topk")
            assert b.hits_host(at, k) == S.hits_of_row(rows[at], docs, 0, k), (ix.name, T, z, k)
        if witness:
            witness(b)
    b.close()
    if rank and z == 0:
        offs, hits = s.search_arrays([q], 0.0, 0)
        oi, od, osc = oracle.search_arrays(oix, q, 0.0, 0)
        assert np.array_equal(hits["doc"], od) and np.array_equal(hits["score"], osc) and len(hits) == ix.num_docs
        top = [d for d in sorted(special) if special[d] == P]
        assert hits["doc"][:len(top)].tolist() == top and (hits["score"][:len(top)] == P).all()      # ties by document id


def _plain_cases():
    """beyond 4096 terms the 12-document index only"""
    return [(name, T) for name in S.SMALL_INDEXES for T in S.PLAIN_T if T <= S.SMALL_T or name == "narrow"]


@pytest.mark.parametrize("name,T", _plain_cases())
def test_plain_scan_at_every_plane_boundary(gpu_lib, oracle, world, oracles, name, T):
    """the default geometry: the query alone and, up to 4096 terms, among short ones"""
    ix = world[name]
    s = gpu_lib.Search(ix.path)
    _plain(gpu_lib, oracle, s, ix, oracles[name], T)
    if T <= S.SMALL_T:
        _plain(gpu_lib, oracle, s, ix, oracles[name], T, mixed=True, rank=False)
    s.close()


def _geometry(want):
    def check(b):
        g = b.scan_geometry()
        assert all(g[k] == v for k, v in want.items()), (g, want)
    return check


@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("tile_w", [8, 64])
@pytest.mark.parametrize("name", ["wide", "compact"])
def test_forced_geometries(gpu_lib, oracle, world, oracles, name, tile_w, waves):
    ix = world[name]
    s = gpu_lib.Search(ix.path)
    s.set_tuning("tile_w", tile_w)
    s.set_tuning("waves", waves)
    s.set_tuning("mq", 0)
    for T in SMALL_T:
        _plain(gpu_lib, oracle, s, ix, oracles[name], T, rank=False,
               witness=_geometry({"tile_w": tile_w, "waves": waves, "mq": False, "lds_staged": False}))
    s.close()


@pytest.mark.parametrize("name", ["wide", "compact"])
def test_multi_query_form(gpu_lib, oracle, world, oracles, name):
    """mq = 1 forces the multi-query form, which exists up to 12 planes (kernels.hpp: scan_has_multi_query): 4095 terms
    take it, 4096 (16 planes) must not"""
    ix = world[name]
    s = gpu_lib.Search(ix.path)
    s.set_tuning("mq", 1)
    s.set_tuning("tile_w", 8)
    for T in SMALL_T:
        for mixed in (False, True):
            _plain(gpu_lib, oracle, s, ix, oracles[name], T, mixed=mixed, rank=False,
                   witness=_geometry({"mq": S.planes_for(T) <= 12, "tile_w": 8}))
    s.close()


SELF_HASH_ENTRIES = 2048 + 64          # kernels.hip: kSelfHashEntries, the row indices a work-group's LDS array holds


@pytest.mark.parametrize("name", ["wide", "compact", "narrow"])
def test_self_hashing_scan(gpu_lib, oracle, world, oracles, name):
    """scan_self_hash = 2: wherever the shape allows, i.e. while (sub-indexes of a tile) x (blocks + 1) x 8 row indices fit
    the LDS array (kernels.hpp: scan_self_hash_fits).  A classic file is one sub-index: every T up to 1024 takes the form.
    The compact file's sub-indexes are one 16-byte chunk wide; the tile width is forced to 8 here, so a tile lies in all
    three whatever the default geometry becomes: up to 256 terms take the form, 1023 and 1024 (3 x 129 x 8 = 3096 entries)
    stay on K1's table -- asserted too, so that a moved limit shows.  Every run of the pass is asked: score rows, rows with
    a threshold and the hits-only pass take the form (no table bytes); a top-k pass keeps K1 by design (geometry.cpp:
    pass_self_hash) and must show its table"""
    ix = world[name]
    s = gpu_lib.Search(ix.path)
    s.set_tuning("scan_self_hash", 2)
    s.set_tuning("mq", 0)
    if name == "compact":
        s.set_tuning("tile_w", 8)
    tile_pages = min(len(ix.spec.sigs), 8)           # kernels.hpp: scan_tile_pages for one-chunk sub-indexes (classic: 1)
    took = 0
    for T in [T for T in SMALL_T if T <= 1024]:
        expect = tile_pages * ((T + 7) // 8 + 1) * 8 <= SELF_HASH_ENTRIES
        assert expect or (name == "compact" and T >= 1023)
        seen = []

        def each_run(b, kind):
            assert (b.scan_geometry()["tile_w"] == 8 or name != "compact") and not b.scan_geometry()["mq"]
            assert (b.stats()["table_bytes"] == 0) == (expect and kind != "topk"), (name, T, kind)
            seen.append(kind)

        before = s.self_hash_passes
        _plain(gpu_lib, oracle, s, ix, oracles[name], T, rank=False, run_witness=each_run)
        assert seen == ["rows", "rows", "hits", "rows", "hits", "topk", "topk", "topk"]
        assert s.self_hash_passes == before + (5 if expect else 0)
        took += expect
    assert took == (4 if name == "compact" else 6)
    s.close()


@pytest.mark.parametrize("waves", [2, 4])
def test_lds_staged_at_1023(gpu_lib, oracle, world, oracles, waves):
    for name in ("wide", "compact"):
        ix = world[name]
        s = gpu_lib.Search(ix.path)
        s.set_tuning("lds_staged", 1)
        s.set_tuning("waves", waves)
        s.set_tuning("mq", 0)
        _plain(gpu_lib, oracle, s, ix, oracles[name], 1023, rank=False, witness=_geometry({"lds_staged": True, "waves": waves}))
        s.close()


@pytest.mark.parametrize("name", S.SMALL_INDEXES)
def test_wide_row_indices(gpu_lib, oracle, world, oracles, name, monkeypatch):
    """COBS_GPU_IDX64 (read when a handle is opened): 64-bit row indices, a table twice as large"""
    ix = world[name]
    plain = gpu_lib.Search(ix.path)
    monkeypatch.setenv("COBS_GPU_IDX64", "1")
    s = gpu_lib.Search(ix.path)
    monkeypatch.delenv("COBS_GPU_IDX64")
    for T in SMALL_T:
        sizes = []
        for h in (plain, s):
            b = gpu_lib.Batch(h)
            b.set_queries([ix.query(T)])
            sizes.append(b.stats()["table_bytes"])
            b.close()
        assert sizes[1] == 2 * sizes[0] > 0
        _plain(gpu_lib, oracle, s, ix, oracles[name], T)
    s.close()
    plain.close()


def test_three_hash_functions(gpu_lib, oracle, world, oracles):
    """H = 3, the generic-H row loop: a table three entries per term"""
    ix, one = world["narrow_h3"], world["narrow"]
    s, s1 = gpu_lib.Search(ix.path), gpu_lib.Search(one.path)
    assert ix.num_hashes == 3 and s.info(0).num_hashes == 3
    for T in SMALL_T:
        sizes = []
        for h, x in ((s1, one), (s, ix)):
            b = gpu_lib.Batch(h)
            b.set_queries([x.query(T)])
            sizes.append(b.stats()["table_bytes"])
            b.close()
        assert sizes[1] == 3 * sizes[0] > 0
        _plain(gpu_lib, oracle, s, ix, oracles["narrow_h3"], T)
        _plain(gpu_lib, oracle, s, ix, oracles["narrow_h3"], T, mixed=True, rank=False)
    s.close()
    s1.close()


@pytest.mark.parametrize("name,T", _plain_cases())
def test_findere(gpu_lib, oracle, world, oracles, name, T):
    """z = 3: T terms are T - 3 positions, the planes follow the terms"""
    ix = world[name]
    s = gpu_lib.Search(ix.path, findere=S.FINDERE_Z)
    assert s.findere == S.FINDERE_Z
    _plain(gpu_lib, oracle, s, ix, oracles[name], T, z=S.FINDERE_Z)
    if T <= S.SMALL_T:
        _plain(gpu_lib, oracle, s, ix, oracles[name], T, z=S.FINDERE_Z, mixed=True)
    s.close()


# ---- B: the scans with their own counters -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weighted(tmp_path_factory, oracle):
    return S.weighted_file(tmp_path_factory.mktemp("saturation_weighted"))


@pytest.mark.parametrize("n", S.WEIGHTED_N)
def test_weighted_top_score(gpu_lib, weighted, n):
    """every position weighs 15: the one full document scores 15 n, the largest value of the planes chosen for n"""
    path, fb = weighted
    for z in (0, S.FINDERE_Z):
        s = gpu_lib.Search(path, findere=z)
        q = S.weighted_query(n, z)
        assert (s.position_weights(q)[0] == 15).all() and len(s.position_weights(q)[0]) == n
        for t in (0.0, 1.0, S.thresholds(15 * n)[1]):
            total, want = S.weighted_expected(n, t)
            offs, hits, tw = s.search_weighted_arrays([q], t, 0)
            assert int(tw[0, 0]) == total and _rows(offs, hits) == want, (n, z, t)
            if n <= S.WEIGHTED_CHECKED:
                assert want == W.results([fb], q, z, t, 0)
        s.close()


def _coverage_cases():
    out = [("narrow", L, z) for L in S.COVERAGE_L for z in (0, S.FINDERE_Z)]
    out += [(name, L, z) for name in ("wide", "compact") for L in S.COVERAGE_L if L <= S.SMALL_T for z in (0, S.FINDERE_Z)]
    return out + [("narrow_k248", L, 7) for L in (4095, 4096)]


@pytest.mark.parametrize("name,L,z", _coverage_cases())
def test_coverage_of_a_full_document(gpu_lib, world, name, L, z):
    ix = world[name]
    q = ix.src[:L]
    special = S.coverage_special(ix, L, z)
    s = gpu_lib.Search(ix.path, findere=z)
    tabs = CC.tables([ix.fb], q, z)
    for t, bound in ((0.0, 0),) + tuple(zip(S.thresholds(L), (L, L - 1))):
        got = _rows(*s.search_coverage_arrays([q], t, 0))
        assert got == CC.results_from(tabs, t, 0), (name, L, z, t)
        # (a set position covers k + z bases: random documents reach full coverage too, so the list is the checker's and
        # the special documents are looked up in it)
        by_doc = {d: c for (_f, d, c) in got}
        assert {d: by_doc.get(d) for d in special if special[d] >= max(bound, 1)} == {d: v for d, v in special.items() if v >= max(bound, 1)}
        if bound:
            assert (ix.near0 in by_doc) == (bound < L)           # one base short: in at L - 1, out at L
            assert ix.empty not in by_doc
        else:
            assert len(got) == ix.num_docs                       # every real document, the padding slots never
    s.close()


def _window_cases():
    out = []
    for Wd in S.WINDOW_W:
        for n in S.window_positions(Wd):
            out += [(name, Wd, n) for name in S.SMALL_INDEXES if n <= S.SMALL_T or name == "narrow"]
    return out


@pytest.mark.parametrize("seg", [None, "13"])
@pytest.mark.parametrize("name,Wd,n", _window_cases())
def test_best_window_of_a_full_document(gpu_lib, world, monkeypatch, name, Wd, n, seg):
    ix = world[name]
    if seg is None:
        monkeypatch.delenv("COBS_GPU_WINDOW_SEG", raising=False)
    else:
        monkeypatch.setenv("COBS_GPU_WINDOW_SEG", seg)
    q = ix.query(n)
    w = min(Wd, n)
    special = S.window_special(ix, Wd, n)
    s = gpu_lib.Search(ix.path)
    tabs = B.tables([ix.fb], q, 0, Wd)
    for t, bound in zip((0.0,) + S.thresholds(w), (1, w, w - 1)):
        offs, hits = s.search_window_arrays([q], Wd, t, 0)
        got = _rows(offs, hits)
        assert got == B.results_from(tabs, t, 0), (name, Wd, n, seg, t)
        by_doc = {d: c for (_f, d, c) in got}
        assert {d: by_doc.get(d) for d, v in special.items() if v >= bound} == {d: v for d, v in special.items() if v >= bound}
        assert by_doc[ix.full[0]] == w and (t == 0.0 or min(by_doc.values()) >= bound)
        # the best window over a hit's positions is its score: every hit of every list, the t = 0 list with its random
        # and empty documents included
        bo, bits = s.hit_positions([q], offs, hits)
        for h, (_f, _d, sc) in enumerate(got):
            assert gpu_lib.best_window(bits[int(bo[h]):int(bo[h + 1])], n, Wd)[0] == sc, (name, Wd, n, seg, t, h)
    s.close()


# ---- C: counters across documents and members -------------------------------------------------------------------------------
@pytest.mark.parametrize("members", S.GROUP_MEMBERS)
def test_group_totals_and_best_of_group(gpu_lib, world, members):
    """255-term members are a pass of u8 rows; the totals of 2, 257 and 258 of them in a full document are 510, 2^16 - 1
    and 65 790 (the sums are 32-bit: a group whose total could reach 2^32 is refused, groups.cpp, so there is no boundary
    above 2^16 to put a case on).  Best-of-group: every member ties in a full document, and the first one is chosen."""
    ix = world["narrow"]
    queries = S.group_queries(ix, members)
    offsets = [0, members]
    total = members * S.GROUP_TERMS
    s = gpu_lib.Search(ix.path)
    for t in (0.0, 1.0):
        offs, hits, _pos = s.search_groups_arrays(queries, offsets, t, 1.0, 0)
        got = _rows(offs, hits)
        assert got == G.results([ix.fb], queries, offsets, 0, "error", t, 1.0, 0)[0][0], (members, t)
        assert [r for r in got if r[1] in ix.full] == [(0, d, total, members) for d in ix.full]
        got = _rows(*s.search_best_arrays(queries, offsets, t, 0))
        assert got == BC.results([ix.fb], queries, offsets, 0, "error", t, 0)[0], (members, t)
        assert [r for r in got if r[1] in ix.full] == [(0, d, 0, S.GROUP_TERMS, S.GROUP_TERMS, members) for d in ix.full]
    s.close()


def _all_ones_file(tmp_path, num_docs, sig=257):
    from oracle import construct as C
    from tests import cases
    from tests import findere_check as F
    m = cases.mask_padding_docs(np.full((sig, (num_docs + 7) // 8), 0xFF, dtype=np.uint8), 0, num_docs)
    path = str(tmp_path / ("ones_%d.cobs_classic" % num_docs))
    C.write_classic(path, S.K, 1, ["doc_%05d" % i for i in range(num_docs)], sig, 1, m)
    return path, F.FileBits(S.K, 1, 1, [m], num_docs)


@pytest.mark.parametrize("num_docs", S.SET_SIZES + (65535, 65536))
def test_prevalence_of_rows_everybody_holds(gpu_lib, oracle, tmp_path, num_docs):
    """every document holds every row: the count of every position is D (an 8 KiB row at 65 536 documents).  The counts are
    32-bit (prevalence_kernels.hip) and a file holds fewer than 2^32 documents, so the accumulator itself has no boundary
    a test can reach; the sides chosen are where a narrower partial count would wrap -- 255 / 256 / 257 for a byte, 65 535 /
    65 536 for 16 bits -- and where the row grows past one wave's 64 chunks"""
    path, fb = _all_ones_file(tmp_path, num_docs)
    s = gpu_lib.Search(path)
    for z in (0, S.FINDERE_Z):
        s.set_findere(z)
        q = oracle.random_sequence(300 + z, 77)
        offs, counts = s.prevalence_arrays([q])
        assert len(counts) == 270 and (counts == num_docs).all(), (num_docs, z)
        if num_docs <= 257:
            assert np.array_equal(counts, V.prevalence(fb, q, z))
    s.close()


@pytest.mark.parametrize("size", S.SET_SIZES)
def test_set_counts_of_rows_everybody_holds(gpu_lib, oracle, tmp_path, size):
    """one set of `size` members and one of 3, all of them holding every row: any = all = core = P for both, the member
    count per position is the set size, and a quorum of 1.0 or just above (m - 1) / m keeps the set.  The member counts of
    sets.cpp and set_quorum.cpp are 32-bit and a set has fewer than 2^32 members: no boundary of the accumulator is
    reachable, so the set sizes 255 / 256 / 257 stand where a byte-wide partial count would wrap"""
    import math
    path, fb = _all_ones_file(tmp_path, size + 3)
    labels = np.array([0] * size + [1] * 3, dtype=np.int64)
    s = gpu_lib.Search(path)
    s.set_doc_sets(labels, 0)
    q = oracle.random_sequence(330, 78)
    P = 300
    for rank_by in ("any", "all"):
        got = _rows(*s.search_sets_arrays([q], 1.0, rank_by, 0))
        assert got == SC.results([fb], [labels], q, 0, 1.0, rank_by, 0) and [r[2:] for r in got] == [(P, P), (P, P)]
    just_above = math.nextafter((size - 1) / size, 1.0)
    assert Q.need(just_above, size) == size and Q.need(1.0, size) == size
    for quorum in (1.0, just_above):
        got = _rows(*s.search_sets_quorum_arrays([q], quorum, 1.0, 0))
        assert got == Q.results([fb], [labels], q, 0, quorum, 1.0, 0) and [r[2:] for r in got] == [(P, P), (P, P)]
    offs, counts = s.set_prevalence_arrays([q])
    assert counts.tolist() == [size] * P + [3] * P
    s.close()


@pytest.mark.parametrize("sig", S.FLUSH_SIGS)
def test_fill_and_shared_bits_around_the_flush(gpu_lib, tmp_path, sig):
    """kFillPlanes = kSimPlanes = 12: a lane flushes its planes after 4088 rows.  Documents with every row set count
    exactly sig bits, and share sig bits with each other, on both sides of one and of two flushes"""
    from tests import fill_check
    from tests import similarity_check
    path, fb = _all_ones_file(tmp_path, 40, sig)
    s = gpu_lib.Search(path)
    bits = s.doc_bits(0)
    assert np.array_equal(bits, fill_check.bits_of_file(path)) and (bits[:40] == sig).all() and not bits[40:].any()
    refs = [0, 7, 39]
    shared = s.doc_shared_bits(refs, 0)
    want = similarity_check.shared_of_file(path, refs)
    for got, w in zip(shared, want):
        assert np.array_equal(got, w) and (got[:40] == sig).all()
    s.close()
