"""GPU: the self-hashing scan (tuning key scan_self_hash; kernels.hip: SH) bit for bit against K1's table path on the same
handle, and against the oracle.

With the switch on, a pass over whole resident sub-indexes of 31-mers with one hash function launches no K1: every scan
work-group hashes its query's terms into LDS for the sub-indexes its tile lies in.  The LDS array holds kSelfHashEntries =
2112 row indices, (sub-indexes of a tile) x (blocks of the longest query + a padding block) x 8 of them are needed; a pass
that needs more stays on the table as a whole.  Which path a run took is read from stats()["table_bytes"]: what K1 wrote
for the run, 0 when it did not run.

The compact index has 200-byte pages: 13 sixteen-byte chunks per row, so under W = 8 a tile lies in up to two sub-indexes,
under W = 64 in up to six, and the last tile of a page is partly empty.  The classic index is one sub-index whatever W."""
import numpy as np
import pytest

from tests import kmer_edges

pytestmark = pytest.mark.gpu

SIGS = [64, 1000, 4099, 70001]
PAGE = 200
NDOCS = 4 * 8 * PAGE - 37
CLASSIC_SIG = 1021
CLASSIC_DOCS = 1500
# one term, a full block, a block plus one, a u16 score width, the headline length, the LDS array's limit
LENS = [31, 38, 39, 286, 1030, 2078]
ENTRIES = 2048 + 64
ON, DEFAULT = 2, 1      # scan_self_hash: wherever the shape allows | by the size of K1's table (the shipped default)


def _tile_sub_indexes(kind, tile_w):
    """geometry.cpp: tile_sub_indexes for the two indexes of this file (13 chunks per sub-index, 4 sub-indexes)"""
    if kind == "classic":
        return 1
    return min(4, 1 + (tile_w - 1 + 13 - 1) // 13)


def _expect_self_hash(kind, tile_w, queries):
    blocks = max((len(q) - 31 + 1 + 7) // 8 for q in queries)
    return _tile_sub_indexes(kind, tile_w) * (blocks + 1) * 8 <= ENTRIES


@pytest.fixture(scope="module")
def world(gpu_lib, oracle):
    """both indexes, their oracle twins with the same planted documents, the queries and the oracle's counts (made once)"""
    text = oracle.random_sequence(2300, 4711)
    out = {"text": text}
    for kind, sigs, nd, page in (("compact", SIGS, NDOCS, PAGE), ("classic", [CLASSIC_SIG], CLASSIC_DOCS, 0)):
        s = gpu_lib.Search.synthetic(kind, sigs, nd, page_size=page, term_size=31, canonicalize=1, num_hashes=1, seed=5)
        ix = oracle.Index.synthetic(1 if kind == "compact" else 0, 31, 1, 1, page, sigs, nd, 5)
        docs, keep = [0, 3, nd // 2, nd - 1], [1000, 900, 800, 500]
        s.plant(text, docs, keep, salt=99)
        ix.plant(text, docs, keep, salt=99)
        s.set_tuning("mq", 0)            # one query per work-group: the shape class of the self-hashing scan
        out[kind] = (s, ix)
    # planted text at the front of every length, random text behind the headline query
    import bench
    qs = [text[7:7 + n] for n in LENS] + [bench.make_queries(1, 1000, seed=3)[0]]
    out["queries"] = qs
    out["want"] = {kind: [out[kind][1].counts(q) for q in qs] for kind in ("compact", "classic")}
    return out


def _counts(b, n):
    return [b.counts_host(i) for i in range(n)]


def _run_both(s, b, n, run):
    """the same run with the switch off and on -> (counts off, counts on, table bytes off, table bytes on)"""
    res = []
    for on in (0, 1):
        s.set_tuning("scan_self_hash", ON if on else 0)
        run()
        b.sync()
        res.append((_counts(b, n), b.stats()["table_bytes"]))
    s.set_tuning("scan_self_hash", DEFAULT)
    return res[0][0], res[1][0], res[0][1], res[1][1]


@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("tile_w", [8, 64])
@pytest.mark.parametrize("kind", ["compact", "classic"])
def test_counts_equal_table_path_and_oracle(gpu_lib, world, kind, tile_w, waves):
    s, _ = world[kind]
    qs, want = world["queries"], world["want"][kind]
    s.set_tuning("tile_w", tile_w)
    s.set_tuning("waves", waves)
    took_new_path = 0
    try:
        b = gpu_lib.Batch(s)
        groups = [list(range(len(qs)))] + [[i] for i in range(len(qs))]      # one batch, then every length alone
        for g in groups:
            sub = [qs[i] for i in g]
            b.set_queries(sub)
            off, on, tb_off, tb_on = _run_both(s, b, len(sub), lambda: b.run(0.0))
            assert tb_off > 0
            expect = _expect_self_hash(kind, tile_w, sub)
            assert (tb_on == 0) == expect, (kind, tile_w, waves, g, tb_on)
            took_new_path += expect
            for j, i in enumerate(g):
                assert np.array_equal(on[j], off[j]), (kind, tile_w, waves, g, i)
                assert np.array_equal(on[j], want[i]), (kind, tile_w, waves, g, i)
    finally:
        s.set_tuning("tile_w", 0)
        s.set_tuning("waves", 0)
    assert took_new_path >= 4          # the short lengths at the least, whatever W


def test_query_shorter_than_k_is_refused_alike(gpu_lib, world):
    s, _ = world["compact"]
    b = gpu_lib.Batch(s)
    msgs = []
    for on in (0, 1):
        s.set_tuning("scan_self_hash", ON if on else 0)
        with pytest.raises(gpu_lib.CobsGpuError) as e:
            b.set_queries([world["queries"][3], world["text"][:30]])
        msgs.append(str(e.value))
    s.set_tuning("scan_self_hash", 0)
    assert msgs[0] == msgs[1] and "too short" in msgs[0]


def _with_n(q, positions):
    a = bytearray(q)
    for p in positions:
        a[p] = ord("N")
    return bytes(a)


@pytest.mark.parametrize("kind", ["compact", "classic"])
def test_invalid_bases(gpu_lib, world, kind):
    """N at position 0, in the middle and at the last position: `error` fails sync() with the same query and message on
    both paths (bad query 2 is the first of the pass); `miss` sends such terms to the zero row -- equal counts and equal
    valid positions"""
    nd, sigs, page = (NDOCS, SIGS, PAGE) if kind == "compact" else (CLASSIC_DOCS, [CLASSIC_SIG], 0)
    base = world["queries"][4]
    clean = world["queries"][3]
    qs = [clean, base, _with_n(base, [0]), _with_n(base, [500]), _with_n(base, [len(base) - 1]), _with_n(clean, [0, 100, len(clean) - 1])]
    s, _ = world[kind]
    s.set_tuning("tile_w", 8)
    b = gpu_lib.Batch(s)
    b.set_queries(qs)
    msgs = []
    for on in (0, 1):
        s.set_tuning("scan_self_hash", ON if on else 0)
        b.run(0.0)
        with pytest.raises(gpu_lib.CobsGpuError) as e:
            b.sync()
        msgs.append(str(e.value))
        assert (b.stats()["table_bytes"] == 0) == bool(on)
    s.set_tuning("scan_self_hash", 0)
    s.set_tuning("tile_w", 0)
    assert msgs[0] == msgs[1] and "(query 2)" in msgs[0]

    m = gpu_lib.Search.synthetic(kind, sigs, nd, page_size=page, term_size=31, canonicalize=1, num_hashes=1, seed=5,
                                 invalid_bases="miss")
    m.set_tuning("mq", 0)
    m.set_tuning("tile_w", 8)
    bm = gpu_lib.Batch(m)
    bm.set_queries(qs)
    got = []
    for on in (0, 1):
        m.set_tuning("scan_self_hash", ON if on else 0)
        bm.run(0.0)
        bm.sync()
        assert (bm.stats()["table_bytes"] == 0) == bool(on)
        got.append((_counts(bm, len(qs)), list(bm.scored_positions(0))))
    for i in range(len(qs)):
        assert np.array_equal(got[0][0][i], got[1][0][i]), (kind, i)
    assert got[0][1] == got[1][1]
    assert got[1][1][0] == len(clean) - 30 and got[1][1][2] == 999 and got[1][1][3] == 1000 - 31 and got[1][1][4] == 999


@pytest.mark.parametrize("kind", ["compact", "classic"])
def test_adversarial_canonicalisation(gpu_lib, oracle, world, kind):
    """every deciding position of canonicalize_kmer, both outcomes, the ties and the hand-picked 31-mers as query text"""
    s, ix = world[kind]
    kmers = [k for _, k in kmer_edges.edge_kmers(31, 17)]
    text = b"".join(kmers)
    qs = [text[o:o + 1030] for o in range(0, len(text) - 1030, 997)] + kmers[:40]
    s.set_tuning("tile_w", 8)
    b = gpu_lib.Batch(s)
    b.set_queries(qs)
    off, on, tb_off, tb_on = _run_both(s, b, len(qs), lambda: b.run(0.0))
    s.set_tuning("tile_w", 0)
    assert tb_off > 0 and tb_on == 0
    for i, q in enumerate(qs):
        assert np.array_equal(on[i], off[i]), (kind, i)
        assert np.array_equal(on[i], ix.counts(q)), (kind, i)


@pytest.mark.parametrize("kind", ["compact", "classic"])
def test_thresholded_and_hits_only(gpu_lib, oracle, world, kind):
    """threshold 0.8 over planted documents: run() keeps the score rows and selects, run_hits() selects from the planes"""
    s, ix = world[kind]
    qs = [world["queries"][i] for i in (2, 3, 4, 6)]
    want = [[(0, d, sc) for (_, d, _n, sc) in oracle.search(ix, q, 0.8)] for q in qs]
    # (the planted text saturates the 64-row sub-index for its documents: they pass for every query; most documents do not)
    assert all(2 <= len(w) < 50 for w in want)
    s.set_tuning("tile_w", 8)
    b = gpu_lib.Batch(s)
    b.set_queries(qs)
    for run in (lambda: b.run(0.8), lambda: b.run_hits(0.8)):
        lists = []
        for on in (0, 1):
            s.set_tuning("scan_self_hash", ON if on else 0)
            run()
            b.sync()
            assert (b.stats()["table_bytes"] == 0) == bool(on)
            lists.append([b.hits_host(i, 0) for i in range(len(qs))])
        assert lists[0] == lists[1] == want
    s.set_tuning("scan_self_hash", 0)
    s.set_tuning("tile_w", 0)


def test_fallbacks_keep_k1(gpu_lib, oracle, world):
    """findere, three hash functions, an HBM budget, a top-k run and the multi-query geometry, each with the switch on: K1
    runs and the results are the oracle's"""
    qs = [world["queries"][i] for i in (3, 4)]

    def check(s, ix, run=None, want=None):
        s.set_tuning("scan_self_hash", ON)
        b = gpu_lib.Batch(s)
        b.set_queries(qs)
        (run or (lambda bb: bb.run(0.0)))(b)
        b.sync()
        assert b.stats()["table_bytes"] > 0
        if want is None:
            for i, q in enumerate(qs):
                assert np.array_equal(b.counts_host(i), ix.counts(q))
        return b

    # findere z = 1: the window counts with the switch on are those with it off (tests/test_gpu_findere.py holds the
    # table path to its own restatement), and below the plain counts: a window needs two present terms
    s = gpu_lib.Search.synthetic("compact", SIGS, NDOCS, page_size=PAGE, seed=5, findere=1)
    s.set_tuning("mq", 0)
    b = check(s, None, want=False)
    on = _counts(b, len(qs))
    s.set_tuning("scan_self_hash", 0)
    b.run(0.0)
    b.sync()
    plain = world["want"]["compact"]
    for i, qi in enumerate((3, 4)):
        assert np.array_equal(b.counts_host(i), on[i])
        assert (on[i] <= plain[qi]).all() and on[i].sum() < plain[qi].sum()

    s3 = gpu_lib.Search.synthetic("compact", SIGS, NDOCS, page_size=PAGE, num_hashes=3, seed=5)
    s3.set_tuning("mq", 0)
    check(s3, oracle.Index.synthetic(1, 31, 1, 3, PAGE, SIGS, NDOCS, 5))

    sb = gpu_lib.Search.synthetic("compact", SIGS, NDOCS, page_size=PAGE, seed=5, hbm_budget=8 << 20)
    sb.set_tuning("mq", 0)
    check(sb, oracle.Index.synthetic(1, 31, 1, 1, PAGE, SIGS, NDOCS, 5))

    s, ix = world["compact"]
    b = check(s, ix, run=lambda bb: bb.run_topk(0.0, 5), want=False)
    for i, q in enumerate(qs):
        assert b.hits_host(i, 5) == [(0, d, sc) for (_, d, _n, sc) in oracle.search(ix, q, 0.0, 5)]
    s.set_tuning("mq", -1)               # 100-bp reads pick the multi-query geometry by themselves
    try:
        reads = [world["text"][o:o + 100] for o in (0, 50, 1000)]
        b.set_queries(reads)
        b.run(0.0)
        b.sync()
        assert b.stats()["table_bytes"] > 0
        for i, q in enumerate(reads):
            assert np.array_equal(b.counts_host(i), ix.counts(q))
    finally:
        s.set_tuning("mq", 0)
        s.set_tuning("scan_self_hash", 0)


def test_alternation_with_graph_replay(gpu_lib, oracle, world):
    """on, off and on again on one handle; every phase runs a small host-buffer pass three times -- the second sighting of
    a shape class captures its graph, the third replays it -- and a batch run: a graph of one path is never replayed on
    the other (the results stay the oracle's, and the batch reports the path it took)"""
    s, ix = world["compact"]
    s.set_tuning("tile_w", 8)
    qa = [world["queries"][i] for i in (3, 4)]
    qb = [world["queries"][6], world["queries"][3]]          # same shape class as qa reversed in length: other text
    want_a = [[(0, d, sc) for (_, d, _n, sc) in oracle.search(ix, q, 0.8)] for q in qa]
    want_b = [[(0, d, sc) for (_, d, _n, sc) in oracle.search(ix, q, 0.8)] for q in qb]
    b = gpu_lib.Batch(s)
    b.set_queries(qa)
    try:
        for on in (1, 0, 1):
            s.set_tuning("scan_self_hash", ON if on else 0)
            for rep in range(3):
                assert s.search_hits(qa, 0.8, 0) == want_a, (on, rep)
                assert s.search_hits(qb, 0.8, 0) == want_b, (on, rep)
            b.run(0.0)
            b.sync()
            assert (b.stats()["table_bytes"] == 0) == bool(on)
            for i, q in enumerate(qa):
                assert np.array_equal(b.counts_host(i), ix.counts(q)), (on, i)
    finally:
        s.set_tuning("scan_self_hash", 0)
        s.set_tuning("tile_w", 0)


def test_default_goes_by_table_size(gpu_lib, oracle, world):
    """the shipped default (scan_self_hash = 1): a pass hashes for itself when K1's table of one sub-index is larger than
    4 MiB -- 32 bytes per block and padding block: 1100 queries of 1030 characters are 4.4 MB, 1000 of them 4.03 MB"""
    import bench
    s, ix = world["classic"]        # (one sub-index: every tile's indices fit the LDS array under the geometry's own W)
    s.set_tuning("scan_self_hash", DEFAULT)
    many = bench.make_queries(1100, 1000, seed=11)
    many[5] = world["queries"][4]
    b = gpu_lib.Batch(s)
    try:
        for n, self_hashed in ((1000, False), (1100, True)):
            assert ((125 + 1) * 32 * n > 4 << 20) == self_hashed
            b.set_queries(many[:n])
            b.run(0.0)
            b.sync()
            assert (b.stats()["table_bytes"] == 0) == self_hashed, n
            for i in (0, 5, n - 1):
                assert np.array_equal(b.counts_host(i), ix.counts(many[i])), (n, i)
    finally:
        s.set_tuning("scan_self_hash", 0)


@pytest.mark.parametrize("kind", ["compact", "classic"])
def test_skip_policy_both_ways(gpu_lib, world, kind):
    """invalid_bases = skip: without a threshold the pass takes the self-hashing form and tile 0 records the valid positions
    K1 would; with a threshold the thresholds are made from K1's valid positions, so K1 runs whatever the switch says"""
    nd, sigs, page = (NDOCS, SIGS, PAGE) if kind == "compact" else (CLASSIC_DOCS, [CLASSIC_SIG], 0)
    base, clean = world["queries"][4], world["queries"][3]
    qs = [clean, base, _with_n(base, [0]), _with_n(base, [500]), _with_n(base, [len(base) - 1])]
    s = gpu_lib.Search.synthetic(kind, sigs, nd, page_size=page, term_size=31, canonicalize=1, num_hashes=1, seed=5,
                                 invalid_bases="skip")
    docs, keep = [0, 3, nd // 2, nd - 1], [1000, 900, 800, 500]
    s.plant(world["text"], docs, keep, salt=99)
    s.set_tuning("mq", 0)
    s.set_tuning("tile_w", 8)
    b = gpu_lib.Batch(s)
    b.set_queries(qs)
    got = []
    for on in (0, 1):
        s.set_tuning("scan_self_hash", ON if on else 0)
        b.run(0.0)
        b.sync()
        assert (b.stats()["table_bytes"] == 0) == bool(on)
        got.append((_counts(b, len(qs)), list(b.scored_positions(0))))
    for i in range(len(qs)):
        assert np.array_equal(got[0][0][i], got[1][0][i]), (kind, i)
    assert got[0][1] == got[1][1]
    assert got[1][1] == [len(clean) - 30, 1000, 999, 1000 - 31, 999]
    lists = []
    for on in (0, 1):
        s.set_tuning("scan_self_hash", ON if on else 0)
        b.run_hits(0.8)
        b.sync()
        assert b.stats()["table_bytes"] > 0          # K1 ran on both
        lists.append([b.hits_host(i, 0) for i in range(len(qs))])
    assert lists[0] == lists[1] and all(len(h) >= 2 for h in lists[1])


def test_shard_cut_inside_a_sub_index_keeps_k1(gpu_lib, world):
    """two column shards of the one-sub-index classic file: each holds part of a sub-index, the pass stays on the table"""
    qs = [world["queries"][i] for i in (3, 4)]
    for rank in (0, 1):
        s = gpu_lib.Search.synthetic("classic", [CLASSIC_SIG], CLASSIC_DOCS, term_size=31, canonicalize=1, num_hashes=1,
                                     seed=5, shard_rank=rank, shard_count=2)
        s.set_tuning("mq", 0)
        b = gpu_lib.Batch(s)
        b.set_queries(qs)
        off, on, tb_off, tb_on = _run_both(s, b, len(qs), lambda: b.run(0.0))
        assert tb_off > 0 and tb_on == tb_off
        for i in range(len(qs)):
            assert np.array_equal(on[i], off[i]) and on[i].any()
