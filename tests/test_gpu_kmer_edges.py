"""GPU: canonicalisation with adversarial k-mers on every device path, and hash % S at the extreme signature sizes.

The suite's other files compare the device with the oracle on RANDOM sequences, where the decision of
canonicalize_kmer (reference cobs/util/query.cpp:143-199) falls at position s with probability (3/4) * 4^-s: the
fourth compared word of canon31 (positions 12-14, the `>>= 8` that leaves out position 15) and the tie branch are
never reached.  tests/kmer_edges.py builds k-mers whose deciding position and outcome are chosen; this file sends them
through

  hash_kernel_k31 / hash_kernel   a WITNESS index per (k, H): document 0 holds the canonical form of every edge k-mer,
                                  document 1 the other orientation, document 2 nothing -- one-k-mer queries, the four
                                  byte alignments of a term inside its query, long concatenations through every pass
  build_kernel                    documents made of the edge set (in memory, FASTA, text), files byte for byte
  plant_kernel                    Search.plant of a text of edge k-mers against the oracle's plant
  qg_pack                         generate-queries at k = 4 .. 7 (ties are common) and over the k = 31 edge set
  fast_mod                        a compact index with S = 1, 2, 3, 64, 65, 4096, 4097, 65535, 65536, 2^20

Every fixture property (a witness is CLEAN: the oracle counts [1, 0, 0, ...] for it) is asserted from the oracle
before the device is touched."""
import collections
import math
import os

import numpy as np
import pytest

from tests import cases
from tests import kmer_edges as E

pytestmark = pytest.mark.gpu

SEED = 20
S_WITNESS = 1000003
KS = [31, 3, 4, 5, 20, 30, 32, 33, 63, 64, 65, 131]        # 31 -> hash_kernel_k31, the others -> hash_kernel
HS = [1, 3]
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


# ---- the witness index -----------------------------------------------------------------------------------------------

class Witness:
    """classic, 8 documents, no random bits: document 0 = the right orientation of every edge k-mer (canonicalize 1:
    its canonical form; canonicalize 0: the k-mer as it is), document 1 = the other orientation where that is another
    string, documents 2 .. 7 empty.  Rows from the oracle's XXH64 of those bytes."""

    def __init__(self, oracle, construct, directory, k, H, canonicalize=1):
        self.k, self.H, self.canonicalize = k, H, canonicalize
        self.items = E.witness_kmers(k, SEED)
        self.kmers = [t for _, t in self.items]
        right = [E.canonical(t) if canonicalize else t for t in self.kmers]
        wrong = [E.revcomp(r) for r in right if E.revcomp(r) != r]

        def hashes(terms):
            return np.concatenate([oracle.term_hashes(t, k, 0, H)[0] for t in terms])
        docs = [construct.Doc("right", "right", 0, len(right), hashes(right)),
                construct.Doc("wrong", "wrong", 0, len(wrong), hashes(wrong))]
        docs += [construct.Doc("empty%d" % i, "empty%d" % i, 0, 0, np.zeros((0, H), dtype=np.uint64)) for i in range(6)]
        self.path = os.path.join(str(directory), "w_k%d_h%d_c%d.cobs_classic" % (k, H, canonicalize))
        construct.write_classic(self.path, k, canonicalize, [d.name for d in docs], S_WITNESS, H,
                                construct.build_matrix(docs, S_WITNESS, 1))
        self.ix = oracle.Index.open(self.path)
        # the fixture condition, from the oracle alone
        self.want = [self.ix.counts(t) for t in self.kmers]
        clean_row = np.array([1] + [0] * (self.ix.counts_size - 1), dtype=np.uint32)
        self.clean = [np.array_equal(w, clean_row) for w in self.want]
        assert all(w[0] == 1 for w in self.want), (k, H)          # (every witness finds its right orientation)
        if k >= 12:
            assert self.clean.count(False) <= 0.01 * len(self.kmers), (k, H, self.clean.count(False))
            kept = collections.Counter()
            for (label, t), c in zip(self.items, self.clean):
                kept[(label, chr(t[k // 2]) if k % 2 else "")] += c
            for s in list(range(k // 2)) + [None]:
                for outcome in (("tie",) if s is None else ("fwd", "rc")):
                    for mid in ("ACGT" if k % 2 else [""]):
                        assert kept[((s, outcome), mid)] >= 1, (k, H, s, outcome, mid)


@pytest.fixture(scope="module")
def witnesses(oracle, construct, tmp_path_factory):
    d = tmp_path_factory.mktemp("witness")
    cache = {}

    def get(k, H, canonicalize=1):
        if (k, H, canonicalize) not in cache:
            cache[(k, H, canonicalize)] = Witness(oracle, construct, d, k, H, canonicalize)
        return cache[(k, H, canonicalize)]
    return get


def _rows(gpu, s, queries):
    b = gpu.Batch(s)
    b.set_queries(queries)
    b.run(0.0)
    b.sync()
    out = [b.counts_host(i) for i in range(len(queries))]
    b.close()
    return out


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("k", KS)
def test_every_edge_kmer_as_its_own_query(gpu_lib, witnesses, k, H):
    """T = 1, one batch per k: the device's counts equal the oracle's for every witness, clean or not -- and a clean
    witness scores [1, 0, 0, ...]: found in the right orientation, not in the other"""
    w = witnesses(k, H)
    s = gpu_lib.Search(w.path)
    got = _rows(gpu_lib, s, w.kmers)
    for (label, t), g, want, clean in zip(w.items, got, w.want, w.clean):
        assert np.array_equal(g, want), (k, H, label, t, g[:3], want[:3])
        if clean:
            assert g[0] == 1 and not g[1:].any(), (k, H, label, t)
    # the host call, one k-mer at a time (small passes: the captured-graph path of host_api.cpp)
    for (label, t), want in list(zip(w.items, w.want))[::7]:
        assert np.array_equal(s.counts(t), want), (k, H, label, t)
    s.close()


@pytest.mark.parametrize("k", [31, 33])
def test_canonicalize_0_reverses_nothing(gpu_lib, witnesses, k):
    """an index with canonicalize = 0, once per kernel: document 0 holds the k-mers as they are, document 1 their
    reverse complements"""
    w = witnesses(k, 1, canonicalize=0)
    s = gpu_lib.Search(w.path)
    assert s.info(0).canonicalize == 0
    for (label, t), g, want, clean in zip(w.items, _rows(gpu_lib, s, w.kmers), w.want, w.clean):
        assert np.array_equal(g, want), (k, label, t)
        if clean:
            assert g[0] == 1 and not g[1:].any(), (k, label, t)
    s.close()


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("k", KS)
def test_every_alignment_of_a_term_in_its_query(gpu_lib, oracle, witnesses, k, H):
    """hash_kernel_k31 reads a term as nine dwords around `text + i` and shifts by (text + i) & 3.  The engine lays
    every query of a batch at a multiple of 8 bytes (and refuses a query shorter than k, as the reference does), so the
    alignment of a term is its position i in its query: every edge k-mer behind 0, 1, 2 and 3 other bases, as the LAST
    term of its query (nothing but padding behind it), and the last query of each batch ends in an edge k-mer; then
    the same k-mers in the middle of a query, at every offset mod 4, with bases behind them"""
    w = witnesses(k, H)
    s = gpu_lib.Search(w.path)
    filler = oracle.random_sequence(len(w.kmers) * 8 + 16, 5 + k)
    for a in range(4):
        queries = [filler[8 * n:8 * n + a] + t for n, t in enumerate(w.kmers)]
        want = [w.ix.counts(q) for q in queries]
        assert all(x[0] >= 1 for x in want)
        for (label, t), g, x in zip(w.items, _rows(gpu_lib, s, queries), want):
            assert np.array_equal(g, x), (k, H, "last term at", a, label, t)
        queries = [filler[8 * n:8 * n + 4 + a] + t + filler[8 * n + 9:8 * n + 9 + (n % 7)] for n, t in enumerate(w.kmers)]
        want = [w.ix.counts(q) for q in queries]
        for (label, t), g, x in zip(w.items, _rows(gpu_lib, s, queries), want):
            assert np.array_equal(g, x), (k, H, "inside at", 4 + a, label, t)
    s.close()


def _long_queries(w):
    """concatenations of edge k-mers with 255, 256, 1023 and 1024 terms, 1500 terms from another start, and all"""
    k = w.k
    text = b"".join(w.kmers)
    while len(text) < 1600 + k:
        text += text
    out = [text[:T + k - 1] for T in (255, 256, 1023, 1024)]
    out.append(text[k + 1:k + 1 + 1500 + k - 1])
    out.append(text[:4000])
    return out


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("k", KS)
def test_concatenated_edge_kmers_through_every_pass(gpu_lib, oracle, witnesses, k, H):
    w = witnesses(k, H)
    s = gpu_lib.Search(w.path)
    queries = _long_queries(w)
    rows = [w.ix.counts(q) for q in queries]
    assert all(r[0] >= (len(q) - k + 1) // k - 1 for r, q in zip(rows, queries))  # the edge k-mers themselves
    # thresholds: document 0 of the first query exactly on ceil(t * T), just above it, and a low one
    T0 = len(queries[0]) - k + 1
    t_on = int(rows[0][0]) / T0
    while math.ceil(t_on * T0) > int(rows[0][0]):
        t_on = math.nextafter(t_on, 0.0)
    ts = [t_on, min(1.0, (int(rows[0][0]) + 0.5) / T0), 0.001]
    b = gpu_lib.Batch(s)
    b.set_queries(queries)
    b.run(0.0)
    b.sync()
    for i, r in enumerate(rows):
        assert np.array_equal(b.counts_host(i), r), (k, H, i)
    for t in ts:
        want = [cases.oracle_results([w.ix], q, t, 0) for q in queries]
        b.run(t)
        b.sync()
        for i, r in enumerate(rows):
            assert b.hits_host(i) == want[i], ("run", k, H, t, i)
            assert np.array_equal(b.counts_host(i), r), ("run", k, H, t, i)
        b.run_hits(t)
        b.sync()
        for i in range(len(queries)):
            assert b.hits_host(i) == want[i], ("run_hits", k, H, t, i)
        for keep in (True, False):
            b.run_topk(t, 2, keep_counts=keep)
            b.sync()
            for i in range(len(queries)):
                assert b.hits_host(i, 2) == want[i][:2], ("run_topk", keep, k, H, t, i)
    b.close()
    for q, r in zip(queries[:3], rows):
        assert np.array_equal(s.counts(q), r)
        for t in ts[:2]:
            got = s.search(q.decode(), t)
            assert [(x.doc_name, x.score) for x in got] == [(n, sc) for (_, _, n, sc) in oracle.search(w.ix, q, t)], (k, H, t)
    assert s.search_hits(queries, ts[0], 0) == [cases.oracle_results([w.ix], q, ts[0], 0) for q in queries]
    s.close()


# ---- hash % S at the extreme signature sizes -------------------------------------------------------------------------

SIGS = [1, 2, 3, 64, 65, 4096, 4097, 65535, 65536, 1 << 20]


@pytest.mark.parametrize("k", [31, 20])
@pytest.mark.parametrize("H", [1, 2])
def test_signature_sizes_from_1_to_2_pow_20(gpu_lib, oracle, tmp_path, k, H):
    """one sub-index per S (page_size 1: eight documents each), random bits and planted documents; S = 1 puts every
    term on row 0 and the padding term on row 1; the reciprocal ~0 / S is 2^64 - 1 there.  Counts, thresholded hits
    and top-k against the oracle, resident and -- with one hash function -- under an HBM budget that streams the file
    (with two the planner streams column slices, and a 16-byte slice of the 2^20-row sub-index, buffered twice, is
    larger than the whole 19 MB file: no budget streams it, the open is refused below the resident size)"""
    D = 8 * len(SIGS) - 3
    src = oracle.random_sequence(400, 90 + k)
    planted = {8 * p + (p % 8 if 8 * p + p % 8 < D else 0): (1.0, 0.8, 0.55)[p % 3] for p in range(len(SIGS))}
    path = cases.make_compact(str(tmp_path / "sigs.cobs_compact"), D, 1, SIGS, H, k, 1, 0.3, 7 + H, planted, src)
    ix = oracle.Index.open(path)
    assert [ix.signature_size(p) for p in range(ix.num_pages)] == SIGS
    queries = [src, src[50:50 + k], src[100:100 + k + 254], src[3:3 + k + 255], oracle.random_sequence(300, 4),
               E.TIE31_FORWARD_IS_LARGER * 3]
    rows = [ix.counts(q) for q in queries]
    assert rows[0][0] == len(src) - k + 1                       # the planted document of the S = 1 sub-index
    s0 = gpu_lib.Search(path)
    budget = int(0.6 * s0.info(0).hbm_bytes)
    for s in (s0, gpu_lib.Search(path, hbm_budget=budget)) if H == 1 else (s0,):
        assert (s.stream_plan()[3] > 0) == (s is not s0)
        assert [s.signature_size(0, p) for p in range(len(SIGS))] == SIGS
        for q, r in zip(queries, rows):
            assert np.array_equal(s.counts(q), r), (k, H, s is s0)
        for g, r in zip(_rows(gpu_lib, s, queries), rows):
            assert np.array_equal(g, r), (k, H, s is s0)
        for t, lim in ((0.0, 0), (0.5, 0), (0.8, 0), (1.0, 0), (0.0, 5), (0.3, 11)):
            assert s.search_hits(queries, t, lim) == [cases.oracle_results([ix], q, t, lim) for q in queries], (k, H, t, lim)
        s.close()


# ---- construction: build_kernel --------------------------------------------------------------------------------------

def _edge_docs(k, with_invalid):
    """documents made of the edge set: -> [(name, [sequences])]; every k-mer as a sequence of its own, concatenations
    (every window across two of them is a term too), and -- with_invalid -- the variants with one byte outside ACGT"""
    valid = [t for _, t in E.edge_kmers(k, SEED)]
    pool = valid + ([t for _, t in E.edge_kmers_invalid(k, SEED)] if with_invalid else [])
    docs = []
    n = max(1, (len(pool) + 18) // 19)
    for d in range(19):
        part = pool[d * n:(d + 1) * n] or [valid[d % len(valid)]]
        seqs = list(part) if d % 2 == 0 else [b"".join(part)]
        if d % 5 == 4:
            seqs = [b"".join(part[:len(part) // 2])] + part[len(part) // 2:]
        docs.append(("edge_%02d" % d, seqs))
    return docs


@pytest.mark.parametrize("k,canonicalize,num_hashes,with_invalid", [
    (31, 1, 1, False), (31, 1, 3, False), (31, 1, 1, True), (31, 1, 3, True), (31, 0, 1, True),
    (4, 1, 3, True), (20, 1, 1, True), (32, 1, 3, True), (65, 1, 1, True), (20, 0, 3, True), (65, 0, 1, False)])
def test_in_memory_edge_documents_vs_restatement(gpu_lib, oracle, construct, tmp_path, k, canonicalize, num_hashes,
                                                 with_invalid):
    """k = 31 over ACGT: the register path of build_kernel (canon31); with the invalid variants the same launch falls to
    the byte view for those terms; other k: the byte loop.  Classic and compact files byte for byte against the
    checker's construction, both ways of setting bits; then every valid edge k-mer of a document scores in it"""
    docs = _edge_docs(k, with_invalid)
    dl = gpu_lib.DocumentList()
    kdocs = []
    for name, seqs in docs:
        dl.add_document(name, seqs)
        hs = [oracle.term_hashes(s, k, canonicalize, num_hashes)[0] for s in seqs if len(s) >= k]
        text_len = len(b"\n".join(seqs)) + 1
        kdocs.append(construct.Doc(name, name, text_len, sum(max(len(s) - k + 1, 0) for s in seqs), np.concatenate(hs)))
    for kind in ("classic", "compact"):
        p = gpu_lib.ClassicIndexParameters() if kind == "classic" else gpu_lib.CompactIndexParameters()
        p.term_size, p.canonicalize, p.num_hashes, p.false_positive_rate = k, canonicalize, num_hashes, 0.1
        p.clobber = True
        got, want = str(tmp_path / ("g.cobs_" + kind)), str(tmp_path / ("w.cobs_" + kind))
        if kind == "classic":
            construct.classic_construct(kdocs, want, term_size=k, canonicalize=canonicalize, num_hashes=num_hashes,
                                        false_positive_rate=0.1)
        else:
            p.page_size = 1
            construct.compact_construct(kdocs, want, term_size=k, canonicalize=canonicalize, num_hashes=num_hashes,
                                        false_positive_rate=0.1, page_size=1)
        for mode in (1, 2):                              # atomicOr into the matrix / byte planes + packing pass
            p.set_bits_mode = mode
            (gpu_lib.classic_construct if kind == "classic" else gpu_lib.compact_construct)(list=dl, out_file=got, index_params=p)
            assert open(got, "rb").read() == open(want, "rb").read(), (kind, mode)
        s = gpu_lib.Search(got)
        names = [s.doc_name(0, d) for d in range(s.info(0).num_docs)]
        for name, seqs in docs:
            terms = [t for q in seqs for t in (q[i:i + k] for i in range(0, len(q) - k + 1, k)) if set(t) <= set(b"ACGT")]
            for t, res in zip(terms, s.search_hits(terms, 0.0, 0)):
                assert dict((names[d], sc) for (_, d, sc) in res).get(name, 0) == 1, (kind, name, t)
        s.close()


@pytest.mark.parametrize("k,canonicalize,num_hashes", [(31, 1, 1), (31, 1, 3), (31, 0, 1), (20, 1, 3), (32, 1, 1), (65, 1, 3), (4, 1, 1)])
def test_edge_documents_from_files(gpu_lib, oracle, construct, tmp_path, k, canonicalize, num_hashes):
    """the edge set as FASTA files (lines of 60 and of 61 columns: terms end at a line end, start behind one, and lie
    at every address mod 4; one record per k-mer; the invalid variants) and as a text document (a raw stretch: the
    line ends are characters of its terms)"""
    from oracle import documents as D
    from tests.test_gpu_construct import _build_both
    valid = [t for _, t in E.edge_kmers(k, SEED)]
    invalid = [t for _, t in E.edge_kmers_invalid(k, SEED)]
    root = tmp_path / "docs"
    root.mkdir()

    def wrap(text, cols):
        return b"".join(text[i:i + cols] + b"\n" for i in range(0, len(text), cols))
    (root / "a60.fasta").write_bytes(b">a60\n" + wrap(b"".join(valid), 60))
    (root / "b61.fasta").write_bytes(b">b61\n" + wrap(b"".join(valid[::-1]), 61))
    (root / "c_records.fasta").write_bytes(b"".join(b">r%d\n%s\n" % (i, t) for i, t in enumerate(valid)))
    (root / "d_invalid.fasta").write_bytes(b">d\n" + wrap(b"".join(invalid[:400]), 61) + b">d2\n" +
                                           b"".join(t + b"\n;c\n" for t in invalid[400:500]))
    (root / "e_text.txt").write_bytes(b"".join(valid) + b"\n" + b"".join(invalid[:64]) + b"\n")
    pc, pk = _build_both(gpu_lib, construct, D, str(root), tmp_path, "edges", k=k, canonicalize=canonicalize,
                         num_hashes=num_hashes, fpr=0.1, page_size=1)
    for p in (pc, pk):
        s = gpu_lib.Search(p)
        names = [s.doc_name(0, d) for d in range(s.info(0).num_docs)]
        for res, t in zip(s.search_hits(valid, 0.0, 0), valid):
            score = dict((names[d], sc) for (_, d, sc) in res)
            assert score["a60"] == score["b61"] == score["c_records"] == score["e_text"] == 1, (p, t)
        s.close()


# ---- plant_kernel ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,k,H", [("compact", 31, 3), ("classic", 31, 1), ("compact", 20, 3), ("classic", 33, 3)])
def test_plant_of_edge_kmers(gpu_lib, oracle, kind, k, H):
    """Search.plant(text of concatenated edge k-mers) on a procedural index against the oracle's plant: the full count
    row of the text as a query, of its halves, and of every tie k-mer on its own"""
    ps = 16 if kind == "compact" else 0
    sigs = [5003, 7001, 6007] if kind == "compact" else [9001]
    D = 3 * 8 * 16 - 5 if kind == "compact" else 200
    items = E.witness_kmers(k, SEED)
    text = b"".join(t for _, t in items)
    s = gpu_lib.Search.synthetic(kind, sigs, D, page_size=ps, term_size=k, num_hashes=H, seed=9)
    ix = oracle.Index.synthetic(1 if kind == "compact" else 0, k, 1, H, ps, sigs, D, 9)
    docs, keep = [0, 7, 130, D - 1], [1000, 500, 1000, 500]
    s.plant(text, docs, keep, salt=77)
    ix.plant(text, docs, keep, salt=77)
    T = len(text) - k + 1
    want = ix.counts(text)
    assert want[0] == T and want[130] == T and 0.3 * T < want[7] < T
    assert np.array_equal(s.counts(text), want)
    for q in (text[:len(text) // 2], text[len(text) // 2:]):
        assert np.array_equal(s.counts(q), ix.counts(q))
    ties = [t for (label, t) in items if label[1] == "tie"]
    assert len(ties) >= (4 if k % 2 else 1)
    for t, g in zip(ties, _rows(gpu_lib, s, ties)):
        x = ix.counts(t)
        assert x[0] == 1 and x[130] == 1 and np.array_equal(g, x), (kind, k, t)
    s.close()


# ---- generate-queries: qg_pack ---------------------------------------------------------------------------------------

def _tie_case(k, negative):
    """-> (seed, documents [(name, [sequences])]) for generate-queries at size = k: a seed whose candidates hold at
    least three ties; the documents hold one tie candidate as it is, the REVERSE COMPLEMENT of another tie candidate
    (odd k: another string, itself a tie and its own canonical form, so that candidate stays; even k: the same
    string) and the reverse complements of two candidates that are no ties"""
    from tests.test_querygen_cpu import Draws
    ncand = (3 * negative + 1) // 2
    for seed in range(1, 400):
        rng = Draws(seed * 31 + k)
        chosen = set()
        while len(chosen) < 2:                           # the two positives out of the four terms come first
            chosen.add(rng.next() % 4)
        cands = [rng.bases(k) for _ in range(ncand)]
        ties = [c for c in dict.fromkeys(cands) if E.decide(c)[1] == "tie"]
        rest = [c for c in dict.fromkeys(cands) if E.decide(c)[1] != "tie"]
        if len(ties) >= 3:
            return seed * 31 + k, [("t0", [ties[0], E.revcomp(rest[0])]), ("t1", [E.revcomp(ties[1]), E.revcomp(rest[1])])]
    raise AssertionError("no seed with three tie candidates")


@pytest.mark.parametrize("k,negative", [(4, 40), (5, 60), (6, 200), (7, 300)])
def test_generate_queries_where_ties_are_common(gpu_lib, oracle, k, negative):
    """The negative candidates come from the seeded generator, so at k = 31 a deep decision or a tie cannot be steered
    into qg_pack through the API (a tie among 30 candidates has probability 30 * 4^-15) and no hook is added for it.
    At k = 4 and 5 one candidate in 16 is a tie, at k = 6 and 7 one in 64: rows and negatives_removed against the
    restatement, which must have removed a tie candidate and kept one"""
    import cobs_amd
    from tests.test_querygen_cpu import restate
    seed, texts = _tie_case(k, negative)
    mem = cobs_amd.DocumentList()
    docs = []
    for name, seqs in texts:
        mem.add_document(name, seqs)
        docs.append((name, len(seqs), lambda t=seqs: t))
    canon = lambda t: oracle.canonicalize_kmer(t)[0]                 # noqa: E731
    for canonical in (True, False):
        want, st = restate(docs, k, 2, negative, True, k, seed, canonical, canon)
        if canonical:
            # from the restatement: which candidates went, which stayed
            from tests.test_querygen_cpu import Draws
            rng = Draws(seed)
            chosen = set()
            while len(chosen) < 2:
                chosen.add(rng.next() % 4)
            cands = [rng.bases(k) for _ in range((3 * negative + 1) // 2)]
            seen = {canon(t) for _, seqs in texts for t in seqs}
            gone = [c for c in cands if canon(c) in seen]
            assert len(gone) == st["negatives_removed"]
            assert any(E.decide(c)[1] == "tie" for c in gone)
            assert any(E.decide(c)[1] == "tie" for c in cands if canon(c) not in seen)
            assert any(E.decide(c)[1] != "tie" for c in gone)
        got = cobs_amd.generate_queries(mem, term_size=k, positive=2, negative=negative, size=k, seed=seed,
                                        true_negatives=True, canonical=canonical, device=0, text_batch_bytes=128)
        assert [tuple(r) for r in got] == want, (k, canonical)
        assert got.stats["negatives_removed"] == st["negatives_removed"], (k, canonical)


def test_generate_queries_over_the_k31_edge_set(gpu_lib, oracle):
    """documents made of the k = 31 edge set (every deciding position, ties): output and statistics equal the
    restatement's -- no candidate is removed by a document term packed or canonicalised wrongly"""
    import cobs_amd
    from tests.test_querygen_cpu import restate
    k = 31
    mem = cobs_amd.DocumentList()
    docs = []
    for name, seqs in _edge_docs(k, True):
        mem.add_document(name, seqs)
        terms = [q[i:i + k] for q in seqs for i in range(len(q) - k + 1)]
        docs.append((name, len(terms), lambda t=terms: t))
    canon = lambda t: oracle.canonicalize_kmer(t)[0]                 # noqa: E731
    for canonical in (True, False):
        want, st = restate(docs, k, 20, 30, True, 45, 123, canonical, canon)
        got = cobs_amd.generate_queries(mem, term_size=k, positive=20, negative=30, size=45, seed=123,
                                        true_negatives=True, canonical=canonical, device=0, text_batch_bytes=512)
        assert [tuple(r) for r in got] == want
        assert got.stats["negatives_removed"] == st["negatives_removed"] == 0
        assert got.stats["documents_read"] == st["documents_read"] == len(docs)
