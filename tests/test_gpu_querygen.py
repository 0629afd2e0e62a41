"""generate-queries on the GPU against a Python restatement of its contract
(tests/test_querygen_cpu.restate) over the checker's own document readers (oracle/documents.py:
document_list, Entry.terms / num_terms) and canonicalize_kmer (oracle/oracle.py)."""
import os
import subprocess

import pytest

import cobs_amd
from cobs_amd import _capi
from oracle import documents as OD
from oracle import oracle as O
from tests.test_querygen_cpu import NotEnoughNegatives, Unreached, file_text, restate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INPUTS = ["fasta"] + [os.path.join("documents", d) for d in ("text", "cortex", "fastq", "fasta_multi")]
_TERMS = {}


def _docs(root, k):
    out = []
    for e in OD.document_list(os.path.join(GOLDEN, root)):
        def terms(e=e):
            key = (e.path, e.subdoc_index, k)
            if key not in _TERMS:
                _TERMS[key] = list(e.terms(k))
            return _TERMS[key]
        out.append((e.name, e.num_terms(k), terms))
    return out


def _canon(t):
    return O.canonicalize_kmer(t)[0]


def _expect(root, k, **kw):
    docs = _docs(root, k)
    total = sum(nt for _, nt, _ in docs)
    kw["positive"] = min(kw.get("positive", 0), total)
    try:
        return kw, restate(docs, k, kw["positive"], kw["negative"], kw["true_negatives"], kw["size"], kw["seed"],
                           kw.get("canonical", False), _canon)
    except Unreached:
        return kw, None


def _check(root, k, batch=1 << 12, tmp=None, **kw):
    kw, want = _expect(root, k, **kw)
    path = os.path.join(GOLDEN, root)
    if want is None:
        with pytest.raises(cobs_amd.CobsGpuError) as e:
            cobs_amd.generate_queries(path, term_size=k, device=0, text_batch_bytes=batch, **kw)
        assert e.value.status == _capi.ERR_FORMAT
        return None
    recs, st = want
    out = os.path.join(tmp, "q.fa") if tmp else None
    got = cobs_amd.generate_queries(path, out_file=out, term_size=k, device=0, text_batch_bytes=batch, **kw)
    assert [tuple(r) for r in got] == recs, (root, k, kw)
    assert got.stats["documents_read"] == st["documents_read"]
    assert got.stats["negatives_removed"] == st["negatives_removed"]
    if out:
        assert open(out, "rb").read() == file_text(recs)
    return got


@pytest.mark.parametrize("root", INPUTS)
@pytest.mark.parametrize("k", [31, 15, 40])
def test_exact_output_matrix(root, k, tmp_path):
    for i, (extra, mode) in enumerate([(0, None), (9, "raw"), (5, "canonical")]):
        _check(root, k, tmp=str(tmp_path), positive=25, negative=12, size=k + extra, seed=11 + 7 * i + k,
               true_negatives=mode is not None, canonical=mode == "canonical")


def test_golden_set_spans_many_batches():
    # the golden FASTA set is ~5 KiB of term text: 256-byte batches hold one document each
    for batch in (256, 1000, 0):
        _check("fasta", 31, batch=batch, positive=60, negative=20, size=40, seed=5, true_negatives=True)


def test_removal_and_too_few_survivors():
    got = _check("fasta", 9, positive=10, negative=40, size=30, seed=3, true_negatives=True)
    assert got.stats["negatives_removed"] >= 1 and got.stats["terms_probed"] > 0
    got = _check("fasta", 9, positive=10, negative=40, size=30, seed=3, true_negatives=True, canonical=True)
    assert got.stats["negatives_removed"] >= 1
    # 5-mers: the documents hold nearly all 1024 of them
    with pytest.raises(NotEnoughNegatives):
        _expect("fasta", 5, positive=0, negative=30, size=40, seed=2, true_negatives=True)
    with pytest.raises(cobs_amd.CobsGpuError) as e:
        cobs_amd.generate_queries(os.path.join(GOLDEN, "fasta"), term_size=5, negative=30, size=40, seed=2,
                                  true_negatives=True, device=0)
    assert e.value.status == _capi.ERR_ARG and "not enough true negatives" in str(e.value)


def test_same_seed_same_file_at_any_batch_size(tmp_path):
    outs = []
    for i, batch in enumerate((0, 300, 0, 4096)):
        f = str(tmp_path / ("q%d.fa" % i))
        cobs_amd.generate_queries(os.path.join(GOLDEN, "fasta"), out_file=f, positive=50, negative=30, size=45,
                                  seed=77, true_negatives=True, device=0, text_batch_bytes=batch)
        outs.append(open(f, "rb").read())
    assert all(o == outs[0] for o in outs) and outs[0].count(b">doc:") == 50


def test_documents_read_without_true_negatives():
    root = os.path.join(GOLDEN, "fasta")
    got = cobs_amd.generate_queries(root, positive=2, seed=9, device=0)
    holding = {r.doc_index for r in got}
    assert got.stats["documents_read"] == len(holding) < 7
    assert got.stats["terms_probed"] == 0
    got = cobs_amd.generate_queries(root, positive=2, seed=9, device=0, true_negatives=True)
    assert got.stats["documents_read"] == 7


def test_cli_matches_python(tmp_path):
    tool = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")
    root = os.path.join(GOLDEN, "fasta")
    want = tmp_path / "py.fa"
    cobs_amd.generate_queries(root, out_file=str(want), term_size=21, positive=30, negative=10, size=50, seed=123,
                              true_negatives=True, device=0)
    args = [tool, "generate-queries", root, "-k", "21", "-p", "30", "-n", "10", "-s", "50", "-S", "123", "-N", "-T", "4"]
    r = subprocess.run(args, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want.read_bytes()
    assert b"Given 7 documents containing" in r.stderr
    out = tmp_path / "cli.fa"
    r = subprocess.run(args + ["-o", str(out)], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b"" and out.read_bytes() == want.read_bytes()
    r = subprocess.run([tool, "generate-queries", root, "-k", "5", "-n", "30", "-s", "40", "-S", "2", "-N"],
                       capture_output=True, timeout=120)
    assert r.returncode == 1 and b"EXCEPTION:" in r.stderr and r.stdout == b""


def test_positives_are_found_in_built_indexes(tmp_path):
    root = os.path.join(GOLDEN, "fasta")
    k = 31
    got = cobs_amd.generate_queries(root, term_size=k, positive=40, seed=4, device=0)
    names = [e.name for e in OD.document_list(root)]
    for kind, fn, ext in (("classic", cobs_amd.classic_construct, ".cobs_classic"),
                          ("compact", cobs_amd.compact_construct, ".cobs_compact")):
        p = cobs_amd.CompactIndexParameters()
        p.term_size = k
        path = str(tmp_path / ("ix" + ext))
        fn(root, path, p, device=0)
        s = cobs_amd.Search(path, device=0)
        n = 0
        for r in got:
            if any(c not in b"ACGT" for c in r.sequence):
                continue
            res = s.search(r.sequence.decode(), 1.0)
            assert names[r.doc_index] in [x.doc_name for x in res], (kind, r.header)
            n += 1
        assert n >= 20                      # (the golden FASTA holds N runs: some positives are not ACGT)


# ---- -N must find real matches: documents that hold some of the drawn candidates' terms ---------------

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _revcomp(s):
    return s.translate(_COMP)[::-1]


def _planted_docs(k, seed, positive, negative, size, nseq=3, length=300):
    """nseq random sequences of `length` bases, into which k-mers of the candidates that `seed` draws are
    written: candidates 0 and 3 forward, candidates 1 and 5 as their reverse complement"""
    from tests.test_querygen_cpu import Draws
    import random
    rnd = random.Random(seed * 1000 + k)
    seqs = [bytearray(rnd.choice(b"ACGT") for _ in range(length)) for _ in range(nseq)]
    total = nseq * (length - k + 1)
    rng = Draws(seed)
    chosen = set()
    while len(chosen) < positive:
        chosen.add(rng.next() % total)
    cands = [rng.bases(max(size, k)) for _ in range((3 * negative + 1) // 2)]
    plant = [(0, 20, cands[0][2:2 + k]), (1, 150, cands[3][:k]),
             (2, 40, _revcomp(cands[1][1:1 + k])), (0, length - k - 10, _revcomp(cands[5][:k]))]
    for d, at, kmer in plant:
        seqs[d][at:at + k] = kmer
    return [bytes(s) for s in seqs]


@pytest.mark.parametrize("k", [31, 40, 15])
def test_true_negative_matches_are_found(k, tmp_path):
    kw = dict(positive=10, negative=10, size=k + 6, seed=1000 + k)
    seqs = _planted_docs(k, **kw)
    root = tmp_path / "docs"
    root.mkdir()
    for i, s in enumerate(seqs):
        (root / ("d%d.fasta" % i)).write_bytes(b">d%d\n" % i + s + b"\n")
    raw = _check(str(root), k, batch=256, true_negatives=True, **kw)
    assert raw.stats["negatives_removed"] >= 2            # candidates 0 and 3 occur forward
    can = _check(str(root), k, batch=256, true_negatives=True, canonical=True, **kw)
    assert can.stats["negatives_removed"] > raw.stats["negatives_removed"]   # + 1 and 5, planted reverse-complemented
    assert _check(str(root), k, true_negatives=False, **kw).stats["negatives_removed"] == 0


def test_in_memory_list(tmp_path):
    k = 31
    kw = dict(positive=12, negative=10, size=40, seed=321)
    seqs = _planted_docs(k, nseq=4, length=200, **kw)
    # documents of two sequences each: no term spans the separator
    texts = [(seqs[0][:120], seqs[1]), (seqs[2],), (seqs[3][:90], seqs[3][90:], seqs[0][120:])]
    mem = cobs_amd.DocumentList()
    docs = []
    for i, parts in enumerate(texts):
        mem.add_document("mem%d" % i, list(parts))
        terms = [p[j:j + k] for p in parts for j in range(len(p) - k + 1)]
        docs.append(("mem%d" % i, len(terms), lambda t=terms: t))
    for canonical in (False, True):
        want, st = restate(docs, k, kw["positive"], kw["negative"], True, kw["size"], kw["seed"], canonical, _canon)
        got = cobs_amd.generate_queries(mem, term_size=k, true_negatives=True, canonical=canonical, device=0,
                                        text_batch_bytes=128, out_file=str(tmp_path / "m.fa"), **kw)
        assert [tuple(r) for r in got] == want
        assert got.stats["negatives_removed"] == st["negatives_removed"] >= 2 and got.stats["documents_read"] == 3
        assert (tmp_path / "m.fa").read_bytes() == file_text(want)


def test_unreached_positive_names_the_document(tmp_path):
    # a FASTA file that shrinks after it was listed: its recorded num_terms (70 at k = 31) overstates it
    f = tmp_path / "shrinks.fasta"
    f.write_bytes(b">s\n" + b"ACGTTGCA" * 12 + b"ACGT\n")
    dl = cobs_amd.DocumentList(str(f))
    assert dl[0].num_terms(31) == 70
    f.write_bytes(b">s\n" + b"ACGTTGCA" * 7 + b"ACGT\n")
    with pytest.raises(cobs_amd.CobsGpuError) as e:
        cobs_amd.generate_queries(dl, positive=70, seed=1, device=0)
    assert e.value.status == _capi.ERR_FORMAT and str(f) in str(e.value)
