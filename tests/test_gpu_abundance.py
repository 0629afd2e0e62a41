"""The k-mer abundance cutoff of index construction (min_count) on the GPU: the files the builders
write equal, byte for byte, the oracle's construction over the occurrences the plain-Python
restatement keeps (tests/abundance_check.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import abundance_check as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")


def _doclist(cobs, docs):
    dl = cobs.DocumentList()
    for name, seqs in docs:
        dl.add_document(name, seqs)
    return dl


def _params(cobs, kind, k, canonicalize, num_hashes, c, mode=0, batch=A.TEXT_BATCH, fpr=0.1):
    p = cobs.CompactIndexParameters() if kind == "compact" else cobs.ClassicIndexParameters()
    p.term_size, p.canonicalize, p.num_hashes, p.false_positive_rate = k, canonicalize, num_hashes, fpr
    if kind == "compact":
        p.page_size = 2
    p.text_batch_bytes, p.set_bits_mode, p.clobber = batch, mode, True
    if c is not None:
        p.min_count = c
    return p


def _want(construct, kind, kdocs, path, k, canonicalize, num_hashes, fpr=0.1):
    if kind == "compact":
        construct.compact_construct(kdocs, path, term_size=k, canonicalize=canonicalize, num_hashes=num_hashes,
                                    false_positive_rate=fpr, page_size=2)
    else:
        construct.classic_construct(kdocs, path, term_size=k, canonicalize=canonicalize, num_hashes=num_hashes,
                                    false_positive_rate=fpr)
    return open(path, "rb").read()


def _build(cobs, kind, dl, path, p):
    (cobs.compact_construct if kind == "compact" else cobs.classic_construct)(list=dl, out_file=path, index_params=p)
    return open(path, "rb").read()


@pytest.mark.parametrize("canonicalize,num_hashes,k", A.PARAMS)
def test_files_equal_the_filtered_construction(gpu_lib, oracle, construct, tmp_path, canonicalize, num_hashes, k):
    """classic and compact, c in {1, 2, 3, 5}, both ways of setting bits; the corpus takes several
    text batches of several documents each and holds one segment once in each of twelve neighbouring
    documents (cross-document leakage would keep it)"""
    docs = A.make_corpus(7 + k, k)
    dl = _doclist(gpu_lib, docs)
    for c in A.CUTOFFS:
        kdocs, kept, total = A.memory_docs(oracle, construct, docs, k, canonicalize, num_hashes, c)
        print("k=%d canonicalize=%d c=%d: kept %d of %d occurrences" % (k, canonicalize, c, kept, total))
        if c >= 2:
            assert 0.10 * total <= kept <= 0.90 * total
        for kind in ("classic", "compact"):
            want = _want(construct, kind, kdocs, str(tmp_path / ("w.cobs_" + kind)), k, canonicalize, num_hashes)
            for mode in (1, 2):
                got = _build(gpu_lib, kind, dl, str(tmp_path / ("g.cobs_" + kind)),
                             _params(gpu_lib, kind, k, canonicalize, num_hashes, c, mode))
                assert got == want, (kind, c, mode)
            # the batching does not matter: one document per batch, and everything in one batch
            if c == 3:
                for batch in (1, 0):
                    got = _build(gpu_lib, kind, dl, str(tmp_path / ("g.cobs_" + kind)),
                                 _params(gpu_lib, kind, k, canonicalize, num_hashes, c, 0, batch=batch))
                    assert got == want, (kind, c, "batch", batch)


def test_cutoff_one_equals_a_build_without_the_field(gpu_lib, oracle, construct, tmp_path):
    """c = 0 and c = 1 write today's bytes; a caller whose struct ends before min_count (an older
    struct_size) is not read past its end"""
    from cobs_amd import _capi
    from cobs_amd.construct import _params as to_c
    k = 31
    docs = A.make_corpus(5, k, ndocs=16)
    dl = _doclist(gpu_lib, docs)
    plain, _, _ = A.memory_docs(oracle, construct, docs, k, 1, 2, 1)
    lib = _capi.load()
    for kind, fn in (("classic", lib.cobs_gpu_build_classic_list), ("compact", lib.cobs_gpu_build_compact_list)):
        want = _want(construct, kind, plain, str(tmp_path / ("w.cobs_" + kind)), k, 1, 2)
        for c in (None, 0, 1):
            assert _build(gpu_lib, kind, dl, str(tmp_path / ("g.cobs_" + kind)), _params(gpu_lib, kind, k, 1, 2, c)) == want
        b = to_c(_params(gpu_lib, kind, k, 1, 2, 9), -1)
        b.struct_size = _capi.BuildParams.set_bits_mode.offset           # the struct as it was before set_bits_mode
        out = str(tmp_path / ("old.cobs_" + kind))
        _capi.check(fn(dl._h, C.byref(b), os.fsencode(out)))
        assert open(out, "rb").read() == want


def _write_reads(root, k):
    """a FASTQ file of reads with coverage (every read drawn from one genome, many overlap) and a
    FASTA file with repeated records, lines wrapped"""
    rng = np.random.default_rng(11)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    os.makedirs(root)
    for f in range(3):
        genome = acgt[rng.integers(0, 4, 1200)].tobytes()
        with open(os.path.join(root, "reads%d.fastq" % f), "wb") as fq:
            for r in range(45):
                at = int(rng.integers(0, len(genome) - 80))
                read = bytearray(genome[at:at + 80])
                if r % 7 == 0:
                    read[int(rng.integers(0, 80))] = ord("N")
                if r % 5 == 0:
                    read = bytearray(A.revcomp(bytes(read).replace(b"N", b"A")))
                fq.write(b"@r%d\n" % r + bytes(read) + b"\n+\n" + b"I" * 80 + b"\n")
        with open(os.path.join(root, "asm%d.fasta" % f), "wb") as fa:
            for r in range(9):
                seq = genome[100 * (r % 6):100 * (r % 6) + 170]
                fa.write(b">rec%d\n" % r + b"\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + b"\n")


@pytest.mark.parametrize("canonicalize", [1, 0])
def test_fastq_and_fasta_files_through_a_document_list(gpu_lib, oracle, construct, tmp_path, canonicalize):
    from oracle import documents as D
    k, nh = 31, 2
    root = str(tmp_path / "reads")
    _write_reads(root, k)
    ents = D.document_list(root)
    assert len(ents) == 6
    for c in (2, 3):
        kdocs, kept, total = A.entry_docs(oracle, construct, ents, k, canonicalize, nh, c)
        print("files canonicalize=%d c=%d: kept %d of %d occurrences" % (canonicalize, c, kept, total))
        assert 0.10 * total <= kept <= 0.90 * total
        for kind in ("classic", "compact"):
            want = _want(construct, kind, kdocs, str(tmp_path / ("w.cobs_" + kind)), k, canonicalize, nh)
            for batch in (3000, 0):
                p = _params(gpu_lib, kind, k, canonicalize, nh, c, batch=batch)
                out = str(tmp_path / ("g.cobs_" + kind))
                (gpu_lib.compact_construct if kind == "compact" else gpu_lib.classic_construct)(root, out, p)
                assert open(out, "rb").read() == want, (kind, c, batch)


def test_resident_handle_counts_like_the_file(gpu_lib, oracle, construct, tmp_path):
    """cobs_gpu_build_index*: the handle built with the cutoff answers like the oracle on the file
    built with the same cutoff"""
    k, canon, nh, c = 31, 1, 2, 3
    docs = A.make_corpus(21, k, ndocs=24)
    kdocs, kept, total = A.memory_docs(oracle, construct, docs, k, canon, nh, c)
    assert 0 < kept < total
    queries = [s for _, seqs in docs[:6] for s in seqs[:2] if len(s) >= k and set(s) <= set(b"ACGT")]
    assert queries
    for kind in ("classic", "compact"):
        path = str(tmp_path / ("w.cobs_" + kind))
        _want(construct, kind, kdocs, path, k, canon, nh)
        ix = oracle.Index.open(path)
        unfiltered = str(tmp_path / ("u.cobs_" + kind))
        _want(construct, kind, A.memory_docs(oracle, construct, docs, k, canon, nh, 1)[0], unfiltered, k, canon, nh)
        ux = oracle.Index.open(unfiltered)
        s = gpu_lib.build_search(list=_doclist(gpu_lib, docs), index_params=_params(gpu_lib, kind, k, canon, nh, c), kind=kind)
        differs = False
        for q in queries:
            assert np.array_equal(s.counts(q), ix.counts(q))
            differs |= not np.array_equal(ix.counts(q), ux.counts(q))
        assert differs                                        # the cutoff is visible to a query


def test_cutoff_above_every_multiplicity(gpu_lib, oracle, construct, tmp_path):
    """the file is valid, its matrix all zero, it opens and searches"""
    k = 31
    docs = A.make_corpus(9, k, ndocs=10)
    p = _params(gpu_lib, "classic", k, 1, 1, 1000)
    out = str(tmp_path / "z.cobs_classic")
    _build(gpu_lib, "classic", _doclist(gpu_lib, docs), out, p)
    kk, canon, names, sig, nh, m = construct.read_classic(out)
    assert (kk, canon, nh, len(names)) == (31, 1, 1, 10) and sig > 0 and not m.any()
    plain = str(tmp_path / "p.cobs_classic")
    p.min_count = 1
    _build(gpu_lib, "classic", _doclist(gpu_lib, docs), plain, p)
    assert construct.read_classic(plain)[3] == sig           # sized from the unfiltered terms
    s = gpu_lib.Search(out)
    q = next(s for s in docs[0][1] if len(s) >= 60 and set(s) <= set(b"ACGT"))[:60]
    assert not s.counts(q).any() and gpu_lib.Search(plain).counts(q).any()


def test_cli_flag(gpu_lib, oracle, construct, tmp_path):
    from oracle import documents as D
    root = str(tmp_path / "reads")
    _write_reads(root, 31)
    ents = D.document_list(root)
    for kind, ext in (("classic", ".cobs_classic"), ("compact", ".cobs_compact")):
        tool = kind + "-construct"
        extra = ["-p", "2"] if kind == "compact" else []
        kdocs, _, _ = A.entry_docs(oracle, construct, ents, 31, 1, 2, 2)
        want = _want(construct, kind, kdocs, str(tmp_path / ("w" + ext)), 31, 1, 2)
        out = str(tmp_path / ("cli" + ext))
        r = subprocess.run([TOOL, tool, root, out, "-h", "2", "-f", "0.1", "--min-count", "2"] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert "min_count: 2\n" in r.stdout
        assert open(out, "rb").read() == want
        # without the flag the output is what it was
        plain, _, _ = A.entry_docs(oracle, construct, ents, 31, 1, 2, 1)
        want = _want(construct, kind, plain, str(tmp_path / ("w" + ext)), 31, 1, 2)
        r = subprocess.run([TOOL, tool, root, out, "-h", "2", "-f", "0.1", "-C"] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert "min_count" not in r.stdout
        assert open(out, "rb").read() == want
    r = subprocess.run([TOOL, "classic-construct"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--min-count" in r.stderr


def test_two_builds_in_a_row_and_release(gpu_lib, oracle, construct, tmp_path):
    """buffer reuse and clearing: a second build in the same process, with another cutoff and other
    documents, starts from an empty table; after release_build_buffers the next build allocates anew"""
    from cobs_amd import construct as construct_api
    k, canon, nh = 31, 1, 1
    first, second = A.make_corpus(31, k, ndocs=14), A.make_corpus(32, k, ndocs=9)
    runs = [(first, 2), (second, 3), (first, 5), (first, 2)]
    for i, (docs, c) in enumerate(runs):
        kdocs, kept, total = A.memory_docs(oracle, construct, docs, k, canon, nh, c)
        assert 0 < kept < total
        want = _want(construct, "classic", kdocs, str(tmp_path / "w.cobs_classic"), k, canon, nh)
        got = _build(gpu_lib, "classic", _doclist(gpu_lib, docs), str(tmp_path / "g.cobs_classic"),
                     _params(gpu_lib, "classic", k, canon, nh, c, batch=0 if i % 2 else 5000))
        assert got == want, i
        if i == 2:
            construct_api.release_build_buffers()
    construct_api.release_build_buffers()
