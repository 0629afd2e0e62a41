"""The counting table of the min_count builder at its edges, on the GPU: known keys on the collision, wrap and
saturation paths of abundance_count_kernel (tests/abundance_table.py).  Every fixture is built classic and compact with
both ways of setting bits, and every build is checked twice: the file equals, byte for byte, the oracle's construction
over the occurrences abundance_check keeps, and the table the device leaves behind (cobs_gpu_last_count_table) equals
the linear-probing model -- same occupied slots, every owner a key with that tag, every count exact below the cutoff
and within [c, occurrences] from it on."""
import os

import numpy as np
import pytest

from tests import abundance_check as A
from tests import abundance_table as T

pytestmark = pytest.mark.gpu

NUM_HASHES = 2


def _doclist(cobs, docs):
    dl = cobs.DocumentList()
    for name, seqs in docs:
        dl.add_document(name, seqs)
    return dl


def _params(cobs, kind, k, canonicalize, c, mode, batch):
    p = cobs.CompactIndexParameters() if kind == "compact" else cobs.ClassicIndexParameters()
    p.term_size, p.canonicalize, p.num_hashes, p.false_positive_rate = k, canonicalize, NUM_HASHES, 0.1
    if kind == "compact":
        p.page_size = 2
    p.text_batch_bytes, p.set_bits_mode, p.clobber, p.min_count = batch, mode, True, c
    return p


def _want(construct, kind, kdocs, path, k, canonicalize):
    if kind == "compact":
        construct.compact_construct(kdocs, path, term_size=k, canonicalize=canonicalize, num_hashes=NUM_HASHES,
                                    false_positive_rate=0.1, page_size=2)
    else:
        construct.classic_construct(kdocs, path, term_size=k, canonicalize=canonicalize, num_hashes=NUM_HASHES,
                                    false_positive_rate=0.1)
    return open(path, "rb").read()


def _last_table():
    from cobs_amd import construct as construct_api
    return construct_api.last_count_table()


def _run(cobs, oracle, construct, tmp_path, fx, model=None, inp=None, kdocs=None):
    """the fixture through every builder: files against the filtered construction, tables against the model
    -> the tables read back"""
    assert len(fx.docs) <= 16 and [n for n, _ in fx.docs] == sorted(n for n, _ in fx.docs)    # one compact group, columns in list order
    model = model or T.last_batch_model(fx)
    assert model.cap == fx.cap
    if kdocs is None:
        kdocs, kept, total = A.memory_docs(oracle, construct, fx.docs, fx.k, fx.canonicalize, NUM_HASHES, fx.c)
        assert (kept > 0) == bool(fx.keep)
    tables = []
    for kind in ("classic", "compact"):
        want = _want(construct, kind, kdocs, str(tmp_path / ("w.cobs_" + kind)), fx.k, fx.canonicalize)
        build = cobs.compact_construct if kind == "compact" else cobs.classic_construct
        for mode in (1, 2):
            out = str(tmp_path / ("g.cobs_" + kind))
            p = _params(cobs, kind, fx.k, fx.canonicalize, fx.c, mode, fx.batch)
            if inp is None:
                build(list=_doclist(cobs, fx.docs), out_file=out, index_params=p)
            else:
                build(inp, out, p)
            table = _last_table()
            seen = T.check_table(model, table, fx.c)
            assert open(out, "rb").read() == want, (fx.name, kind, mode)
            for col, t in fx.keep:
                assert table[3][seen[model.key(col, t)]] >= fx.c
            for col, t in fx.drop:
                key = model.key(col, t)
                assert table[3][seen[key]] == model.multiplicity(key) < fx.c
            tables.append((table, seen))
    return model, tables


def _equal_tags_side_by_side(model, tables, key_a, key_b):
    """the two colliding keys sit in their common home slot and the next one, under one tag"""
    assert model.home[key_a] == model.home[key_b] and model.tag[key_a] == model.tag[key_b]
    home = model.home[key_a]
    for (cap, _, owner, _), seen in tables:
        assert {seen[key_a], seen[key_b]} == {home, (home + 1) & (cap - 1)}
        assert int(owner[home]) >> T.OFFSET_BITS == int(owner[(home + 1) & (cap - 1)]) >> T.OFFSET_BITS == model.tag[key_a]


PAIR_FIXTURES = T.pair_fixtures()


@pytest.mark.parametrize("fx", PAIR_FIXTURES, ids=[f.name for f in PAIR_FIXTURES])
def test_two_terms_of_one_document_with_equal_tag_and_home(gpu_lib, oracle, construct, tmp_path, fx):
    """P1 .. P6: only the compare of the hashed bytes keeps x and y apart (registers, byte view, one of each)"""
    model, tables = _run(gpu_lib, oracle, construct, tmp_path, fx)
    pair = next(p for n, p, _, _ in T.PAIRS if fx.name.startswith(n))
    _equal_tags_side_by_side(model, tables, model.key(0, pair[0]), model.key(0, pair[1]))


P7_FIXTURES = T.p7_fixtures()


@pytest.mark.parametrize("fx", P7_FIXTURES, ids=[f.name for f in P7_FIXTURES])
def test_one_term_in_two_documents_with_equal_tag_and_home(gpu_lib, oracle, construct, tmp_path, fx):
    """P7: only the document check keeps the two documents' counts apart"""
    model, tables = _run(gpu_lib, oracle, construct, tmp_path, fx)
    x, a, b = T.P7
    _equal_tags_side_by_side(model, tables, model.key(a, x), model.key(b, x))


@pytest.mark.parametrize("canonicalize", [1, 0])
@pytest.mark.parametrize("c", [2, 3])
def test_one_document_two_records(gpu_lib, oracle, construct, tmp_path, canonicalize, c):
    """a FASTA document with x once in each of two records: the same document, so the two occurrences count together"""
    from oracle import documents as D
    x = T.P7[0]
    root = str(tmp_path / "docs")
    os.makedirs(root)
    with open(os.path.join(root, "two.fasta"), "wb") as f:
        f.write(b">r1\n" + x + b"\n>r2\n" + x + b"\n")
    size = os.path.getsize(os.path.join(root, "two.fasta"))
    ents = D.document_list(root)
    assert len(ents) == 1
    kdocs, kept, total = A.entry_docs(oracle, construct, ents, 31, canonicalize, NUM_HASHES, c)
    assert total == 2 and kept == (2 if c == 2 else 0)
    fx = T.Fixture("two-records", 31, canonicalize, c, [("two", [x, x])], 512, [(0, x)] if c == 2 else [],
                   [] if c == 2 else [(0, x)], 1024)
    model = T.last_batch_model(fx, bounds=[size + 1])
    assert model.total == size + 1 and model.multiplicity(model.key(0, x)) == 2
    _run(gpu_lib, oracle, construct, tmp_path, fx, model=model, inp=root, kdocs=kdocs)


WRAP_FIXTURES = T.wrap_fixtures()


@pytest.mark.parametrize("fx", WRAP_FIXTURES, ids=[f.name for f in WRAP_FIXTURES])
def test_cluster_wraps_over_the_last_slot(gpu_lib, oracle, construct, tmp_path, fx):
    """slots 1020 .. 1023 and 0 .. 2 are one cluster; the terms found in slots 0 .. 2 have their home in slot 1023
    and were counted to their multiplicity there"""
    model, tables = _run(gpu_lib, oracle, construct, tmp_path, fx)
    for (cap, _, owner, count), seen in tables:
        wrapped = [key for key, s in seen.items() if s < 3]
        assert len(wrapped) == 3 and all(model.home[key] == 1023 for key in wrapped)
        assert sum(1 for key in wrapped if count[seen[key]] >= fx.c) >= 2


BOUNDARY_FIXTURES = T.boundary_fixtures()


@pytest.mark.parametrize("fx", BOUNDARY_FIXTURES, ids=[f.name for f in BOUNDARY_FIXTURES])
def test_multiplicity_on_the_cutoff(gpu_lib, oracle, construct, tmp_path, fx):
    """c - 1, c and c + 1 occurrences at c = 2, 255, 256, 300"""
    _run(gpu_lib, oracle, construct, tmp_path, fx)


HOT_FIXTURES = T.hot_fixtures()


@pytest.mark.parametrize("fx", HOT_FIXTURES, ids=[f.name for f in HOT_FIXTURES])
def test_thousands_of_threads_on_one_slot(gpu_lib, oracle, construct, tmp_path, fx):
    """a homopolymer: one build per case, kept or dropped exactly at the cutoff"""
    model, tables = _run(gpu_lib, oracle, construct, tmp_path, fx)
    assert len(model.occupied) == 1


CAPACITY_FIXTURES = T.capacity_fixtures()


@pytest.mark.parametrize("fx", CAPACITY_FIXTURES, ids=[f.name for f in CAPACITY_FIXTURES])
def test_table_size_at_the_doubling_boundaries(gpu_lib, oracle, construct, tmp_path, fx):
    """512 | 513 and 1024 | 1025 text bytes, and one document of exactly k bytes"""
    model, tables = _run(gpu_lib, oracle, construct, tmp_path, fx)
    for (cap, total, owner, _), _ in tables:
        assert cap == fx.cap and total == model.total and 2 * int(np.count_nonzero(owner)) <= cap


def test_a_smaller_table_after_a_larger_one_and_release(gpu_lib, oracle, construct, tmp_path):
    """the table of a build holds nothing of the build before it, whichever was larger; without min_count the last
    table stays as it was; after release_build_buffers there is none"""
    from cobs_amd import construct as construct_api
    by_name = {f.name: f for f in T.all_fixtures()}
    caps = []
    for name in ("capacity-1025", "wrap-canon1-c2", "hot-A5000-canon1-c2", "smallest-k31", "capacity-513"):
        model, tables = _run(gpu_lib, oracle, construct, tmp_path, by_name[name])
        caps.append(tables[-1][0][0])
    assert caps == [4096, 1024, 16384, 1024, 2048]
    before = _last_table()
    fx = by_name["capacity-512"]
    gpu_lib.classic_construct(list=_doclist(gpu_lib, fx.docs), out_file=str(tmp_path / "plain.cobs_classic"),
                              index_params=_params(gpu_lib, "classic", fx.k, fx.canonicalize, 1, 1, fx.batch))
    after = _last_table()
    assert after[:2] == before[:2] and np.array_equal(after[2], before[2]) and np.array_equal(after[3], before[3])
    construct_api.release_build_buffers()
    assert _last_table() is None
    _run(gpu_lib, oracle, construct, tmp_path, by_name["wrap-canon0-c3"])
    construct_api.release_build_buffers()
    assert _last_table() is None
