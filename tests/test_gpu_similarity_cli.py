"""GPU: `cobs_gpu_query doc-similarity` (ClassicSearch::doc_shared_bits / similar_documents, the C++ mirror, through the
tool) against the numpy checker (tests/similarity_check.py): a classic index of 300 documents with planted duplicates and
a compact index of three pages of 16.  Integers compare exactly, floats after parsing within the tolerance of the estimate
test (test_similarity_cpu.py: 1e-12 * max(1, n(t_or)))."""
import os
import subprocess

import numpy as np
import pytest

from oracle import construct as K
from tests import fill_check
from tests import similarity_check as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")
H = 3


def _run(*args):
    assert os.path.exists(TOOL), "build cobs_amd/cobs_gpu_query first (make -C cobs_amd/csrc)"
    return subprocess.run([TOOL, "doc-similarity"] + list(args), capture_output=True, text=True, timeout=300)


def _columns(rng, S, slots, D, density=0.3):
    cols = (rng.random((S, slots)) < density).astype(np.uint8)
    cols[:, D:] = 0
    return cols


def _make_classic(d):
    """D = 300: 17 a copy of 5, 250 a copy of 5 with a tenth of its bits cleared, 299 a copy of 298, 40 saturated"""
    rng = np.random.default_rng(7)
    S, D = 2003, 300
    cols = _columns(rng, S, 304, D)
    cols[:, 17] = cols[:, 5]
    cols[:, 250] = cols[:, 5] & (rng.random(S) < 0.9)
    cols[:, 299] = cols[:, 298]
    cols[:, 40] = 1
    p = os.path.join(str(d), "a.cobs_classic")
    K.write_classic(p, 31, 1, ["doc_%05d" % i for i in range(D)], S, H, np.packbits(cols, axis=1, bitorder="little"))
    return p, fill_check.read_index(p)


def _make_compact(d):
    """page_size 2, three pages of 16 slots with their own S_p, 43 documents (the last page holds 5 padding slots);
    duplicates inside pages 0 and 2, and document 20 (page 1) a copy of document 3's bits as far as its shorter page goes"""
    rng = np.random.default_rng(8)
    sigs, ps, D = [601, 97, 1301], 2, 43
    cols = [_columns(rng, s, 16, D - 16 * i) for i, s in enumerate(sigs)]
    cols[0][:, 9] = cols[0][:, 3]
    cols[1][:, 4] = cols[0][:97, 3]
    cols[2][:, 10] = cols[2][:, 0]
    cols[2][:, 7] = cols[2][:, 0] & (rng.random(1301) < 0.8)
    p = os.path.join(str(d), "b.cobs_compact")
    K.write_compact(p, 31, 1, ps, [(s, H) for s in sigs], ["doc_%05d" % i for i in range(D)],
                    [np.packbits(c, axis=1, bitorder="little") for c in cols])
    return p, fill_check.read_index(p)


@pytest.fixture(scope="module")
def classic(tmp_path_factory):
    return _make_classic(tmp_path_factory.mktemp("simcli"))


@pytest.fixture(scope="module")
def compact(tmp_path_factory):
    return _make_compact(tmp_path_factory.mktemp("simcli"))


def _bits(ix, d):
    per = SC.page_docs(ix)
    return int(SC.unpack(ix["mats"][d // per])[:, d % per].sum())


def _want_like(ix, ref, **kw):
    """the checker's lines of one reference: (ref, doc, sub-index, shared, bit_jaccard, jaccard, c_ref_in_doc, c_doc_in_ref, tol)"""
    per = SC.page_docs(ix)
    p = ref // per
    names = ix["names"]
    out = []
    for name, j, cab, cba, sh in SC.similar(ix, ref, **kw):
        a, b = _bits(ix, ref), _bits(ix, names.index(name))
        t_or = a + b - sh
        tol = 1e-12 * max(1.0, SC.n_of(t_or, ix["sigs"][p], ix["num_hashes"])) if t_or < ix["sigs"][p] else 1e-12
        out.append((names[ref], name, p, sh, sh / t_or if t_or else 0.0, j, cab, cba, tol))
    return out


def _want_pairs(ix, J):
    names = ix["names"]
    out = []
    for a, b, p, sh, bj, j, cab, cba in SC.all_pairs(ix, J):
        t_or = _bits(ix, a) + _bits(ix, b) - sh
        tol = 1e-12 * max(1.0, SC.n_of(t_or, ix["sigs"][p], ix["num_hashes"])) if t_or < ix["sigs"][p] else 1e-12
        out.append((names[a], names[b], p, sh, bj, j, cab, cba, tol))
    return out


def _assert_lines(stdout, want):
    lines = stdout.splitlines()
    assert len(lines) == len(want), (len(lines), len(want))
    for ln, w in zip(lines, want):
        f = ln.split("\t")
        assert len(f) == 8, ln
        assert (f[0], f[1], int(f[2]), int(f[3])) == w[:4], (ln, w)
        for g, x in zip(f[4:], w[4:8]):
            g = float(g)
            assert (g != g and x != x) or abs(g - x) <= w[8], (ln, w)


def test_like(gpu_lib, classic, compact):
    p, ix = classic
    r = _run(p, "--like", "doc_00005")
    assert r.returncode == 0, r.stderr
    want = _want_like(ix, 5)
    assert len(want) == 299 and [w[1] for w in want[:2]] == ["doc_00017", "doc_00250"] and want[0][5] == 1.0
    assert want[-1][1] == "doc_00040" and want[-1][5] != want[-1][5]          # the saturated filter: NaN, after every finite one
    _assert_lines(r.stdout, want)
    # several references (any order, one repeated), a threshold and -l N
    r = _run(p, "--like", "doc_00299,doc_00005,doc_00040,doc_00299", "--min-jaccard", "0.5", "-l", "1")
    assert r.returncode == 0, r.stderr
    want = [w for ref in (299, 5, 40, 299) for w in _want_like(ix, ref, min_jaccard=0.5, num_results=1)]
    assert [(w[0], w[1]) for w in want] == [("doc_00299", "doc_00298"), ("doc_00005", "doc_00017"), ("doc_00299", "doc_00298")]
    _assert_lines(r.stdout, want)
    r = _run(p, "--like", "doc_00005", "-l", "7")
    assert r.returncode == 0, r.stderr
    _assert_lines(r.stdout, _want_like(ix, 5, num_results=7))
    # compact: a reference's list stays inside its page
    p, ix = compact
    r = _run(p, "--like", "doc_00003,doc_00020,doc_00042")
    assert r.returncode == 0, r.stderr
    want = [w for ref in (3, 20, 42) for w in _want_like(ix, ref)]
    assert len(want) == 15 + 15 + 10 and want[0][:3] == ("doc_00003", "doc_00009", 0)
    assert all(w[2] == int(w[0][4:]) // 16 == int(w[1][4:]) // 16 for w in want)
    _assert_lines(r.stdout, want)


def test_all_pairs(gpu_lib, classic, compact):
    p, ix = classic
    r = _run(p, "--all-pairs", "--min-jaccard", "0.5")
    assert r.returncode == 0, r.stderr
    want = _want_pairs(ix, 0.5)
    assert [(w[0], w[1]) for w in want] == [("doc_00005", "doc_00017"), ("doc_00005", "doc_00250"), ("doc_00017", "doc_00250"),
                                            ("doc_00298", "doc_00299")]
    _assert_lines(r.stdout, want)
    p, ix = compact
    for J in (0.4, 0.0):                # 0: no threshold, every pair of every page
        r = _run(p, "--all-pairs", "--min-jaccard", repr(J))
        assert r.returncode == 0, r.stderr
        want = _want_pairs(ix, J)
        _assert_lines(r.stdout, want)
        pairs = [tuple(ln.split("\t")[:2]) for ln in r.stdout.splitlines()]
        assert len(set(pairs)) == len(pairs) and all(a < b for a, b in pairs)               # each pair once, a < b
        assert all(int(a[4:]) // 16 == int(b[4:]) // 16 for a, b in pairs)                  # none across pages
        assert pairs == sorted(pairs)                                                        # sub-index by sub-index, (a, b) order
    assert len(pairs) == 2 * (16 * 15 // 2) + 11 * 10 // 2
    want = [(w[0], w[1]) for w in _want_pairs(ix, 0.4)]
    assert want == [("doc_00003", "doc_00009"), ("doc_00032", "doc_00039"), ("doc_00032", "doc_00042"), ("doc_00039", "doc_00042")]
    assert ("doc_00003", "doc_00020") not in pairs          # equal bits in different sub-indexes: not comparable, not listed


def test_refused_invocations(gpu_lib, classic):
    p, _ix = classic
    r = _run(p, "--all-pairs")
    assert r.returncode != 0 and "--min-jaccard" in r.stderr and r.stdout == ""
    r = _run(p, "--like", "doc_00005,no_such_doc")
    assert r.returncode != 0 and "no_such_doc" in r.stderr and r.stdout == ""
