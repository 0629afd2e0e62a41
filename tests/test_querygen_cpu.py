"""generate-queries without a device: the C ABI and its bindings, argument errors ahead of any device
work, and a Python restatement of the random draws (the contract of cobs_gpu_generate_queries, which
tests/test_gpu_querygen.py checks the library against on the GPU)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

_G = 0x9E3779B97F4A7C15
_M = (1 << 64) - 1


def draw(seed, i):
    """draw i of seed S: the splitmix64 finaliser of S + i * 0x9E3779B97F4A7C15 (+ its own increment)"""
    z = (seed + i * _G + _G) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


class Draws:
    def __init__(self, seed):
        self.seed, self.i = seed, 0

    def next(self):
        v = draw(self.seed, self.i)
        self.i += 1
        return v

    def bases(self, n):
        return bytes(b"ACGT"[self.next() % 4] for _ in range(n))


class Unreached(Exception):
    pass


class NotEnoughNegatives(Exception):
    pass


def restate(docs, k, positive, negative, true_negatives, size, seed, canonical=False, canon=None):
    """The contract, step by step.  docs: [(name, num_terms, terms_fn)] in list order, where
    terms_fn() gives the document's terms in process_terms order.  -> (records, stats) where a
    record is (header, sequence, doc_index, term_index)."""
    prefix = [0]
    for _, nt, _ in docs:
        prefix.append(prefix[-1] + nt)
    total = prefix[-1]
    size = max(size, k)
    rng = Draws(seed)
    chosen = set()
    while len(chosen) < positive:
        chosen.add(rng.next() % total)
    pos = sorted(chosen)
    ncand = (3 * negative + 1) // 2
    cands = [rng.bases(size) for _ in range(ncand)]
    # the documents read: all of them with -N, else those holding a positive
    doc_terms, read = {}, 0
    out_pos = []
    for d, (name, nt, terms_fn) in enumerate(docs):
        mine = [g - prefix[d] for g in pos if prefix[d] <= g < prefix[d + 1]]
        if not mine and not true_negatives:
            continue
        read += 1
        terms = terms_fn()
        doc_terms[d] = terms
        for t in mine:
            if t >= len(terms):
                raise Unreached(name)
            out_pos.append((d, t, terms[t]))
    removed = 0
    survivors = cands
    if true_negatives and ncand:
        key = (lambda t: canon(t)) if canonical else (lambda t: t)
        seen = set()
        for terms in doc_terms.values():
            for t in terms:
                if all(c in b"ACGT" for c in t):
                    seen.add(key(t))
        hit = [any(key(c[i:i + k]) in seen for i in range(size - k + 1)) for c in cands]
        removed = sum(hit)
        survivors = [c for c, h in zip(cands, hit) if not h]
    if len(survivors) < negative:
        raise NotEnoughNegatives()
    q = []
    for d, t, term in out_pos:
        if size > k:
            pad = size - k
            front = rng.next() % pad
            f = rng.bases(front)
            b = rng.bases(pad - front)
            term = f + term + b
        q.append((d, t, term))
    q += [(-1, 0, c) for c in survivors[:negative]]
    for i in range(len(q) - 1, 0, -1):
        j = rng.next() % (i + 1)
        q[i], q[j] = q[j], q[i]
    recs, neg = [], 0
    for d, t, s in q:
        if d < 0:
            recs.append(("negative%d" % neg, s, -1, 0))
            neg += 1
        else:
            recs.append(("doc:%d:term:%d:%s" % (d, t, docs[d][0]), s, d, t))
    return recs, {"documents_read": read, "negatives_removed": removed}


def file_text(records):
    return b"".join(b">" + h.encode("latin-1") + b"\n" + s + b"\n" for h, s, _, _ in records)


# ---------------------------------------------------------------------------------------------

def test_symbols_bound_and_declared():
    from cobs_amd import _capi
    lib = _capi.load()
    text = open(os.path.join(ROOT, "include", "cobs_gpu_construct.h")).read()
    for n in ("cobs_gpu_generate_queries", "cobs_gpu_query_set_size", "cobs_gpu_query_set_entry",
              "cobs_gpu_query_set_write", "cobs_gpu_query_set_stats", "cobs_gpu_query_set_free"):
        assert n in _capi.SYMBOLS and hasattr(lib, n)
        assert re.search(r"\b%s\s*\(" % n, text)
        assert n not in open(os.path.join(ROOT, "include", "cobs_gpu.h")).read()
    import cobs_amd
    assert cobs_amd.generate_queries is not None and "generate_queries" in cobs_amd.__all__


def test_params_struct_matches_header(tmp_path):
    from cobs_amd import _capi
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cobs_gpu_construct.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(cobs_gpu_querygen_params), '
                   'offsetof(cobs_gpu_querygen_params, text_batch_bytes), sizeof(cobs_gpu_querygen_stats), '
                   'offsetof(cobs_gpu_querygen_stats, kernel_ms)); return 0; }\n')
    import subprocess
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_capi.QuerygenParams), _capi.QuerygenParams.text_batch_bytes.offset,
                   C.sizeof(_capi.QuerygenStats), _capi.QuerygenStats.kernel_ms.offset]


def test_argument_errors_come_before_the_device():
    import cobs_amd
    from cobs_amd import _capi
    fasta = os.path.join(GOLDEN, "fasta")
    for kw in (dict(term_size=0, positive=1), dict(positive=10 ** 9)):
        with pytest.raises(cobs_amd.CobsGpuError) as e:
            cobs_amd.generate_queries(fasta, seed=1, **kw)
        assert e.value.status == _capi.ERR_ARG, kw
    lib = _capi.load()
    p = _capi.QuerygenParams()
    p.struct_size = 8
    p.term_size = 31
    h = C.c_void_p()
    dl = cobs_amd.DocumentList(fasta)
    assert lib.cobs_gpu_generate_queries(dl._h, C.byref(p), C.byref(h)) == _capi.ERR_ARG
    # an in-memory list is a list like any other
    mem = cobs_amd.DocumentList()
    mem.add_document("m", [b"ACGTACGTAC"])
    with pytest.raises(cobs_amd.CobsGpuError) as e:
        cobs_amd.generate_queries(mem, term_size=4, positive=8, seed=1)
    assert e.value.status == _capi.ERR_ARG          # 7 terms


def test_draws_pinned_splitmix64_vector():
    assert [draw(0, i) for i in range(3)] == [0xe220a8397b1dcdaf, 0x6e789e6aa1b965f4, 0x06c45d188009454f]


def test_hand_sized_selection_padding_and_shuffle():
    """Two documents of 3 and 2 terms (k = 2), pinned by hand from the draws of seed 0.
    draw % 5 = 0, 0, 4: the positives are global terms {0, 4} = a:0 "AC" and b:1 "TA".
    ceil(1.5 * 1) = 2 candidates of 4 bases, draws 3..10 % 4: 0 3 2 1 -> "ATGC", then the second.
    Padding (pad 2, ascending index): "AC" -> front 0, back "TT"; "TA" -> front "T", back "C".
    Then the shuffle of [ACTT, TTAC, ATGC] from the end."""
    assert [draw(0, i) % 5 for i in range(3)] == [0, 0, 4]
    assert bytes(b"ACGT"[draw(0, i) % 4] for i in range(3, 7)) == b"ATGC"
    docs = [("a", 3, lambda: [b"AC", b"CG", b"GT"]), ("b", 2, lambda: [b"TT", b"TA"])]
    recs, st = restate(docs, 2, 2, 1, False, 4, 0)
    assert recs == [("doc:1:term:1:b", b"TTAC", 1, 1), ("doc:0:term:0:a", b"ACTT", 0, 0), ("negative0", b"ATGC", -1, 0)]
    assert st == {"documents_read": 2, "negatives_removed": 0}
    assert file_text(recs) == b">doc:1:term:1:b\nTTAC\n>doc:0:term:0:a\nACTT\n>negative0\nATGC\n"
    # size = k: no padding draws; 3 positives and 2 negatives of seed 7
    recs, _ = restate(docs, 2, 3, 2, False, 2, 7)
    assert recs == [("doc:1:term:1:b", b"TA", 1, 1), ("negative0", b"CG", -1, 0), ("doc:0:term:2:a", b"GT", 0, 2),
                    ("negative1", b"TG", -1, 0), ("doc:0:term:1:a", b"CG", 0, 1)]
