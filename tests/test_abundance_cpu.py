"""The abundance cutoff (min_count) without a GPU: known answers of the plain-Python restatement
(tests/abundance_check.py), the corpora of the GPU test are not vacuous, and the public interface
carries the field (Python parameters, C ABI)."""
import os
import subprocess

import numpy as np
import pytest

from tests import abundance_check as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

S40 = b"ACGGTCATTGCAAGCTTAGGCATCGATCCGTAAGCTTGCA"          # 40 bases, no 31-mer repeats inside
T35 = b"TTGACCGTAGGCTAACGTCAGGATCCATGCAAGTC"


def _kept(seqs, k, canon, c):
    kept, total = A.kept_occurrences(seqs, k, canon, c)
    return kept.tolist(), total


def test_sequence_repeated_one_two_three_times():
    n = len(S40) - 31 + 1                                    # 10 terms per copy
    for copies in (1, 2, 3):
        seqs = [S40] * copies
        for c in (0, 1, 2, 3, 4):
            kept, total = _kept(seqs, 31, 1, c)
            assert total == copies * n
            assert kept == (list(range(total)) if copies >= max(c, 1) else []), (copies, c)
    # a second, different sequence next to two copies: only the copies' terms reach 2
    kept, total = _kept([S40, T35, S40], 31, 1, 2)
    assert total == 10 + 5 + 10 and kept == list(range(10)) + list(range(15, 25))


def test_reverse_complement_counts_together_only_when_canonical():
    rc = A.revcomp(S40)
    assert rc != S40
    # canonicalize = 1: term i of S40 and term 9 - i of its reverse complement are the same term
    kept, total = _kept([S40, rc], 31, 1, 2)
    assert total == 20 and kept == list(range(20))
    assert A.canonical_bytes(S40[:31], 1) == A.canonical_bytes(rc[9:40], 1)
    # canonicalize = 0: they are different byte strings, nothing occurs twice
    assert _kept([S40, rc], 31, 0, 2) == ([], 20)
    assert _kept([S40, rc, S40], 31, 0, 2) == (list(range(10)) + list(range(20, 30)), 30)


def test_invalid_characters_follow_the_builder():
    a, b = bytearray(S40), bytearray(S40)
    a[12], b[12] = ord("N"), ord("X")
    # canonicalize = 1 maps both to 0: every term occurs twice; canonicalize = 0 keeps the 9 terms
    # that do not cover position 12 ... of which there are none below 31 + 12 - 40: terms 0..9 all cover it
    assert _kept([bytes(a), bytes(b)], 31, 1, 2) == (list(range(20)), 20)
    assert _kept([bytes(a), bytes(b)], 31, 0, 2) == ([], 20)
    assert _kept([bytes(a), bytes(b)], 20, 0, 2)[0] == list(range(13, 21)) + list(range(21 + 13, 42))


def test_repeat_across_a_sequence_boundary_is_not_a_term():
    # S40 once whole and once cut into two sequences: the cut copy holds only the terms that fit
    # into one of its pieces, so only those occur twice
    cut = [S40[:35], S40[35:]]
    kept, total = _kept([S40] + cut, 31, 1, 2)
    assert total == 10 + 5 + 0
    assert kept == [0, 1, 2, 3, 4, 10, 11, 12, 13, 14]
    # glued together instead, every term of S40 occurs twice and the junction terms once
    kept, total = _kept([S40 + S40], 31, 1, 2)
    assert total == 50 and kept == list(range(10)) + list(range(40, 50))


@pytest.mark.parametrize("canonicalize,num_hashes,k", A.PARAMS)
def test_corpora_are_not_vacuous(canonicalize, num_hashes, k):
    """every parametrised corpus of the GPU test keeps a non-empty strict subset at c >= 2"""
    docs = A.make_corpus(7 + k, k)
    text = sum(len(b"\n".join(s)) + 1 for _, s in docs)
    assert text > 4 * A.TEXT_BATCH                           # several batches ...
    assert max(len(b"\n".join(s)) + 1 for _, s in docs) * 3 < A.TEXT_BATCH     # ... of several documents each
    for c in A.CUTOFFS:
        kept = total = 0
        for _, seqs in docs:
            kp, tt = A.kept_occurrences(seqs, k, canonicalize, c)
            kept += len(kp)
            total += tt
        print("k=%d canonicalize=%d c=%d kept %d of %d" % (k, canonicalize, c, kept, total))
        if c == 1:
            assert kept == total
        else:
            assert 0.10 * total <= kept <= 0.90 * total, (c, kept, total)
    # the shared segment occurs once in each of documents 8..19: twelve times in the batch-spanning
    # corpus, never twice in a document
    _, shared = A.make_corpus(7 + k, k, return_shared=True)
    want = [A.canonical_bytes(shared[i:i + k], canonicalize) for i in range(len(shared) - k + 1)]
    for name, seqs in docs[8:20]:
        keys = [A.canonical_bytes(s[i:i + k], canonicalize) for s in seqs for i in range(len(s) - k + 1)]
        assert all(keys.count(w) == 1 for w in want), name


def test_cutoff_one_is_the_unfiltered_index(oracle, construct, tmp_path):
    """at c = 1 the restatement keeps every occurrence: the oracle-built files equal the unfiltered ones"""
    k, canon, nh = 31, 1, 2
    docs = A.make_corpus(3, k, ndocs=12)
    plain = []
    for name, seqs in docs:
        hs = [oracle.term_hashes(s, k, canon, nh)[0] for s in seqs if len(s) >= k]
        plain.append(construct.Doc(name, name, len(b"\n".join(seqs)) + 1, sum(max(len(s) - k + 1, 0) for s in seqs),
                                   np.concatenate(hs)))
    for c in (0, 1):
        kdocs, kept, total = A.memory_docs(oracle, construct, docs, k, canon, nh, c)
        assert kept == total
        a, b = str(tmp_path / "a.cobs_classic"), str(tmp_path / "b.cobs_classic")
        construct.classic_construct(plain, a, num_hashes=nh, false_positive_rate=0.1)
        construct.classic_construct(kdocs, b, num_hashes=nh, false_positive_rate=0.1)
        assert open(a, "rb").read() == open(b, "rb").read()
        a, b = str(tmp_path / "a.cobs_compact"), str(tmp_path / "b.cobs_compact")
        construct.compact_construct(plain, a, num_hashes=nh, false_positive_rate=0.1, page_size=1)
        construct.compact_construct(kdocs, b, num_hashes=nh, false_positive_rate=0.1, page_size=1)
        assert open(a, "rb").read() == open(b, "rb").read()
    # and a cutoff of 2 changes the matrix but not its geometry
    kdocs, kept, total = A.memory_docs(oracle, construct, docs, k, canon, nh, 2)
    assert 0 < kept < total
    b2 = str(tmp_path / "b2.cobs_classic")
    construct.classic_construct(kdocs, b2, num_hashes=nh, false_positive_rate=0.1)
    x, y = open(a.replace("compact", "classic"), "rb").read(), open(b2, "rb").read()
    assert len(x) == len(y) and x != y


def test_python_parameters_carry_min_count():
    import cobs_amd
    from cobs_amd import _capi, construct as K
    assert cobs_amd.ClassicIndexParameters().min_count == 1
    assert cobs_amd.CompactIndexParameters().min_count == 1
    p = cobs_amd.CompactIndexParameters()
    p.min_count = 3
    b = K._params(p, -1)
    assert b.min_count == 3 and b.struct_size == 64
    assert _capi.BuildParams.min_count.offset == 60 and _capi.BuildParams.min_count.size == 4
    assert K._params(cobs_amd.ClassicIndexParameters(), -1).min_count == 1


C_UNIT = r"""
#include <stddef.h>
#include "cobs_gpu_construct.h"
/* the layout of the struct before the field had a name: the last word was `reserved` */
typedef struct before {
    uint32_t struct_size, term_size, canonicalize, num_hashes;
    double false_positive_rate;
    uint64_t signature_size, page_size;
    int32_t device;
    uint32_t text_batch_bytes;
    const uint64_t* doc_terms;
    uint32_t set_bits_mode;
    uint32_t reserved;
} before;
#define SAME(name, x) typedef char name[(x) ? 1 : -1]
SAME(size_is_the_old_one, sizeof(cobs_gpu_build_params) == sizeof(before));
SAME(size_is_64, sizeof(cobs_gpu_build_params) == 64);
SAME(min_count_took_the_reserved_word, offsetof(cobs_gpu_build_params, min_count) == offsetof(before, reserved));
SAME(set_bits_mode_stays, offsetof(cobs_gpu_build_params, set_bits_mode) == offsetof(before, set_bits_mode));
SAME(doc_terms_stays, offsetof(cobs_gpu_build_params, doc_terms) == offsetof(before, doc_terms));
int main(void) {
    cobs_gpu_build_params p = {0};
    p.struct_size = sizeof p;
    p.min_count = 2;
    return p.min_count == 2 ? 0 : 1;
}
"""


def test_c99_unit_sets_min_count(tmp_path):
    src = tmp_path / "unit.c"
    src.write_text(C_UNIT)
    exe = str(tmp_path / "unit")
    cc = os.environ.get("CC", "cc")
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", exe])
    assert subprocess.call([exe]) == 0
