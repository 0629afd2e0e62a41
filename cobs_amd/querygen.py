"""`cobs generate-queries` (reference src/cobs.cpp:734-959): labelled query sets drawn from a document
list.  Positives are random terms of the documents, negatives random ACGT sequences; with
true_negatives every document term is looked up on the GPU and negatives that hold one are dropped
(libcobs_gpu.so: cobs_amd/csrc/querygen.cpp, querygen_kernels.hip).  This module only binds it."""
import collections
import ctypes as C
import os

from . import _capi
from ._capi import QuerygenParams, QuerygenStats, check
from .construct import DocumentList

# header: the line of the query file without '>' ("doc:D:term:T:NAME" or "negativeI");
# doc_index is -1 for a negative (its term_index is then 0)
QueryRecord = collections.namedtuple("QueryRecord", "header sequence doc_index term_index")


class QuerySet(list):
    """the records in output order; .seed the seed used, .stats what the call read and probed"""
    seed = None
    stats = None


def generate_queries(input, out_file=None, term_size=31, positive=0, negative=0, true_negatives=False, size=0,
                     seed=None, file_type="any", canonical=False, device=-1, text_batch_bytes=0):
    """cobs generate-queries PATH [-k K] [-p N] [-n N] [-N] [-s SIZE] [-S SEED] [-o OUT]: `input` is a
    path or a DocumentList; the file (if out_file is given) is byte for byte the reference's format"""
    docs = input if isinstance(input, DocumentList) else DocumentList(input, file_type)
    if seed is None:
        seed = int.from_bytes(os.urandom(8), "little")
    p = QuerygenParams()
    p.struct_size = C.sizeof(QuerygenParams)
    p.term_size, p.num_positive, p.num_negative, p.size, p.seed = term_size, positive, negative, size, seed
    p.true_negatives, p.canonical, p.device = int(bool(true_negatives)), int(bool(canonical)), device
    p.text_batch_bytes = text_batch_bytes
    lib = _capi.load()
    h = C.c_void_p()
    check(lib.cobs_gpu_generate_queries(docs._h, C.byref(p), C.byref(h)))
    try:
        if out_file is not None:
            check(lib.cobs_gpu_query_set_write(h, docs._h, os.fsencode(out_file)))
        out = QuerySet()
        out.seed = seed
        st = QuerygenStats()
        check(lib.cobs_gpu_query_set_stats(h, C.byref(st)))
        out.stats = {f: getattr(st, f) for f, _ in QuerygenStats._fields_}
        names = {}
        text, n, d, t = C.c_void_p(), C.c_size_t(), C.c_uint64(), C.c_uint64()
        negatives = 0
        for i in range(lib.cobs_gpu_query_set_size(h)):
            check(lib.cobs_gpu_query_set_entry(h, i, C.byref(text), C.byref(n), C.byref(d), C.byref(t)))
            seq = C.string_at(text.value, n.value) if n.value else b""
            if d.value == 0xFFFFFFFFFFFFFFFF:
                out.append(QueryRecord("negative%d" % negatives, seq, -1, 0))
                negatives += 1
            else:
                di = int(d.value)
                if di not in names:
                    names[di] = docs[di].name
                out.append(QueryRecord("doc:%d:term:%d:%s" % (di, t.value, names[di]), seq, di, int(t.value)))
        return out
    finally:
        lib.cobs_gpu_query_set_free(h)
