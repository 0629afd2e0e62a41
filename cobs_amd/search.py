"""Host-side mirror of the reference's Python operator API for the query path.

Reference: python/module.cpp:351-386 --
    cobs_index.Search(path).search(query, threshold=0.0, num_results=0)
        -> list[SearchResult(doc_name: str, score: int)]
Same names, argument meaning and defaults.  Everything is computed by
libcobs_gpu.so on the GPU; this file only marshals arguments.  Where the
reference terminates the process on bad input (short query, non-ACGT base,
unreadable index: classic_search.cpp:431-433, :93-96, :61-63) this mirror raises
CobsGpuError carrying the C-ABI status instead.
"""
import collections.abc
import ctypes as C
import os
import sys

import numpy as np

from . import _capi
from ._capi import BestHit, CobsGpuError, GroupHit, Hit, IndexInfo, Options, SetHit, SetQuorumHit, Synth, check


class SearchResult:
    """cobs::SearchResult (query/search.hpp:17-27) as exposed by python/module.cpp:351-362."""
    __slots__ = ("doc_name", "score")

    def __init__(self, doc_name="", score=0):
        self.doc_name = doc_name
        self.score = score

    def __repr__(self):
        return "SearchResult(doc_name=%r, score=%d)" % (self.doc_name, self.score)

    def __eq__(self, other):
        return (isinstance(other, SearchResult) and self.doc_name == other.doc_name
                and self.score == other.score)


class GroupResult:
    """one document of a group's result (Search.search_groups): the sum of the scores of the group's queries in it and the
    number of those queries it was a hit of at read_threshold"""
    __slots__ = ("doc_name", "score", "votes")

    def __init__(self, doc_name="", score=0, votes=0):
        self.doc_name = doc_name
        self.score = score
        self.votes = votes

    def __repr__(self):
        return "GroupResult(doc_name=%r, score=%d, votes=%d)" % (self.doc_name, self.score, self.votes)

    def __eq__(self, other):
        return (isinstance(other, GroupResult) and self.doc_name == other.doc_name and self.score == other.score
                and self.votes == other.votes)


class BestResult:
    """one document of a group's result (Search.search_best): the group's best query in it -- `query`, its index in the
    call --, that query's score and the positions the score is out of, and how many of the group's queries fit equally
    well (ties, the best one included)"""
    __slots__ = ("doc_name", "file_no", "doc", "query", "score", "positions", "ties")

    def __init__(self, doc_name="", file_no=0, doc=0, query=0, score=0, positions=0, ties=0):
        self.doc_name = doc_name
        self.file_no = file_no
        self.doc = doc
        self.query = query
        self.score = score
        self.positions = positions
        self.ties = ties

    def _key(self):
        return (self.doc_name, self.file_no, self.doc, self.query, self.score, self.positions, self.ties)

    def __repr__(self):
        return "BestResult(doc_name=%r, file_no=%d, doc=%d, query=%d, score=%d, positions=%d, ties=%d)" % self._key()

    def __eq__(self, other):
        return isinstance(other, BestResult) and self._key() == other._key()


class AdjustedResult(SearchResult):
    """a SearchResult that also says what its score is worth (Search.search_adjusted): expected_fp = the positions the
    document's filter fill alone is expected to hit, adjusted = the estimate of the positions that are truly shared"""
    __slots__ = ("expected_fp", "adjusted")

    def __init__(self, doc_name="", score=0, expected_fp=0.0, adjusted=0.0):
        SearchResult.__init__(self, doc_name, score)
        self.expected_fp = expected_fp
        self.adjusted = adjusted

    def __repr__(self):
        return "AdjustedResult(doc_name=%r, score=%d, expected_fp=%.2f, adjusted=%.2f)" % (
            self.doc_name, self.score, self.expected_fp, self.adjusted)


class WeightedResult(SearchResult):
    """one document of a weighted result (Search.search_weighted): score = the sum of the IDF weights of the query positions
    the document holds, total_weight = W(q, f), the sum over all positions of the query in the document's file"""
    __slots__ = ("total_weight",)

    def __init__(self, doc_name="", score=0, total_weight=0):
        SearchResult.__init__(self, doc_name, score)
        self.total_weight = total_weight

    def __repr__(self):
        return "WeightedResult(doc_name=%r, score=%d, total_weight=%d)" % (self.doc_name, self.score, self.total_weight)


class SetResult:
    """one set of documents of a set result (Search.search_sets): any = the positions of the query at least one member of
    the set holds, all = the positions every member holds; name = the set's name (its number as text when the labels were
    given as numbers)"""
    __slots__ = ("file_no", "set", "name", "any", "all")

    def __init__(self, file_no=0, set=0, name="", any=0, all=0):
        self.file_no = file_no
        self.set = set
        self.name = name
        self.any = any
        self.all = all

    def __repr__(self):
        return "SetResult(file_no=%d, set=%d, name=%r, any=%d, all=%d)" % (self.file_no, self.set, self.name, self.any, self.all)

    def __eq__(self, other):
        return (isinstance(other, SetResult) and (self.file_no, self.set, self.name, self.any, self.all) ==
                (other.file_no, other.set, other.name, other.any, other.all))


class SetQuorumResult:
    """one set of documents of a quorum result (Search.search_sets_quorum): core = the positions of the query that at least
    need = max(1, ceil(quorum * members)) members of the set hold, any = the positions at least one member holds; name = the
    set's name (its number as text when the labels were given as numbers)"""
    __slots__ = ("file_no", "set", "name", "core", "any")

    def __init__(self, file_no=0, set=0, name="", core=0, any=0):
        self.file_no = file_no
        self.set = set
        self.name = name
        self.core = core
        self.any = any

    def __repr__(self):
        return "SetQuorumResult(file_no=%d, set=%d, name=%r, core=%d, any=%d)" % (self.file_no, self.set, self.name, self.core, self.any)

    def __eq__(self, other):
        return (isinstance(other, SetQuorumResult) and (self.file_no, self.set, self.name, self.core, self.any) ==
                (other.file_no, other.set, other.name, other.core, other.any))


def doc_set_labels(labels, doc_names):
    """the labels of one file as cobs_gpu_set_doc_sets takes them -> (uint32 [len(doc_names)], set names): `labels` is an
    integer array with one entry per document, -1 (or 0xFFFFFFFF) for "in no set" -- the sets are then named by their
    numbers --, or a {document name: set name} mapping -- the set names are numbered in sorted order, a document the mapping
    does not name is in no set, a name the index does not hold is a ValueError that names it.  Host arithmetic only."""
    n = len(doc_names)
    if isinstance(labels, collections.abc.Mapping):
        known = {name: d for d, name in enumerate(doc_names)}
        for name in labels:
            if name not in known:
                raise ValueError("set_doc_sets: the index holds no document named %r" % (name,))
        names = sorted({str(v) for v in labels.values()})
        number = {s: i for i, s in enumerate(names)}
        out = np.full(n, _capi.NO_SET, dtype=np.uint32)
        for name, s in labels.items():
            out[known[name]] = number[str(s)]
        return out, names
    arr = np.asarray(labels)
    if arr.ndim != 1 or len(arr) != n:
        raise ValueError("set_doc_sets: one label per document (%d), got shape %s" % (n, arr.shape))
    if arr.dtype.kind not in "iu":
        raise ValueError("set_doc_sets: integer labels, -1 for a document in no set")
    wide = arr.astype(np.int64)
    wide[wide == _capi.NO_SET] = -1
    if (wide < -1).any() or (wide >= _capi.NO_SET).any():
        raise ValueError("set_doc_sets: a label is a set number >= 0, or -1")
    out = np.where(wide < 0, _capi.NO_SET, wide).astype(np.uint32)
    n_sets = int(wide.max()) + 1 if n and wide.max() >= 0 else 0
    return out, [str(i) for i in range(n_sets)]


def fpr_adjust(score, positions, bits, sig, num_hashes, z=0):
    """What a score is worth, from the document's filter fill (host arithmetic in double, no device; scalars or arrays):
    fill = bits / sig, fpr = fill ** num_hashes (a k-mer unrelated to the document hits it), q = fpr ** (z + 1) (a findere
    window of z + 1 such k-mers), expected_fp = positions * q, and the method-of-moments estimate of the positions that
    are truly shared, adjusted = max(0, (score - expected_fp) / (1 - q)), 0 where q >= 1 (a saturated filter says nothing).
    -> (expected_fp, adjusted) as float64"""
    s = np.asarray(score, dtype=np.float64)
    P = np.asarray(positions, dtype=np.float64)
    fill = np.asarray(bits, dtype=np.float64) / np.asarray(sig, dtype=np.float64)
    q = np.power(np.power(fill, float(num_hashes)), float(int(z) + 1))
    expected = P * q
    sat = q >= 1.0
    adjusted = np.where(sat, 0.0, np.maximum(0.0, (s - expected) / np.where(sat, 1.0, 1.0 - q)))
    if adjusted.ndim == 0:
        return float(expected), float(adjusted)
    return expected, adjusted


class ResultList(collections.abc.Sequence):
    """The result of one query when it is long (the default call returns every document of the index): behaves
    like the reference's list of SearchResult -- len(), indexing, slicing, iteration, equality with a list -- but
    creates a SearchResult only when one is looked at.  100 000 results cost 0.1 ms instead of the ~100 ms a list
    of 100 000 Python objects takes to build; .doc / .score / .file_no are the columns (numpy)."""
    __slots__ = ("_search", "file_no", "doc", "score")

    def __init__(self, search, seg):
        self._search = search
        self.file_no, self.doc, self.score = seg["file_no"], seg["doc"], seg["score"]

    def __len__(self):
        return len(self.doc)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        return SearchResult(self._search._names(int(self.file_no[i]))[int(self.doc[i])], int(self.score[i]))

    def __eq__(self, other):
        return len(self) == len(other) and all(a == b for a, b in zip(self, other))

    def __repr__(self):
        return "ResultList(%d results, first %r)" % (len(self), self[0] if len(self) else None)


def _split_segments(hits, offs, nq, threshold, num_results, search):
    """per-query result lists of cobs_gpu_sharded_search_batch_split on THIS rank.  In the all-documents call the
    ranks share the ranking: a rank fills only the places of the queries it owns and writes only hit_offsets[q + 1]
    of those (hit_offsets[q], the start of its first owned query, belongs to the previous owner -- another
    process's array unless one process holds all ranks).  Every query yields exactly one result per real document
    there, so a query's segment is taken from its END; queries of other owners come back empty.  Any other call
    (threshold > 0 or a limit) returns every query on every rank with complete offsets."""
    topk = num_results if num_results < search.total_counts else 0
    if threshold <= 0.0 and topk == 0:
        per_query = sum(int(search.info(f).num_docs) for f in range(search.num_files))
        return [hits[int(offs[q + 1]) - per_query:int(offs[q + 1])].tolist() if int(offs[q + 1]) >= per_query and offs[q + 1] > 0 else []
                for q in range(nq)]
    rows = hits[:int(offs[nq])].tolist()
    return [rows[int(offs[q]):int(offs[q + 1])] for q in range(nq)]


def unpack_positions(words, n):
    """the words of one hit (Search.hit_positions) -> bool [n]: position p is bit p % 64 of word p // 64"""
    w = np.ascontiguousarray(words, dtype="<u8")
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)


def covered_bases(words, n, span):
    """cobs_gpu_covered_bases: the query bases covered by the set positions of one hit's words (Search.hit_positions; n
    positions, a set position covers span = term size + findere bases) -- what Search.search_coverage scores the
    document with.  Host arithmetic, no device; bits at or beyond n are ignored."""
    w = np.ascontiguousarray(words, dtype="<u8")
    n = int(n)
    if n < 0 or len(w) * 64 < n:
        raise ValueError("words holds fewer than n positions")
    return int(_capi.load().cobs_gpu_covered_bases(C.cast(w.ctypes.data, C.POINTER(C.c_uint64)), n, int(span)))


def jaccard_estimate(sig, num_hashes, bits_a, bits_b, shared_ab):
    """cobs_gpu_jaccard_estimate -> (bit_jaccard, jaccard, containment_a_in_b, containment_b_in_a, n_inter): the
    Bloom-filter estimate of two documents' k-mer set similarity from their set bits (Search.doc_bits), their shared bits
    (Search.doc_shared_bits) and their sub-index's signature size and hash count.  Host arithmetic, no device; the three
    estimates and n_inter are NaN when the union of the two filters is saturated."""
    out = (C.c_double * 5)()
    check(_capi.load().cobs_gpu_jaccard_estimate(int(sig), int(num_hashes), int(bits_a), int(bits_b), int(shared_ab), C.byref(out)))
    return tuple(float(v) for v in out)


def best_window(bits_or_words, n, window):
    """cobs_gpu_best_window -> (best, start): the largest number of set positions in any min(window, n) consecutive
    positions of one hit (its Search.hit_positions words, or a bool vector of at least n positions), and the smallest
    start that reaches it -- what Search.search_window scores the document with.  Host arithmetic, no device; bits at
    or beyond n are ignored."""
    a = np.asarray(bits_or_words)
    if a.dtype == np.bool_:
        a = np.packbits(np.concatenate([a, np.zeros(-len(a) % 64, dtype=bool)]), bitorder="little").view("<u8")
    w = np.ascontiguousarray(a, dtype="<u8")
    n = int(n)
    if n < 0 or len(w) * 64 < n:
        raise ValueError("fewer than n positions given")
    start = C.c_size_t(0)
    best = _capi.load().cobs_gpu_best_window(C.cast(w.ctypes.data, C.POINTER(C.c_uint64)), n, int(window), C.byref(start))
    return int(best), int(start.value)


def _as_bytes(q):
    return q.encode("latin-1") if isinstance(q, str) else bytes(q)


def _options(device, shard_rank, shard_count, hbm_budget=0, shard_mode=0):
    o = Options()
    o.struct_size = C.sizeof(Options)
    o.device = device
    o.shard_rank = shard_rank
    o.shard_count = shard_count
    o.shard_mode = shard_mode
    o.hbm_budget_bytes = int(hbm_budget)
    return o


INVALID_BASES = ("error", "miss", "skip")     # COBS_GPU_INVALID_ERROR / _MISS / _SKIP


def _invalid_bases_mode(mode):
    if isinstance(mode, str) and mode in INVALID_BASES:
        return INVALID_BASES.index(mode)
    if not isinstance(mode, str) and mode in (0, 1, 2):
        return int(mode)
    raise ValueError("invalid_bases: 'error', 'miss' or 'skip'")


class Search:
    """cobs_index.Search: open one or several index files (classic or compact,
    auto-detected per file) and query them on the GPU."""

    def __init__(self, path, device=-1, shard_rank=0, shard_count=1, hbm_budget=0, shard_mode=0, _handle=None,
                 invalid_bases="error", findere=0):
        self._lib = _capi.load()
        self._h = C.c_void_p()
        mode = _invalid_bases_mode(invalid_bases)
        if _handle is not None:
            self._h = _handle
            if findere:
                self.set_findere(findere)
            if mode:
                self.invalid_bases = mode
            return
        paths = [path] if isinstance(path, (str, bytes, os.PathLike)) else list(path)
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        opts = _options(device, shard_rank, shard_count, hbm_budget, shard_mode)
        check(self._lib.cobs_gpu_open(arr, len(paths), C.byref(opts), C.byref(self._h)))
        try:
            if findere:
                self.set_findere(findere)
            if mode:
                self.invalid_bases = mode
        except Exception:
            self.close()
            raise

    @classmethod
    def synthetic(cls, kind, signature_sizes, num_docs, page_size=0, term_size=31, canonicalize=1,
                  num_hashes=1, seed=1, device=-1, shard_rank=0, shard_count=1, hbm_budget=0, shard_mode=0,
                  invalid_bases="error", findere=0):
        """Procedural index generated directly in HBM (benchmark / large parity runs)."""
        lib = _capi.load()
        sigs = (C.c_uint64 * len(signature_sizes))(*[int(s) for s in signature_sizes])
        d = Synth()
        d.kind = 1 if kind in (1, "compact") else 0
        d.term_size, d.canonicalize, d.num_pages = term_size, canonicalize, len(signature_sizes)
        d.num_hashes, d.page_size, d.num_docs, d.seed = num_hashes, page_size, num_docs, seed
        d.signature_sizes = C.cast(sigs, C.POINTER(C.c_uint64))
        h = C.c_void_p()
        opts = _options(device, shard_rank, shard_count, hbm_budget, shard_mode)
        check(lib.cobs_gpu_open_synthetic(C.byref(d), C.byref(opts), C.byref(h)))
        s = cls(None, _handle=h)
        try:
            if findere:
                s.set_findere(findere)
            s.invalid_bases = invalid_bases
        except Exception:
            s.close()
            raise
        return s

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cobs_gpu_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- geometry ------------------------------------------------------------
    @property
    def num_files(self):
        return int(self._lib.cobs_gpu_num_files(self._h))

    def info(self, file_no=0):
        i = IndexInfo()
        check(self._lib.cobs_gpu_info(self._h, file_no, C.byref(i)))
        return i

    @property
    def total_counts(self):
        return int(self._lib.cobs_gpu_total_counts(self._h))

    @property
    def local_counts(self):
        return int(self._lib.cobs_gpu_local_counts(self._h))

    def doc_name(self, file_no, doc):
        return self._lib.cobs_gpu_doc_name(self._h, file_no, doc).decode()

    def _names(self, file_no):
        """document names of one file, fetched once (search() of a 100k-document index names
        100k results per query)"""
        cache = self.__dict__.setdefault("_name_cache", {})
        if file_no not in cache:
            fn, h = self._lib.cobs_gpu_doc_name, self._h
            cache[file_no] = [fn(h, file_no, d).decode() for d in range(int(self.info(file_no).num_docs))]
        return cache[file_no]

    def signature_size(self, file_no=0, page=0):
        return int(self._lib.cobs_gpu_signature_size(self._h, file_no, page))

    def read_row(self, file_no, page, row, nbytes):
        out = np.zeros(nbytes, dtype=np.uint8)
        check(self._lib.cobs_gpu_read_row(self._h, file_no, page, row, out.ctypes.data, nbytes))
        return out

    def page_columns(self, file_no, page):
        """-> (col0, ncols): the row bytes of sub-index `page` this shard holds"""
        c0, n = C.c_uint64(0), C.c_uint64(0)
        check(self._lib.cobs_gpu_page_columns(self._h, file_no, page, C.byref(c0), C.byref(n)))
        return int(c0.value), int(n.value)

    def set_tuning(self, key, value):
        """per-handle tuning hook of the scan launch (see cobs_gpu_set_tuning)"""
        check(self._lib.cobs_gpu_set_tuning(self._h, key.encode(), int(value)))

    @property
    def findere(self):
        """findere z (0..7): a position of a query scores in a document only when its z + 1 consecutive
        k-mers are all present there; 0 = the plain COBS count (see cobs_gpu_set_findere)"""
        z = C.c_uint32()
        check(self._get_findere_call(C.byref(z)))
        return z.value

    def set_findere(self, z):
        """set findere z (0..7) for every later search, count and batch run of this handle"""
        z = int(z)
        if not 0 <= z <= 7:
            raise ValueError("findere: z is 0 .. 7")
        check(self._set_findere_call(z))

    def _set_findere_call(self, z):
        return self._lib.cobs_gpu_set_findere(self._h, z)

    def _get_findere_call(self, zp):
        return self._lib.cobs_gpu_get_findere(self._h, zp)

    @property
    def invalid_bases(self):
        """what a character outside ACGT in a query does: "error" (the call fails, as `cobs query` does), "miss" (a k-mer
        that holds one is absent from every document) or "skip" (... and leaves the threshold's denominator too); see
        cobs_gpu_set_invalid_bases"""
        m = C.c_uint32()
        check(self._get_invalid_bases_call(C.byref(m)))
        return INVALID_BASES[m.value]

    @invalid_bases.setter
    def invalid_bases(self, mode):
        check(self._set_invalid_bases_call(_invalid_bases_mode(mode)))

    def _set_invalid_bases_call(self, mode):
        return self._lib.cobs_gpu_set_invalid_bases(self._h, mode)

    def _get_invalid_bases_call(self, mp):
        return self._lib.cobs_gpu_get_invalid_bases(self._h, mp)

    def read_rows(self, file_no, page, row0, nrows, out=None):
        """bulk D2H of whole rows of one held sub-index -> uint8 [nrows, held row bytes]"""
        width = self.page_columns(file_no, page)[1]
        if out is None:
            out = np.empty((nrows, width), dtype=np.uint8)
        check(self._lib.cobs_gpu_read_rows(self._h, file_no, page, row0, nrows, out.ctypes.data, width))
        return out

    def plant(self, text, docs, keep_permille=1000, salt=0, file_no=0):
        """True positives for a resident index (cobs_gpu_plant): documents `docs` additionally contain the terms of `text`,
        document docs[i] the share keep_permille[i] / 1000 of them (one value = the same for all)."""
        if isinstance(text, str):
            text = text.encode()
        docs = np.ascontiguousarray(docs, dtype=np.uint32)
        keep = np.ascontiguousarray(np.broadcast_to(np.asarray(keep_permille, dtype=np.uint32), docs.shape))
        u32p = C.POINTER(C.c_uint32)
        check(self._lib.cobs_gpu_plant(self._h, file_no, text, len(text), docs.ctypes.data_as(u32p),
                                       keep.ctypes.data_as(u32p), len(docs), int(salt)))

    # -- filter fill: what a score is worth ------------------------------------
    def doc_bits(self, file_no=0):
        """cobs_gpu_doc_bits: the bits set in every document's Bloom filter -> uint64 [slot_count], one entry per score
        slot this handle holds of the file (padding slots included; the whole file on an unsharded handle).  Counted on
        the device on the first request and cached by the library."""
        need = C.c_size_t(0)
        st = self._lib.cobs_gpu_doc_bits(self._h, int(file_no), None, 0, C.byref(need))
        if st != _capi.ERR_CAPACITY:
            check(st)
        out = np.zeros(need.value, dtype=np.uint64)
        check(self._lib.cobs_gpu_doc_bits(self._h, int(file_no), out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size, C.byref(need)))
        return out

    def _doc_sigs(self, file_no):
        """signature size S_p of the sub-index of every real document of a file -> uint64 [num_docs]"""
        i = self.info(file_no)
        n = int(i.num_docs)
        if int(i.kind) == 0:
            return np.full(n, self.signature_size(file_no, 0), dtype=np.uint64)
        sigs = np.array([self.signature_size(file_no, p) for p in range(int(i.num_pages))], dtype=np.uint64)
        return sigs[np.arange(n) // (8 * int(i.page_size))]

    def _real_doc_bits(self, file_no):
        i = self.info(file_no)
        if int(i.slot_begin) != 0 or int(i.slot_count) < int(i.num_docs):
            raise CobsGpuError(_capi.ERR_UNSUPPORTED, "this handle holds a shard of the file's documents: use doc_bits")
        return self.doc_bits(file_no)[:int(i.num_docs)]       # (document d is score slot d; padding slots follow the last)

    def doc_fill(self, file_no=0):
        """fill ratio of every real document's filter, bits / S_p -> float64 [num_docs]"""
        return self._real_doc_bits(file_no).astype(np.float64) / self._doc_sigs(file_no).astype(np.float64)

    def doc_fpr(self, file_no=0):
        """the probability that a k-mer unrelated to a document hits it, fill ** num_hashes -> float64 [num_docs]"""
        return np.power(self.doc_fill(file_no), float(int(self.info(file_no).num_hashes)))

    def doc_bits_ms(self):
        """the doc_bits sweeps of this handle so far: kernel ms, index bytes read, PCIe copy ms, sweeps"""
        t = (C.c_double * 4)()
        check(self._lib.cobs_gpu_doc_bits_ms(self._h, C.byref(t)))
        return {"kernel_ms": t[0], "bytes_read": int(t[1]), "pcie_ms": t[2], "passes": int(t[3])}

    # -- document similarity: shared filter bits ---------------------------------
    def doc_shared_bits(self, refs, file_no=0):
        """cobs_gpu_doc_shared_bits: for every reference document refs[i] of the file, in how many rows it and every
        document of ITS sub-index both have their bit set -> list of uint64 arrays, one per reference, one entry per
        score slot of that sub-index in slot order (classic: counts_size entries; compact: 8 * page_size; entry of the
        reference itself = its doc_bits).  Documents of different sub-indexes are not comparable and never paired."""
        r = np.ascontiguousarray(refs, dtype=np.uint32).reshape(-1)
        n = len(r)
        offs = np.zeros(n + 1, dtype=np.uint64)
        need = C.c_size_t(0)
        rp, op = r.ctypes.data_as(C.POINTER(C.c_uint32)), offs.ctypes.data_as(C.POINTER(C.c_uint64))
        check(self._lib.cobs_gpu_doc_shared_bits(self._h, int(file_no), rp, n, op, None, 0, C.byref(need)))
        out = np.zeros(need.value, dtype=np.uint64)
        check(self._lib.cobs_gpu_doc_shared_bits(self._h, int(file_no), rp, n, op, out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size,
                                                 C.byref(need)))
        return [out[int(offs[i]):int(offs[i + 1])] for i in range(n)]

    def similarity_ms(self):
        """the doc_shared_bits panels of this handle since the last read (reset by the read): extraction ms, sweep ms,
        index bytes the sweeps read, sweeps"""
        t = (C.c_double * 4)()
        check(self._lib.cobs_gpu_similarity_ms(self._h, C.byref(t)))
        return {"extract_ms": t[0], "sweep_ms": t[1], "bytes_read": int(t[2]), "sweeps": int(t[3])}

    def _sub_index_of(self, file_no, doc):
        """-> (sub-index, its first document, S_p) of a real document"""
        i = self.info(file_no)
        per = int(i.counts_size) if int(i.kind) == 0 else 8 * int(i.page_size)
        pg = int(doc) // per
        return pg, pg * per, self.signature_size(file_no, pg)

    def similar_documents(self, ref, file_no=0, min_jaccard=0.0, num_results=0):
        """the real documents of ref's sub-index other than ref itself, by the Bloom-filter estimate of the Jaccard index of
        their k-mer sets (jaccard_estimate over doc_bits and doc_shared_bits) -> list of (doc_name, jaccard,
        containment_ref_in_doc, containment_doc_in_ref, shared), estimated Jaccard descending, then document index; documents
        whose estimate is NaN (a saturated filter) follow every finite one, ordered by bit_jaccard descending.  min_jaccard
        <= 0 is no threshold; a positive one keeps the documents whose ESTIMATE reaches it, so a NaN estimate passes no
        threshold (the one rule, also of `cobs_gpu_query doc-similarity`); num_results > 0 cuts the list.  ref is a document
        index or name."""
        names = self._names(file_no)
        if isinstance(ref, (str, bytes)):
            name = ref.decode() if isinstance(ref, bytes) else ref
            if name not in names:
                raise KeyError("no document named %r" % name)
            ref = names.index(name)
        ref = int(ref)
        if not 0 <= ref < len(names):
            raise CobsGpuError(_capi.ERR_ARG, "similar_documents: reference %d is not a document of the file" % ref)
        shared = self.doc_shared_bits([ref], file_no)[0]
        bits = self._real_doc_bits(file_no)
        _pg, d0, sig = self._sub_index_of(file_no, ref)
        H = int(self.info(file_no).num_hashes)
        rows = []
        for s in range(min(len(shared), len(names) - d0)):
            d = d0 + s
            if d == ref:
                continue
            bj, j, c_ab, c_ba, _n = jaccard_estimate(sig, H, int(bits[ref]), int(bits[d]), int(shared[s]))
            nan = j != j
            if min_jaccard > 0 and not j >= min_jaccard:
                continue
            rows.append(((nan, -(bj if nan else j), d), (names[d], j, c_ab, c_ba, int(shared[s]))))
        rows.sort(key=lambda t: t[0])
        out = [r for _k, r in rows]
        return out[:num_results] if num_results and num_results > 0 else out

    def search_adjusted(self, query, threshold=0.0, num_results=0):
        """search() whose results also carry expected_fp and adjusted (fpr_adjust over the document's fill, the handle's
        findere z and the positions the search scored: T - z, or the valid positions V under invalid_bases "skip").
        -> list of AdjustedResult in search()'s order.  [search() itself keeps the reference's signature.]"""
        q = _as_bytes(query)
        hits = self.search_hits([q], threshold, num_results)[0]
        z = self.findere
        valid = None
        if self.invalid_bases == "skip":
            b = Batch(self)
            try:
                b.set_queries([q])
                b.run(0.0)
                b.sync()
                valid = [int(b.scored_positions(f)[0]) for f in range(self.num_files)]
            finally:
                b.close()
        per_file = {}
        out = []
        for f, d, s in hits:
            if f not in per_file:
                i = self.info(f)
                P = valid[f] if valid is not None else len(q) - int(i.term_size) + 1 - z
                per_file[f] = (self._real_doc_bits(f), self._doc_sigs(f), int(i.num_hashes), P)
            bits, sigs, H, P = per_file[f]
            e, a = fpr_adjust(s, P, int(bits[d]), int(sigs[d]), H, z)
            out.append(AdjustedResult(self._names(f)[d], s, e, a))
        return out

    # -- queries -------------------------------------------------------------
    def search(self, query, threshold=0.0, num_results=0):
        """Same contract as cobs_index.Search.search (python/module.cpp:372-386)."""
        if type(self)._search_batch_call is not Search._search_batch_call:
            return self.search_batch([query], threshold, num_results)[0]
        # one query: cobs_gpu_search straight into a reused result buffer (no numpy marshalling of a batch of one)
        q = query if type(query) is bytes else _as_bytes(query)
        total = self.total_counts
        if num_results > 0:
            cap = min(num_results, total)
        elif threshold <= 0:
            cap = total
        else:
            cap = 1024
        n = C.c_size_t(0)
        while True:
            hits = self._result_buffer(max(cap, 1))
            st = self._lib.cobs_gpu_search(self._h, q, len(q), float(threshold), int(num_results),
                                           C.cast(hits.ctypes.data, C.POINTER(Hit)), len(hits), C.byref(n))
            if st == _capi.ERR_CAPACITY and n.value > cap:
                cap = n.value
                continue
            check(st)
            break
        seg = hits[:n.value]
        if n.value <= 64:
            return [SearchResult(self.doc_name(f, d), s) for (f, d, s) in seg.tolist()]
        return ResultList(self, seg)

    HIT_DTYPE = np.dtype([("file_no", "<u4"), ("doc", "<u4"), ("score", "<u4")])
    reuse_result_buffers = True     # see _result_buffer

    def search_arrays(self, queries, threshold=0.0, num_results=0, out=None):
        """-> (offsets uint64 [nq + 1], hits structured array of (file_no, doc, score)):
        the hits of query i are hits[offsets[i]:offsets[i + 1]], in result order.  The columnar form of
        search(): no per-result Python objects (the default call returns every document of the index)."""
        qs = [q if type(q) is bytes else _as_bytes(q) for q in queries]
        offsets = np.zeros(len(qs) + 1, dtype=np.uint64)
        np.cumsum(np.fromiter(map(len, qs), dtype=np.uint64, count=len(qs)), out=offsets[1:])
        return self.search_packed(b"".join(qs), offsets, threshold, num_results, out=out)

    @staticmethod
    def _packed_args(text, offsets):
        """-> (char** queries, size_t* lens, nq, what keeps them alive) for queries packed back to back"""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nq = len(offsets) - 1
        if nq < 0:
            raise ValueError("offsets needs nq + 1 entries")
        if isinstance(text, np.ndarray):
            text = np.ascontiguousarray(text, dtype=np.uint8)
            base, size = text.ctypes.data, text.size
        else:
            text = bytes(text) if not isinstance(text, bytes) else text
            base, size = C.cast(C.c_char_p(text), C.c_void_p).value or 0, len(text)
        if nq and (int(offsets[-1]) > size or np.any(offsets[1:] < offsets[:-1])):
            raise ValueError("offsets are not ascending positions inside text")
        ptrs_np = (offsets[:-1] + np.uint64(base)) if nq else np.zeros(1, dtype=np.uint64)
        lens_np = (offsets[1:] - offsets[:-1]) if nq else np.zeros(1, dtype=np.uint64)
        ptrs_np = np.ascontiguousarray(ptrs_np)
        lens_np = np.ascontiguousarray(lens_np)
        arr = C.cast(ptrs_np.ctypes.data, C.POINTER(C.c_char_p))
        lens = C.cast(lens_np.ctypes.data, C.POINTER(C.c_size_t))
        return arr, lens, nq, (text, ptrs_np, lens_np)

    def search_packed(self, text, offsets, threshold=0.0, num_results=0, out=None):
        """The same for queries packed back to back: query i is text[offsets[i]:offsets[i + 1]]
        (text: bytes or a uint8 array, e.g. the sequence lines of a FASTQ block; offsets: nq + 1
        integers).  No per-query Python objects: the pointer array is built with numpy.
        out: an optional HIT_DTYPE array to receive the hits (a caller that repeats large calls keeps
        one buffer instead of page-faulting a fresh one per call); it is used when large enough."""
        arr, lens, nq, _keep = self._packed_args(text, offsets)
        if num_results > 0:
            cap = nq * min(num_results, self.total_counts)
        elif threshold <= 0:
            cap = nq * self.total_counts          # every document is a result
        elif type(self)._search_batch_call is not Search._search_batch_call:
            cap = 16 * nq + 1024                  # (several GPUs behind one handle: grown on demand, the call repeated)
        else:
            # the number of hits is only known when the search has run (ERR_CAPACITY reports it, and the WHOLE call would
            # be made a second time): the view call collects them in the arena the library grows as the passes come
            # home; the finished lists are copied out of it once (12 bytes per hit)
            hp, op, bad = C.POINTER(Hit)(), C.POINTER(C.c_size_t)(), C.c_size_t(0)
            check(self._lib.cobs_gpu_search_batch_view(self._h, arr, lens, nq, float(threshold), 0,
                                                       C.byref(hp), C.byref(op), C.byref(bad)))
            offs = np.array(np.ctypeslib.as_array(op, shape=(nq + 1,)).view(np.uint64))
            n = int(offs[nq])
            if out is not None and out.dtype == self.HIT_DTYPE and out.flags.c_contiguous and out.size >= n:
                hits = out
            else:
                hits = self._result_buffer(max(n, 1))
            if n:
                C.memmove(hits.ctypes.data, hp, n * 12)
            return offs, hits[:n]
        cap = max(1, cap)
        offs = np.zeros(nq + 1, dtype=np.uint64)
        bad = C.c_size_t(0)
        while True:
            if out is not None and out.dtype == self.HIT_DTYPE and out.flags.c_contiguous and out.size >= cap:
                hits, cap = out, out.size
            else:
                hits = self._result_buffer(cap)
            st = self._search_batch_call(
                arr, lens, nq, float(threshold), int(num_results),
                C.cast(hits.ctypes.data, C.POINTER(Hit)), cap,
                C.cast(offs.ctypes.data, C.POINTER(C.c_size_t)), C.byref(bad))
            if st == _capi.ERR_CAPACITY and int(offs[nq]) > cap:
                cap = int(offs[nq])
                continue
            check(st)
            break
        return offs, hits[:int(offs[nq])]

    def _search_batch_call(self, *args):
        return self._lib.cobs_gpu_search_batch(self._h, *args)

    def _result_buffer(self, cap):
        """a HIT_DTYPE array of `cap` records for the results of a call.  A buffer of an EARLIER call that nothing
        references any more (neither the array that call returned nor a slice or ResultList made from it: they all keep
        the raw buffer alive through .base) is used again -- its pages are there, where a fresh 307 MB array (the default
        call of 256 queries x 100 000 documents) costs 75 000 first-touch page faults, 5.6 ms against 3.4.  A caller that
        drops the results of one call before it makes the next never allocates; one that keeps them gets fresh memory."""
        need = cap * self.HIT_DTYPE.itemsize
        pool = self.__dict__.setdefault("_result_pool", [])
        # "Nothing references it" is read off CPython's reference count of the raw buffer: exact there for every numpy
        # object made from the results (views keep the raw buffer through .base); a raw address taken from a result
        # (.ctypes.data) dangles once the result is dropped whether or not the memory is used again.  An interpreter
        # without reference counts gets a fresh buffer per call, and Search.reuse_result_buffers = False turns the
        # reuse off for a caller that wants that anyway [ADVICE r5].
        if not (self.reuse_result_buffers and sys.implementation.name == "cpython"):
            return np.empty(max(need, 1), dtype=np.uint8)[:need].view(self.HIT_DTYPE)
        for i in range(len(pool)):
            # references: the pool's, and getrefcount's argument
            if pool[i].nbytes >= need and sys.getrefcount(pool[i]) == 2:
                return pool[i][:need].view(self.HIT_DTYPE)
        raw = np.empty(max(need, 1), dtype=np.uint8)
        if need >= (1 << 20):
            # keep a few large buffers (small results are cheap to allocate): free ones first to go
            if len(pool) >= 3:
                free = [i for i in range(len(pool)) if sys.getrefcount(pool[i]) == 2]
                del pool[free[0] if free else 0]
            pool.append(raw)
        return raw[:need].view(self.HIT_DTYPE)

    def search_view(self, queries, threshold=0.0, num_results=0):
        """cobs_gpu_search_batch_view: the results stay in the arena the LIBRARY keeps on this handle.
        -> (offsets uint64 [nq + 1], hits HIT_DTYPE array) -- both views of that arena, valid until the next search call on
        this handle (copy what has to live longer)."""
        qs = [q if type(q) is bytes else _as_bytes(q) for q in queries]
        nq = len(qs)
        arr = (C.c_char_p * max(nq, 1))(*qs)
        lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in qs])
        hp, op, bad = C.POINTER(Hit)(), C.POINTER(C.c_size_t)(), C.c_size_t(0)
        check(self._lib.cobs_gpu_search_batch_view(self._h, arr, lens, nq, float(threshold), int(num_results),
                                                   C.byref(hp), C.byref(op), C.byref(bad)))
        offs = np.ctypeslib.as_array(op, shape=(nq + 1,)).view(np.uint64)
        n = int(offs[nq])
        if n == 0:
            return offs, np.zeros(0, dtype=self.HIT_DTYPE)
        raw = np.ctypeslib.as_array(C.cast(hp, C.POINTER(C.c_uint8)), shape=(n * 12,))
        return offs, raw.view(self.HIT_DTYPE)

    def sharded_search_arrays(self, comm, queries, threshold=0.0, num_results=0, split=False):
        """cobs_gpu_sharded_search_batch[_split]: collective over `comm` (every rank, same queries)
        -> (offsets uint64 [nq + 1], hits HIT_DTYPE array), the GLOBAL results in result order (split: see below).
        queries: a list, or a (text, offsets) pair of queries packed back to back."""
        if isinstance(queries, tuple):         # (text, offsets): queries packed back to back, as search_packed takes them
            arr, lens, nq, _keep = self._packed_args(*queries)
        else:
            qs = [q if type(q) is bytes else _as_bytes(q) for q in queries]
            nq = len(qs)
            arr = (C.c_char_p * max(nq, 1))(*qs)
            lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in qs])
        if num_results > 0:
            cap = nq * min(num_results, self.total_counts)
        elif threshold <= 0:
            cap = nq * self.total_counts
        else:
            # (a buffer that proves too small costs a second, collective, run of the whole search: sized by the hits per
            # query of the earlier thresholded calls on this handle -- the same on every rank, as the results are)
            cap = max(16 * nq, int((0.0 if split else self.__dict__.get("_sharded_hits_per_query", 0.0)) * nq * 1.25)) + 1024
        cap = max(1, cap)
        offs = np.zeros(nq + 1, dtype=np.uint64)
        bad = C.c_size_t(0)
        fn = self._lib.cobs_gpu_sharded_search_batch_split if split else self._lib.cobs_gpu_sharded_search_batch
        while True:
            hits = self._result_buffer(cap)        # (a buffer of an earlier call that nothing references any more: its pages are there)
            offs[:] = 0
            st = fn(self._h, comm._h, arr, lens, nq, float(threshold), int(num_results),
                    C.cast(hits.ctypes.data, C.POINTER(Hit)), cap,
                    C.cast(offs.ctypes.data, C.POINTER(C.c_size_t)), C.byref(bad))
            if st == _capi.ERR_CAPACITY and int(offs[nq]) > cap:
                cap = int(offs[nq])
                continue
            check(st)
            break
        if threshold > 0 and num_results == 0 and nq and not split:
            self._sharded_hits_per_query = max(int(offs[nq]) / nq, 0.95 * self.__dict__.get("_sharded_hits_per_query", 0.0))
        return offs, hits[:int(offs[nq])] if not split else hits

    def sharded_search_hits(self, comm, queries, threshold=0.0, num_results=0, split=False):
        """-> per query the GLOBAL list of (file_no, doc, score) in result order.
        split=True: cobs_gpu_sharded_search_batch_split -- for the all-documents search the ranks share the
        ranking and this rank's return holds the results of the queries it owns (empty lists for the others)."""
        offs, hits = self.sharded_search_arrays(comm, queries, threshold, num_results, split)
        nq = len(queries)
        if split:
            return _split_segments(hits, offs, nq, threshold, num_results, self)
        rows = hits[:int(offs[nq])].tolist()
        return [rows[int(offs[q]):int(offs[q + 1])] for q in range(nq)]

    def search_hits(self, queries, threshold=0.0, num_results=0):
        """-> per query: list of (file_no, doc, score) in result order."""
        offs, hits = self.search_arrays(queries, threshold, num_results)
        rows = hits.tolist()
        return [rows[int(offs[q]):int(offs[q + 1])] for q in range(len(queries))]

    def search_batch(self, queries, threshold=0.0, num_results=0):
        offs, hits = self.search_arrays(queries, threshold, num_results)
        out = []
        for q in range(len(queries)):
            seg = hits[int(offs[q]):int(offs[q + 1])]
            if len(seg) <= 64:
                out.append([SearchResult(self.doc_name(f, d), s) for (f, d, s) in seg.tolist()])
                continue
            # many results (the default call ranks every document): a lazy sequence over the columns
            out.append(ResultList(self, seg))
        return out

    def counts(self, query):
        """Raw per-document counts (incl. padding slots) over all files, uint32."""
        q = _as_bytes(query)
        out = np.zeros(self.total_counts, dtype=np.uint32)
        check(self._lib.cobs_gpu_counts(self._h, q, len(q), out.ctypes.data, out.size))
        return out

    # -- positions: WHERE in each query its hits matched --------------------------
    def hit_positions(self, queries, offsets, hits):
        """cobs_gpu_hit_positions over a hit list as search_arrays returned it (hits[offsets[i]:offsets[i + 1]] belong to
        query i; the scores are ignored, so any (file_no, doc) pairs may be asked about)
        -> (bit_offsets uint64 [n_hits + 1], bits uint64): hit i owns the words bits[bit_offsets[i]:bit_offsets[i + 1]];
        position p of its query is bit p % 64 of word p // 64 and is set when the terms p .. p + findere are all present
        in the document -- the popcount of a hit's words is its score (unpack_positions gives the bool vector)."""
        if type(self)._search_batch_call is not Search._search_batch_call:
            raise CobsGpuError(_capi.ERR_UNSUPPORTED, "positions: not on a device-list handle (a document's rows live on one rank)")
        qs = [q if type(q) is bytes else _as_bytes(q) for q in queries]
        nq = len(qs)
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        if len(offs) != nq + 1:
            raise ValueError("offsets needs nq + 1 entries")
        n = int(offs[nq])
        hits = np.ascontiguousarray(hits, dtype=self.HIT_DTYPE)
        if len(hits) < n:
            raise ValueError("hits is shorter than offsets[nq]")
        arr = (C.c_char_p * max(nq, 1))(*qs)
        lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in qs])
        bit_offsets = np.zeros(n + 1, dtype=np.uint64)
        need, bad = C.c_size_t(0), C.c_size_t(0)
        # the number of words is host arithmetic (the call refuses a buffer that is too small before any device work):
        # ask for it, then make the call
        bits = np.zeros(0, dtype=np.uint64)
        while True:
            st = self._lib.cobs_gpu_hit_positions(
                self._h, arr, lens, nq, C.cast(hits.ctypes.data, C.POINTER(Hit)),
                C.cast(offs.ctypes.data, C.POINTER(C.c_size_t)), C.cast(bits.ctypes.data, C.POINTER(C.c_uint64)), bits.size,
                C.cast(bit_offsets.ctypes.data, C.POINTER(C.c_size_t)), C.byref(need), C.byref(bad))
            if st == _capi.ERR_CAPACITY and need.value > bits.size:
                bits = np.zeros(need.value, dtype=np.uint64)
                continue
            check(st)
            break
        return bit_offsets, bits

    def search_positions(self, queries, threshold=0.0, num_results=0):
        """search_arrays followed by hit_positions -> (offsets, hits, bit_offsets, bits)"""
        qs = [q if type(q) is bytes else _as_bytes(q) for q in queries]
        offsets, hits = self.search_arrays(qs, threshold, num_results)
        bit_offsets, bits = self.hit_positions(qs, offsets, hits)
        return offsets, hits, bit_offsets, bits

    def search_with_positions(self, query, threshold=0.0, num_results=0):
        """one query -> [(SearchResult, bool ndarray of its n positions)] in result order"""
        q = _as_bytes(query)
        offsets, hits, bit_offsets, bits = self.search_positions([q], threshold, num_results)
        out = []
        for i, (f, d, sc) in enumerate(hits.tolist()):
            n = len(q) - int(self.info(f).term_size) + 1 - self.findere
            out.append((SearchResult(self.doc_name(f, d), sc),
                        unpack_positions(bits[int(bit_offsets[i]):int(bit_offsets[i + 1])], n)))
        return out

    # -- prevalence: HOW MANY documents hold each position of a query ---------------
    def prevalence_arrays(self, queries):
        """cobs_gpu_prevalence -> (offsets uint64 [nq * num_files + 1], counts uint32): segment (q, f) is
        counts[offsets[q * num_files + f]:offsets[q * num_files + f + 1]], one count per position of query q in file f
        (n = T_f - findere): the real documents of the file in which terms p .. p + findere are all present.  On one shard
        of several the counts cover the shard's own documents; the parts of all shards add up."""
        if type(self)._search_batch_call is not Search._search_batch_call:
            raise CobsGpuError(_capi.ERR_UNSUPPORTED, "prevalence: not on a device-list handle (ask the shards: shard(rank).prevalence, and add)")
        qs = [q if type(q) is bytes else _as_bytes(q) for q in queries]
        nq = len(qs)
        arr = (C.c_char_p * max(nq, 1))(*qs)
        lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in qs])
        offsets = np.zeros(nq * self.num_files + 1, dtype=np.uint64)
        need, bad = C.c_size_t(0), C.c_size_t(0)
        # the number of cells is host arithmetic (the call refuses a buffer that is too small before any device work)
        counts = np.zeros(0, dtype=np.uint32)
        while True:
            st = self._lib.cobs_gpu_prevalence(
                self._h, arr, lens, nq, C.cast(counts.ctypes.data, C.POINTER(C.c_uint32)), counts.size,
                C.cast(offsets.ctypes.data, C.POINTER(C.c_size_t)), C.byref(need), C.byref(bad))
            if st == _capi.ERR_CAPACITY and need.value > counts.size:
                counts = np.zeros(need.value, dtype=np.uint32)
                continue
            check(st)
            break
        return offsets, counts

    def prevalence(self, queries):
        """per query a list with one uint32 array per file (prevalence_arrays, cut up); one str / bytes query -> its list"""
        single = isinstance(queries, (str, bytes, bytearray))
        qs = [queries] if single else list(queries)
        offsets, counts = self.prevalence_arrays(qs)
        nf = self.num_files
        out = [[counts[int(offsets[q * nf + f]):int(offsets[q * nf + f + 1])] for f in range(nf)] for q in range(len(qs))]
        return out[0] if single else out

    def prevalence_ms(self):
        """kernel times of the prevalence calls since the previous call of this method (HIP events, summed over passes)"""
        t = (C.c_double * 3)()
        check(self._lib.cobs_gpu_prevalence_ms(self._h, C.byref(t)))
        return {"kernel_ms": t[0], "hash_ms": t[1], "passes": int(t[2])}

    # -- weighted search: rare k-mers count for more ---------------------------------
    def search_weighted_arrays(self, queries, threshold=0.0, num_results=0):
        """cobs_gpu_search_weighted -> (offsets uint64 [nq + 1], hits HIT_DTYPE, total_weight uint64 [nq, num_files]): the
        records of query q are hits[offsets[q]:offsets[q + 1]], by weighted score descending, then (file_no, doc); a
        position held by c of a file's D documents weighs idf_weight(D, c) = 1 + min(14, floor(log2(D / c))), 0 for
        c = 0; a document is a hit when its score reaches max(1, ceil(threshold * total_weight[q, file]))."""
        if type(self)._search_batch_call is not Search._search_batch_call:
            raise CobsGpuError(_capi.ERR_UNSUPPORTED, "weighted: not on a device-list handle (the weights need every shard's counts)")
        qs = [q if type(q) is bytes else _as_bytes(q) for q in queries]
        nq = len(qs)
        arr = (C.c_char_p * max(nq, 1))(*qs)
        lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in qs])
        offs = np.zeros(nq + 1, dtype=np.uint64)
        total = np.zeros((nq, self.num_files), dtype=np.uint64)
        bad = C.c_size_t(0)
        if num_results > 0:
            cap = nq * min(int(num_results), self.total_counts)
        elif threshold <= 0:
            cap = nq * self.total_counts
        else:
            # (a buffer that proves too small costs a second run of the whole call: sized by the hits per query of the
            # earlier thresholded weighted calls on this handle)
            cap = max(16 * nq, int(self.__dict__.get("_weighted_hits_per_query", 0.0) * nq * 1.25)) + 1024
        cap = max(1, cap)
        while True:
            hits = np.zeros(cap, dtype=self.HIT_DTYPE)
            st = self._lib.cobs_gpu_search_weighted(
                self._h, arr, lens, nq, float(threshold), int(num_results), C.cast(hits.ctypes.data, C.POINTER(Hit)), cap,
                C.cast(offs.ctypes.data, C.POINTER(C.c_size_t)), C.cast(total.ctypes.data, C.POINTER(C.c_uint64)), C.byref(bad))
            if st == _capi.ERR_CAPACITY and int(offs[nq]) > cap:
                cap = int(offs[nq])
                continue
            check(st)
            break
        if threshold > 0 and num_results == 0 and nq:
            self._weighted_hits_per_query = max(int(offs[nq]) / nq, 0.95 * self.__dict__.get("_weighted_hits_per_query", 0.0))
        return offs, hits[:int(offs[nq])], total

    def search_weighted(self, query, threshold=0.0, num_results=0):
        """one query -> [WeightedResult] in result order (doc_name, the weighted score, the total weight of the query in the
        document's file)"""
        _offs, hits, total = self.search_weighted_arrays([query], threshold, num_results)
        return [WeightedResult(self.doc_name(f, d), sc, int(total[0, f])) for (f, d, sc) in hits.tolist()]

    def position_weights(self, query):
        """per file a uint8 array: the weight of every position of the query (host arithmetic over prevalence_arrays with
        cobs_gpu_idf_weight)"""
        offsets, counts = self.prevalence_arrays([query])
        out = []
        for f in range(self.num_files):
            docs = int(self.info(f).num_docs)
            seg = counts[int(offsets[f]):int(offsets[f + 1])]
            out.append(np.array([self._lib.cobs_gpu_idf_weight(docs, int(c)) for c in seg], dtype=np.uint8))
        return out

    def weighted_ms(self):
        """stage times of the weighted searches since the previous call of this method (HIP events, summed over passes)"""
        t = (C.c_double * 5)()
        check(self._lib.cobs_gpu_weighted_ms(self._h, C.byref(t)))
        return {"hash_ms": t[0], "prevalence_ms": t[1], "weights_ms": t[2], "scan_ms": t[3], "passes": int(t[4])}

    # -- coverage search: score documents by the query bases they cover ---------------
    def search_coverage_arrays(self, queries, threshold=0.0, num_results=0):
        """cobs_gpu_search_coverage -> (offsets uint64 [nq + 1], hits HIT_DTYPE): the records of query q are
        hits[offsets[q]:offsets[q + 1]], by coverage descending, then (file_no, doc); `score` is the number of query bases
        that lie inside a set position (span = term size + findere bases from the position on); a document is a hit when
        its coverage reaches max(1, ceil(threshold * len(query)))."""
        if type(self)._search_batch_call is not Search._search_batch_call:
            raise CobsGpuError(_capi.ERR_UNSUPPORTED, "coverage: not on a device-list handle (the call has no counterpart there)")
        qs = [q if type(q) is bytes else _as_bytes(q) for q in queries]
        nq = len(qs)
        arr = (C.c_char_p * max(nq, 1))(*qs)
        lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in qs])
        offs = np.zeros(nq + 1, dtype=np.uint64)
        bad = C.c_size_t(0)
        if num_results > 0:
            cap = nq * min(int(num_results), self.total_counts)
        elif threshold <= 0:
            cap = nq * self.total_counts
        else:
            # (a buffer that proves too small costs a second run of the whole call: sized by the hits per query of the
            # earlier thresholded coverage calls on this handle)
            cap = max(16 * nq, int(self.__dict__.get("_coverage_hits_per_query", 0.0) * nq * 1.25)) + 1024
        cap = max(1, cap)
        while True:
            hits = np.zeros(cap, dtype=self.HIT_DTYPE)
            st = self._lib.cobs_gpu_search_coverage(
                self._h, arr, lens, nq, float(threshold), int(num_results), C.cast(hits.ctypes.data, C.POINTER(Hit)), cap,
                C.cast(offs.ctypes.data, C.POINTER(C.c_size_t)), C.byref(bad))
            if st == _capi.ERR_CAPACITY and int(offs[nq]) > cap:
                cap = int(offs[nq])
                continue
            check(st)
            break
        if threshold > 0 and num_results == 0 and nq:
            self._coverage_hits_per_query = max(int(offs[nq]) / nq, 0.95 * self.__dict__.get("_coverage_hits_per_query", 0.0))
        return offs, hits[:int(offs[nq])]

    def search_coverage(self, query, threshold=0.0, num_results=0):
        """one query -> [SearchResult] in result order (doc_name, covered bases); a list or tuple of queries -> one such
        list per query"""
        many = isinstance(query, (list, tuple))
        offs, hits = self.search_coverage_arrays(list(query) if many else [query], threshold, num_results)
        rows = hits.tolist()
        out = [[SearchResult(self.doc_name(f, d), sc) for (f, d, sc) in rows[int(offs[i]):int(offs[i + 1])]]
               for i in range(len(offs) - 1)]
        return out if many else out[0]

    def coverage_ms(self):
        """stage times of the coverage searches since the previous call of this method (HIP events, summed over passes)"""
        t = (C.c_double * 3)()
        check(self._lib.cobs_gpu_coverage_ms(self._h, C.byref(t)))
        return {"hash_ms": t[0], "scan_ms": t[1], "passes": int(t[2])}

    # -- window search: score documents by their best window of the query -------------
    def search_window_arrays(self, queries, window, threshold=0.0, num_results=0):
        """cobs_gpu_search_window -> (offsets uint64 [nq + 1], hits HIT_DTYPE): the records of query q are
        hits[offsets[q]:offsets[q + 1]], by best descending, then (file_no, doc); `score` is the largest number of set
        positions in any w = min(window, the query's positions) consecutive positions of the query; a document is a hit
        when it reaches max(1, ceil(threshold * w))."""
        if type(self)._search_batch_call is not Search._search_batch_call:
            raise CobsGpuError(_capi.ERR_UNSUPPORTED, "window: not on a device-list handle (the call has no counterpart there)")
        window = int(window)
        if not 0 <= window <= 0xFFFFFFFF:
            raise CobsGpuError(_capi.ERR_ARG, "window: not a 32-bit count of positions")
        qs = [q if type(q) is bytes else _as_bytes(q) for q in queries]
        nq = len(qs)
        arr = (C.c_char_p * max(nq, 1))(*qs)
        lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in qs])
        offs = np.zeros(nq + 1, dtype=np.uint64)
        bad = C.c_size_t(0)
        if num_results > 0:
            cap = nq * min(int(num_results), self.total_counts)
        elif threshold <= 0:
            cap = nq * self.total_counts
        else:
            # (a buffer that proves too small costs a second run of the whole call: sized by the hits per query of the
            # earlier thresholded window calls on this handle)
            cap = max(16 * nq, int(self.__dict__.get("_window_hits_per_query", 0.0) * nq * 1.25)) + 1024
        cap = max(1, cap)
        while True:
            hits = np.zeros(cap, dtype=self.HIT_DTYPE)
            st = self._lib.cobs_gpu_search_window(
                self._h, arr, lens, nq, window, float(threshold), int(num_results), C.cast(hits.ctypes.data, C.POINTER(Hit)),
                cap, C.cast(offs.ctypes.data, C.POINTER(C.c_size_t)), C.byref(bad))
            if st == _capi.ERR_CAPACITY and int(offs[nq]) > cap:
                cap = int(offs[nq])
                continue
            check(st)
            break
        if threshold > 0 and num_results == 0 and nq:
            self._window_hits_per_query = max(int(offs[nq]) / nq, 0.95 * self.__dict__.get("_window_hits_per_query", 0.0))
        return offs, hits[:int(offs[nq])]

    def search_window(self, query, window, threshold=0.0, num_results=0):
        """one query -> [SearchResult] in result order (doc_name, best window); a list or tuple of queries -> one such
        list per query"""
        many = isinstance(query, (list, tuple))
        offs, hits = self.search_window_arrays(list(query) if many else [query], window, threshold, num_results)
        rows = hits.tolist()
        out = [[SearchResult(self.doc_name(f, d), sc) for (f, d, sc) in rows[int(offs[i]):int(offs[i + 1])]]
               for i in range(len(offs) - 1)]
        return out if many else out[0]

    def window_ms(self):
        """stage times of the window searches since the previous call of this method (HIP events, summed over passes)"""
        t = (C.c_double * 3)()
        check(self._lib.cobs_gpu_window_ms(self._h, C.byref(t)))
        return {"hash_ms": t[0], "scan_ms": t[1], "passes": int(t[2])}

    # -- document sets: score a query against labelled groups of documents ----------
    SET_HIT_DTYPE = np.dtype([("file_no", "<u4"), ("set", "<u4"), ("any", "<u4"), ("all", "<u4")])
    SETS_RANK_BY = ("any", "all")           # COBS_GPU_SETS_BY_ANY / _BY_ALL

    def _sets_refuse_device_list(self):
        if type(self)._search_batch_call is not Search._search_batch_call:
            raise CobsGpuError(_capi.ERR_UNSUPPORTED, "sets: not on a device-list handle (any and all are not additive over shards)")

    def set_doc_sets(self, labels, file_no=0):
        """cobs_gpu_set_doc_sets: label the documents of file `file_no` with sets -- an integer array (-1: in no set) or a
        {doc_name: set_name} mapping (doc_set_labels) -- and return the set names, set number i -> names[i].  None clears
        the file's labels."""
        self._sets_refuse_device_list()
        names_of = self.__dict__.setdefault("_set_names", {})
        if labels is None:
            check(self._lib.cobs_gpu_set_doc_sets(self._h, int(file_no), None, 0, 0))
            names_of.pop(int(file_no), None)
            return []
        arr, names = doc_set_labels(labels, self._names(int(file_no)))
        arr = np.ascontiguousarray(arr, dtype=np.uint32)
        check(self._lib.cobs_gpu_set_doc_sets(self._h, int(file_no), C.cast(arr.ctypes.data, C.POINTER(C.c_uint32)), len(arr),
                                              len(names)))
        names_of[int(file_no)] = names
        return names

    def doc_sets(self, file_no=0):
        """cobs_gpu_get_doc_sets -> (set names, members uint32 [n_sets]): how many documents every set of the file holds;
        ([], empty) for a file without labels"""
        n = C.c_uint32(0)
        check(self._lib.cobs_gpu_get_doc_sets(self._h, int(file_no), C.byref(n), None, 0))
        members = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            check(self._lib.cobs_gpu_get_doc_sets(self._h, int(file_no), C.byref(n), C.cast(members.ctypes.data, C.POINTER(C.c_uint32)),
                                                  members.size))
        names = self.__dict__.get("_set_names", {}).get(int(file_no))
        if names is None or len(names) != n.value:
            names = [str(i) for i in range(n.value)]
        return list(names), members

    def search_sets_arrays(self, queries, threshold=0.0, rank_by="any", num_results=0):
        """cobs_gpu_search_sets -> (offsets uint64 [nq + 1], hits SET_HIT_DTYPE): the records of query q are
        hits[offsets[q]:offsets[q + 1]] -- one per non-empty set of every labelled file whose key (any or all, by rank_by)
        reaches max(1, ceil(threshold * P)) --, by key descending, then the other count descending, then (file_no, set)."""
        self._sets_refuse_device_list()
        if rank_by not in self.SETS_RANK_BY:
            raise ValueError("rank_by: 'any' or 'all'")
        qs = [q if type(q) is bytes else _as_bytes(q) for q in queries]
        nq = len(qs)
        arr = (C.c_char_p * max(nq, 1))(*qs)
        lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in qs])
        offs = np.zeros(nq + 1, dtype=np.uint64)
        bad = C.c_size_t(0)
        per_query = sum(int(np.count_nonzero(self.doc_sets(f)[1])) for f in range(self.num_files))
        cap = max(1, nq * (min(int(num_results), per_query) if num_results > 0 else per_query))
        while True:
            hits = np.zeros(cap, dtype=self.SET_HIT_DTYPE)
            st = self._lib.cobs_gpu_search_sets(
                self._h, arr, lens, nq, float(threshold), self.SETS_RANK_BY.index(rank_by), int(num_results),
                C.cast(hits.ctypes.data, C.POINTER(SetHit)), cap, C.cast(offs.ctypes.data, C.POINTER(C.c_size_t)), C.byref(bad))
            if st == _capi.ERR_CAPACITY and int(offs[nq]) > cap:
                cap = int(offs[nq])
                continue
            check(st)
            break
        return offs, hits[:int(offs[nq])]

    def search_sets(self, queries, threshold=0.0, rank_by="any", num_results=0):
        """-> one list per query of SetResult(file_no, set, name, any, all) in result order; one str / bytes query -> its list"""
        single = isinstance(queries, (str, bytes, bytearray))
        qs = [queries] if single else list(queries)
        offs, hits = self.search_sets_arrays(qs, threshold, rank_by, num_results)
        names = {f: self.doc_sets(f)[0] for f in range(self.num_files)}
        rows = hits.tolist()
        out = [[SetResult(f, s, names[f][s], a, b) for (f, s, a, b) in rows[int(offs[q]):int(offs[q + 1])]] for q in range(len(qs))]
        return out[0] if single else out

    def sets_ms(self):
        """stage times of the set searches since the previous call of this method (HIP events, summed over passes; the
        ordering on the host clock)"""
        t = (C.c_double * 5)()
        check(self._lib.cobs_gpu_sets_ms(self._h, C.byref(t)))
        return {"hash_ms": t[0], "presence_ms": t[1], "select_ms": t[2], "order_ms": t[3], "passes": int(t[4])}

    # -- document sets: the soft core of a set and the prevalence per set -----------
    SET_QUORUM_HIT_DTYPE = np.dtype([("file_no", "<u4"), ("set", "<u4"), ("core", "<u4"), ("any", "<u4")])

    def search_sets_quorum_arrays(self, queries, quorum, threshold=0.0, num_results=0):
        """cobs_gpu_search_sets_quorum -> (offsets uint64 [nq + 1], hits SET_QUORUM_HIT_DTYPE): the records of query q are
        hits[offsets[q]:offsets[q + 1]] -- one per non-empty set of every labelled file whose core (the positions at least
        max(1, ceil(quorum * members)) members hold, 0 < quorum <= 1) reaches max(1, ceil(threshold * P)) --, by core
        descending, then any descending, then (file_no, set)."""
        self._sets_refuse_device_list()
        qs = [q if type(q) is bytes else _as_bytes(q) for q in queries]
        nq = len(qs)
        arr = (C.c_char_p * max(nq, 1))(*qs)
        lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in qs])
        offs = np.zeros(nq + 1, dtype=np.uint64)
        bad = C.c_size_t(0)
        per_query = sum(int(np.count_nonzero(self.doc_sets(f)[1])) for f in range(self.num_files))
        cap = max(1, nq * (min(int(num_results), per_query) if num_results > 0 else per_query))
        while True:
            hits = np.zeros(cap, dtype=self.SET_QUORUM_HIT_DTYPE)
            st = self._lib.cobs_gpu_search_sets_quorum(
                self._h, arr, lens, nq, float(threshold), float(quorum), int(num_results),
                C.cast(hits.ctypes.data, C.POINTER(SetQuorumHit)), cap, C.cast(offs.ctypes.data, C.POINTER(C.c_size_t)), C.byref(bad))
            if st == _capi.ERR_CAPACITY and int(offs[nq]) > cap:
                cap = int(offs[nq])
                continue
            check(st)
            break
        return offs, hits[:int(offs[nq])]

    def search_sets_quorum(self, query, quorum, threshold=0.0, num_results=0):
        """-> one list per query of SetQuorumResult(file_no, set, name, core, any) in result order; one str / bytes query ->
        its list"""
        single = isinstance(query, (str, bytes, bytearray))
        qs = [query] if single else list(query)
        offs, hits = self.search_sets_quorum_arrays(qs, quorum, threshold, num_results)
        names = {f: self.doc_sets(f)[0] for f in range(self.num_files)}
        rows = hits.tolist()
        out = [[SetQuorumResult(f, s, names[f][s], c, a) for (f, s, c, a) in rows[int(offs[q]):int(offs[q + 1])]] for q in range(len(qs))]
        return out[0] if single else out

    def set_prevalence_arrays(self, queries):
        """cobs_gpu_set_prevalence -> (offsets uint64 [nq * num_files + 1], counts uint32): segment (q, f) is
        counts[offsets[q * num_files + f]:offsets[q * num_files + f + 1]], the file's non-empty sets (ascending set number) x
        the n = T_f - findere positions of query q, set-major: how many members of the set hold the position.  A file
        without labels has an empty segment."""
        self._sets_refuse_device_list()
        qs = [q if type(q) is bytes else _as_bytes(q) for q in queries]
        nq = len(qs)
        arr = (C.c_char_p * max(nq, 1))(*qs)
        lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in qs])
        offsets = np.zeros(nq * self.num_files + 1, dtype=np.uint64)
        need, bad = C.c_size_t(0), C.c_size_t(0)
        # the number of cells is host arithmetic (the call refuses a buffer that is too small before any device work)
        counts = np.zeros(0, dtype=np.uint32)
        while True:
            st = self._lib.cobs_gpu_set_prevalence(
                self._h, arr, lens, nq, C.cast(counts.ctypes.data, C.POINTER(C.c_uint32)), counts.size,
                C.cast(offsets.ctypes.data, C.POINTER(C.c_size_t)), C.byref(need), C.byref(bad))
            if st == _capi.ERR_CAPACITY and need.value > counts.size:
                counts = np.zeros(need.value, dtype=np.uint32)
                continue
            check(st)
            break
        return offsets, counts

    def set_prevalence(self, query):
        """per query a list with one uint32 array [non-empty sets, n] per file (set_prevalence_arrays, cut up; row c belongs to
        the c-th set with members, ascending set number); one str / bytes query -> its list"""
        single = isinstance(query, (str, bytes, bytearray))
        qs = [query] if single else list(query)
        offsets, counts = self.set_prevalence_arrays(qs)
        nf = self.num_files
        nsets = [int(np.count_nonzero(self.doc_sets(f)[1])) for f in range(nf)]
        out = [[counts[int(offsets[q * nf + f]):int(offsets[q * nf + f + 1])].reshape(nsets[f], -1) if nsets[f] else
                np.zeros((0, 0), dtype=np.uint32) for f in range(nf)] for q in range(len(qs))]
        return out[0] if single else out

    def set_quorum_ms(self):
        """stage times of the quorum searches and set prevalences since the previous call of this method (HIP events, summed
        over passes; the ordering on the host clock)"""
        t = (C.c_double * 5)()
        check(self._lib.cobs_gpu_set_quorum_ms(self._h, C.byref(t)))
        return {"hash_ms": t[0], "count_ms": t[1], "select_ms": t[2], "order_ms": t[3], "passes": int(t[4])}

    # -- grouped search: which documents a SET of queries comes from -----------------
    GROUP_HIT_DTYPE = np.dtype([("file_no", "<u4"), ("doc", "<u4"), ("score", "<u4"), ("votes", "<u4")])

    def search_groups_arrays(self, queries, group_offsets, threshold=0.0, read_threshold=0.0, num_results=0):
        """cobs_gpu_search_groups: group g is queries[group_offsets[g]:group_offsets[g + 1]] (contiguous; n_groups + 1
        non-decreasing offsets from 0 to len(queries))
        -> (hit_offsets uint64 [n_groups + 1], hits GROUP_HIT_DTYPE, positions uint64 [n_groups, num_files]): the records of
        group g are hits[hit_offsets[g]:hit_offsets[g + 1]], by score (the sum over the group's queries) descending, then
        (file_no, doc); votes = the group's queries the document was a hit of at read_threshold."""
        if type(self)._search_batch_call is not Search._search_batch_call:
            raise CobsGpuError(_capi.ERR_UNSUPPORTED, "groups: not on a device-list handle (a group's totals are per shard)")
        qs = [q if type(q) is bytes else _as_bytes(q) for q in queries]
        nq = len(qs)
        goffs = np.ascontiguousarray(group_offsets, dtype=np.uint64)
        if goffs.ndim != 1 or len(goffs) < 1:
            raise ValueError("group_offsets needs n_groups + 1 entries")
        ng = len(goffs) - 1
        arr = (C.c_char_p * max(nq, 1))(*qs)
        lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in qs])
        offs = np.zeros(ng + 1, dtype=np.uint64)
        pos = np.zeros((ng, max(self.num_files, 1)), dtype=np.uint64)
        bad = C.c_size_t(0)
        if num_results > 0:
            cap = ng * min(num_results, self.total_counts)
        elif threshold <= 0:
            cap = ng * self.total_counts
        else:
            cap = 16 * ng + 1024           # (too small: the call reports the needed size and is made again)
        cap = max(1, cap)
        while True:
            hits = np.zeros(cap, dtype=self.GROUP_HIT_DTYPE)
            st = self._lib.cobs_gpu_search_groups(
                self._h, arr, lens, nq, C.cast(goffs.ctypes.data, C.POINTER(C.c_size_t)), ng, float(threshold),
                float(read_threshold), int(num_results), C.cast(hits.ctypes.data, C.POINTER(GroupHit)), cap,
                C.cast(offs.ctypes.data, C.POINTER(C.c_size_t)), C.cast(pos.ctypes.data, C.POINTER(C.c_uint64)), C.byref(bad))
            if st == _capi.ERR_CAPACITY and int(offs[ng]) > cap:
                cap = int(offs[ng])
                continue
            check(st)
            break
        return offs, hits[:int(offs[ng])], pos[:, :self.num_files]

    def search_groups(self, queries, group_offsets, threshold=0.0, read_threshold=0.0, num_results=0, return_positions=False):
        """-> one list per group of GroupResult(doc_name, score, votes); return_positions=True: (that, P uint64
        [n_groups, num_files]), the positions every group was scored over per file (see cobs_gpu_search_groups)"""
        offs, hits, pos = self.search_groups_arrays(queries, group_offsets, threshold, read_threshold, num_results)
        rows = hits.tolist()
        out = [[GroupResult(self._names(f)[d], s, v) for (f, d, s, v) in rows[int(offs[g]):int(offs[g + 1])]]
               for g in range(len(offs) - 1)]
        return (out, pos) if return_positions else out

    def search_paired(self, reads1, reads2, threshold=0.0, read_threshold=0.0, num_results=0, return_positions=False):
        """groups of two: pair i is (reads1[i], reads2[i])"""
        if len(reads1) != len(reads2):
            raise ValueError("reads1 and reads2 differ in length")
        queries = [r for pair in zip(reads1, reads2) for r in pair]
        return self.search_groups(queries, np.arange(len(reads1) + 1, dtype=np.uint64) * 2, threshold, read_threshold,
                                  num_results, return_positions)

    def groups_ms(self):
        """the last search_groups call: accumulate kernel and select kernel (HIP events), host ordering; milliseconds"""
        t = (C.c_double * 3)()
        check(self._lib.cobs_gpu_groups_ms(self._h, C.byref(t)))
        return {"accumulate_ms": t[0], "select_ms": t[1], "order_ms": t[2]}

    # -- best of a group: every document's best query of a group ------------------------
    BEST_HIT_DTYPE = np.dtype([("file_no", "<u4"), ("doc", "<u4"), ("query", "<u4"), ("score", "<u4"), ("positions", "<u4"),
                               ("ties", "<u4")])

    def search_best_arrays(self, queries, group_offsets=None, threshold=0.0, num_results=0, group_size=None):
        """cobs_gpu_search_best: group g is queries[group_offsets[g]:group_offsets[g + 1]] (contiguous; n_groups + 1
        non-decreasing offsets from 0 to len(queries)), or every group_size consecutive queries
        -> (hit_offsets uint64 [n_groups + 1], hits BEST_HIT_DTYPE): the records of group g are
        hits[hit_offsets[g]:hit_offsets[g + 1]], one per document whose best query of the group reaches threshold of its
        own positions, by score / positions descending, then score descending, then (file_no, doc)."""
        if type(self)._search_batch_call is not Search._search_batch_call:
            raise CobsGpuError(_capi.ERR_UNSUPPORTED, "best: not on a device-list handle (ask every shard for its documents)")
        qs = [q if type(q) is bytes else _as_bytes(q) for q in queries]
        nq = len(qs)
        if (group_offsets is None) == (group_size is None):
            raise ValueError("give group_offsets or group_size")
        if group_offsets is None:
            if int(group_size) < 1:
                raise ValueError("group_size needs to be at least 1")
            group_offsets = list(range(0, nq, int(group_size))) + [nq]
        goffs = np.ascontiguousarray(group_offsets, dtype=np.uint64)
        if goffs.ndim != 1 or len(goffs) < 1:
            raise ValueError("group_offsets needs n_groups + 1 entries")
        ng = len(goffs) - 1
        arr = (C.c_char_p * max(nq, 1))(*qs)
        lens = (C.c_size_t * max(nq, 1))(*[len(q) for q in qs])
        offs = np.zeros(ng + 1, dtype=np.uint64)
        bad = C.c_size_t(0)
        if num_results > 0:
            cap = ng * min(num_results, self.total_counts)
        elif threshold <= 0:
            cap = ng * self.total_counts
        else:
            cap = 16 * ng + 1024           # (too small: the call reports the needed size and is made again)
        cap = max(1, cap)
        while True:
            hits = np.zeros(cap, dtype=self.BEST_HIT_DTYPE)
            st = self._lib.cobs_gpu_search_best(
                self._h, arr, lens, nq, C.cast(goffs.ctypes.data, C.POINTER(C.c_size_t)), ng, float(threshold),
                int(num_results), C.cast(hits.ctypes.data, C.POINTER(BestHit)), cap,
                C.cast(offs.ctypes.data, C.POINTER(C.c_size_t)), C.byref(bad))
            if st == _capi.ERR_CAPACITY and int(offs[ng]) > cap:
                cap = int(offs[ng])
                continue
            check(st)
            break
        return offs, hits[:int(offs[ng])]

    def search_best(self, queries, group_offsets=None, threshold=0.0, num_results=0, group_size=None):
        """-> one list per group of BestResult(doc_name, file_no, doc, query, score, positions, ties): for every document
        the group's best query (see cobs_gpu_search_best)"""
        offs, hits = self.search_best_arrays(queries, group_offsets, threshold, num_results, group_size)
        rows = hits.tolist()
        return [[BestResult(self._names(f)[d], f, d, q, s, p, t) for (f, d, q, s, p, t) in rows[int(offs[g]):int(offs[g + 1])]]
                for g in range(len(offs) - 1)]

    def best_ms(self):
        """the last search_best call: best-member and merge kernels, select kernel (HIP events), host ordering;
        milliseconds -- and how it was launched: device passes, spans that owned their cells, partial states, split groups"""
        t = (C.c_double * 3)()
        check(self._lib.cobs_gpu_best_ms(self._h, C.byref(t)))
        n = (C.c_uint64 * 4)()
        check(self._lib.cobs_gpu_best_counts(self._h, C.byref(n)))
        return {"best_ms": t[0], "select_ms": t[1], "order_ms": t[2], "passes": int(n[0]), "own_spans": int(n[1]),
                "pieces": int(n[2]), "split_groups": int(n[3])}

    def positions_ms(self):
        """kernel times of the hit_positions calls since the previous call of this method (HIP events, summed over passes)"""
        t = (C.c_double * 3)()
        check(self._lib.cobs_gpu_positions_ms(self._h, C.byref(t)))
        return {"presence_ms": t[0], "hash_ms": t[1], "passes": int(t[2])}

    @property
    def graph_replays(self):
        """small host-API passes served by a captured hipGraph so far"""
        return int(self._lib.cobs_gpu_graph_replays(self._h))

    @property
    def host_passes(self):
        """device passes the host-buffer calls have launched on this handle so far"""
        return int(self._lib.cobs_gpu_host_passes(self._h))

    @property
    def self_hash_passes(self):
        """passes on this handle so far that ran in the self-hashing form of the scan (no K1), graph replays included"""
        return int(self._lib.cobs_gpu_self_hash_passes(self._h))

    def stream_counters(self):
        """out-of-core handles: (chunks fetched row by row, chunks copied whole) over all passes so far"""
        c = (C.c_uint64 * 2)()
        check(self._lib.cobs_gpu_stream_counters(self._h, C.byref(c)))
        return int(c[0]), int(c[1])

    def stream_traffic(self):
        """... and (bytes of looked-up rows fetched, bytes of whole chunks copied): what the passes asked of PCIe"""
        c = (C.c_uint64 * 4)()
        check(self._lib.cobs_gpu_stream_traffic(self._h, C.byref(c)))
        return int(c[0]), int(c[1]), int(c[2]), int(c[3])

    def stream_plan(self):
        """out-of-core handles: (bytes of one stream buffer, bytes of the streamed files kept resident beside the buffers,
        row bytes a whole-chunk pass moves over PCIe, streamed chunks)"""
        c = (C.c_uint64 * 4)()
        check(self._lib.cobs_gpu_stream_plan(self._h, C.byref(c)))
        return int(c[0]), int(c[1]), int(c[2]), int(c[3])

    def stream_layout(self, file_no=0):
        """how file `file_no` is held: (slices resident in HBM, streamed chunks of whole slices, streamed column slices,
        streamed row ranges)"""
        c = (C.c_uint64 * 4)()
        check(self._lib.cobs_gpu_stream_layout(self._h, int(file_no), C.byref(c)))
        return int(c[0]), int(c[1]), int(c[2]), int(c[3])

    def timers(self, reset=False):
        t = (C.c_double * 5)()
        check(self._lib.cobs_gpu_timers(self._h, C.byref(t), 1 if reset else 0))
        return dict(zip(["hashes", "h2d", "scan", "d2h", "rank"], list(t)))


class MultiSearch(Search):
    """The same Search over SEVERAL GPUs of one node from ONE process (cobs_gpu_multi_*): the
    index is sharded by sub-index block over `devices`, the library runs one worker thread per
    device and the exchange over RCCL; search / search_batch / search_arrays / search_packed
    return exactly what Search returns on one GPU."""

    def __init__(self, path, devices, hbm_budget=0, shard_mode=0, findere=0, invalid_bases="error"):
        self._lib = _capi.load()
        self._m = C.c_void_p()
        self._h = C.c_void_p()
        paths = [path] if isinstance(path, (str, bytes, os.PathLike)) else list(path)
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        devs = (C.c_int * max(1, len(devices)))(*[int(d) for d in devices])
        opts = _options(-1, 0, 1, hbm_budget, shard_mode)
        check(self._lib.cobs_gpu_multi_open(arr, len(paths), devs, len(devices), C.byref(opts), C.byref(self._m)))
        # rank 0's shard handle answers the geometry / name calls of the base class (not owned)
        self._h = C.c_void_p(self._lib.cobs_gpu_multi_index(self._m, 0))
        try:
            if findere:
                self.set_findere(findere)
            self.invalid_bases = invalid_bases
        except Exception:
            self.close()
            raise

    def close(self):
        if getattr(self, "_m", None):
            self._lib.cobs_gpu_multi_close(self._m)
            self._m = C.c_void_p()
            self._h = C.c_void_p()

    @property
    def comm_size(self):
        return int(self._lib.cobs_gpu_multi_size(self._m))

    def shard(self, rank):
        """geometry view of one rank's shard (a borrowed handle: valid until close())"""
        h = self._lib.cobs_gpu_multi_index(self._m, rank)
        if not h:
            raise IndexError(rank)
        v = Search(None, _handle=C.c_void_p(h))
        v.close = lambda: None          # the multi handle owns it
        return v

    def search_view(self, queries, threshold=0.0, num_results=0):
        raise NotImplementedError("the library-owned result arena belongs to a one-device handle; use search_arrays")

    def _search_batch_call(self, *args):
        return self._lib.cobs_gpu_multi_search_batch(self._m, *args)

    def _set_findere_call(self, z):
        return self._lib.cobs_gpu_multi_set_findere(self._m, z)

    def _get_findere_call(self, zp):
        return self._lib.cobs_gpu_multi_get_findere(self._m, zp)

    def _set_invalid_bases_call(self, mode):
        return self._lib.cobs_gpu_multi_set_invalid_bases(self._m, mode)

    def _get_invalid_bases_call(self, mp):
        return self._lib.cobs_gpu_multi_get_invalid_bases(self._m, mp)

    def counts(self, query):
        raise NotImplementedError("raw counts are per shard: use shard(rank).counts(query)")

    def doc_bits(self, file_no=0):
        """refused: a document's filter lives on one rank (doc_fill, doc_fpr and search_adjusted follow)"""
        raise CobsGpuError(_capi.ERR_UNSUPPORTED, "doc_bits: not on a device-list handle (ask the shards: shard(rank).doc_bits)")

    def doc_shared_bits(self, refs, file_no=0):
        """refused: a sub-index's columns may be cut between the ranks (similar_documents follows)"""
        raise CobsGpuError(_capi.ERR_UNSUPPORTED, "doc_shared_bits: not on a device-list handle")

    def similar_documents(self, ref, file_no=0, min_jaccard=0.0, num_results=0):
        raise CobsGpuError(_capi.ERR_UNSUPPORTED, "similar_documents: not on a device-list handle")


class _DevArray:
    """__cuda_array_interface__ view of HBM owned by libcobs_gpu (zero copy into torch)."""

    def __init__(self, ptr, shape, typestr, owner):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False),
                                         "version": 2, "strides": None}
        self._owner = owner


class Batch:
    """Device-resident query batch (cobs_gpu_batch_*): inputs are copied to HBM
    once, run() launches the hot path asynchronously, counts stay in HBM."""

    def __init__(self, search, max_queries=0, max_query_len=0, _borrowed=None):
        self._s = search
        self._lib = search._lib
        self._h = C.c_void_p()
        self._owned = _borrowed is None
        if _borrowed is not None:           # a sub-batch of a ShardedBatch: the library object owns it
            self._h = C.c_void_p(_borrowed)
        else:
            check(self._lib.cobs_gpu_batch_create(search._h, max_queries, max_query_len, C.byref(self._h)))
        self.nq = 0

    def close(self):
        if getattr(self, "_h", None):
            if self._owned:
                self._lib.cobs_gpu_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_queries(self, queries):
        qs = [_as_bytes(q) for q in queries]
        arr = (C.c_char_p * max(len(qs), 1))(*qs)
        lens = (C.c_size_t * max(len(qs), 1))(*[len(q) for q in qs])
        check(self._lib.cobs_gpu_batch_set_queries(self._h, arr, lens, len(qs)))
        self.nq = len(qs)

    def run(self, threshold=0.0, stream=0):
        check(self._lib.cobs_gpu_batch_run(self._h, float(threshold), C.c_void_p(stream)))

    def run_hits(self, threshold, stream=0):
        """hot path without score rows: only the documents reaching the threshold are recorded"""
        check(self._lib.cobs_gpu_batch_run_hits(self._h, float(threshold), C.c_void_p(stream)))

    def run_topk(self, threshold=0.0, num_results=10, stream=0, keep_counts=True):
        """hot path + on-device selection of the num_results best documents per query;
        keep_counts=False: no score rows (K2 selects per tile, K3 merges the candidates)"""
        fn = self._lib.cobs_gpu_batch_run_topk if keep_counts else self._lib.cobs_gpu_batch_run_topk_only
        check(fn(self._h, float(threshold), int(num_results), C.c_void_p(stream)))

    def sync(self, stream=0):
        bad = C.c_size_t(0)
        check(self._lib.cobs_gpu_batch_sync(self._h, C.c_void_p(stream), C.byref(bad)))

    def scored_positions(self, file_no=0):
        """positions every query was scored over in one file (after sync): the valid ones under invalid_bases "miss" and
        "skip", len - k + 1 - findere under "error" -- what a score is divided by"""
        out = np.zeros(max(self.nq, 1), dtype=np.uint32)
        check(self._lib.cobs_gpu_batch_scored_positions(self._h, file_no, out.ctypes.data))
        return out[:self.nq]

    def counts_device(self):
        """-> (device pointer, element bytes, row stride bytes)"""
        eb, rs = C.c_uint32(0), C.c_uint64(0)
        p = self._lib.cobs_gpu_batch_counts_device(self._h, C.byref(eb), C.byref(rs))
        return p, eb.value, rs.value

    def counts_tensor(self):
        """torch view [nq, local_counts]: uint8 scores when no query of the batch has more than 255
        terms (the reference's uint8_t path), else int16 / int32 bit patterns of u16 / u32 scores."""
        import torch
        p, eb, rs = self.counts_device()
        n = self._s.local_counts
        if self.nq == 0 or n == 0:
            return torch.empty((self.nq, n), dtype={1: torch.uint8, 2: torch.int16}.get(eb, torch.int32),
                               device="cuda")
        return torch.as_tensor(_DevArray(p, (self.nq, n), {1: "|u1", 2: "<i2"}.get(eb, "<i4"), self), device="cuda")

    # -- multi-GPU exchange (native RCCL, comm.cpp) ---------------------------------------
    def exchange_counts(self, comm, mode=_capi.XCHG_ALLTOALL, stream=0):
        check(self._lib.cobs_gpu_batch_exchange_counts(self._h, comm._h, int(mode), C.c_void_p(stream)))

    def exchange_hits(self, comm, stream=0):
        """-> True if some shard's hit pool overflowed (lists incomplete)"""
        over = C.c_int(0)
        check(self._lib.cobs_gpu_batch_exchange_hits(self._h, comm._h, C.c_void_p(stream), C.byref(over)))
        return bool(over.value)

    def exchange_hits_owned(self, comm, stream=0):
        """every hit record to the rank that owns its query -> (overflowed, first owned query, owned queries)"""
        over, q0, qn = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        check(self._lib.cobs_gpu_batch_exchange_hits_owned(self._h, comm._h, C.c_void_p(stream), C.byref(over),
                                                           C.byref(q0), C.byref(qn)))
        return bool(over.value), int(q0.value), int(qn.value)

    def bucketed_hits(self, nranks):
        """diagnostics: the hit pool of the last run bucketed by query owner as `nranks` ranks would
        -> (counts per owner, records uint32 [n][4] = query, file, doc, score)"""
        counts = (C.c_uint64 * nranks)()
        n = C.c_size_t(0)
        cap = 1 << 16
        while True:
            rec = np.zeros((cap, 4), dtype=np.uint32)
            st = self._lib.cobs_gpu_batch_bucketed_hits(self._h, nranks, counts, rec.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                        cap, C.byref(n))
            if st == _capi.ERR_CAPACITY and n.value > cap:
                cap = n.value
                continue
            check(st)
            return list(counts), rec[:n.value]

    def exchange_topk(self, comm, stream=0):
        check(self._lib.cobs_gpu_batch_exchange_topk(self._h, comm._h, C.c_void_p(stream)))

    def exchange_bytes(self):
        return int(self._lib.cobs_gpu_batch_exchange_bytes(self._h))

    def global_counts_tensor(self):
        """after exchange_counts: (q_begin, q_count, torch view [q_count, total_counts]) of the
        assembled rows this rank holds (global document order)"""
        import torch
        q0, qn, eb, rs = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        p = self._lib.cobs_gpu_batch_global_counts_device(self._h, C.byref(q0), C.byref(qn), C.byref(eb), C.byref(rs))
        n = self._s.total_counts
        dt = {1: torch.uint8, 2: torch.int16}.get(eb.value, torch.int32)
        if not p or qn.value == 0 or n == 0:
            return int(q0.value), int(qn.value), torch.empty((int(qn.value), n), dtype=dt, device="cuda")
        t = torch.as_tensor(_DevArray(p, (int(qn.value), n), {1: "|u1", 2: "<i2"}.get(eb.value, "<i4"), self),
                            device="cuda")
        return int(q0.value), int(qn.value), t

    def counts_host(self, query_no):
        out = np.zeros(self._s.total_counts, dtype=np.uint32)
        check(self._lib.cobs_gpu_batch_counts_host(self._h, query_no, out.ctypes.data, out.size))
        return out

    def score_histogram(self, nbins):
        """distribution of the scores of the last run over its real documents (`cobs benchmark-fpr --dist`) -> uint64[nbins]"""
        h = np.zeros(nbins, dtype=np.uint64)
        check(self._lib.cobs_gpu_batch_score_histogram(self._h, h.ctypes.data_as(C.POINTER(C.c_uint64)), nbins))
        return h

    def hits_host(self, query_no, num_results=0):
        cap = max(1, self._s.total_counts if num_results == 0 else min(num_results, self._s.total_counts))
        hits = (Hit * cap)()
        n = C.c_size_t(0)
        check(self._lib.cobs_gpu_batch_hits_host(self._h, query_no, int(num_results), hits, cap, C.byref(n)))
        return [(hits[i].file_no, hits[i].doc, hits[i].score) for i in range(n.value)]

    def stats(self):
        s = (C.c_uint64 * 4)()
        check(self._lib.cobs_gpu_batch_stats(self._h, C.byref(s)))
        return {"algorithmic_bytes": int(s[0]), "scan_launches": int(s[1]), "kmer_lookups": int(s[2]),
                "table_bytes": int(s[3])}

    def scan_geometry(self):
        """the launch geometry of the last scan launch outside a replayed graph (diagnostics)"""
        g = (C.c_uint32 * 4)()
        check(self._lib.cobs_gpu_batch_scan_geometry(self._h, C.byref(g)))
        return {"tile_w": int(g[0]), "waves": int(g[1]), "mq": bool(g[2]), "lds_staged": bool(g[3])}

    def kernel_ms(self):
        a, b = C.c_float(0), C.c_float(0)
        check(self._lib.cobs_gpu_batch_kernel_ms(self._h, C.byref(a), C.byref(b)))
        return {"scan_ms": a.value, "hash_ms": b.value}


__all__ = ["Search", "SearchResult", "GroupResult", "BestResult", "AdjustedResult", "Batch", "CobsGpuError", "unpack_positions", "fpr_adjust"]


class ShardedBatch:
    """The device-resident form of the sharded search (cobs_gpu_sharded_batch_*): ONE batch of queries, uploaded once;
    step() scans it on this rank's shard and exchanges the count rows over the communicator -- cut into sub-batches
    whose hashing, scan and exchange overlap inside the library (three streams tied by events), also across steps.
    Collective: every rank makes the same calls.  sub(i) are the sub-batches as Batch views (global / local count rows)."""

    def __init__(self, search, comm, sub_batches=1):
        self._s, self._comm = search, comm
        self._lib = search._lib
        self._h = C.c_void_p()
        check(self._lib.cobs_gpu_sharded_batch_create(search._h, comm._h, int(sub_batches), C.byref(self._h)))
        self.nq = 0
        self._subs = []

    def close(self):
        if getattr(self, "_h", None):
            for b in self._subs:
                b.close()
            self._lib.cobs_gpu_sharded_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_queries(self, queries):
        qs = [_as_bytes(q) for q in queries]
        arr = (C.c_char_p * max(len(qs), 1))(*qs)
        lens = (C.c_size_t * max(len(qs), 1))(*[len(q) for q in qs])
        check(self._lib.cobs_gpu_sharded_batch_set_queries(self._h, arr, lens, len(qs)))
        self.nq = len(qs)
        self._subs = []
        for i in range(int(self._lib.cobs_gpu_sharded_batch_subs(self._h))):
            q0, qn = C.c_size_t(0), C.c_size_t(0)
            h = self._lib.cobs_gpu_sharded_batch_sub(self._h, i, C.byref(q0), C.byref(qn))
            b = Batch(self._s, _borrowed=h)
            b.nq, b.q_begin = int(qn.value), int(q0.value)
            self._subs.append(b)

    @property
    def subs(self):
        return list(self._subs)

    def step(self, threshold=0.0, mode=_capi.XCHG_ALLTOALL):
        check(self._lib.cobs_gpu_sharded_batch_step(self._h, float(threshold), int(mode)))

    def sync(self):
        bad = C.c_size_t(0)
        check(self._lib.cobs_gpu_sharded_batch_sync(self._h, C.byref(bad)))

    def times(self):
        """after sync(): per step, summed over the sub-batches, averaged over the steps since the previous call"""
        t = (C.c_double * 8)()
        check(self._lib.cobs_gpu_sharded_batch_times(self._h, C.byref(t)))
        return {"scan_ms": t[0], "hash_ms": t[1], "exchange_ms": t[2], "algorithmic_bytes": int(t[3]),
                "received_bytes": int(t[4]), "scan_launches": int(t[5]), "steps": int(t[6])}
