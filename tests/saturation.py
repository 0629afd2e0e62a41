"""Counters at their largest value (test infrastructure): fixtures whose documents hold EVERY row, the plane boundaries
every score counter of the engine changes at, and the values such documents have to reach, stated analytically.  Nothing
here loads the GPU library; the index files are written with oracle/construct.py and read by both sides.

The boundaries, beside the source line each comes from -- a change of one of these tables shows which cases to move:

  counter                    source                                        planes / rows                 cases here
  plain and findere scan     kernels.hip: scan_planes_for                  4 | 8 | 10 | 12 | 16 | 20     PLAIN_T = 15/16, 255/256, 1023/1024,
                             (bit width of max_terms; kernels.hpp:         | 24 | 32; u8 rows up to 8,   4095/4096, 65 535/65 536, 2^20 - 1/2^20
                             scan_score_bytes)                             u16 up to 16, u32 above       (2^24 - 1/2^24: PLAIN_T_HUGE, see below)
  weighted scan              weighted_kernels.hip: weighted_planes_for     8 | 12 | 14 | 16 | 20 for     WEIGHTED_N = 17/18, 273/274, 1092/1093,
                             (15 n < 2^planes)                             the top score 15 n            4369/4370, 69 905 (the refusal limit)
  coverage scan              coverage_kernels.hip: coverage_planes_for     8 | 12 | 16 | 20 by the       COVERAGE_L = 255/256, 4095/4096,
                             (len < 2^planes)                              query length                  65 535/65 536, 2^20 - 1
  window scan                window_kernels.hip: window_planes_for         6 | 8 | 10 | 12 by W          WINDOW_W = 63/64, 255/256, 1023/1024, 4095
                             (W < 2^planes)
  fill, similarity           fill_kernels.hpp: kFillPlanes = 12,           a flush every 4088 rows       FLUSH_SIGS = 4087/4088/4089, 8176/8177 in
                             similarity_kernels.hpp: kSimPlanes = 12                                     test_fill_and_shared_bits_around_the_flush
  group totals, best-of      groups.cpp / best.cpp: row bytes of a pass    u8 | u16 | u32 member rows,   GROUP_MEMBERS = 2, 257, 258 members of
                             (terms <= 255 ? 1 : terms <= 65535 ? 2 : 4),  32-bit sums (refused from     255 terms: totals 510, 65 535, 65 790
                             32-bit sums                                   2^32 on)
  prevalence, set counts     prevalence_kernels.hip, sets.cpp,             32-bit counts per position    SET_SIZES = 255, 256, 257 documents
                             set_quorum.cpp                                                              (prevalence also 65 535 / 65 536)

The pair 2^24 - 1 / 2^24 (24 -> 32 planes) has no GPU case: it was to stay only if it cost no more GPU time than
tests/test_gpu_rank.py::test_three_radix_passes, and it costs more.  Measured in one process on an MI355X, on a 12-document
index of 2^25 + 35 rows (large enough to leave the near-full documents' rows to their terms): run(0.0) and run(1.0) of both
queries take 382 ms around their GPU calls, 147 ms of it in kernels (four scans of 36.7 ms over 17 M gathered rows each);
the search_arrays call of test_three_radix_passes takes 153 ms, 146 ms on the device (119 ms of it its upload).  The CPU
test still holds PLAIN_T_HUGE against the plane table.

The fixture idea.  A document whose column is all ones holds every term of every query, whatever k, H or z: its plain
score is T - z, its coverage len(q), its best window min(W, n), its weighted score the total weight.  Every index holds such
FULL documents at the slots 0, 7, 8, 127, 128 and D - 1 (the first and last bit of a byte, the edge of a 16-byte chunk, the
last real document; a slot the index is too small for is left out), an EMPTY document, NEAR0 = every row but the row of term
0 of the index's source text, NEAR_MID = every row but the row of term 30, and 0.3-density random documents around them.
The source text of an index is chosen (seed_of) so that those two rows belong to NO other term of its longest query: NEAR0
then misses exactly term 0 and NEAR_MID exactly term 30 of every query SRC[:T + k - 1] cut from it.
"""
import functools
import os

import numpy as np

K = 31
MID_TERM = 30
FULL_SLOTS = (0, 7, 8, 127, 128)
SMALL_T = 4096                                   # up to here the numpy checkers restate every case, and every index runs

PLAIN_T = (15, 16, 255, 256, 1023, 1024, 4095, 4096, 65535, 65536, 2 ** 20 - 1, 2 ** 20)
PLAIN_T_HUGE = (2 ** 24 - 1, 2 ** 24)
PLAIN_PLANES = {15: 4, 16: 8, 255: 8, 256: 10, 1023: 10, 1024: 12, 4095: 12, 4096: 16, 65535: 16, 65536: 20,
                2 ** 20 - 1: 20, 2 ** 20: 24, 2 ** 24 - 1: 24, 2 ** 24: 32}
FINDERE_Z = 3
WEIGHTED_N = (17, 18, 273, 274, 1092, 1093, 4369, 4370, 69905)
WEIGHTED_CHECKED = 274                           # the checker restates the weighted cases up to here
WEIGHTED_DOCS, WEIGHTED_SIG, WEIGHTED_FULL = 40000, 257, 12345
COVERAGE_L = (255, 256, 4095, 4096, 65535, 65536, 2 ** 20 - 1)
WINDOW_W = (63, 64, 255, 256, 1023, 1024, 4095)
GROUP_MEMBERS = (2, 257, 258)
GROUP_TERMS = 255
SET_SIZES = (255, 256, 257)
FLUSH_SIGS = (4087, 4088, 4089, 8176, 8177)


def planes_for(T):
    """kernels.hip: scan_planes_for, restated"""
    need = max(1, int(T).bit_length())
    return [v for v in (4, 8, 10, 12, 16, 20, 24, 32) if v >= need][0]


def score_bytes(T):
    """kernels.hpp: scan_score_bytes"""
    p = planes_for(T)
    return 1 if p <= 8 else 2 if p <= 16 else 4


def window_positions(W):
    return (W - 1, W, W + 1, 2 * W + 3)


# ---- the indexes ------------------------------------------------------------------------------------------------------------
class Spec:
    def __init__(self, name, kind, num_docs, sigs, page_size=0, num_hashes=1, k=K, tmax=SMALL_T, mask=True, near_page=0):
        self.name, self.kind, self.num_docs, self.sigs, self.page_size = name, kind, num_docs, sigs, page_size
        self.num_hashes, self.k, self.tmax, self.mask, self.near_page = num_hashes, k, tmax, mask, near_page


SPECS = {
    # the padding slots 12 .. 15 of its two-byte rows keep their random and all-ones bits: they must not come back
    "narrow": Spec("narrow", "classic", 12, [(1 << 21) + 17], tmax=2 ** 20, mask=False),
    "narrow_h3": Spec("narrow_h3", "classic", 12, [(1 << 17) + 29], num_hashes=3),
    "narrow_k248": Spec("narrow_k248", "classic", 12, [(1 << 15) + 3], k=248),
    "wide": Spec("wide", "classic", 1027, [2003]),
    # three sub-indexes of 128 documents, the last one holds 44; the near-full documents live in the 4097-row one
    "compact": Spec("compact", "compact", 300, [1, 65, 4097], page_size=16, near_page=2),
}
SMALL_INDEXES = ("narrow", "wide", "compact")


def _rows_of(spec, text, sig):
    from oracle import oracle as O
    h, good = O.term_hashes(text, spec.k, 1, spec.num_hashes)
    assert good.all()
    return (h % np.uint64(sig)).astype(np.int64)           # [T, H]


@functools.lru_cache(maxsize=None)
def seed_of(name):
    """the first seed from 1000 on whose text has the rows of (term 0, hash 0) and (term MID_TERM, hash 0) to themselves
    among all (term, hash) rows of its tmax-term query, in the sub-index of the near-full documents"""
    from oracle import oracle as O
    spec = SPECS[name]
    sig = spec.sigs[spec.near_page]
    for seed in range(1000, 6000):
        short = _rows_of(spec, O.random_sequence(min(spec.tmax, 512) + spec.k - 1, seed), sig).reshape(-1)
        if (short == short[0]).sum() != 1 or (short == short[MID_TERM * spec.num_hashes]).sum() != 1:
            continue                                       # (the first 512 terms decide most seeds cheaply)
        rows = _rows_of(spec, O.random_sequence(spec.tmax + spec.k - 1, seed), sig)
        flat = rows.reshape(-1)
        if (flat == rows[0, 0]).sum() == 1 and (flat == rows[MID_TERM, 0]).sum() == 1:
            return seed
    raise AssertionError("no source text with two rows of its own: " + name)


def _random_bits(rng, shape):
    """uint8 bits of density 1 - (3/4)(15/16) = 0.297, from whole random bytes (a 2^21-row matrix in milliseconds)"""
    b = [rng.integers(0, 256, size=shape, dtype=np.uint8) for _ in range(6)]
    return (b[0] & b[1]) | (b[2] & b[3] & b[4] & b[5])


class Index:
    """one fixture index: its file, its FileBits twin, its source text and the slots of its special documents"""

    def __init__(self, name, directory):
        from oracle import construct as C
        from oracle import oracle as O
        from tests import cases
        from tests import findere_check as F
        spec = SPECS[name]
        self.spec, self.name, self.k, self.num_docs, self.num_hashes = spec, name, spec.k, spec.num_docs, spec.num_hashes
        self.src = O.random_sequence(spec.tmax + spec.k - 1 + FINDERE_Z, seed_of(name))
        D = spec.num_docs
        per = 8 * spec.page_size if spec.kind == "compact" else 8 * ((D + 7) // 8)
        base = spec.near_page * per
        self.full = sorted(set([s for s in FULL_SLOTS if s < D] + [D - 1]))
        self.empty, self.near0, self.near_mid = base + 1, base + 2, base + 3
        assert not {self.empty, self.near0, self.near_mid} & set(self.full) and self.near_mid < D
        rng = np.random.default_rng(seed_of(name))
        rows = _rows_of(spec, self.src[:MID_TERM + spec.k], spec.sigs[spec.near_page])
        mats = []
        for p, sig in enumerate(spec.sigs):
            width = per // 8
            # (a filter of a few rows makes a random document full or empty: no random documents there)
            m = _random_bits(rng, (sig, width)) if sig >= 64 else np.zeros((sig, width), dtype=np.uint8)
            if not spec.mask:
                m[:, (D - p * per) // 8] |= np.uint8(0xFF & ~((1 << (D - p * per) % 8) - 1))     # padding slots: all ones
            for slot in self.full + [self.near0, self.near_mid]:
                if p * per <= slot < (p + 1) * per:
                    m[:, (slot - p * per) // 8] |= np.uint8(1 << (slot % 8))
            if p == spec.near_page:
                m[:, (self.empty - base) // 8] &= np.uint8(0xFF ^ (1 << (self.empty % 8)))
                m[rows[0, 0], (self.near0 - base) // 8] &= np.uint8(0xFF ^ (1 << (self.near0 % 8)))
                m[rows[MID_TERM, 0], (self.near_mid - base) // 8] &= np.uint8(0xFF ^ (1 << (self.near_mid % 8)))
            if spec.mask:
                m = cases.mask_padding_docs(m, p * per, D)
            mats.append(m)
        names = ["doc_%05d" % i for i in range(D)]
        self.path = os.path.join(str(directory), "%s.cobs_%s" % (name, spec.kind))
        if spec.kind == "classic":
            C.write_classic(self.path, spec.k, 1, names, spec.sigs[0], spec.num_hashes, mats[0])
        else:
            C.write_compact(self.path, spec.k, 1, spec.page_size, [(s, spec.num_hashes) for s in spec.sigs], names, mats)
        self.fb = F.FileBits(spec.k, 1, spec.num_hashes, mats, D)
        self.slots = self.fb.slots

    def query(self, T):
        """the query of T terms (T - z positions under findere z)"""
        assert T <= self.spec.tmax + FINDERE_Z
        return self.src[:T + self.k - 1]

    def padding_has_bits(self):
        """some padding slot holds every row (the fixture that leaves them unmasked)"""
        pad = self.fb.doc_of_slot() < 0
        cols = np.concatenate([np.unpackbits(m, axis=1, bitorder="little").all(axis=0) for m in self.fb.mats])
        return bool((cols & pad).any())


def build(directory, names):
    return {n: Index(n, directory) for n in names}


# ---- what the special documents have to reach -------------------------------------------------------------------------------
def lost(m, P, z):
    """the positions of [0, P) whose terms p .. p + z include term m"""
    return len(range(max(0, m - z), min(m, P - 1) + 1))


def plain_special(ix, T, z=0):
    """{slot: score} of the special documents for the T-term query: the full ones T - z, the near-full ones less the
    positions that need their missing term"""
    P = T - z
    out = {s: P for s in ix.full}
    out[ix.empty] = 0
    out[ix.near0] = P - lost(0, P, z)
    out[ix.near_mid] = P - lost(MID_TERM, P, z)
    return out


def coverage_special(ix, L, z=0):
    """a near-full document loses position 0 and with it base 0; the bases of positions 30 - z .. 30 stay covered by their
    neighbours (span = k + z > z + 1)"""
    return {**{s: L for s in ix.full}, ix.empty: 0, ix.near0: L - 1, ix.near_mid: L}


def window_special(ix, W, n):
    """best window at z = 0: a missing term m costs one where it lies in every window, n - w <= m <= w - 1"""
    w = min(W, n)

    def near(m):
        return w - 1 if (m < n and n - w <= m <= w - 1) else w

    return {**{s: w for s in ix.full}, ix.empty: 0, ix.near0: near(0), ix.near_mid: near(MID_TERM)}


def hits_of(special, bound, limit=0):
    """[(0, doc, key)] of the special documents reaching the bound, key descending, then document ascending"""
    out = sorted(((0, d, v) for d, v in special.items() if v >= bound), key=lambda h: (-h[2], h[1]))
    return out[:limit] if limit else out


def hits_of_row(row, docs, bound, limit=0):
    """the same list from a whole score row (every document of the file)"""
    row = np.asarray(row).astype(np.int64)
    slots = np.nonzero((docs >= 0) & (row >= bound))[0]
    order = np.lexsort((docs[slots], -row[slots]))
    out = [(0, int(docs[s]), int(row[s])) for s in slots[order]]
    return out[:limit] if limit else out


def thresholds(P):
    """(1.0, t_near): the bounds P and P - 1"""
    from tests import threshold_edges as E
    t = E.on_and_above(P - 1, P)[0]
    assert E.bound(1.0, P) == P and E.bound(t, P) == P - 1
    return 1.0, t


def mixed_batch(ix, T):
    """the T-term query among short ones: the batch gets the planes of the longest (a 15-term query counted in 12)"""
    return [ix.query(15), ix.query(T), ix.query(100), ix.query(16)]


# ---- the weighted fixture ---------------------------------------------------------------------------------------------------
def weighted_file(directory):
    """40 000 documents, all zeros but one all-ones column: every position is held by one document and weighs 15"""
    from oracle import construct as C
    from tests import findere_check as F
    m = np.zeros((WEIGHTED_SIG, WEIGHTED_DOCS // 8), dtype=np.uint8)
    m[:, WEIGHTED_FULL // 8] = np.uint8(1 << (WEIGHTED_FULL % 8))
    path = os.path.join(str(directory), "weighted.cobs_classic")
    C.write_classic(path, K, 1, ["doc_%05d" % i for i in range(WEIGHTED_DOCS)], WEIGHTED_SIG, 1, m)
    return path, F.FileBits(K, 1, 1, [m], WEIGHTED_DOCS)


def weighted_query(n, z):
    from oracle import oracle as O
    return O.random_sequence(n + z + K - 1, 600 + n)


def weighted_expected(n, t):
    """(total weight, hits): the full document scores 15 n, nobody else anything"""
    from tests import threshold_edges as E
    total = 15 * n
    if not t > 0:
        rest = [(0, d, 0) for d in range(WEIGHTED_DOCS) if d != WEIGHTED_FULL]
        return total, [(0, WEIGHTED_FULL, total)] + rest
    assert E.bound(t, total, True) <= total
    return total, [(0, WEIGHTED_FULL, total)]


# ---- groups, best-of-group, sets: documents that every member / every position reaches ------------------------------------
def group_queries(ix, members):
    """`members` queries of GROUP_TERMS terms each, cut from the source one character apart"""
    return [ix.src[i:i + GROUP_TERMS + ix.k - 1] for i in range(members)]
