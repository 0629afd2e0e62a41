"""Score order on designed score distributions (test infrastructure): index files in which every document has a CHOSEN
score for each of several short queries, the radix plans of the selection (K3) and of the full ranking restated, the
profiles that put scores on the digit boundaries, tie splits and counts those plans turn on, and the contract both
stages have to meet, in numpy.  Nothing here loads the GPU library; the files are written with oracle/construct.py.

The plans, beside the source line each comes from:

  k3_plan(planes)    pass.cpp: ta.levels = (planes + 11) / 12, ta.level_bits = ceil(planes / levels);
                     topk_kernels.hip: lastbits = score_bits - (levels - 1) * level_bits
  rank_plan(planes)  rank.cpp: j.npasses = (planes + 11) / 12, j.pbits = ceil(planes / npasses)
  planes_for(T)      kernels.hip: scan_planes_for (tests/saturation.py restates it) -- of the LONGEST query of a batch: one
                     long filler query sends every short query of its batch through the 2- or 3-level code
  wave_per(n, r)     topk_kernels.hip / rank_kernels.hip: per = ceil(ceil(n / nranges) / 512) * 512 elements per wave

The fixture idea.  The background of an index is zero, and document d holds the rows of the first targets[q][d] CLEAN
terms of designed query q, so it scores exactly targets[q][d].  A term is clean in a sub-index when its row there belongs
to no other term of any designed query.  (Choosing the text so that ALL rows are pairwise distinct, as saturation.seed_of
does for two rows, is not possible here: profiles that reach the second digit of a 10-bit plan need about 3000 terms, and
that many random rows collide in any filter that a test can afford.  Rows that collide are left out of every document
instead: their terms score 0 everywhere, and every target is still met exactly.)  The designed queries are cut from
disjoint stretches of one source text.  A compact file leaves the padding slots of its last sub-index ALL ONES: a padding
document that leaks ranks first."""
import math
import os

import numpy as np

from tests import saturation

K = 31
SIG = 65521
SRC_SEED = 9091
CLEAN_SHARE = 0.55                       # the text of a designed query is cut this much longer than its largest target
FILLERS = {8: 255, 12: 4095, 16: 40000, 20: 70000, 24: 2 ** 20, 32: 2 ** 24 + 77}        # planes -> terms of the filler
SORT_LIMIT = 8192                        # engine.hpp: kTopkSortLimit
TILE_TOPK_MAX = 128                      # the largest k of the tile-level selection (test_gpu_topk_tiles.py)


def planes_for(T):
    return saturation.planes_for(T)


def k3_plan(planes):
    """-> (levels, level_bits, last_bits) of the K3 descent"""
    levels = (planes + 11) // 12
    level_bits = (planes + levels - 1) // levels
    return levels, level_bits, planes - (levels - 1) * level_bits


def rank_plan(planes):
    """-> (npasses, pbits) of the ranking's LSD radix sort"""
    npasses = (planes + 11) // 12
    return npasses, (planes + npasses - 1) // npasses


def wave_per(n, nranges=4):
    return ((n + nranges - 1) // nranges + 511) // 512 * 512


def digit_edges(planes):
    """the score bits at which a K3 level or a ranking pass ends, lowest first (empty for one level and one pass)"""
    levels, lb, last = k3_plan(planes)
    npasses, pb = rank_plan(planes)
    return sorted({last + i * lb for i in range(levels - 1)} | {pb * (i + 1) for i in range(npasses - 1)})


# ---- the profiles: (num_docs, b, ...) -> scores -----------------------------------------------------------------------------
def all_equal(n, s):
    """every document scores s: the order is pure document order, every tie split takes its ties in it"""
    return np.full(n, s, dtype=np.int64)


def low_wrap(n, b, ms=(1, 2)):
    """m 2^b - 1 and m 2^b, interleaved by document so that neither value is contiguous: the low digit is all ones against
    0 where the next digit differs by one -- a digit taken from the wrong bits orders these wrongly"""
    vals = np.array([v for m in ms for v in (m * 2 ** b - 1, m * 2 ** b)], dtype=np.int64)
    return vals[np.arange(n) % len(vals)]


def same_low_digit(n, b, v=None, steps=3):
    """v, v + 2^b, v + 2 2^b, interleaved (steps = 2: the first two): equal in the low digit, different in the next.  A
    descent that forgets the prefix it found counts them all in one bin of the low level; a later ranking pass that is not
    stable loses the document order of each value"""
    v = 2 ** b // 3 + 1 if v is None else v
    d = np.arange(n)
    return (v + ((d + d // 64) % steps) * 2 ** b).astype(np.int64)


def staircase_up(n, top):
    """scores rising with the document number up to `top` (distinct where top = n - 1): rank order is the REVERSE of
    document order"""
    return (np.arange(n, dtype=np.int64) * min(top, n - 1)) // (n - 1)


def staircase_down(n, top):
    """scores falling with the document number: rank order IS document order"""
    return staircase_up(n, top)[::-1].copy()


def sawtooth(n, m):
    """d mod m: every value is spread over every wave range, block and lane"""
    return np.arange(n, dtype=np.int64) % m


def tie_run_at_cut(n, k, where, c=5, per=None):
    """k - 1 documents above the score c, a run of documents AT c longer than two wave ranges, everybody else at c - 1.
    `where` places the documents above the cut and the run:
      "last"    above: the last k - 1 documents (the last wave's range); the run starts 20 documents before the first
                range edge: a top-k of k takes its tie from wave 0 alone, larger ones cross into wave 1 and 2
      "first"   above: the first k - 1 documents; the run is the END of the file: wave 0 has no tie
      "wave3"   above: the first k - 1 documents; a SHORT run of 100 documents that lies wholly in the last wave's range (a
                run longer than two ranges cannot): every tie comes from the last wave
      "spread"  above: every (n // k)-th document; the run as in "last": every wave holds documents on both sides
      "padding" above: spread; the ONLY document at c is the last real one (what follows it is padding), so the k-th
                result is the last document, and the (k + 1)-th the first of the c - 1 ties
    -> (scores, first document of the run, run length)"""
    per = per or wave_per(n)
    run = 2 * per + 70
    assert 2 <= k and c >= 2 and run + k + 40 < n
    s = np.full(n, c - 1, dtype=np.int64)
    r0 = per - 20 if where in ("last", "spread") else n - run if where == "first" else 3 * per + 10 if where == "wave3" else n - 1
    if where == "padding":
        run = 1
    if where == "wave3":
        run = 100
        assert 3 * per < r0 and r0 + run < n
    s[r0:r0 + run] = c
    if where == "last":
        above = np.arange(n - (k - 1), n)
    elif where in ("first", "wave3"):
        above = np.arange(k - 1)
    else:
        above = (np.arange(k - 1) * (n // k)) + 1
        above = above[above != n - 1] if where == "padding" else above
        if len(above) < k - 1:
            above = np.append(above, n - 3)
    s[above] = c + 1 + (above % 3)
    return s, r0, run


def exactly(n, k, c=40):
    """k - 1 documents at c + 1, one at c, one at c - 1 (spread over the file), everybody else below: the bounds c + 1, c
    and c - 1 let exactly k - 1, k and k + 1 documents pass -> (scores, (c + 1, c, c - 1))"""
    assert k + 1 <= n and c >= 3
    s = np.arange(n, dtype=np.int64) % (c - 1)
    pos = (np.arange(k + 1) * n) // (k + 1)
    s[pos[:k - 1]] = c + 1
    s[pos[k - 1]] = c
    s[pos[k]] = c - 1
    return s, (c + 1, c, c - 1)


def tie_ks(n_above, r0, run, n):
    """top-k sizes whose last tie lies on each side of an 8-slot, a 64-lane and a 512-block (= wave range) edge inside
    a contiguous tie run that starts at document r0 behind n_above better documents"""
    out = set()
    for unit in (8, 64, 512, 1024):
        e = (r0 // unit + 1) * unit
        if e < r0 + run:
            out |= {n_above + (e - r0), n_above + (e - r0) + 1}
    return sorted(k for k in out if 1 <= k <= n)


def edge_ks(n, per):
    """1, 2, both sides of every wave-range edge, n - 1, n, n + 1"""
    ks = {1, 2, n - 1, n, n + 1}
    for e in (per, 2 * per, 3 * per):
        if e + 1 < n:
            ks |= {e - 1, e, e + 1}
    return sorted(ks)


def profiles(n, b, cap, tie_k=40):
    """{name: scores} of one fixture: every profile, for the digit width b, scores up to cap"""
    mid = min(cap, 2 ** b + 1)
    out = {
        "all_equal_0": all_equal(n, 0),
        "all_equal_1": all_equal(n, 1),
        "all_equal_mid": all_equal(n, mid),
        "all_equal_top": all_equal(n, cap),
        "staircase_up": staircase_up(n, cap),
        "staircase_down": staircase_down(n, cap),
        "sawtooth_3": sawtooth(n, 3),
        "sawtooth_wide": sawtooth(n, min(2 ** b + 1, cap + 1)),
        "exactly": exactly(n, tie_k)[0],
    }
    if 2 ** (b + 1) <= cap:
        out["low_wrap"] = low_wrap(n, b, (1, 2))
    elif 2 ** b <= cap:
        out["low_wrap"] = low_wrap(n, b, (1,))
    if 2 ** b // 3 + 1 + 2 * 2 ** b <= cap:
        out["same_low_digit"] = same_low_digit(n, b)
    else:                                # (the 12-bit design: 40 and 40 + 4096)
        assert 40 + 2 ** b <= cap
        out["same_low_digit"] = same_low_digit(n, b, v=40, steps=2)
    for where in ("last", "first", "wave3", "spread", "padding"):
        out["tie_run_" + where] = tie_run_at_cut(n, tie_k, where, c=mid if where == "spread" else 5)[0]
    return out


# ---- the files --------------------------------------------------------------------------------------------------------------
class Design:
    """one index file with its designed queries: .path, .queries {name: text}, .targets {name: scores}, .num_docs"""


def _source(total):
    from oracle import oracle as O
    return O.random_sequence(total, SRC_SEED)


def build(path, kind, targets, num_docs, sigs, page_size=0, lengths=None):
    """writes the file -> Design.  targets: {name: scores[num_docs]}; lengths: {name: terms of the query} (by default the
    largest target over CLEAN_SHARE, at least 2 terms -- a query of one term is ranked in index order)"""
    from oracle import construct as C
    from oracle import oracle as O
    names = list(targets)
    lengths = dict(lengths or {})
    for nm in names:
        lengths.setdefault(nm, max(2, int(math.ceil(int(np.max(targets[nm])) / CLEAN_SHARE)) + 8))
    src = _source(sum(lengths[nm] + K - 1 for nm in names))
    queries, off = {}, 0
    for nm in names:
        queries[nm] = src[off:off + lengths[nm] + K - 1]
        off += lengths[nm] + K - 1
    hashes = {}
    for nm in names:
        h, good = O.term_hashes(queries[nm], K, 1, 1)
        assert good.all() and len(h) == lengths[nm]
        hashes[nm] = h[:, 0]
    per_page = 8 * page_size if kind == "compact" else 8 * ((num_docs + 7) // 8)
    assert (len(sigs) - 1) * per_page < num_docs <= len(sigs) * per_page
    mats, clean_rows = [], []
    for p, sig in enumerate(sigs):
        lo, hi = p * per_page, min((p + 1) * per_page, num_docs)
        m = np.zeros((sig, per_page // 8), dtype=np.uint8)
        rows = {nm: (hashes[nm] % np.uint64(sig)).astype(np.int64) for nm in names}
        uses = np.bincount(np.concatenate(list(rows.values())), minlength=sig)
        clean_rows.append({})
        for nm in names:
            clean = rows[nm][uses[rows[nm]] == 1]                  # in term order
            clean_rows[-1][nm] = clean
            t = np.asarray(targets[nm][lo:hi], dtype=np.int64)
            assert t.min() >= 0 and t.max() <= len(clean), ("not enough clean terms", nm, p, int(t.max()), len(clean))
            held = np.zeros((int(t.max()), per_page), dtype=bool)
            held[:, :hi - lo] = np.arange(int(t.max()))[:, None] < t[None, :]
            m[clean[:int(t.max())]] |= np.packbits(held, axis=1, bitorder="little")
        if kind == "compact" and hi - lo < per_page:
            pad = np.zeros(per_page, dtype=bool)
            pad[hi - lo:] = True
            m |= np.packbits(pad, bitorder="little")[None, :]      # padding slots: all ones
        mats.append(m)
    docs = ["doc_%05d" % i for i in range(num_docs)]
    if kind == "classic":
        C.write_classic(path, K, 1, docs, sigs[0], 1, mats[0])
    else:
        C.write_compact(path, K, 1, page_size, [(s, 1) for s in sigs], docs, mats)
    d = Design()
    d.path, d.kind, d.num_docs, d.queries, d.page_size = path, kind, num_docs, queries, page_size
    d.targets = {nm: np.asarray(targets[nm], dtype=np.int64) for nm in names}
    d.terms = lengths
    d.sigs, d.per_page, d.clean_rows = list(sigs), per_page, clean_rows
    return d


def design_scores(d, query):
    """the scores ANY query has over a designed file, from row multiplicities: document j holds the first targets[nm][j]
    clean rows of every designed query nm and nothing else, so it scores the sum of the multiplicities of those rows
    among the query's terms -- one bincount per sub-index, one prefix sum per designed query.  This is how the 2^20- and
    2^24 + 77-term fillers get their expected lists without minutes of oracle time"""
    from oracle import oracle as O
    hs, good = O.term_hashes(query, K, 1, 1)
    assert good.all()
    out = np.zeros(d.num_docs, dtype=np.int64)
    for p, sig in enumerate(d.sigs):
        lo, hi = p * d.per_page, min((p + 1) * d.per_page, d.num_docs)
        mult = np.bincount((hs[:, 0] % np.uint64(sig)).astype(np.int64), minlength=sig)
        for nm, clean in d.clean_rows[p].items():
            out[lo:hi] += np.concatenate([[0], np.cumsum(mult[clean])])[d.targets[nm][lo:hi]]
    return out


def pool_takes(k, tile_w, planes, row_slots, pages=None, page_size=None):
    """whether run_topk without rows selects per tile into the candidate pool, restated so that a test can say which path
    it means: setup of run_impl in pass.cpp -- k <= kTileTopkMax, and the pool (cand_stride = tiles x k entries rounded up to
    8, 8 bytes each) no larger than the score rows it replaces (local_counts x element bytes; kernels.hpp:
    scan_score_bytes); a tile is tile_w of the file's 16-byte column chunks (geometry.cpp, pass.cpp: cand_tiles).  A
    sub-index counted in row ranges is one tile (tile_w = 0 here)"""
    pages, page_size = pages or len(PAGED_SIGS), page_size or PAGED_PAGE
    tiles = (pages * ((page_size + 15) // 16) + tile_w - 1) // tile_w if tile_w else pages
    elem = 1 if planes <= 8 else 2 if planes <= 16 else 4
    return k <= TILE_TOPK_MAX and 8 * ((tiles * k + 7) // 8 * 8) <= row_slots * elem


SMALL_DOCS = 1797                        # four waves own 512 / 512 / 512 / 261 documents; the last byte is ragged
PAGED_PAGE, PAGED_SIGS = 40, [65521, 65537, 65539, 65543, 65551, 65557]
PAGED_DOCS = 5 * 8 * PAGED_PAGE + 200    # 1800: six sub-indexes of 320 slots, the last one holds 200 documents
WIDE_DOCS, WIDE_SIG = 8200, 8009
# the digit width a fixture is designed for and the largest score it holds -> the plans (planes) it runs under
# (32 planes: K3 levels end at the bits 10 and 21, ranking passes at 11 and 22; the 10-bit design has 1023 | 1024 and
# 2047 | 2048 in low_wrap and v, v + 1024, v + 2048 in same_low_digit: both low edges.  The high ones need `coarse`.)
WIDTHS = {4: (120, (8,)), 8: (2 * 256 + 100, (12, 16)), 10: (2 * 1024 + 400, (20, 32))}
WIDTH_24 = (12, 4096 + 60)               # 2 x 12 bits: only `small` runs it, in one test
SIG_24 = 131071                          # (its queries are four times as long: a filter twice as large keeps them clean)


def build_small(directory, b):
    cap, sig = (WIDTH_24[1], SIG_24) if b == WIDTH_24[0] else (WIDTHS[b][0], SIG)
    return build(os.path.join(str(directory), "small_b%d.cobs_classic" % b), "classic", profiles(SMALL_DOCS, b, cap),
                 SMALL_DOCS, [sig])


def build_paged(directory, b):
    return build(os.path.join(str(directory), "paged_b%d.cobs_compact" % b), "compact", profiles(PAGED_DOCS, b, WIDTHS[b][0]),
                 PAGED_DOCS, PAGED_SIGS, PAGED_PAGE)


def wide_targets():
    """`wide`, for the sort limit only: all_equal, staircase_up, and exactly(8192): 8191, 8192 or 8193 documents pass"""
    sc, bounds = exactly(WIDE_DOCS, SORT_LIMIT, c=40)
    return {"all_equal": all_equal(WIDE_DOCS, 7), "staircase_up": staircase_up(WIDE_DOCS, 200), "exactly": sc}, bounds


def build_wide(directory):
    return build(os.path.join(str(directory), "wide.cobs_classic"), "classic", wide_targets()[0], WIDE_DOCS, [WIDE_SIG])


def filler(planes):
    """the query that sets the plan of its batch"""
    from oracle import oracle as O
    return O.random_sequence(FILLERS[planes] + K - 1, 7000 + planes)


# ---- `coarse`: scores up to 2^24 from row multiplicities ------------------------------------------------------------------
COARSE_SIG, COARSE_DOCS = 1511, 1800


def coarse_heights():
    """h_d of every document: 64 distinct values between 0 and 1511, about 28 documents each, interleaved"""
    vals = np.unique(np.concatenate([[0, 1, 2, COARSE_SIG], np.linspace(3, COARSE_SIG - 1, 60).astype(np.int64)]))
    d = np.arange(COARSE_DOCS)
    return vals[(d * 37 + d // 64) % len(vals)]


def build_coarse(directory):
    """document d holds the rows [0, h_d): under a query whose row r is hit mult[r] times it scores sum(mult[:h_d])"""
    from oracle import construct as C
    h = coarse_heights()
    held = np.arange(COARSE_SIG)[:, None] < h[None, :]
    m = np.packbits(held, axis=1, bitorder="little")
    path = os.path.join(str(directory), "coarse.cobs_classic")
    C.write_classic(path, K, 1, ["doc_%05d" % i for i in range(COARSE_DOCS)], COARSE_SIG, 1, m)
    return path, h


def coarse_scores(query, heights):
    """one bincount of term_hashes % sig, then a prefix sum"""
    from oracle import oracle as O
    hs, good = O.term_hashes(query, K, 1, 1)
    assert good.all()
    mult = np.bincount((hs[:, 0] % np.uint64(COARSE_SIG)).astype(np.int64), minlength=COARSE_SIG)
    return np.concatenate([[0], np.cumsum(mult)])[heights].astype(np.int64)


# ---- the contract -----------------------------------------------------------------------------------------------------------
def expected(scores, bound=0, k=0, by_score=True, file_no=0):
    """[(file, document, score)]: keep score >= bound, stable sort by score descending over document order (a query with a
    single hash stays in index order), the first k (0: all).  Written independently of the oracle."""
    scores = np.asarray(scores, dtype=np.int64)
    docs = np.nonzero(scores >= bound)[0]
    if by_score:
        docs = docs[np.argsort(-scores[docs], kind="stable")]
    if k:
        docs = docs[:k]
    return [(file_no, int(d), int(scores[d])) for d in docs]


def threshold_for(c, P):
    """the largest double t with ceil(t * P) == c"""
    from tests import threshold_edges as E
    return E.on_and_above(c, P)[0]


def bound_of(t, P):
    from tests import threshold_edges as E
    return E.bound(t, P)
