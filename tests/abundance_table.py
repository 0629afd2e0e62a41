"""The counting table of the min_count builder (cobs_amd/csrc/abundance_kernels.hip) restated in plain
Python -- TEST INFRASTRUCTURE ONLY; it shares no code with the library.

The key of an occurrence is (document, canonical bytes):
    h    = mix64(XXH64(canonical bytes, seed 0x5851F42D4C957F2D) ^ document * 0x9E3779B97F4A7C15)
    tag  = h >> 40                  (24 bits, stored in the owner word above the 40-bit offset)
    home = h & (cap - 1)            (linear probing from there, wrapping at cap)
mix64 is the splitmix64 finaliser (it adds the golden ratio first), the canonical bytes are
abundance_check.canonical_bytes, XXH64 is the oracle's (pinned against published vectors in
test_oracle_pins.py).

`document` is the document's COLUMN in the matrix being built (build.cpp: build_into stages
docs[b0, b1) and stage_batch gives document docs[i] the column i, counted from the first document of
the matrix, not of the batch -- the kernels subtract col_base only to find a byte-map plane).  A
classic index is one matrix in list order; a compact index is one matrix per group of 8 * page_size
documents, columns restarting at 0, documents in path order inside a group.

`total` of a batch is the sum of the text BOUNDS of its documents, not of the bytes they use: an
in-memory document of L bytes (sequences joined by '\\n') is bounded by L + 1 (it is staged with a
closing '\\n'), a FASTA / FASTQ file by its size + 1.  A batch takes documents while the sum of bounds
stays <= text_batch_bytes (at least one); document i of the batch begins at the sum of the bounds
before it.  cap = the power of two >= max(1024, 2 * total).

The constants below come from tests/tools/abundance_collide.cpp (a CPU search, not part of the suite);
tests/test_abundance_table_cpu.py re-derives every property they claim from this restatement, and the
GPU tests read the device's table back, so a wrong restatement fails instead of testing nothing.
"""
import collections

import numpy as np

from tests import abundance_check as A

KEY_SEED = 0x5851F42D4C957F2D
PHI = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
OFFSET_BITS = 40
OFFSET_MASK = (1 << OFFSET_BITS) - 1
MIN_CAP = 1024
DEFAULT_TEXT_BATCH = 256 << 20

# ---- adversarial keys: every pair shares the 24-bit tag AND the home slot at cap 1024 (34 bits) ----
# P1: two valid 31-mers of one document, canonicalize = 1 (register path)
P1 = (b"AGTCAATCTGGATGCTACGATTTGATTCTCC", b"AATGTAGAACCGACGTGAAATCCCGTCAGCG")
# P2: the same with canonicalize = 0
P2 = (b"AATGGTCGTAGGTTGCCGCAGCCAAGCGGAA", b"ATCCTGGAAATAAGTGTATGTACTAATTCTA")
# P3: a valid 31-mer (register path) and one that holds an N (byte view), canonicalize = 1
P3 = (b"AGGTCCAGTAATTCCACGGTAAGTTAACGAT", b"AATACACCACTGGGTAATCCANCCTTCAGTA")
# P4: two 31-mers that both hold an invalid character and differ after its mapping to 0, canonicalize = 1
P4 = (b"GGAXTCGCTTCCTGGAAAATTCTGCGTCACG", b"CGCGTCATTNACTTGATAAGCGAGCAACTGA")
# P5, P6: k = 20 and k = 40; both k-mers are their own canonical form, so the pair holds with canonicalize = 0 and 1
P5 = (b"CGAAAAATTTTCTCCCATTA", b"AGCAGACTTAGAGCACGCCC")
P6 = (b"CACTCAAGGGGCTAAGCGCTACGGAGGGATCCGCAGGTGA", b"AGTATCCGTTCCGAGTATAGGTTAGTAACACATGGATAGG")
# P7: ONE 31-mer (its own canonical form) whose keys in the documents of columns 3 and 4 collide
P7 = (b"GCTAGGTCTGCGTATCGCGGATTGAAGTATA", 3, 4)
# (name, pair, k, the canonicalize values under which the pair collides); all in document 0
PAIRS = [("P1", P1, 31, (1,)), ("P2", P2, 31, (0,)), ("P3", P3, 31, (1,)), ("P4", P4, 31, (1,)),
         ("P5", P5, 20, (1, 0)), ("P6", P6, 40, (1, 0))]
# keys needed by their home slot only: 31-mers of document 0 (their own canonical form) by home slot at cap 1024
HOME_1024 = {
    1020: (b"GGTGACACCGACAGATGTCCGCGGATGCCTA", b"ATCGGTATAACCGGCCGACGGTGGCGTGCTG", b"AAAAGCTACGCTTTACCCACTCCCTTTGAGG", b"GCCCCACACTACAACGCTAGTTAAGCGGTAA"),
    1021: (b"ATAACGTAGTCCTGGAATTCACTTCCCACTA", b"CCTGCTAACCCTGGTTAAGTCTCGGTCTGAC", b"ACGATGGAGAAGGGCCCTCTCATTATGTGCA", b"TAACGTCCATTCTTAGTGCTAATACCTAGGA"),
    1022: (b"ACTCTCATTAACGTCTCATGGTCCGTTCCCT", b"CCATCGTAACCTCACCGAGCAAGGCTTACAG", b"ATGAGATGTTTGTGGTAACTCCTAAATCTGG", b"CATCCGGCTTCTCCCTAATGATCAAGTGCAC"),
    1023: (b"AGCTGCAGCCTAAGTTGTCCCCTTGTAGTTC", b"AGTTCAGATGACTGATAACGAAGTAGTCCCC", b"GTAACACGACCTCTGAACTCTCTGAATAGAC", b"AACGCCCTCGGGGCAGCAAGACGTACCTCCA"),
}

_RC = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A")}


def revcomp(s):
    """the reverse strand as TEXT: an invalid character stays what it is (it maps to 0 on either strand)"""
    return bytes(_RC.get(c, c) for c in reversed(s))


_xxh = None


def xxh64(data, seed):
    global _xxh
    if _xxh is None:
        from oracle import oracle as O
        O.build()
        _xxh = O.xxh64
    return _xxh(bytes(data), seed)


def mix64(z):
    z = (z + PHI) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key_hash(key_bytes, doc):
    return mix64(xxh64(key_bytes, KEY_SEED) ^ ((doc * PHI) & M64))


def tag_of(h):
    return h >> OFFSET_BITS


def home_of(h, cap):
    return h & (cap - 1)


def capacity(total):
    cap = MIN_CAP
    while cap < 2 * total:
        cap <<= 1
    return cap


# ---- staging: which documents share a batch, and where their text lies -----------------------------

Batch = collections.namedtuple("Batch", "docs total")      # docs: [(column, begin, staged text)]


def stage(docs, text_batch=0):
    """docs in column order, each (sequences, bound or None) -> the batches stage_batch forms"""
    limit = text_batch or DEFAULT_TEXT_BATCH
    out, cur, total = [], [], 0
    for col, (seqs, bound) in enumerate(docs):
        joined = b"\n".join(seqs)
        bound = len(joined) + 1 if bound is None else bound
        text = joined + b"\n"
        assert len(text) <= bound
        if cur and total + bound > limit:
            out.append(Batch(cur, total))
            cur, total = [], 0
        cur.append((col, total, text))
        total += bound
    out.append(Batch(cur, total))
    return out


def occurrences(batch, k, canonicalize):
    """-> [(batch offset, column, canonical bytes)] of the term positions of a staged batch"""
    occ = []
    for col, begin, text in batch.docs:
        for i in range(len(text) - k + 1):
            w = text[i:i + k]
            if b"\n" not in w:
                occ.append((begin + i, col, A.canonical_bytes(w, canonicalize)))
    return occ


def probe_insert(occupied, home, cap):
    """the slot a key with this home takes in a table with these occupied slots"""
    s = home
    while s in occupied:
        s = (s + 1) & (cap - 1)
    return s


def clusters_of(occupied, cap):
    """maximal cyclic runs of occupied slots -> {slot: first slot of its run}"""
    start = {}
    for s in sorted(occupied):
        if s in start:
            continue
        b = s
        while ((b - 1) & (cap - 1)) in occupied and ((b - 1) & (cap - 1)) != s:
            b = (b - 1) & (cap - 1)
        t = b
        while t in occupied and t not in start:
            start[t] = b
            t = (t + 1) & (cap - 1)
    return start


class Model:
    """the linear-probing model of one staged batch: what does NOT depend on the insertion order"""

    def __init__(self, batch, k, canonicalize):
        self.k, self.canonicalize = k, canonicalize
        self.total = batch.total
        self.cap = capacity(batch.total)
        self.offsets = collections.OrderedDict()       # key (column, canonical bytes) -> offsets of its occurrences
        self.at_offset = {}                            # batch offset -> key
        for off, col, kb in occurrences(batch, k, canonicalize):
            self.offsets.setdefault((col, kb), []).append(off)
            self.at_offset[off] = (col, kb)
        self.hash = {key: key_hash(key[1], key[0]) for key in self.offsets}
        self.tag = {key: tag_of(h) for key, h in self.hash.items()}
        self.home = {key: home_of(h, self.cap) for key, h in self.hash.items()}
        self.occupied = set()
        for key in self.offsets:
            self.occupied.add(probe_insert(self.occupied, self.home[key], self.cap))
        self.cluster = clusters_of(self.occupied, self.cap)
        self.cluster_tags = collections.defaultdict(list)      # first slot of a cluster -> sorted tags of its keys
        for key in self.offsets:
            self.cluster_tags[self.cluster[self.home[key]]].append(self.tag[key])
        for v in self.cluster_tags.values():
            v.sort()

    def multiplicity(self, key):
        return len(self.offsets.get(key, ()))

    def kept(self, c):
        return {key for key, offs in self.offsets.items() if len(offs) >= max(c, 1)}

    def key(self, column, term):
        return (column, A.canonical_bytes(term, self.canonicalize))


def brute_force(model, order):
    """insert the model's keys one by one in this order -> {slot: key}"""
    slots = {}
    for key in order:
        slots[probe_insert(slots, model.home[key], model.cap)] = key
    return slots


def check_table(model, table, c):
    """what a table read back from the device (slots, text bytes, owner words, count words) must satisfy"""
    assert table is not None, "no table to read back"
    cap, total, owner, count = table
    assert (cap, total) == (model.cap, model.total)
    assert len(owner) == cap and len(count) == cap
    occupied = set(int(s) for s in np.nonzero(owner)[0])
    assert occupied == model.occupied, (sorted(occupied ^ model.occupied)[:8], len(occupied), len(model.occupied))
    assert 2 * len(occupied) <= cap
    assert not count[owner == 0].any()
    seen, tags = {}, collections.defaultdict(list)
    for slot in sorted(occupied):
        v = int(owner[slot])
        key = model.at_offset.get((v & OFFSET_MASK) - 1)
        assert key is not None, ("owner offset is no occurrence", slot, hex(v))
        assert model.tag[key] == v >> OFFSET_BITS, ("owner tag is not its key's", slot, hex(v))
        assert key not in seen, ("one key owns two slots", slot, seen[key])
        seen[key] = slot
        s = model.home[key]                            # every slot from the key's home to its own is taken
        while s != slot:
            assert s in occupied, ("a free slot between a key's home and its slot", slot)
            s = (s + 1) & (cap - 1)
        tags[model.cluster[slot]].append(v >> OFFSET_BITS)
        m, n = model.multiplicity(key), int(count[slot])
        if m < c:
            assert n == m, ("count below the cutoff is not exact", slot, n, m)
        else:
            assert c <= n <= m, ("saturated count out of range", slot, n, m, c)
    assert set(seen) == set(model.offsets)
    assert {b: sorted(t) for b, t in tags.items()} == dict(model.cluster_tags)
    return seen


# ---- fixtures: known keys on every path of the count kernel ------------------------------------------

# name, k, canonicalize, c, docs [(name, sequences)], text_batch_bytes, keep / drop [(column, term)], cap of the LAST batch
Fixture = collections.namedtuple("Fixture", "name k canonicalize c docs batch keep drop cap")


def _copies(term, m, canonicalize):
    """m copies, each a sequence of its own; with canonicalize = 1 every other one on the reverse strand"""
    return [revcomp(term) if (canonicalize and j % 2) else term for j in range(m)]


def _rand(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def pair_fixtures():
    """P1 .. P6: x c - 1 times and y once -> neither kept; x c times and y c - 1 times -> only x kept"""
    out, c = [], 3
    for name, (x, y), k, canons in PAIRS:
        for canon in canons:
            for case, mx, my in (("below", c - 1, 1), ("at", c, c - 1)):
                for first in (0, 1):                    # either key's first occurrence comes first in the text
                    seqs = _copies(x, mx, canon) + _copies(y, my, canon)
                    if first:
                        seqs = seqs[::-1]
                    keep = [(0, x)] if mx >= c else []
                    drop = [(0, y)] + ([] if mx >= c else [(0, x)])
                    out.append(Fixture("%s-canon%d-%s-%d" % (name, canon, case, first), k, canon, c,
                                       [("doc_0000", seqs)], 512, keep, drop, 1024))
    return out


def p7_fixtures():
    """the same 31-mer in the documents of columns 3 and 4 of one batch"""
    x, a, b = P7
    out, c = [], 2
    rng = np.random.default_rng(77)
    fill = [_rand(rng, 31) for _ in range(3)]
    for canon in (1, 0):
        for case, ma, mb in (("once-each", 1, 1), ("twice-in-a", 2, 1), ("twice-in-b", 1, 2)):
            docs = [("doc_%04d" % d, [fill[d]]) for d in range(a)]
            docs.append(("doc_%04d" % a, [x] * ma))
            docs.append(("doc_%04d" % b, [x] * mb))
            keep = [(col, x) for col, m in ((a, ma), (b, mb)) if m >= c]
            drop = [(col, x) for col, m in ((a, ma), (b, mb)) if m < c] + [(d, fill[d]) for d in range(a)]
            out.append(Fixture("P7-canon%d-%s" % (canon, case), 31, canon, c, docs, 512, keep, drop, 1024))
    return out


def wrap_fixtures():
    """fillers with homes 1020 .. 1022 once each and FOUR terms with home 1023, each repeated to c: at most one of
    them can own slot 1023, so at least three kept terms land in slot 0 or later whatever the order of the claims"""
    out = []
    for canon in (1, 0):
        for c in (2, 3):
            seqs, keep, drop = [], [], []
            for home in (1020, 1021, 1022):
                seqs.append(HOME_1024[home][0])
                drop.append((0, HOME_1024[home][0]))
            for j, t in enumerate(HOME_1024[1023]):
                m = c if j < 3 or c == 2 else c - 1      # at c = 3 the fourth one stays one short (a dropped term that wraps)
                seqs += _copies(t, m, canon)
                (keep if m >= c else drop).append((0, t))
            out.append(Fixture("wrap-canon%d-c%d" % (canon, c), 31, canon, c, [("doc_0000", seqs)], 512, keep, drop, 1024))
    return out


def boundary_fixtures():
    """multiplicities c - 1, c and c + 1 of three terms of one document, every copy a sequence of its own"""
    out = []
    rng = np.random.default_rng(5)
    terms = [_rand(rng, 31) for _ in range(3)]
    for c in (2, 255, 256, 300):
        for canon in (1, 0):
            seqs = []
            for t, m in zip(terms, (c - 1, c, c + 1)):
                seqs += _copies(t, m, canon)
            order = np.random.default_rng(c).permutation(len(seqs))
            seqs = [seqs[i] for i in order]
            cap = capacity(32 * len(seqs))
            out.append(Fixture("boundary-c%d-canon%d" % (c, canon), 31, canon, c, [("doc_0000", seqs)], 0,
                               [(0, terms[1]), (0, terms[2])], [(0, terms[0])], cap))
    return out


def hot_fixtures():
    """thousands of threads on one slot: a homopolymer is 4970 occurrences of one key, A and T runs counted
    together under canonicalize = 1 are 5940"""
    a, t = b"A" * 31, b"T" * 31
    out = []
    for name, canon, seqs, term, m in (("A5000", 1, [b"A" * 5000], a, 4970), ("A5000", 0, [b"A" * 5000], a, 4970),
                                       ("T5000", 0, [b"T" * 5000], t, 4970),
                                       ("A3000+T3000", 1, [b"A" * 3000, b"T" * 3000], a, 5940)):
        for c in (2, 4970, 4971) + ((5940, 5941) if m == 5940 else ()):
            keep, drop = ([(0, term)], []) if m >= c else ([], [(0, term)])
            total = len(b"\n".join(seqs)) + 1
            out.append(Fixture("hot-%s-canon%d-c%d" % (name, canon, c), 31, canon, c, [("doc_0000", seqs)], 0,
                               keep, drop, capacity(total)))
    return out


def capacity_fixtures():
    """batches of exactly 512 / 513 and 1024 / 1025 text bytes (the table doubles in between), and the smallest
    batch there is: one document of exactly k bytes"""
    out = []
    for total, cap in ((512, 1024), (513, 2048), (1024, 2048), (1025, 4096)):
        rng = np.random.default_rng(total)
        seg = _rand(rng, 45)
        text = seg + _rand(rng, total - 1 - 2 * len(seg) - 1) + b"G" + seg       # the first 15 terms occur twice
        assert len(text) + 1 == total
        keep = [(0, seg[i:i + 31]) for i in range(15)]
        out.append(Fixture("capacity-%d" % total, 31, 1, 2, [("doc_0000", [text])], 0, keep, [(0, text[50:81])], cap))
    for k in (20, 31, 40):
        term = _rand(np.random.default_rng(k), k)
        out.append(Fixture("smallest-k%d" % k, k, 1, 2, [("doc_0000", [term])], 0, [], [(0, term)], 1024))
    return out


def all_fixtures():
    return pair_fixtures() + p7_fixtures() + wrap_fixtures() + boundary_fixtures() + hot_fixtures() + capacity_fixtures()


def last_batch_model(fx, bounds=None):
    """the model of the batch whose table stays behind after the fixture's build"""
    docs = [(seqs, bounds[i] if bounds else None) for i, (_, seqs) in enumerate(fx.docs)]
    return Model(stage(docs, fx.batch)[-1], fx.k, fx.canonicalize)
