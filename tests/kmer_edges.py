"""Adversarial k-mers for canonicalize_kmer (reference cobs/util/query.cpp:143-199) -- test infrastructure.

The rule: among the first k // 2 positions, the first strict difference between the forward base
kmer[s] and the complement of the mirrored base kmer[k - 1 - s] decides (forward smaller: the k-mer
as it is; forward larger: its reverse complement); the middle base of an odd k is never compared; no
difference keeps the forward k-mer.  On a random k-mer position s decides with probability
(3/4) * 4^-s, so random sequences never reach the deep positions or the tie.  This module builds,
with plain Python (no GPU, no oracle), k-mers whose deciding position and outcome are chosen:

  a random left half L, the right half = the mirrored complement of L (a tie), every base in the
  middle (odd k), and ONE mirror base k - 1 - s changed so that position s is the first difference.

Labels are (s, outcome): outcome "fwd" (forward kept), "rc" (reverse complement taken) or, with
s = None, "tie".
"""
import random

BASES = b"ACGT"
_COMP = bytes.maketrans(b"ACGT", b"TGCA")

# (halves mirror each other, middle base G): the reverse complement is the smaller string and the
# reference still keeps the forward 31-mer
TIE31_FORWARD_IS_LARGER = b"CGGTGCTAGCTCGTGGCACGAGCTAGCACCG"


def revcomp(kmer):
    return bytes(kmer).translate(_COMP)[::-1]


def decide(kmer):
    """(s, outcome) by the rule above for a k-mer over ACGT"""
    k = len(kmer)
    for s in range(k // 2):
        f, r = kmer[s], _COMP[kmer[k - 1 - s]]
        if f != r:
            return (s, "fwd" if f < r else "rc")
    return (None, "tie")


def canonical(kmer):
    return revcomp(kmer) if decide(kmer)[1] == "rc" else bytes(kmer)


def _left(rnd, n):
    return bytes(rnd.choice(BASES) for _ in range(n))


def _tie(rnd, k, mid):
    left = _left(rnd, k // 2)
    return left + (bytes([mid]) if k % 2 else b"") + revcomp(left)


def edge_kmers(k, seed, copies=1):
    """-> list of (label, kmer): for every deciding position s < k // 2 both outcomes, and the full tie, each with every
    base in the middle position (odd k); every k-mer from a fresh random left half (two odd-k ties that share their
    halves would be each other's "other orientation": the reverse complement of a tie with middle base G is the tie
    with middle base C).  Then the hand-picked ones (homopolymers; A^h X T^h; the 31-mer above) under their own labels.
    For even k a tie is a reverse palindrome: the k-mer equals its reverse complement.  copies: that many k-mers per
    (label, middle base), each from its own left half."""
    rnd = random.Random(seed * 1000003 + k)
    mids = (BASES if k % 2 else b"A") * copies
    out = []
    for s in range(k // 2):
        for outcome in ("fwd", "rc"):
            for mid in mids:
                t = bytearray(_tie(rnd, k, mid))
                f = t[s]
                # the complement of the changed mirror base must be larger (fwd) / smaller (rc) than the forward base
                if outcome == "fwd" and f == ord("T"):
                    f = t[s] = rnd.choice(b"ACG")
                if outcome == "rc" and f == ord("A"):
                    f = t[s] = rnd.choice(b"CGT")
                pool = [c for c in BASES if (c > f if outcome == "fwd" else c < f)]
                t[k - 1 - s] = _COMP[rnd.choice(pool)]
                out.append(((s, outcome), bytes(t)))
    for mid in mids:
        out.append(((None, "tie"), _tie(rnd, k, mid)))
    hand = [bytes([b]) * k for b in BASES]
    if k % 2:
        hand += [b"A" * (k // 2) + bytes([x]) + b"T" * (k // 2) for x in BASES]
    else:
        hand += [b"A" * (k // 2) + b"T" * (k // 2)]
    if k == 31:
        hand.append(TIE31_FORWARD_IS_LARGER)
    out += [(decide(h), h) for h in hand]
    return out


def edge_kmers_invalid(k, seed):
    """-> list of (tag, kmer): the k-mers of edge_kmers(k, seed) with ONE byte replaced by 'N', by a lower-case base
    and by 'X', at the deciding position s, at its mirror, at the middle, and at a position behind the deciding one.
    (The reference maps such a byte to 0 and still compares it; construction hashes the mapped buffer.)  For a tie the
    positions are 0, its mirror, the middle and 1.  One junk byte per position, cycling N / lower case / X, and all
    three at the deciding position."""
    rnd = random.Random(seed * 7919 + k)
    out = []
    for n, ((s, outcome), kmer) in enumerate(edge_kmers(k, seed)):
        s0 = 0 if s is None else s
        where = [("at", s0), ("mirror", k - 1 - s0), ("middle", k // 2), ("behind", min(s0 + 1, k - 1))]
        for w, (name, pos) in enumerate(where):
            junks = [b"N"[0], bytes([kmer[pos]]).lower()[0], b"X"[0]]
            pick = junks if name == "at" else [junks[(n + w) % 3]]
            for j in pick:
                t = bytearray(kmer)
                t[pos] = j
                out.append(((s, outcome, name, chr(j)), bytes(t)))
    rnd.shuffle(out)
    return out


def witness_kmers(k, seed):
    """the valid edge k-mers for a witness index, in a fixed order: duplicates removed (hand-picked ones may repeat a
    generated one for tiny k), two k-mers per label and middle base (one row of a witness may collide with a row of
    another by chance: hash % S; a label keeps a clean witness all the same), and of two k-mers that are each other's reverse complement only the later one (the
    "other orientation" of A^h A T^h is A^h T T^h, canonical in its own right: both in one index would make each other
    unclean by construction).  -> list of (label, kmer)"""
    items = edge_kmers(k, seed, copies=2)
    last = {kmer: n for n, (_, kmer) in enumerate(items)}
    out = []
    for n, (label, kmer) in enumerate(items):
        rc = revcomp(kmer)
        if last[kmer] == n and not (rc != kmer and last.get(rc, -1) > n):
            out.append((label, kmer))
    return out
