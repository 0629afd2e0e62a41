"""canonicalize_kmer and hash % S at their edges, without a device: the adversarial k-mer set (tests/kmer_edges.py)
against the oracle and a second restatement, the host copy of the rule in cobs_gpu_query (print-kmers, doc-dump), and
the arithmetic of the kernels' fast_mod.  tests/test_gpu_kmer_edges.py runs the same set through every device path."""
import collections
import os
import random
import subprocess

import pytest

from tests import kmer_edges as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")
KS = [3, 4, 5, 12, 20, 30, 31, 32, 33, 47, 63, 64, 65, 100, 131]
SEED = 20


def restate_canon(kmer):
    """canonicalize_kmer once more, as a comparison of two strings (util/query.cpp:143-199): bytes outside ACGT map to
    0 in both directions; the first k // 2 bytes of the mapped k-mer against the first k // 2 of its mapped reverse
    complement -- the reverse complement only when it is strictly smaller there.  -> (bytes, good)"""
    k = len(kmer)
    fwd = bytes(c if c in b"ACGT" else 0 for c in kmer)
    rc = bytes({65: 84, 67: 71, 71: 67, 84: 65}.get(c, 0) for c in reversed(kmer))
    out = rc if rc[:k // 2] < fwd[:k // 2] else fwd
    return out, 0 not in out


def test_labels_against_the_oracle_and_a_restatement(oracle):
    total = 0
    for k in KS:
        kmers = E.edge_kmers(k, SEED)
        seen = collections.Counter()
        for (s, outcome), kmer in kmers:
            assert len(kmer) == k and set(kmer) <= set(b"ACGT")
            want = E.revcomp(kmer) if outcome == "rc" else kmer
            assert oracle.canonicalize_kmer(kmer) == (want, True), (k, s, outcome, kmer)
            assert restate_canon(kmer) == (want, True), (k, s, outcome, kmer)
            assert E.decide(kmer) == (s, outcome) and E.canonical(kmer) == want
            # the label says where: the halves agree before s, differ at s (the restatement of the label itself)
            rc = E.revcomp(kmer)
            h = k // 2
            first = next((i for i in range(h) if kmer[i] != rc[i]), None)
            assert first == s and (outcome == "tie") == (first is None), (k, s, outcome, kmer)
            if outcome == "tie" and k % 2 == 0:
                assert kmer == rc                                    # a reverse palindrome
            seen[(s, outcome, chr(kmer[h]) if k % 2 else "")] += 1
        mids = "ACGT" if k % 2 else [""]
        for m in mids:                                               # every label with every middle base
            assert seen[(None, "tie", m)] >= 1, (k, m)
            for s in range(k // 2):
                assert seen[(s, "fwd", m)] >= 1 and seen[(s, "rc", m)] >= 1, (k, s, m)
        assert len(kmers) == (2 * (k // 2) + 1) * len(mids) + 4 + (4 if k % 2 else 1) + (k == 31)
        total += len(kmers)
    assert total == 1881
    # the 31-mer whose reverse complement is the smaller STRING and which the rule keeps forward: canonical != min()
    t = E.TIE31_FORWARD_IS_LARGER
    assert E.revcomp(t) < t and E.decide(t) == (None, "tie") and oracle.canonicalize_kmer(t) == (t, True)


def test_invalid_variants_against_the_oracle_and_a_restatement(oracle):
    for k in KS:
        inv = E.edge_kmers_invalid(k, SEED)
        places = collections.Counter()
        for (s, outcome, where, junk), kmer in inv:
            assert len(kmer) == k and sum(c not in b"ACGT" for c in kmer) == 1 and 0 not in kmer
            got = oracle.canonicalize_kmer(kmer)
            assert got == restate_canon(kmer) and got[1] is False and got[0].count(b"\0") == 1, (k, where, kmer)
            places[(where, "N" if junk == "N" else "X" if junk == "X" else "lower")] += 1
        for where in ("at", "mirror", "middle", "behind"):
            for junk in ("N", "X", "lower"):
                assert places[(where, junk)] >= 1, (k, where, junk)


# ---- the host copy of the rule: cobs_gpu_query print-kmers / doc-dump -----------------------------------------------

def _want_lines(oracle, terms):
    out = []
    for t in terms:
        canon, good = oracle.canonicalize_kmer(t)
        out.append(canon.decode("latin-1") if good else "Invalid DNA base pair: " + t.decode("latin-1"))
    return out


@pytest.mark.parametrize("k", [31, 20, 4, 65])
def test_host_tools_on_the_edge_set(oracle, tmp_path, k):
    """every edge k-mer, valid and invalid, through `print-kmers` (as windows of one long query: the k-mers themselves
    and every window across two of them) and `doc-dump` (one FASTA record per k-mer)"""
    assert os.path.exists(TOOL), "build cobs_amd/cobs_gpu_query first (make -C cobs_amd/csrc)"
    kmers = [t for _, t in E.edge_kmers(k, SEED)] + [t for _, t in E.edge_kmers_invalid(k, SEED)]
    assert any(E.decide(t)[1] == "tie" for t in kmers[:len(E.edge_kmers(k, SEED))])
    per_call = max(1, 40000 // k)
    for a in range(0, len(kmers), per_call):
        q = b"".join(kmers[a:a + per_call]) + b"A"                   # (print-kmers leaves out a query's last k-mer)
        r = subprocess.run([TOOL, "print-kmers", q.decode("latin-1"), "-k", str(k)], capture_output=True, text=True,
                           encoding="latin-1", timeout=120)
        assert r.returncode == 0, r.stderr
        got = r.stdout.splitlines()
        want = _want_lines(oracle, [q[i:i + k] for i in range(len(q) - k)])
        assert len(got) == len(want) == len(q) - k
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (k, a, i, q[i:i + k])
    d = tmp_path / "docs"
    d.mkdir()
    (d / "edges.fasta").write_bytes(b"".join(b">e%d\n%s\n" % (i, t) for i, t in enumerate(kmers)))
    r = subprocess.run([TOOL, "doc-dump", str(d), "-k", str(k)], capture_output=True, text=True, encoding="latin-1",
                       timeout=120)
    assert r.returncode == 0, r.stderr
    got, want = r.stdout.splitlines(), _want_lines(oracle, kmers)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, i, kmers[i])
    assert sum(ln.startswith("Invalid DNA base pair: ") for ln in got) == len(E.edge_kmers_invalid(k, SEED))
    r = subprocess.run([TOOL, "doc-dump", str(d), "-k", str(k), "--no-canonicalize"], capture_output=True, text=True,
                       encoding="latin-1", timeout=120)
    assert r.returncode == 0 and r.stdout.splitlines() == [t.decode("latin-1") for t in kmers]


# ---- fast_mod as arithmetic ---------------------------------------------------------------------------------------

M64 = (1 << 64) - 1


def fast_mod(n, d):
    """kernels.hip fast_mod with Python integers: m = floor((2^64 - 1) / d), q = hi64(n * m), r = n - q * d, then at
    most two conditional subtractions.  -> (r, subtractions the exact answer needs)"""
    m = M64 // d
    q = (n * m) >> 64
    r = n - q * d
    assert 0 <= r <= M64                                             # the kernel's r is a uint64: no wrap
    need = r // d
    if r >= d:
        r -= d
    if r >= d:
        r -= d
    return r, need


def divisors():
    ds = {1, 2, 3, (1 << 32) - 2, (1 << 32) - 1}
    for j in range(64):
        ds.update(x for x in ((1 << j) - 1, 1 << j, (1 << j) + 1) if 1 <= x <= M64)
    return sorted(ds)


def test_fast_mod_is_exact_with_two_subtractions():
    rnd = random.Random(64)
    worst = 0
    for d in divisors():
        ns = {0, d - 1, d, M64, M64 - 1, (M64 // d) * d, (M64 // d) * d - 1, min((M64 // d) * d + 1, M64)}
        for mult in (1, 2, 3, 7, rnd.randrange(1, M64 // d + 1), M64 // d, M64 // d // 2 + 1):
            ns.update(x for x in (mult * d - 1, mult * d, mult * d + 1) if 0 <= x <= M64)
        ns.update(rnd.getrandbits(64) for _ in range(200))
        ns.update(rnd.getrandbits(rnd.randrange(1, 65)) for _ in range(50))
        for n in ns:
            r, need = fast_mod(n, d)
            assert need <= 2 and r == n % d, (n, d, r, need)
            worst = max(worst, need)
    assert worst >= 1                                                # (d = 1: every n > 0 needs one)
