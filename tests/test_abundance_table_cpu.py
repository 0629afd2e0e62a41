"""The restatement of the min_count builder's counting table (tests/abundance_table.py) checked on the CPU: the
committed adversarial keys have the properties they claim, the order-free model agrees with brute-force insertion in
any order, and the model alone tells every fixture's kept terms from its dropped ones."""
import numpy as np
import pytest

from tests import abundance_check as A
from tests import abundance_table as T


@pytest.fixture(scope="module", autouse=True)
def _oracle_is_built(oracle):
    yield


def test_key_hash_pins():
    """mix64 is the splitmix64 finaliser: its first outputs from state 0 are published"""
    assert T.mix64(0) == 0xE220A8397B1DCDAF
    assert T.mix64(T.PHI) == 0x6E789E6AA1B965F4
    assert T.capacity(0) == 1024 and T.capacity(512) == 1024 and T.capacity(513) == 2048
    assert T.capacity(1024) == 2048 and T.capacity(1025) == 4096


@pytest.mark.parametrize("name,pair,k,canons", T.PAIRS, ids=[p[0] for p in T.PAIRS])
def test_pairs_share_tag_and_home_slot(name, pair, k, canons):
    x, y = pair
    assert len(x) == k and len(y) == k
    for canon in canons:
        bx, by = A.canonical_bytes(x, canon), A.canonical_bytes(y, canon)
        assert bx != by
        hx, hy = T.key_hash(bx, 0), T.key_hash(by, 0)
        assert T.tag_of(hx) == T.tag_of(hy) and T.home_of(hx, 1024) == T.home_of(hy, 1024)
        assert hx != hy
    valid = [set(t) <= set(b"ACGT") for t in pair]
    if name in ("P1", "P2", "P5", "P6"):
        assert all(valid)
    if name == "P3":                                    # one on the register path, one a byte view with a 0 byte
        assert valid == [True, False] and 0 in A.canonical_bytes(y, 1) and 0 not in A.canonical_bytes(x, 1)
    if name == "P4":
        assert valid == [False, False] and 0 in A.canonical_bytes(x, 1) and 0 in A.canonical_bytes(y, 1)
    if name in ("P5", "P6"):                            # their own canonical form: the pair holds either way
        assert A.canonical_bytes(x, 1) == x and A.canonical_bytes(y, 1) == y


def test_p7_collides_across_two_documents():
    x, a, b = T.P7
    assert len(x) == 31 and a != b and A.canonical_bytes(x, 1) == x
    ha, hb = T.key_hash(x, a), T.key_hash(x, b)
    assert ha != hb and T.tag_of(ha) == T.tag_of(hb) and T.home_of(ha, 1024) == T.home_of(hb, 1024)


def test_home_slot_keys():
    for home, terms in T.HOME_1024.items():
        assert len(set(terms)) == len(terms) == 4
        for t in terms:
            assert len(t) == 31 and A.canonical_bytes(t, 1) == t
            assert T.home_of(T.key_hash(t, 0), 1024) == home


def test_stage_follows_the_batch_rule():
    docs = [([b"A" * 99], None), ([b"C" * 199], None), ([b"G" * 211], None), ([b"T" * 600], None), ([b"A" * 10, b"C" * 5], None)]
    b = T.stage(docs, 512)
    assert [[d[0] for d in x.docs] for x in b] == [[0, 1, 2], [3], [4]]
    assert [x.total for x in b] == [512, 601, 17]
    assert [d[1] for d in b[0].docs] == [0, 100, 300]
    assert T.stage(docs, 0)[0].total == 512 + 601 + 17
    assert T.stage([([b"ACGT"], 73)], 0)[0].total == 73


@pytest.mark.parametrize("seed", range(4))
def test_model_equals_brute_force_in_any_order(seed):
    """the occupied set and the tags of every cluster do not depend on the order of insertion -- on a corpus, on a
    nearly half-full table and on the wrapping cluster"""
    corpus = A.make_corpus(seed, 31, ndocs=3)
    models = [T.Model(T.stage([(seqs, None) for _, seqs in corpus], 0)[0], 31, 1)]
    for name in ("capacity-512", "wrap-canon1-c3", "P1-canon1-at-0"):
        models.append(T.last_batch_model(next(f for f in T.all_fixtures() if f.name == name)))
    rng = np.random.default_rng(seed)
    for m in models:
        keys = list(m.offsets)
        for _ in range(3):
            slots = T.brute_force(m, [keys[i] for i in rng.permutation(len(keys))])
            assert set(slots) == m.occupied
            tags = {}
            for s, key in slots.items():
                tags.setdefault(m.cluster[s], []).append(m.tag[key])
            assert {b: sorted(t) for b, t in tags.items()} == dict(m.cluster_tags)
            # the same table, as the device would hand it back, passes the read-back check ...
            owner, count = np.zeros(m.cap, dtype=np.uint64), np.zeros(m.cap, dtype=np.uint32)
            for s, key in slots.items():
                owner[s] = (m.tag[key] << T.OFFSET_BITS) | (m.offsets[key][-1] + 1)
                count[s] = min(len(m.offsets[key]), 2)
            seen = T.check_table(m, (m.cap, m.total, owner, count), 2)
            assert seen == {key: s for s, key in slots.items()}
            # ... and one merged pair of keys, one moved owner or one count off by one does not
            s0 = next(iter(slots))
            for what in ("free", "count", "tag"):
                o2, c2 = owner.copy(), count.copy()
                if what == "free":
                    o2[s0] = 0
                    c2[s0] = 0
                elif what == "count":
                    c2[s0] = len(m.offsets[slots[s0]]) + 1
                else:
                    o2[s0] ^= np.uint64(1 << T.OFFSET_BITS)
                with pytest.raises(AssertionError):
                    T.check_table(m, (m.cap, m.total, o2, c2), 2)


def test_wrapping_cluster_runs_over_the_last_slot():
    for fx in T.wrap_fixtures():
        m = T.last_batch_model(fx)
        assert m.cap == 1024 and m.occupied == {1020, 1021, 1022, 1023, 0, 1, 2}
        assert sum(1 for key in m.offsets if m.home[key] == 1023) == 4
        assert len(m.cluster_tags) == 1


FIXTURES = T.all_fixtures()


@pytest.mark.parametrize("fx", FIXTURES, ids=[f.name for f in FIXTURES])
def test_model_tells_keep_from_drop(fx):
    """every fixture's declared kept and dropped terms, from the table model and -- independently -- from the
    restatement the expected files are made with (abundance_check.kept_occurrences)"""
    batches = T.stage([(seqs, None) for _, seqs in fx.docs], fx.batch)
    assert len(batches) == 1                         # the table that stays behind is the whole build's
    m = T.Model(batches[0], fx.k, fx.canonicalize)
    assert m.cap == fx.cap and 2 * len(m.occupied) <= m.cap
    if fx.batch:
        assert m.total <= fx.batch
    keep, drop = {m.key(col, t) for col, t in fx.keep}, {m.key(col, t) for col, t in fx.drop}
    assert len(keep) == len(fx.keep) and len(drop) == len(fx.drop) and not keep & drop
    kept = m.kept(fx.c)
    assert keep <= kept and not drop & kept and drop <= set(m.offsets)
    if not fx.name.startswith("capacity"):
        assert kept == keep and keep | drop == set(m.offsets)
    for key in keep | drop:                          # the boundary: nothing declared is further than it says
        assert (m.multiplicity(key) >= fx.c) == (key in keep)
    for col, (_, seqs) in enumerate(fx.docs):
        idx, n = A.kept_occurrences(seqs, fx.k, fx.canonicalize, fx.c)
        keys = [A.canonical_bytes(s[i:i + fx.k], fx.canonicalize) for s in seqs for i in range(len(s) - fx.k + 1)]
        assert n == len(keys) and {(col, keys[i]) for i in idx} == {key for key in kept if key[0] == col}
    if fx.name.startswith("P"):                      # two keys of equal tag in one cluster
        assert any(len(t) != len(set(t)) for t in m.cluster_tags.values())
