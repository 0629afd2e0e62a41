"""CPU: tests/threshold_edges.py itself, every checker's bound function against its one statement of the rule, and -- for
the inputs of tests/test_gpu_threshold_edges.py -- that the checkers alone show a document on every bound and one below
it (condition (a)), so that the GPU file leaves no case out (condition (b))."""
import math
import types
from fractions import Fraction

import pytest

from tests import best_check
from tests import coverage_check
from tests import findere_check
from tests import groups_check
from tests import invalid_check
from tests import set_quorum_check
from tests import sets_check
from tests import threshold_edges as E
from tests import weighted_check
from tests import window_check

# the denominators of the GPU file: 100 and 111 positions (31- and 20-mers of a 130-character query), 101 and 112 under
# `miss`, 200 and 222 (a group of two), the 140 characters of the coverage query, a window of 50, 100 members
DENOMINATORS = (100, 111, 101, 112, 200, 222, 140, 50)


def test_on_and_above_are_neighbours_on_both_sides_of_the_bound():
    for P in DENOMINATORS + (1, 3, 7, 64, 1000, 4294967):
        for c in sorted({1, 2, P // 3 + 1, P // 2, P - 1, P, P + 1}):
            if c < 1:
                continue
            t_on, t_above = E.on_and_above(c, P)
            assert math.nextafter(t_on, math.inf) == t_above
            assert math.ceil(float(t_on) * float(P)) == c and math.ceil(float(t_above) * float(P)) == c + 1
            assert E.bound(t_on, P) == c and E.bound(t_above, P) == c + 1
    # monotone in c
    ts = [E.on_and_above(c, 100)[0] for c in range(1, 101)]
    assert ts == sorted(ts) and len(set(ts)) == 100


def test_the_bound_is_monotone_in_the_threshold():
    ts = sorted(t for t in E.CLASSES if t == t) + [0.07, 0.5, 0.999]
    for P in (0, 1, 100, 111):
        for one in (False, True):
            bs = [E.bound(t, P, one) for t in sorted(ts)]
            assert bs == sorted(bs), (P, one, bs)
            assert E.bound(math.nan, P, one) == 0


def test_adversarial_pairs_exist_in_both_directions_for_every_denominator():
    for P in DENOMINATORS:
        adv = E.adversarial([P])
        for direction in ("up", "down"):
            assert [a for a in adv if a[0] == direction], (P, direction)
        for direction, t, p, double_bound, exact in adv:
            assert E.bound(t, p) == double_bound and abs(double_bound - exact) == 1
            if direction == "up":
                c = double_bound - 1
                assert t == c / p and math.ceil(Fraction(c, p) * p) == c == exact
            else:
                assert math.ceil(Fraction(t) * p) == exact == double_bound + 1
                # a bound rounded half up, or formed in float, says something else for at least one of them
    assert ("up", 0.07, 100, 8, 7) in E.adversarial([100])
    assert E.adversarial([64, 128]) == []                      # (a power of two: every product is exact)


def _fake_file(P):
    """a file in which a query of P characters has P positions, all valid (term size 1, canonicalize 0)"""
    return types.SimpleNamespace(term_size=1, canonicalize=0, positions=lambda q, z: len(q) - z)


def _checker_bounds(t, P):
    """{site: (the checker's bound, at least 1, limit)}"""
    fb, q = _fake_file(P), b"A" * P
    out = {
        "findere": (findere_check.threshold_for(t, P), False, E.LIMIT32),
        "invalid miss": (invalid_check.threshold("miss", t, fb, q, 0), False, E.LIMIT32),
        "invalid skip": (invalid_check.threshold("skip", t, fb, q, 0), True, E.LIMIT32),
        "groups read": (groups_check.read_threshold_of(fb, q, 0, "error", t), False, E.LIMIT32),
        "groups read skip": (groups_check.read_threshold_of(fb, q, 0, "skip", t), True, E.LIMIT32),
        "groups": (groups_check.group_threshold(t, P), True, E.LIMIT64),
        "best": (best_check.threshold_of(t, P), True, E.LIMIT32),
        "weighted": (weighted_check.thresholds(t, P), True, E.LIMIT32),
        "coverage": (coverage_check.thresholds(t, P), True, E.LIMIT32),
        "window": (window_check.thresholds(t, P), True, E.LIMIT32),
        "sets": (sets_check.threshold_for(t, P), True, E.LIMIT32),
        "quorum threshold": (set_quorum_check.threshold_for(t, P), True, E.LIMIT32),
    }
    return out


def _thresholds(P):
    ts = list(E.CLASSES)
    if P >= 1:
        for c in sorted({1, max(1, P // 2), P}):
            ts += list(E.on_and_above(c, P))
        ts += [a[1] for a in E.adversarial([P])]
    return ts


@pytest.mark.parametrize("P", (0, 1) + DENOMINATORS)
def test_every_checker_states_the_one_rule(P):
    for t in _thresholds(P):
        for site, (got, one, limit) in _checker_bounds(t, P).items():
            assert got == E.bound(t, P, one, limit), (site, t, P, got)
        # need = max(1, ceil(quorum * members)): the call refuses a quorum outside (0, 1], and so does the checker
        if t > 0 and t <= 1:
            assert set_quorum_check.need(t, P) == E.bound(t, P, True), (t, P)
        else:
            assert E.QuorumNeed.refused(t)
            with pytest.raises(ValueError):
                set_quorum_check.need(t, P)


def test_a_huge_product_is_clamped_not_an_error():
    assert findere_check.threshold_for(1e300, 100) == findere_check.threshold_for(math.inf, 100) == 2 ** 32 - 1
    assert findere_check.threshold_for(math.inf, 0) == 0 and findere_check.threshold_for(math.nan, 100) == 0
    assert findere_check.threshold_for((2 ** 32 - 1.5) / 1.0, 1) == 2 ** 32 - 1
    assert groups_check.group_threshold(1.0, 2 ** 33) == 2 ** 33 and groups_check.group_threshold(math.inf, 5) == 2 ** 64 - 1
    assert E.bound(1.0, 2 ** 33) == 2 ** 32 - 1 and E.bound(1.0, 2 ** 33, limit=E.LIMIT64) == 2 ** 33


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    return E.build_all(tmp_path_factory.mktemp("threshold_edges"))


@pytest.mark.parametrize("handle", sorted(E.HANDLES))
@pytest.mark.parametrize("family", sorted(E.FAMILIES))
def test_the_checker_alone_shows_every_boundary(files, family, handle):
    """conditions (a) and (b) for the inputs of the GPU file: case_list raises where a bound inside [1, P] has no document
    on it or none one below; the expectation of every case then holds the on-bound document and not the one below"""
    fam = E.FAMILIES[family]()
    fbs = [files[name][1] for name in E.HANDLES[handle]]
    for f in range(len(fbs)):
        cases = fam.cases(fbs, f)
        names = [c[0] for c in cases]
        assert names[:4] == ["t_on", "t_above", "adversarial_up", "adversarial_down"] and len(cases) == 4 + len(E.CLASSES)
        P = fam.P(fbs, f)
        assert [a for a in E.adversarial([P]) if a[0] == "up"] and [a for a in E.adversarial([P]) if a[0] == "down"]
        keys = sorted(set(int(k) for k in fam.keys(fbs, f)))
        assert keys[0] == 0 and keys[-1] == P, (family, handle, f, keys[-3:], P)
        (_, t_on, c), (_, t_above, c1) = cases[0], cases[1]
        assert c1 == c + 1 and {c - 1, c, c + 1} <= set(keys)
        if family == "quorum_need":
            continue                    # (its keys are the cells of set 0: the records carry the core, see below)
        for name, t, b in cases[:4]:
            want = fam.expected(fbs, t)
            want = want[0] if family in ("groups", "best") else want
            if family == "groups_read":
                voted = sorted(h[2] for h in want[1] if h[0] == f and h[3] == 1)      # group 1 = [Q]: score = Q's own
                assert voted and voted[0] == b, (family, handle, name, voted[:3], b)
                continue
            col = {"sets_all": 3, "best": 3}.get(family, 2)
            scores = sorted(h[col] for h in want if h[0] == f)
            assert scores and scores[0] == b, (family, handle, f, name, t, scores[:3], b)


def test_the_quorum_moves_the_core_of_the_large_set_by_one(files):
    fam = E.QuorumNeed()
    for handle, names in E.HANDLES.items():
        fbs = [files[n][1] for n in names]
        for f in range(len(fbs)):
            (_, t_on, c), (_, t_above, _c1) = fam.cases(fbs, f)[:2]
            core = [dict(((h[0], h[1]), h[2]) for h in fam.expected(fbs, t))[(f, 0)] for t in (t_on, t_above)]
            assert core == [E.SET0_MEMBERS + 1 - c, E.SET0_MEMBERS - c], (handle, f, c, core)
