"""CPU: the plan of the call-sequence test (tests/call_sequence.py) covers what it says -- every ordered pair of families,
every setting for every family, every label state for the set families, every family after every failure kind --, its
expected values are not vacuous, it is deterministic, and its glue (index building, query cutting) is anchored on the
oracle."""
import itertools
import time

import numpy as np
import pytest

from tests import call_sequence as CS
from tests import invalid_check as I
from tests import positions_check as PC
from tests.test_gpu_window import _partial


@pytest.fixture(scope="module")
def plan():
    return CS.build_plan()


@pytest.fixture(scope="module")
def handles(tmp_path_factory):
    out = {}
    for name in ("compact16", "two_files"):
        paths, files = CS.build_files(tmp_path_factory.mktemp(name), name)
        out[name] = (paths, files, CS.Expect(files))
    return out


def test_every_ordered_pair_of_families(plan):
    assert len(CS.FAMILIES) == 17 and len(set(CS.FAMILIES)) == 17
    pairs = {(a.family, b.family) for a, b in zip(plan, plan[1:])}
    assert pairs == set(itertools.product(CS.FAMILIES, CS.FAMILIES))
    # ... and between two REGULAR steps too (the failure steps were put behind an occurrence of their follower's family)
    regular = {(a.family, b.family) for a, b in zip(plan, plan[1:]) if a.kind == "regular" and b.kind == "regular"}
    assert regular == set(itertools.product(CS.FAMILIES, CS.FAMILIES))
    assert all(st.index == i and st.prev == (plan[i - 1].family if i else None) for i, st in enumerate(plan))
    assert len(plan) == 17 * 17 + 1 + 2 * 3 * 17


def test_every_family_meets_every_setting(plan):
    regular = [st for st in plan if st.kind == "regular"]
    for fam in CS.FAMILIES:
        mine = [st for st in regular if st.family == fam]
        assert {st.z for st in mine} == set(CS.ZS), fam
        assert {st.policy for st in mine} == set(CS.POLICIES), fam
        assert {st.pass_bytes for st in mine} == set(CS.PASS_BYTES), fam
        assert {st.graph for st in mine} == set(CS.GRAPHS), fam
    for fam in CS.SET_FAMILIES:
        assert {st.labels for st in regular if st.family == fam} == set(CS.LABEL_STATES), fam
    # every window (one per plane count of the scan) meets both z, both pass_bytes and all three policies
    for fam in CS.WINDOW_FAMILIES:
        assert {st.params["W"] for st in plan if st.family == fam} == set(CS.WINDOWS), fam
        for W in CS.WINDOWS:
            mine = [st for st in regular if st.family == fam and st.params["W"] == W]
            assert {st.z for st in mine} == set(CS.ZS), (fam, W)
            assert {st.policy for st in mine} == set(CS.POLICIES), (fam, W)
            assert {st.pass_bytes for st in mine} == set(CS.PASS_BYTES), (fam, W)
    # the label states come in time order
    order = [k for k, _g in itertools.groupby(st.labels for st in plan)]
    assert order == list(CS.LABEL_STATES)
    # the query counts cross 1 / 2 / 16 / 17 / 24, the lengths both score widths; a small pass_bytes comes with the batch
    # that needs three passes
    assert {len(st.queries) for st in regular if st.family == "search_small"} == {1, 2, 16}
    # search_large is the pipelined passes: more than the 16 queries of a captured graph in EVERY step, failures included
    large = [st for st in plan if st.family == "search_large"]
    assert {len(st.queries) for st in large} == {24} and {st.kind for st in large} == {"regular"} | set(CS.KINDS)
    assert all(len(st.queries) == 16 for st in plan if st.kind == "overflow" and st.family != "search_large")
    feature = [st for st in regular if st.family not in ("search_small", "search_large", "counts", "doc_bits", "own_batch", "adjusted")]
    assert {len(st.queries) for st in feature} == set(CS.NQS)
    widths = [max(len(q) for q in st.queries) - CS.K_MAX + 1 - st.z > 255 for st in regular]
    assert sum(a != b for a, b in zip(widths, widths[1:])) > 40
    assert all(len(q) - CS.K_MAX + 1 - st.z <= 700 for st in plan for q in st.queries)          # no 32-bit query
    fresh = [st for st in regular if st.params.get("what") != "reread"]              # (a second reading keeps its run's queries
    for st in fresh:                                                                 # and sends nothing to the device)
        if st.pass_bytes and len(st.queries) == 24:
            assert sum(len(q) + 16 for q in st.queries) * 16 > 2 * CS.PASS_SMALL, CS.describe(st)
    assert all(len(q) >= CS.K_MAX + st.z for st in fresh for q in st.queries)
    assert sum(len(st.queries[0]) == CS.K_MAX + st.z for st in fresh) > 50          # the shortest query there is


def test_every_failure_kind_is_followed_by_every_family(plan):
    for kind in CS.KINDS:
        followers = {b.family for a, b in zip(plan, plan[1:]) if a.kind == kind}
        assert followers == set(CS.FAMILIES), kind
        failing = {st.family for st in plan if st.kind == kind}
        assert failing == set(CS.CAN_FAIL[kind]), kind                 # one failing call of every family that can fail this way
    for a, b in zip(plan, plan[1:]):
        if a.kind != "regular":
            assert b.kind == "regular" and b.family != a.family and b.after == a.kind, CS.describe(b)
            assert not (a.family in CS.SET_FAMILIES and a.labels == "cleared")
        else:
            assert b.after is None
    for st in plan:
        z = st.z
        if st.kind == "invalid_base":
            i = st.params["bad"]
            assert st.policy == "error" and b"N" in st.queries[i] and (i > 0 or len(st.queries) == 1)
            assert all(b"N" not in q for j, q in enumerate(st.queries) if j != i)
        elif st.kind == "too_short":
            lens = [len(q) for q in st.queries]
            assert lens[st.params["bad"]] == CS.K_MAX + z - 1 and sum(n < CS.K_MAX + z for n in lens) == 1
        elif st.kind == "regular" and st.policy == "error" and st.params.get("what") != "reread":
            assert all(set(q) <= set(b"ACGT") for q in st.queries), CS.describe(st)


def test_the_own_batch_steps_read_earlier_runs_again(plan):
    mine = [st for st in plan if st.family == "own_batch" and st.kind == "regular"]
    whats = [st.params["what"] for st in mine]
    assert whats[0] == "topk" and {"topk", "counts", "reread"} == set(whats) and whats.count("reread") >= 5
    last = None
    for st in plan:
        if st.family != "own_batch":
            continue
        if st.kind != "regular":
            last = None
        elif st.params["what"] == "reread":
            assert last is not None and st.queries == last.queries and st.params["of"] == last.params["what"]
            assert (st.params["run_z"], st.params["run_policy"]) == (last.z, last.policy)
        else:
            last = st
    # between a run and its second reading the handle's settings changed at least once somewhere
    assert any(st.params["what"] == "reread" and (st.params["run_z"], st.params["run_policy"]) != (st.z, st.policy) for st in mine)


def test_the_builder_is_deterministic():
    a, b, c = CS.build_plan(0), CS.build_plan(0), CS.build_plan(1)
    assert a == b and a != c
    assert [st.family for st in a] != [st.family for st in c]


@pytest.mark.parametrize("name", ["compact16", "two_files"])
def test_the_expectations_are_not_vacuous(plan, handles, name):
    _paths, files, ex = handles[name]
    t0 = time.perf_counter()
    nonempty = {fam: 0 for fam in CS.FAMILIES}
    some_not_all = any_ne_all = partial_cover = n_matters = overflows = 0
    win_partial = win_some_not_all = win_n_matters = w_differs = adjusted_between = adjusted_skip_n = words_anchored = 0
    whole_steps = set()
    for st in plan:
        if st.kind in ("invalid_base", "too_short"):
            continue
        v = ex.value(st)
        nonempty[st.family] += ex.nonempty(st)
        if st.kind == "overflow":
            total = sum(len(x) for x in (v[0] if st.family in ("weighted", "groups") else v))
            assert total > CS.HIT_CAP_SMALL, CS.describe(st)            # the pool of HIT_CAP_SMALL records does overflow
            overflows += 1
            continue
        if st.family in ("search_small", "search_large", "view") and st.params["t"] > 0 and st.params["lim"] == 0:
            every = ex.search(st.queries, st.z, st.policy, 0.0, 0)
            some_not_all += any(0 < len(got) < len(full) for got, full in zip(v, every))
        if st.family == "sets":
            any_ne_all += any(a != b for rows in v for (_f, _s, a, b) in rows)
        if st.family == "coverage" and st.params["t"] == 0 and st.params["lim"] == 0:
            partial_cover += any(0 < cov < len(q) for q, rows in zip(st.queries, v) for (_f, _d, cov) in rows)
        if st.family in ("search_small", "search_large", "view") and st.policy != "error":
            for i, q in enumerate(st.queries):
                if b"N" in q:
                    clean = q.replace(b"N", b"A")
                    n_matters += ex.search((clean,), st.z, st.policy, st.params["t"], st.params["lim"])[0] != v[i]
        if st.family == "window":
            W, t, lim = st.params["W"], st.params["t"], st.params["lim"]
            tabs = [ex.window_tables(q, st.z, W, st.policy) for q in st.queries]
            win_partial += _partial(tabs)                               # not the plain search's answer
            if t > 0 and lim == 0:
                every = ex.window(st.queries, st.z, st.policy, W, 0.0, 0)
                win_some_not_all += any(0 < len(got) < len(full) for got, full in zip(v, every))
            if st.policy != "error":
                for i, q in enumerate(st.queries):
                    if b"N" in q:
                        win_n_matters += ex.window((q.replace(b"N", b"A"),), st.z, st.policy, W, t, lim)[0] != v[i]
            if W == max(CS.WINDOWS) and len(files) > 1:                 # w = n, and n differs between the files
                assert all(tab[f][0] == fb.positions(q, st.z) for q, tab in zip(st.queries, tabs) for f, fb in enumerate(files))
                w_differs += any(len({w for (w, _b, _docs, _sc) in tab}) > 1 for tab in tabs)
        if st.family in ("positions", "window_positions"):
            # Expect.position_words packs all documents of a query at once: against the checker's own two calls, EVERY hit
            # of the first step of each (family, policy, z), some hits of every query of the others
            whole = (st.family, st.policy, st.z) not in whole_steps
            whole_steps.add((st.family, st.policy, st.z))
            for q, hs, ws in zip(st.queries, v[0], v[1]):
                assert len(hs) == len(ws)
                for (f, d, _sc), words in list(zip(hs, ws))[::1 if whole else max(1, len(hs) // 3)]:
                    assert words == [int(x) for x in PC.pack(PC.positions(files, q, st.z, f, d, st.policy))], CS.describe(st)
                    words_anchored += 1
        if st.family == "window_positions" and st.kind == "regular" and st.pass_bytes and len(st.queries) == 24:
            # every candidate of the pass guard has a window hit for every query: none drops out of the pass check
            assert all(len(hits) > 0 for hits in v[0]) and CS.needs_three_passes(st, ex), CS.describe(st)
        if st.family == "adjusted":
            q = st.queries[0]
            floats = ex.adjusted_floats(st)
            assert len(floats) == len(v)
            adjusted_between += any(0.0 < a < sc for (_d, sc), (_e, a) in zip(v, floats))
            if st.policy == "skip" and b"N" in q and len(v) > 0:        # (a step that compares floats)
                adjusted_skip_n += all(0 < ex.valid_positions(q, st.z, "skip", f) < fb.positions(q, st.z) for f, fb in enumerate(files))
    assert all(nonempty.values()), nonempty
    assert win_partial > 0 and win_some_not_all > 0 and win_n_matters > 0 and (w_differs > 0 or len(files) == 1)
    assert adjusted_between > 0 and adjusted_skip_n > 0 and words_anchored > 500
    assert whole_steps == {(fam, pol, z) for fam in ("positions", "window_positions") for pol in CS.POLICIES for z in CS.ZS}
    assert some_not_all > 0 and any_ne_all > 0 and partial_cover > 0 and n_matters > 0 and overflows == len(CS.FAMILIES) == 17
    # a step without labels expects what the library documents: every query's list is empty (and the call succeeds)
    for st in plan:
        if st.family in CS.SET_FAMILIES and st.labels == "cleared" and st.kind == "regular":
            v = ex.value(st)
            assert (v[1] == [] and set(v[0]) == {0}) if st.family == "set_prevalence" else all(rows == [] for rows in v)
    # the pass counters are asserted for every family that has a reader (the guard of the GPU walk lets steps through)
    for fam in CS.PASS_READERS:
        assert sum(CS.needs_three_passes(st, ex) for st in plan if st.family == fam) >= 2, fam
    assert not any(CS.needs_three_passes(st, ex) for st in plan if st.family not in CS.PASS_READERS or st.kind != "regular")
    print("%s: %d steps expected in %.1f s" % (name, len(plan), time.perf_counter() - t0))


def test_anchor_on_the_oracle(plan, handles, oracle):
    """one search_small expectation at z = 0 with all-ACGT queries through oracle.Index: the sequence test's own glue
    (index building, query cutting) is not wrong on both sides"""
    from tests import cases
    for name in ("compact16", "two_files"):
        paths, _files, ex = handles[name]
        ixs = [oracle.Index.open(p) for p in paths]
        done = 0
        for st in plan:
            if st.family == "search_small" and st.kind == "regular" and st.z == 0 and all(set(q) <= set(b"ACGT") for q in st.queries):
                want = [cases.oracle_results(ixs, q, st.params["t"], st.params["lim"]) for q in st.queries]
                assert ex.value(st) == want, CS.describe(st)
                done += 1
        assert done >= 3
        st = next(st for st in plan if st.family == "counts" and st.kind == "regular" and st.z == 0 and b"N" not in st.queries[0])
        assert ex.value(st) == np.concatenate([ix.counts(st.queries[0]) for ix in ixs]).tolist()


def test_the_labels_of_every_state(handles):
    for name, (_paths, files, ex) in handles.items():
        for state in CS.LABEL_STATES:
            labs = ex.labels(state)
            assert len(labs) == len(files)
            for fb, lab in zip(files, labs):
                assert lab is None or (len(lab) == fb.num_docs and lab.min() >= -1 and lab.max() <= 3)
        assert all(lab is None for lab in ex.labels("cleared"))
        assert (ex.labels("initial")[0] is None) == (len(files) > 1) and ex.labels("initial")[-1] is not None
        assert all(lab is not None for lab in ex.labels("relabel1"))
        two = ex.labels("relabel2")[-1]
        assert int((two == 2).sum()) == 1                               # a one-member set
        assert not any(np.array_equal(a, b) for s1, s2 in itertools.combinations([s for s in CS.LABEL_STATES if s != "cleared"], 2)
                       for a, b in zip(ex.labels(s1), ex.labels(s2)) if a is not None and b is not None)
    assert I.MODES == CS.POLICIES[1:]
