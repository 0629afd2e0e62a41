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
    assert len(CS.FAMILIES) == 19 and len(set(CS.FAMILIES)) == 19 and {"best", "similarity"} < set(CS.FAMILIES)
    pairs = {(a.family, b.family) for a, b in zip(plan, plan[1:])}
    assert pairs == set(itertools.product(CS.FAMILIES, CS.FAMILIES))
    # ... and between two REGULAR steps too (the failure steps were put behind an occurrence of their follower's family)
    regular = {(a.family, b.family) for a, b in zip(plan, plan[1:]) if a.kind == "regular" and b.kind == "regular"}
    assert regular == set(itertools.product(CS.FAMILIES, CS.FAMILIES))
    assert all(st.index == i and st.prev == (plan[i - 1].family if i else None) for i, st in enumerate(plan))
    assert len(plan) == 19 * 19 + 1 + 2 * 3 * 19


def test_every_family_meets_every_setting(plan):
    regular = [st for st in plan if st.kind == "regular"]
    for fam in CS.FAMILIES:
        mine = [st for st in regular if st.family == fam]
        assert {st.z for st in mine} == set(CS.ZS), fam
        assert {st.policy for st in mine} == set(CS.POLICIES), fam
        assert {st.pass_bytes for st in mine} == set(CS.PASS_BYTES), fam
        assert {st.graph for st in mine} == set(CS.GRAPHS), fam
        assert {st.self_hash for st in mine} == set(CS.SELF_HASH), fam
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
    feature = [st for st in regular if st.family not in ("search_small", "search_large", "counts", "doc_bits", "own_batch", "adjusted",
                                                         "similarity")]
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
        assert not set(CS.NO_QUERIES) & set(CS.CAN_FAIL[kind]) and "best" in CS.CAN_FAIL[kind]
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
    best_not_first = best_ties = shared_pairs = 0
    whole_steps = set()
    for st in plan:
        if st.kind in ("invalid_base", "too_short"):
            continue
        v = ex.value(st)
        nonempty[st.family] += ex.nonempty(st)
        if st.family == "best":
            best_not_first += any(h[2] != offs for offs, hits in zip(st.params["offsets"], v) for h in hits)
            best_ties += any(h[5] > 1 for hits in v for h in hits)
        if st.family == "similarity":
            for fb, rows in zip(files, v):
                refs = CS.similarity_refs(st, fb)
                bits = ex.value(st._replace(family="doc_bits"))[files.index(fb)]
                per = fb.mats[0].shape[1] * 8
                assert len(rows) == len(refs) == st.params["n"] and all(0 <= r < fb.num_docs for r in refs), CS.describe(st)
                assert all(row[r % per] == bits[r] and len(row) == per for r, row in zip(refs, rows))      # shared(a, a) = bits(a)
                shared_pairs += any(0 < x < bits[r] for r, row in zip(refs, rows) for x in row)
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
    assert best_not_first > 0 and best_ties > 0 and shared_pairs > 0
    assert whole_steps == {(fam, pol, z) for fam in ("positions", "window_positions") for pol in CS.POLICIES for z in CS.ZS}
    assert some_not_all > 0 and any_ne_all > 0 and partial_cover > 0 and n_matters > 0 and overflows == len(CS.FAMILIES) == 19
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


def test_anchor_best_and_similarity_on_their_checkers(plan, handles):
    """one best step and one similarity step against the checkers' own top-level calls (best_check.results over the call's
    arguments; similarity_check.shared_of_file, which reads the index FILE)"""
    from tests import best_check as BC
    from tests import similarity_check as SC
    for name, (paths, files, ex) in handles.items():
        st = next(st for st in plan if st.family == "best" and st.kind == "regular" and st.policy != "error"
                  and any(b"N" in q for q in st.queries) and len(st.params["offsets"]) > 2)
        want = BC.results(files, list(st.queries), list(st.params["offsets"]), st.z, st.policy, st.params["t"], st.params["lim"])
        assert ex.value(st) == want and any(want), CS.describe(st)
        assert all(type(x) is int for hits in ex.value(st) for h in hits for x in h)
        st = next(st for st in plan if st.family == "similarity" and st.params["n"] == 17)
        for path, fb, rows in zip(paths, files, ex.value(st)):
            want = SC.shared_of_file(path, CS.similarity_refs(st, fb))
            assert rows == [w.tolist() for w in want], CS.describe(st)


def test_the_similarity_references(plan, handles):
    mine = [st for st in plan if st.family == "similarity"]
    assert {st.params["n"] for st in mine} == set(CS.SIMILARITY_REFS) and {st.kind for st in mine} == {"regular"}
    in_one = set()                                                      # references of one sub-index in one call: the panels
    repeats = 0
    for name, (_paths, files, _ex) in handles.items():
        for st in mine:
            for fb in files:
                refs = CS.similarity_refs(st, fb)
                per = fb.mats[0].shape[1] * 8
                subs = [r // per for r in refs]
                in_one |= {subs.count(p) for p in set(subs)}
                repeats += len(set(refs)) < len(refs)
                if st.params["n"] > 1:                                  # the first sub-index and the last, partly filled one
                    assert 0 in subs and len(fb.mats) - 1 in subs, CS.describe(st)
                    assert fb.num_docs - 1 in refs and fb.num_docs % per != 0
        ones = {CS.similarity_refs(st, files[-1])[0] // (files[-1].mats[0].shape[1] * 8) for st in mine if st.params["n"] == 1}
        assert ones == {0, len(files[-1].mats) - 1}
    assert {1, 7, 8, 9, 16, 17} <= in_one and repeats > 0               # the 8-reference panel's boundary and a second panel


MUST_FAMILIES = ("search_small", "search_large", "counts", "view", "groups", "best", "adjusted", "own_batch")


def test_the_self_hashing_steps(plan, handles):
    """what the issue of the self-hashing walk asks of the plan, from the plan alone"""
    h = "compact16"
    assert set(CS.RUN_IMPL_FAMILIES) == set(MUST_FAMILIES)
    must = [st for st in plan if CS.must_self_hash(st, h)]
    never = [st for st in plan if CS.never_self_hash(st, h)]
    assert not {st.index for st in must} & {st.index for st in never}
    neither = [st for st in plan if st.kind == "regular" and not CS.must_self_hash(st, h) and not CS.never_self_hash(st, h)]
    assert any(st.pass_bytes for st in neither) and len(must) >= 24
    for other in ("two_files", "two_files_idx64"):
        assert all(CS.never_self_hash(st, other) and not CS.must_self_hash(st, other) for st in plan)
    for st in must:
        assert st.kind == "regular" and st.self_hash == 2 and st.z == 0 and st.pass_bytes == 0 and st.family in MUST_FAMILIES
        assert st.family not in CS.SEARCH_FAMILIES or st.params["lim"] == 0, CS.describe(st)      # (groups, best: cut on the host)
        assert st.params.get("what", "counts") == "counts", CS.describe(st)
        assert max(len(q) for q in st.queries) - CS.K_MAX + 1 <= 520 and CS.self_hash_fits(h, st.queries)
        assert not (st.policy == "skip" and (st.params.get("rt", st.params.get("t", 0.0)) if st.family != "best" else 0.0) > 0)
    for st in never:
        assert (st.self_hash == 0 or st.z != 0 or st.family in CS.OWN_K1_FAMILIES + CS.NO_QUERIES), CS.describe(st)
    # the LDS array's limit: 4 sub-indexes x (blocks + 1) x 8 <= 2112, 65 blocks, 520 terms
    q = lambda terms: [b"A" * (terms + CS.K_MAX - 1)]
    assert CS.self_hash_fits(h, q(520)) and not CS.self_hash_fits(h, q(521)) and CS.self_hash_fits(h, q(1))
    assert CS.self_hash_handle(h) and not CS.self_hash_handle("two_files") and not CS.self_hash_handle("two_files_idx64")
    for fam in MUST_FAMILIES:
        mine = [st for st in must if st.family == fam]
        assert {"error", "miss"} <= {st.policy for st in mine}, fam
        # the same shape on the table path
        assert any(st.family == fam and st.kind == "regular" and st.z == 0 and st.self_hash == 0 and st.pass_bytes == 0
                   and st.params.get("what", "counts") == "counts" for st in plan), fam
    for fam in ("counts", "groups", "best", "own_batch"):
        assert any(st.family == fam and st.policy == "skip" and any(b"N" in q for q in st.queries) for st in must), fam
    # a graph captured in one form and the other form right behind it, both ways round
    small = {st.index: st for st in plan if st.family == "search_small" and st.kind == "regular"}
    on_table = lambda st: st.self_hash == 0 and st.z == 0 and st.graph != 0 and st.pass_bytes == 0
    hashing = lambda st: CS.must_self_hash(st, h) and st.graph != 0
    same = lambda a, b: (a.queries, a.params, a.policy) == (b.queries, b.params, b.policy)
    assert any(i + 1 in small and on_table(a) and hashing(small[i + 1]) and same(a, small[i + 1]) for i, a in small.items())
    # (search_small is directly behind search_small once in the circuit: the other order is the pair around a call that
    # the host refuses before anything is launched)
    assert sum(i + 1 in small for i in small) == 1
    assert any(i + 2 in small and hashing(a) and on_table(small[i + 2]) and same(a, small[i + 2]) and plan[i + 1].kind == "too_short"
               for i, a in small.items())
    # the scan's own report of an invalid base, from a query above index 16
    for fam in ("search_large", "groups", "best"):
        st = next(st for st in plan if st.family == fam and st.kind == "invalid_base")
        assert CS.must_self_hash(st, h, "invalid_base") and st.params["bad"] > 16 and len(st.queries) == 24, CS.describe(st)
        terms = [[len(q) - CS.K_MAX + 1 for q in st.queries] for st in must if st.family == fam]
        assert any(256 <= max(t) <= 520 for t in terms) and any(max(t) <= 255 for t in terms), fam
    # a step's expected value does not depend on the switch
    # (Expect.value's memo key leaves the switch out; computed afresh for both values, not taken from the memo)
    _paths, files, _ex = handles[h]
    fresh = CS.Expect(files)
    for st in [next(st for st in must if st.family == fam) for fam in MUST_FAMILIES]:
        a, b = (fresh._value(s, s.family, s.queries, s.params, s.z, s.policy) for s in (st, st._replace(self_hash=0)))
        assert a == b, CS.describe(st)
    # a top-k host-buffer search at z = 0 and pass_bytes 0 with graph on and the switch at 2 stays in the plan (neither `must`
    # nor `never`: it keeps K1's table), and so does a grouped search under `skip` at z = 0 with a positive read threshold
    assert any(st.family in CS.SEARCH_FAMILIES and st.kind == "regular" and st.z == 0 and st.pass_bytes == 0 and st.graph != 0
               and st.self_hash == 2 and st.policy in ("error", "miss") and st.params["lim"] > 0 for st in plan)
    assert any(st.family == "groups" and st.kind == "regular" and st.z == 0 and st.policy == "skip" and st.params["rt"] > 0 for st in plan)


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
