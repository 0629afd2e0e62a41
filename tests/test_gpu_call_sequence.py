"""GPU: every call family after every other on ONE handle (the plan of tests/call_sequence.py).  The host-buffer search, counts,
the view call, hit positions, prevalence, the weighted, coverage, set, quorum and grouped searches, set prevalence,
doc_bits, the window search (at one W per plane count of its scan), hit positions over window hits, the adjusted search
(which under `skip` opens a short-lived Batch of its own), the best-of-group search (two batches, a stream and a select of
its own) and doc_shared_bits (a workspace of its own beside the fill cache of doc_bits) all work on the handle's scratch
workspace or beside it; a long-lived Batch of the caller's lives beside it.  One Search and one Batch walk the whole plan -- every ordered pair of families, a failing
call of every kind in front of every family, findere z, the invalid-bases policy, the labels, pass_bytes, graph, the query
count, the score width and the form of the scan (tuning key scan_self_hash: K1's table or the self-hashing work-groups)
changing between the steps -- and after EVERY step the answer is compared exactly with the checkers, and the handle's
self_hash_passes counter with what call_sequence.must_self_hash / never_self_hash say about the step.  A failing step names the pair: the previous family, this family and the settings in force."""
import gc
import time

import numpy as np
import pytest

from tests import call_sequence as CS

pytestmark = pytest.mark.gpu

PASS_READERS = CS.PASS_READERS
LEAK_CYCLES = 3


def _lists(offs, hits):
    rows = hits.tolist()
    return [rows[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


def _first_difference(got, want, path=""):
    if type(got) in (list, tuple) and type(want) in (list, tuple):
        if len(got) != len(want):
            return "%s: %d entries, expected %d" % (path or "value", len(got), len(want))
        for i, (a, b) in enumerate(zip(got, want)):
            if a != b:
                return _first_difference(a, b, "%s[%d]" % (path, i))
    return "%s: %r, expected %r" % (path or "value", got, want)


class Walker:
    def __init__(self, lib, search, batch, expect, handle):
        self.lib, self.s, self.b, self.ex, self.handle = lib, search, batch, expect, handle
        self.z, self.policy, self.labels, self.pass_bytes, self.graph = 0, "error", None, 0, -1
        self.self_hash = None                                           # (the shipped default, 1, is neither of the plan's)
        self.not_mine = 0                                               # self-hashing passes of a step's call in front of the family's own
        self.floats = None                                              # (expected_fp, adjusted) of the last search_adjusted

    def settle(self, st):
        """bring the handle to the step's settings (only what differs is set: the calls in between see the changes)"""
        s = self.s
        if st.z != self.z:
            s.set_findere(st.z)
        if st.policy != self.policy:
            s.invalid_bases = st.policy
        if st.labels != self.labels:
            for f, lab in enumerate(self.ex.labels(st.labels)):
                s.set_doc_sets(lab, file_no=f)
        if st.pass_bytes != self.pass_bytes:
            s.set_tuning("pass_bytes", st.pass_bytes)
        if st.graph != self.graph:
            s.set_tuning("graph", st.graph)
        if st.self_hash != self.self_hash:
            s.set_tuning("scan_self_hash", st.self_hash)
        self.z, self.policy, self.labels, self.pass_bytes, self.graph = st.z, st.policy, st.labels, st.pass_bytes, st.graph
        self.self_hash = st.self_hash
        assert s.findere == st.z and s.invalid_bases == st.policy

    def call(self, st):
        """the step's call -> its answer in the form Expect.value gives"""
        s, qs, p = self.s, list(st.queries), st.params
        fam = st.family
        if fam in ("search_small", "search_large"):
            return _lists(*s.search_arrays(qs, p["t"], p["lim"]))
        if fam == "counts":
            return s.counts(qs[0]).tolist()
        if fam == "view":
            offs, hits = s.search_view(qs, p["t"], p["lim"])
            return _lists(np.array(offs), np.array(hits))                # (views of the handle's arena: copied at once)
        if fam == "positions":
            before = s.self_hash_passes
            offs, hits = s.search_arrays(qs, 0.5, 0)                    # (a host-buffer search: it may well hash for itself)
            self.not_mine = s.self_hash_passes - before
            bo, bits = s.hit_positions(qs, offs, hits)
            words = [bits[int(bo[h]):int(bo[h + 1])].tolist() for h in range(len(hits))]
            return (_lists(offs, hits), [words[int(offs[i]):int(offs[i + 1])] for i in range(len(qs))])
        if fam == "prevalence":
            offs, counts = s.prevalence_arrays(qs)
            return (offs.tolist(), counts.tolist())
        if fam == "weighted":
            offs, hits, total = s.search_weighted_arrays(qs, p["t"], p["lim"])
            return (_lists(offs, hits), total.tolist())
        if fam == "coverage":
            return _lists(*s.search_coverage_arrays(qs, p["t"], p["lim"]))
        if fam == "sets":
            return _lists(*s.search_sets_arrays(qs, p["t"], p["rank_by"], p["lim"]))
        if fam == "quorum":
            return _lists(*s.search_sets_quorum_arrays(qs, p["quorum"], p["t"], p["lim"]))
        if fam == "set_prevalence":
            offs, counts = s.set_prevalence_arrays(qs)
            return (offs.tolist(), counts.tolist())
        if fam == "groups":
            offs, hits, pos = s.search_groups_arrays(qs, list(p["offsets"]), p["t"], p["rt"], p["lim"])
            return (_lists(offs, hits), pos.tolist())
        if fam == "doc_bits":
            return [s.doc_bits(f).tolist() for f in range(s.num_files)]
        if fam == "best":
            return _lists(*s.search_best_arrays(qs, list(p["offsets"]), p["t"], p["lim"]))
        if fam == "similarity":
            return [[row.tolist() for row in s.doc_shared_bits(CS.similarity_refs(st, fb), f)] for f, fb in enumerate(self.ex.files)]
        if fam == "window":
            return _lists(*s.search_window_arrays(qs, p["W"], p["t"], p["lim"]))
        if fam == "window_positions":
            offs, hits = s.search_window_arrays(qs, p["W"], 0.5, 0)
            bo, bits = s.hit_positions(qs, offs, hits)                  # (the hits of a window search are a legal input)
            self.window_identities(st, offs, hits, bo, bits)
            words = [bits[int(bo[h]):int(bo[h + 1])].tolist() for h in range(len(hits))]
            return (_lists(offs, hits), [words[int(offs[i]):int(offs[i + 1])] for i in range(len(qs))])
        if fam == "adjusted":
            # (under `skip` the call opens a Batch of its own on the handle, beside the walker's and the scratch batch)
            res = s.search_adjusted(qs[0], p["t"], p["lim"])
            self.floats = [(r.expected_fp, r.adjusted) for r in res]
            docs = [int(r.doc_name[4:]) for r in res]
            assert [r.doc_name for r in res] == ["doc_%05d" % d for d in docs], "%s\n  names %r" % (CS.describe(st), [r.doc_name for r in res][:4])
            return [(d, r.score) for d, r in zip(docs, res)]
        assert fam == "own_batch"
        b = self.b
        what = p["what"]
        if what == "topk":
            b.set_queries(qs)
            b.run_topk(p["t"], p["k"], keep_counts=False)
            b.sync()
        elif what == "counts":
            b.set_queries(qs)
            b.run(0.0)
            b.sync()
        if (p["of"] if what == "reread" else what) == "topk":
            return [b.hits_host(i, p["k"]) for i in range(len(qs))]
        return [b.counts_host(i).tolist() for i in range(len(qs))]

    def window_identities(self, st, offs, hits, bo, bits):
        """for every window hit: best_window over its hit_positions words is its score; with W >= n the popcount is"""
        W = st.params["W"]
        ks = [fb.term_size for fb in self.ex.files]
        if not len(hits):
            return
        assert bits.dtype == np.uint64 and int(bo[len(hits)]) == len(bits), CS.describe(st)
        ones = np.unpackbits(bits.view(np.uint8)).reshape(-1, 64).sum(axis=1)       # the set bits of every word
        pops = np.add.reduceat(ones, bo[:-1].astype(np.int64)).tolist()             # ... of every hit (none has no word)
        files, scores, bo = hits["file_no"].tolist(), hits["score"].tolist(), bo.tolist()
        for i, q in enumerate(st.queries):
            for h in range(int(offs[i]), int(offs[i + 1])):
                n = len(q) - ks[files[h]] + 1 - st.z
                best = self.lib.best_window(bits[bo[h]:bo[h + 1]], n, W)[0]
                assert best == scores[h], "%s\n  query %d, hit %d: best_window %d, score %d" % (CS.describe(st), i, h, best, scores[h])
                if W >= n:
                    assert pops[h] == scores[h], "%s\n  query %d, hit %d: popcount %d, score %d" % (CS.describe(st), i, h, pops[h], scores[h])

    def check(self, st, got, what=""):
        want = self.ex.value(st)
        got = _plain(got)
        if got != _plain(want):
            raise AssertionError("%s%s\n  %s" % (CS.describe(st), what, _first_difference(got, _plain(want))))
        if st.family == "adjusted":                                     # the floats: to the relative 1e-12 of tests/test_gpu_fill.py
            want = self.ex.adjusted_floats(st)
            assert len(self.floats) == len(want), CS.describe(st)
            for r, (got_f, want_f) in enumerate(zip(self.floats, want)):
                for name, a, b in zip(("expected_fp", "adjusted"), got_f, want_f):
                    assert abs(a - b) <= 1e-12 * abs(b), "%s\n  result %d: %s %r, expected %r" % (CS.describe(st), r, name, a, b)

    def step(self, st):
        """the step, and what it did to the handle's self_hash_passes counter"""
        s = self.s
        self.settle(st)
        self.not_mine = 0
        before = s.self_hash_passes
        self.step_call(st)
        grew = s.self_hash_passes - before - self.not_mine
        if CS.must_self_hash(st, self.handle):
            assert grew >= 1, "%s\n  no pass of the step took the self-hashing form" % CS.describe(st)
        if CS.must_self_hash(st, self.handle, "invalid_base"):         # (the scan itself found the bad query)
            assert grew >= 1, "%s\n  the failing pass did not take the self-hashing form" % CS.describe(st)
        if CS.never_self_hash(st, self.handle):
            assert grew == 0, "%s\n  %d passes of the step took the self-hashing form" % (CS.describe(st), grew)

    def step_call(self, st):
        from cobs_amd import _capi
        s = self.s
        if st.kind in ("invalid_base", "too_short"):
            status = _capi.ERR_INVALID_BASE if st.kind == "invalid_base" else _capi.ERR_QUERY_TOO_SHORT
            try:
                self.call(st)
            except self.lib.CobsGpuError as e:
                assert e.status == status, "%s\n  raised %r" % (CS.describe(st), e)
                if st.kind == "invalid_base":
                    assert "(query %d)" % st.params["bad"] in str(e), "%s\n  raised %r" % (CS.describe(st), e)
                return
            raise AssertionError("%s\n  the call did not fail" % CS.describe(st))
        if st.kind == "overflow":
            if st.family == "sets":
                # a caller's buffer one record too small: ERR_CAPACITY and the needed sizes, as tests/test_gpu_sets.py has it
                from tests.test_gpu_sets import _raw_search
                want = self.ex.value(st)
                need = sum(len(x) for x in want)
                st_, _bad, offs, _hits, msg = _raw_search(s, list(st.queries), need - 1, st.params["t"],
                                                          s.SETS_RANK_BY.index(st.params["rank_by"]), st.params["lim"])
                assert st_ == _capi.ERR_CAPACITY and offs.tolist() == np.cumsum([0] + [len(x) for x in want]).tolist(), \
                    "%s\n  status %d, offsets %s (%s)" % (CS.describe(st), st_, offs.tolist()[:8], msg)
                return
            s.set_tuning("hit_cap", CS.HIT_CAP_SMALL)                    # the first pool overflows; the library repeats the pass
            try:
                self.check(st, self.call(st), " (hit_cap %d)" % CS.HIT_CAP_SMALL)
            finally:
                s.set_tuning("hit_cap", 0)
            return
        if st.family == "search_small":
            # the same call three times: plain, captured, replayed (host_pass_begin: candidate, capture, replay)
            before = s.graph_replays
            for n, name in enumerate(("plain", "capture", "replay")):
                hashed = s.self_hash_passes
                self.check(st, self.call(st), " (call %d: %s)" % (n, name))
                if CS.must_self_hash(st, self.handle):                  # the capture and the replay count like the plain pass
                    assert s.self_hash_passes > hashed, "%s\n  call %d (%s) did not take the self-hashing form" % (CS.describe(st), n, name)
            grew = s.graph_replays - before
            if st.graph == 0:
                assert grew == 0, "%s\n  graph is off and graph_replays grew by %d" % (CS.describe(st), grew)
            else:
                assert grew >= 1, "%s\n  three equal calls and no graph replay" % CS.describe(st)
            return
        reader = PASS_READERS.get(st.family)
        if reader:
            getattr(s, reader)()                                        # (reading resets the counters)
        got = self.call(st)
        self.check(st, got)
        if CS.needs_three_passes(st, self.ex):
            passes = getattr(s, reader)()["passes"]
            assert passes >= 3, "%s\n  %d device passes under pass_bytes = %d" % (CS.describe(st), passes, st.pass_bytes)


def _plain(v):
    """lists and tuples alike, down to ints"""
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return int(v)


@pytest.mark.parametrize("handle", CS.HANDLES)
def test_every_family_after_every_other_on_one_handle(gpu_lib, monkeypatch, tmp_path, handle):
    import torch
    paths, files = CS.build_files(tmp_path, handle)
    ex = CS.Expect(files)
    plan = CS.build_plan()
    for st in plan:                                                     # the expected values first: the walk's time is the library's
        if st.kind in ("regular", "overflow"):
            ex.value(st)
            if st.family == "adjusted":
                ex.adjusted_floats(st)
    if handle.endswith("idx64"):
        monkeypatch.setenv("COBS_GPU_IDX64", "1")       # (read when a handle is opened)

    def walk(steps):
        s = gpu_lib.Search(paths if len(paths) > 1 else paths[0])
        b = gpu_lib.Batch(s)
        w = Walker(gpu_lib, s, b, ex, handle)
        t0 = time.perf_counter()
        for st in steps:
            try:
                w.step(st)
            except gpu_lib.CobsGpuError as e:
                raise AssertionError("%s\n  raised %r" % (CS.describe(st), e))
        wall = time.perf_counter() - t0
        stats = (s.graph_replays, s.host_passes, s.self_hash_passes)
        b.close()
        s.close()
        assert not s._h
        return wall, stats

    def free_bytes():
        gc.collect()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    wall, (replays, passes, hashed) = walk(plan)
    print("%s: %d steps walked in %.2f s, %d graph replays, %d host passes, %d self_hash_passes" % (
        handle, len(plan), wall, replays, passes, hashed))
    assert (hashed > 0) == CS.self_hash_handle(handle)
    # no device memory is left: as the leak tests of the suite measure it, over repeated open / walk / close cycles (the
    # whole walk above was the first).  A cycle walks the shortest start of the plan that reaches every family and a failure step.  The bound is 64 KiB per
    # cycle: a handle keeps at least its index on the device, and the smallest index file here has 66 KiB of rows, so a
    # handle that is not given back -- let alone its workspaces, pools and graphs -- is above it
    n = next(n for n in range(len(plan) + 1)
             if {st.family for st in plan[:n]} == set(CS.FAMILIES) and {st.kind for st in plan[:n]} > {"regular"})
    prefix = plan[:n]
    free0 = free_bytes()
    for _ in range(LEAK_CYCLES):
        walk(prefix)
    free1 = free_bytes()
    print("%s: free device memory fell by %d bytes over %d cycles" % (handle, free0 - free1, LEAK_CYCLES))
    assert free0 - free1 < LEAK_CYCLES * (64 << 10), (free0, free1)
