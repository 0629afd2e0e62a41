#!/usr/bin/env python3
"""scripts/best_bench.py -- what the best-of-group kernel costs beside the accumulate kernel of the grouped search.

The procedural C3 index with planted documents and the batch of `bench.py --full`'s end_to_end (10 000 queries of 1000
k-mers with hits).  In one process, alternating, several repetitions each, on the same batch and grouping:
  tens       the whole batch in groups of 10 (one writer per cell in both calls)
  one_1000   the first 1000 queries as ONE group (the grouped call's atomic path, the best call's partial states)
cobs_gpu_search_groups beside cobs_gpu_search_best, with the library's own timers (Search.groups_ms, Search.best_ms: HIP
events).  Both kernels are bound by one read of the score matrix, so the yardstick of the best kernel is the accumulate
kernel's time on the same rows in the same run: the ratio best / accumulate.  Self-check: groups of ONE query give the
plain search's documents and scores.  A table on stdout, the same in --out (default profiles/best_times.txt).

    python scripts/best_bench.py [--queries 10000] [--kmers 1000] [--reps 5] [--scale 1.0] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--kmers", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--threshold", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "best_times.txt"))
    args = ap.parse_args()

    cfg = bench.c3_config(args.scale)
    cfg["plants"] = bench.planted_documents(cfg, args.kmers)
    s = bench.make_index(cfg, 0)
    queries = bench.planted_queries(cfg["plants"], args.queries, args.kmers)
    nq = len(queries)
    shapes = {
        "tens": (queries, np.unique(np.minimum(np.arange(0, nq + 10, 10), nq)).astype(np.uint64)),
        "one_1000": (queries[:1000], np.array([0, min(nq, 1000)], dtype=np.uint64)),
    }
    k = {name: {"acc": [], "gsel": [], "best": [], "bsel": [], "gwall": [], "bwall": []} for name in shapes}
    info = {}
    for rep in range(args.warmup + args.reps):
        for name, (qs, offs) in shapes.items():
            t0 = time.perf_counter()
            _o, gh, _p = s.search_groups_arrays(qs, offs, args.threshold, args.threshold, 0)
            t1 = time.perf_counter()
            g = s.groups_ms()
            t2 = time.perf_counter()
            _o, bh = s.search_best_arrays(qs, offs, args.threshold, 0)
            t3 = time.perf_counter()
            m = s.best_ms()
            info[name] = (len(qs), len(offs) - 1, len(gh), len(bh), m)
            if rep >= args.warmup:
                for key, v in (("acc", g["accumulate_ms"]), ("gsel", g["select_ms"]), ("best", m["best_ms"]), ("bsel", m["select_ms"]),
                               ("gwall", (t1 - t0) * 1e3), ("bwall", (t3 - t2) * 1e3)):
                    k[name][key].append(v)
    # self-check: groups of one query are the plain search
    so, sh = s.search_arrays(queries[:200], args.threshold, 0)
    bo, bh = s.search_best_arrays(queries[:200], np.arange(201, dtype=np.uint64), args.threshold, 0)
    ok = bool(np.array_equal(so, bo) and all(np.array_equal(sh[c], bh[c]) for c in ("file_no", "doc", "score"))
              and np.array_equal(bh["query"], np.repeat(np.arange(200), np.diff(bo).astype(np.int64))) and np.all(bh["ties"] == 1))

    def med(v):
        return statistics.median(v)

    elem = 1 if args.kmers <= 255 else 2 if args.kmers <= 65535 else 4
    lines = ["# scripts/best_bench.py: %d documents, queries of %d k-mers (score rows of %d bytes), threshold %.2f, %d repetitions"
             % (int(s.total_counts), args.kmers, elem, args.threshold, args.reps),
             "# kernel times from HIP events (cobs_gpu_groups_ms | cobs_gpu_best_ms), median (min .. max) in ms; wall = the whole call",
             "%-10s %8s %7s %28s %28s %7s %10s %10s %10s %10s" % ("grouping", "queries", "groups", "accumulate_ms", "best_ms", "ratio",
                                                                 "gsel_ms", "bsel_ms", "gwall_ms", "bwall_ms")]
    for name in shapes:
        n, ng, ngh, nbh, m = info[name]
        v = k[name]
        lines.append("%-10s %8d %7d %28s %28s %7.2f %10.3f %10.3f %10.1f %10.1f" % (
            name, n, ng, "%.3f (%.3f .. %.3f)" % (med(v["acc"]), min(v["acc"]), max(v["acc"])),
            "%.3f (%.3f .. %.3f)" % (med(v["best"]), min(v["best"]), max(v["best"])), med(v["best"]) / max(med(v["acc"]), 1e-9),
            med(v["gsel"]), med(v["bsel"]), med(v["gwall"]), med(v["bwall"])))
        mb = n * int(s.local_counts) * elem / 1e6
        lines.append("#   %s: score matrix %.1f MB; best kernel reads it at %.0f GB/s, accumulate at %.0f GB/s; records %d (groups) %d (best); "
                     "passes %d, own spans %d, partial states %d, split groups %d"
                     % (name, mb, mb / 1e3 / (med(v["best"]) * 1e-3), mb / 1e3 / (med(v["acc"]) * 1e-3), ngh, nbh, m["passes"],
                        m["own_spans"], m["pieces"], m["split_groups"]))
    lines.append("# groups of one query equal the plain search: %s" % ok)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    s.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
