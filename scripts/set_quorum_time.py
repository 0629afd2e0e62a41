#!/usr/bin/env python3
"""scripts/set_quorum_time.py -- what the kernels of the quorum search (cobs_gpu_search_sets_quorum) cost beside the set
search and the prevalence kernel.

The batch and the two labellings of scripts/sets_time.py (profiles/sets_time.txt): the C3 procedural geometry (BASELINE
configs[2]: compact, 100 000 documents, 8 sub-indexes) through cobs_gpu_open_synthetic, 1000 random queries of 1000 k-mers,
  (a) contiguous sets of 100 documents -- a collection sorted by name: a set covers 1-2 column chunks of one page;
  (b) d % 1000 -- every set scattered over every chunk: one inverse record per (column chunk, set) with a member there.
In one process, on one handle; every measured call follows an unmeasured call of its own kind.  hash_ms / count_ms /
select_ms are the library's HIP-event timers (cobs_gpu_set_quorum_ms), presence_ms + select_ms those of cobs_gpu_search_sets
(cobs_gpu_sets_ms), prevalence_ms is cobs_gpu_prevalence_ms' kernel time on the same batch.  `hits` are the sets the call
returned (random queries at quorum 0.95 and threshold 0.5: none, so select_ms is a select that appends nothing).  The GPU
step runs in a child process under its own time limit.  A text table on stdout, the same in --out (default
profiles/set_quorum_time.txt).

    python scripts/set_quorum_time.py [--reps 3] [--queries 1000] [--kmers 1000] [--scale 1.0] [--quorum 0.95]
                                      [--timeout 420] [--out FILE]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step(args):
    import numpy as np

    import bench
    cfg = bench.c3_config(args.scale)
    queries = bench.make_queries(args.queries, args.kmers)
    s = bench.make_index(cfg, 0)
    docs = np.arange(cfg["num_docs"])
    med = statistics.median
    s.prevalence_arrays(queries)
    prev = []
    for _ in range(args.reps):
        s.prevalence_ms()
        s.prevalence_arrays(queries)
        prev.append(s.prevalence_ms()["kernel_ms"])
    lines = []

    def emit(line):                 # (line by line: a long step shows where it is)
        lines.append(line)
        print(line, flush=True)

    def row(name, v):
        emit("  %-36s %10.3f  [%10.3f .. %10.3f]" % (name, med(v), min(v), max(v)))
    emit("# scripts/set_quorum_time.py: C3 procedural (scale %g), %d queries x %d k-mers, quorum %g, threshold 0.5, %d repetitions "
         "(median [min .. max], ms)" % (args.scale, len(queries), args.kmers, args.quorum, args.reps))
    emit("prevalence_ms                          %10.3f  [%10.3f .. %10.3f]" % (med(prev), min(prev), max(prev)))
    for name, labels in (("(a) contiguous sets of 100", docs // 100), ("(b) d % 1000", docs % 1000)):
        s.set_doc_sets(labels)
        offs, _hits = s.search_sets_quorum_arrays(queries, args.quorum, 0.5)
        t = {"hash_ms": [], "count_ms": [], "select_ms": [], "order_ms": []}
        for _ in range(args.reps):
            s.set_quorum_ms()
            s.search_sets_quorum_arrays(queries, args.quorum, 0.5)
            ms = s.set_quorum_ms()
            assert ms["passes"] == 1, ms
            for k in t:
                t[k].append(ms[k])
        s.search_sets_arrays(queries, 0.5)
        old = {"presence_ms": [], "select_ms": []}
        for _ in range(args.reps):
            s.sets_ms()
            s.search_sets_arrays(queries, 0.5)
            ms = s.sets_ms()
            assert ms["passes"] == 1, ms
            for k in old:
                old[k].append(ms[k])
        # (host arithmetic over the labels: a run per (sub-index, set with a member in it), an inverse record per
        # (16-byte column chunk, set with a member in it); a sub-index is a whole number of column chunks here)
        nsets = int(labels.max()) + 1
        runs = len(np.unique((docs // (8 * cfg["page_size"])) * nsets + labels))
        recs = len(np.unique((docs // 128) * nsets + labels))
        emit("%s: %d sets, %d runs, %d inverse records, %d hits" % (name, nsets, runs, recs, int(offs[-1])))
        row("K1 hash_ms", t["hash_ms"])
        row("set_count_kernel count_ms", t["count_ms"])
        row("set_quorum_select_kernel select_ms", t["select_ms"])
        row("order_ms (host)", t["order_ms"])
        row("set_presence_kernel presence_ms", old["presence_ms"])
        row("set_select_kernel select_ms", old["select_ms"])
        emit("  count_ms / presence_ms   = %.2f" % (med(t["count_ms"]) / med(old["presence_ms"])))
        emit("  count_ms / prevalence_ms = %.2f" % (med(t["count_ms"]) / med(prev)))
    s.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--kmers", type=int, default=1000)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--quorum", type=float, default=0.95)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the GPU step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_quorum_time.txt"))
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    # the GPU step in a fresh child process under its own time limit: a step that hangs ends there
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step"] + sys.argv[1:], timeout=args.timeout)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
