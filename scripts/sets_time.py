#!/usr/bin/env python3
"""scripts/sets_time.py -- what the kernels of the set search (cobs_gpu_search_sets) cost beside the prevalence kernel.

There is no earlier time for this call; its yardstick is cobs_gpu_prevalence on the same handle and batch: that call reads
the same rows and writes less.  The C3 procedural geometry (BASELINE configs[2]: compact, 100 000 documents, 8
sub-indexes) through cobs_gpu_open_synthetic, 1000 random queries of 1000 k-mers, two labellings:
  (a) contiguous sets of 100 documents -- a collection sorted by name: 1-2 segment records per 16-byte column chunk;
  (b) d % 1000 -- every set scattered over every chunk: 128 records per chunk, 32 batches of kSetBatch.
In one process, on one handle; every measured call follows an unmeasured call of its own kind.  presence_ms / select_ms
are the library's HIP-event timers (cobs_gpu_sets_ms), prevalence_ms is cobs_gpu_prevalence_ms' kernel time; the ratio is
presence_ms / prevalence_ms.  The GPU step runs in a child process under its own time limit.  A text table on stdout, the
same in --out (default profiles/sets_time.txt).

    python scripts/sets_time.py [--reps 3] [--queries 1000] [--kmers 1000] [--scale 1.0] [--timeout 420] [--out FILE]
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
    emit("# scripts/sets_time.py: C3 procedural (scale %g), %d queries x %d k-mers, threshold 0.5 by any, %d repetitions "
         "(median [min .. max], ms)" % (args.scale, len(queries), args.kmers, args.reps))
    emit("prevalence_ms              %10.3f  [%10.3f .. %10.3f]" % (med(prev), min(prev), max(prev)))
    for name, labels in (("(a) contiguous sets of 100", docs // 100), ("(b) d % 1000", docs % 1000)):
        s.set_doc_sets(labels)
        offs, _hits = s.search_sets_arrays(queries, 0.5)
        t = {"presence_ms": [], "select_ms": [], "hash_ms": [], "order_ms": []}
        for _ in range(args.reps):
            s.sets_ms()
            s.search_sets_arrays(queries, 0.5)
            ms = s.sets_ms()
            assert ms["passes"] == 1, ms
            for k in t:
                t[k].append(ms[k])
        emit("%s: %d sets, %d records" % (name, int(labels.max()) + 1, int(offs[-1])))
        for k in ("presence_ms", "select_ms", "hash_ms", "order_ms"):
            emit("  %-24s %10.3f  [%10.3f .. %10.3f]" % (k, med(t[k]), min(t[k]), max(t[k])))
        emit("  presence_ms / prevalence_ms = %.2f" % (med(t["presence_ms"]) / med(prev)))
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
    ap.add_argument("--timeout", type=int, default=420, help="seconds the GPU step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sets_time.txt"))
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    # the GPU step in a fresh child process under its own time limit: a step that hangs ends there
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step"] + sys.argv[1:], timeout=args.timeout)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
