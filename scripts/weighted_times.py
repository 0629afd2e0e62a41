#!/usr/bin/env python3
"""scripts/weighted_times.py -- what the stages of the weighted search (cobs_gpu_search_weighted) cost, beside the two
existing kernels they are built from.

The C3 procedural geometry with planted documents and the headline batch (10 000 x 1000-k-mer queries cut from the
planted sequences) at threshold 0.8.  In one process, on one handle, alternating, several repetitions each (every
measured call follows an unmeasured call of its own kind): the four
stages of the weighted call (cobs_gpu_weighted_ms: K1, prevalence, weights, weighted scan), the plain scan of
cobs_gpu_search_batch at the same threshold (the handle's "scan" timer: K2 with its threshold epilogue) and the
prevalence kernel of cobs_gpu_prevalence (cobs_gpu_prevalence_ms) -- the yardsticks, code the weighted call does not
change.  Algorithmic bytes: the weighted scan moves K2's row bytes (positions x H x row bytes per sub-index) plus 1 byte
per position; the whole call moves them twice plus 5 bytes per position.  A text table on stdout, the same in --out
(default profiles/weighted_times.txt).

    python scripts/weighted_times.py [--reps 5] [--queries 10000] [--kmers 1000] [--scale 1.0] [--threshold 0.8] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--kmers", type=int, default=1000)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--threshold", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_times.txt"))
    args = ap.parse_args()
    cfg = bench.c3_config(args.scale)
    plants = bench.planted_documents(cfg, args.kmers)
    cfg["plants"] = plants
    queries = bench.planted_queries(plants, args.queries, args.kmers)
    s = bench.make_index(cfg, 0)
    stages = ("hash_ms", "prevalence_ms", "weights_ms", "scan_ms")
    w = {k: [] for k in stages}
    k2, prev = [], []
    hits_w = hits_k2 = 0
    for rep in range(args.reps):
        # every measured call follows an unmeasured call of its own kind: clocks and caches as in a stream of such calls
        s.search_weighted_arrays(queries, args.threshold, 0)
        s.weighted_ms()
        offs, hits, _total = s.search_weighted_arrays(queries, args.threshold, 0)
        t = s.weighted_ms()
        assert t["passes"] == 1, t               # (one run of one pass: the result buffer of the mirror was large enough)
        hits_w = int(offs[-1])
        s.search_arrays(queries, args.threshold, 0)
        s.timers(reset=True)
        offs, hits = s.search_arrays(queries, args.threshold, 0)
        hits_k2 = int(offs[-1])
        scan = s.timers(reset=True)["scan"] * 1e3
        s.prevalence_arrays(queries)
        s.prevalence_ms()
        s.prevalence_arrays(queries)
        p = s.prevalence_ms()["kernel_ms"]
        for k in stages:
            w[k].append(t[k])
        k2.append(scan)
        prev.append(p)
    med = statistics.median
    positions = len(queries) * args.kmers
    row_bytes = cfg["page_size"] * len(cfg["signature_sizes"]) * cfg["num_hashes"]
    scan_bytes = positions * (row_bytes + 1)
    call_bytes = positions * (2 * row_bytes + 5)
    lines = ["# scripts/weighted_times.py: C3 procedural (scale %g), %d queries x %d k-mers from planted sequences, threshold %g, "
             "%d repetitions (median [min .. max], ms)" % (args.scale, len(queries), args.kmers, args.threshold, args.reps)]
    for k in stages:
        lines.append("weighted %-14s %9.3f  [%9.3f .. %9.3f]" % (k, med(w[k]), min(w[k]), max(w[k])))
    lines.append("K2 scan (search_batch)  %9.3f  [%9.3f .. %9.3f]" % (med(k2), min(k2), max(k2)))
    lines.append("prevalence kernel       %9.3f  [%9.3f .. %9.3f]" % (med(prev), min(prev), max(prev)))
    lines.append("hits: weighted %d, plain %d" % (hits_w, hits_k2))
    lines.append("weighted scan: %.3e algorithmic bytes, %.3f TB/s; ratio to K2's time %.3f" %
                 (scan_bytes, scan_bytes / med(w["scan_ms"]) / 1e9, med(w["scan_ms"]) / med(k2)))
    total = sum(med(w[k]) for k in stages[1:])
    lines.append("weighted call (prevalence + weights + scan): %.3e algorithmic bytes, %.3f TB/s; ratio to K2 + prevalence %.3f" %
                 (call_bytes, call_bytes / total / 1e9, total / (med(k2) + med(prev))))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    s.close()


if __name__ == "__main__":
    main()
